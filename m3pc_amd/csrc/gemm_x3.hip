// Split-bf16 ("bf16x3") MFMA GEMM for gfx950: C = epilogue(A * W^T) with A fp32 activations and W given as two bf16 copies,
// hi = bf16(w) and lo = bf16(w - hi) (m3pc_load_weights), lo at W + w_lo_off elements.  A is split the same way while it is
// staged (round to nearest even), and every k-step issues three v_mfma_f32_32x32x16_bf16 into one fp32 accumulator:
//     a . w  ~  a_hi . w_hi + a_hi . w_lo + a_lo . w_hi
// The dropped term a_lo . w_lo and the rounding of lo leave a relative error of ~2^-16 per product; gfx950 has no xf32, and
// this runs three bf16 MFMAs (3 x 8 passes) where the fp32 kernel runs eight v_mfma_f32_32x32x2_f32 (8 x 16 passes) per 16 k.
//
// Tiling as gemm_kernel (gemm.hip): 2x2 waves, 32x32 MFMA tiles, LDS rows of 128 bytes padded to 144, two LDS buffers, the
// global loads of tile k+1 and k+2 in flight in registers while tile k is multiplied.  A k-tile is 32 k; its LDS row holds
//     bytes [0, 64): hi of k 0..31     bytes [64, 128): lo of k 0..31
// for A and W alike, so quarter s of the row (32 B) is one bf16 MFMA fragment exactly as in gemm_kernel: hi is quarters 0, 1,
// lo is quarters 2, 3.  A thread stages 4 floats of A (16 B from global) as 8 B of hi and 8 B of lo; W's hi and lo rows are
// loaded as they are, 16 B per chunk.
//
// Every output element sums its k-tiles in order, and within a k-tile the same six MFMAs in the same order, whatever the tile
// shape: the 64x64 and 128x128 configurations give identical bits, so the choice may depend on the row count.  Split-K (only
// where GemmP::ws is set, i.e. where the caller allows a row-count dependent result) re-associates the K sum.
#include "gemm_epilogue.h"

namespace m3pc {

#define X3_ROW 144

// hi = bf16_rne(x) (v_cvt_pk_bf16_f32), lo = bf16_rne(x - hi); x - hi is exact in fp32
__device__ __forceinline__ void x3_split4(u32x4 raw, u32x2& hi, u32x2& lo) {
    const f32x4 x = __builtin_bit_cast(f32x4, raw);
    bf16x4 h, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        h[e] = (__bf16)x[e];
        l[e] = (__bf16)(x[e] - (float)h[e]);
    }
    hi = __builtin_bit_cast(u32x2, h);
    lo = __builtin_bit_cast(u32x2, l);
}

template <int BM, int BN, int EPI>
__global__ __launch_bounds__(256) void gemm_x3_kernel(GemmP p) {
    constexpr int TM = BM / 64, TN = BN / 64;                // 32x32 MFMA tiles per wave (2x2 waves)
    constexpr int A_CH = BM * 8 / 256, W_CH = BN * 8 / 256;  // 16-byte global chunks per thread per k-tile
    constexpr int BUF = (BM + BN) * X3_ROW;
    __shared__ __attribute__((aligned(16))) char smem[2 * BUF];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    // XCD-aware tile order (as gemm_kernel): each XCD gets a contiguous run of tiles
    const int ntn = p.N / BN;
    const int ntm = (p.M + BM - 1) / BM;
    const int nwg = ntm * ntn;
    int bid = blockIdx.x;
    {
        const int q = nwg / 8, r = nwg % 8, x = bid % 8, i = bid / 8;
        bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
    }
    const int tm = bid / ntn, tn = bid % ntn;
    const int row0 = tm * BM, col0 = tn * BN;

    const char* Ab = (const char*)p.A;
    const char* Wb = (const char*)p.W;
    const long long lda_b = (long long)p.lda * 4, ldw_b = (long long)p.ldw * 2, wlo_b = p.w_lo_off * 2;
    const int nkt = p.K / 32;
    int kt0 = 0, kt1 = nkt;
    if constexpr (EPI & GE_SPLITK) {
        kt0 = (int)((long long)nkt * blockIdx.y / gridDim.y);
        kt1 = (int)((long long)nkt * (blockIdx.y + 1) / gridDim.y);
    }

    // A: chunk c = row c / 8, floats 4 (c % 8) .. +3 of the k-tile -> hi at byte 8 (c % 8), lo at 64 + 8 (c % 8) of the LDS row
    const char* a_src[A_CH];
    int a_dst[A_CH];
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
        const int c = tid + i * 256, r = c >> 3, kc = c & 7;
        int gr = row0 + r;
        if (gr >= p.M) gr = p.M - 1;
        a_src[i] = Ab + (long long)map_row(p.amap, gr) * lda_b + kc * 16 + (long long)kt0 * 128;
        a_dst[i] = r * X3_ROW + kc * 8;
    }
    // W: chunk c = row c / 8, piece c % 8: pieces 0..3 the 64 hi bytes, 4..7 the 64 lo bytes of the k-tile
    const char* w_src[W_CH];
    int w_dst[W_CH];
#pragma unroll
    for (int i = 0; i < W_CH; ++i) {
        const int c = tid + i * 256, r = c >> 3, kc = c & 7;
        w_src[i] = Wb + (long long)(col0 + r) * ldw_b + (kc & 3) * 16 + (kc >> 2) * wlo_b + (long long)kt0 * 64;
        w_dst[i] = BM * X3_ROW + r * X3_ROW + kc * 16;
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int nloc = kt1 - kt0;
    u32x4 ra0[A_CH], rw0[W_CH], ra1[A_CH], rw1[W_CH];
    auto gload = [&](u32x4* ra, u32x4* rw, int kt) {
#pragma unroll
        for (int i = 0; i < A_CH; ++i) ra[i] = *(const u32x4*)(a_src[i] + (long long)kt * 128);
#pragma unroll
        for (int i = 0; i < W_CH; ++i) rw[i] = *(const u32x4*)(w_src[i] + (long long)kt * 64);
    };
    auto lstore = [&](const u32x4* ra, const u32x4* rw, char* buf) {
#pragma unroll
        for (int i = 0; i < A_CH; ++i) {
            u32x2 hi, lo;
            x3_split4(ra[i], hi, lo);
            *(u32x2*)(buf + a_dst[i]) = hi;
            *(u32x2*)(buf + a_dst[i] + 64) = lo;
        }
#pragma unroll
        for (int i = 0; i < W_CH; ++i) *(u32x4*)(buf + w_dst[i]) = rw[i];
    };
    gload(ra0, rw0, 0);
    lstore(ra0, rw0, smem);
    if (nloc > 1) gload(ra0, rw0, 1);
    if (nloc > 2) gload(ra1, rw1, 2);
    __syncthreads();

    const int fragA = (wr * (BM / 2) + (lane & 31)) * X3_ROW + 16 * (lane >> 5);
    const int fragW = BM * X3_ROW + (wc * (BN / 2) + (lane & 31)) * X3_ROW + 16 * (lane >> 5);

    auto compute = [&](const char* cur) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            u32x4 ah[TM], al[TM], wh[TN], wl[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                ah[i] = *(const u32x4*)(cur + fragA + i * 32 * X3_ROW + 32 * s);
                al[i] = *(const u32x4*)(cur + fragA + i * 32 * X3_ROW + 64 + 32 * s);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                wh[j] = *(const u32x4*)(cur + fragW + j * 32 * X3_ROW + 32 * s);
                wl[j] = *(const u32x4*)(cur + fragW + j * 32 * X3_ROW + 64 + 32 * s);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const bf16x8 a_h = __builtin_bit_cast(bf16x8, ah[i]), a_l = __builtin_bit_cast(bf16x8, al[i]);
                    const bf16x8 w_h = __builtin_bit_cast(bf16x8, wh[j]), w_l = __builtin_bit_cast(bf16x8, wl[j]);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_h, w_h, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_h, w_l, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_l, w_h, acc[i][j], 0, 0, 0);
                }
        }
    };
    auto step = [&](u32x4* ra, u32x4* rw, int kt) {
        compute(smem + (kt & 1) * BUF);
        if (kt + 1 < nloc) lstore(ra, rw, smem + ((kt + 1) & 1) * BUF);
        __syncthreads();
        if (kt + 3 < nloc) gload(ra, rw, kt + 3);
    };
    for (int kt = 0; kt < nloc; kt += 2) {
        step(ra0, rw0, kt);
        if (kt + 1 < nloc) step(ra1, rw1, kt + 1);
    }

    // acc[i][j][reg]: row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), column lane & 31 of the 32x32 tile
    if constexpr (EPI & GE_SPLITK) {
        float* slab = p.ws + (long long)blockIdx.y * p.M * p.N;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int r = row0 + wr * (BM / 2) + i * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
                if (r < p.M) {
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        slab[(long long)r * p.N + col0 + wc * (BN / 2) + j * 32 + (lane & 31)] = acc[i][j][reg];
                }
            }
        return;
    } else {
        const int wu = __builtin_amdgcn_readfirstlane(wid);
        const int rbase = row0 + (wu >> 1) * (BM / 2), cbase = col0 + (wu & 1) * (BN / 2);
        gemm_epilogue<EPI, TM, TN>(p, acc, rbase, cbase, row0, BM, lane);
    }
}

// hi / lo bf16 copies of an fp32 tensor (weights: m3pc_load_weights; the lab GEMM entry's W)
__global__ __launch_bounds__(256) void f32_split_bf16_kernel(const float* in, bf16_t* hi, bf16_t* lo, long long n) {
    for (long long x = blockIdx.x * 256LL + threadIdx.x; x < n; x += (long long)gridDim.x * 256) {
        const float v = in[x];
        const bf16_t b = (bf16_t)v;
        hi[x] = b;
        lo[x] = (bf16_t)(v - (float)b);
    }
}
void launch_f32_split_bf16(const float* in, bf16_t* hi, bf16_t* lo, long long n, hipStream_t st) {
    if (n <= 0) return;
    const long long g = (n + 255) / 256;
    hipLaunchKernelGGL(f32_split_bf16_kernel, dim3((unsigned)(g < 4096 ? g : 4096)), dim3(256), 0, st, in, hi, lo, n);
}

template <int BM, int BN, int EPI>
static void x3_launch(const GemmP& p, int S, hipStream_t st) {
    const int grid = ((p.M + BM - 1) / BM) * (p.N / BN);
    M3PC_GEMM_LAUNCH((gemm_x3_kernel<BM, BN, EPI>), dim3(grid, S), dim3(256), 0, st, p);
}

template <int EPI>
static int x3_launch_epi(const GemmP& p, hipStream_t st) {
    // tile choice and split-K as the fp32 kernel's (launch_epi, gemm.hip): 128x128 tiles where they fill the chip twice over,
    // else 64x64; split K over blocks only where the caller allows it (p.ws) and the tiles alone do not fill the chip
    const long long big_tiles = (long long)((p.M + 127) / 128) * (p.N / 128);
    if ((p.N % 128) == 0 && big_tiles >= 512) {
        M3PC_GEMM_PICK(13, 1, 0, 0);
        x3_launch<128, 128, EPI>(p, 1, st);
        return 0;
    }
    const long long tiles = (long long)((p.M + 63) / 64) * (p.N / 64);
    const int nkt = p.K / 32;
    int S = 1;
    if (p.ws && tiles < 768 && (tiles < 200 || nkt > 16)) {
        S = (int)((1023 + tiles) / tiles);
        if (S > nkt / 4) S = nkt / 4;
        if (S > 16) S = 16;
        while (S > 1 && (long long)S * p.M * p.N * 4 > p.ws_bytes) --S;
    }
    M3PC_GEMM_PICK(12, S, 0, 0);
    if (S > 1) {
        x3_launch<64, 64, GE_SPLITK>(p, S, st);
        return launch_splitk_reduce(p, S, 1, st);
    }
    x3_launch<64, 64, EPI>(p, 1, st);
    return 0;
}

// returns 1 when the LayerNorm of p.ln_* was applied (split-K reduce), 0 otherwise, -1 when the problem is not covered
int launch_gemm_x3(const GemmP& p, hipStream_t st) {
    if (p.M <= 0) return 0;
    if (p.K % 32 != 0 || p.N % 64 != 0 || p.w_lo_off <= 0 || p.w_lo_off % 8 != 0 || (p.Cf == nullptr) == (p.Cb == nullptr)) return -1;
    if (((uintptr_t)p.A & 15) || ((uintptr_t)p.W & 15) || p.lda % 4 != 0 || p.ldw % 8 != 0 || p.a_ln_g) return -1;
    const int epi = epi_flags(p) | (p.gelu ? GE_GELU_EXACT : 0);
    switch (epi) {
        case GE_F32OUT: return x3_launch_epi<GE_F32OUT>(p, st);
        case GE_GELU | GE_GELU_EXACT | GE_F32OUT: return x3_launch_epi<GE_GELU | GE_GELU_EXACT | GE_F32OUT>(p, st);
        case GE_RES | GE_F32OUT: return x3_launch_epi<GE_RES | GE_F32OUT>(p, st);
        case GE_ROWTAB | GE_F32OUT: return x3_launch_epi<GE_ROWTAB | GE_F32OUT>(p, st);
        case 0: return x3_launch_epi<0>(p, st);
        case GE_GELU | GE_GELU_EXACT: return x3_launch_epi<GE_GELU | GE_GELU_EXACT>(p, st);
        default: return -1;  // no caller combines the remaining flags
    }
}

}  // namespace m3pc
