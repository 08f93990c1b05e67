// The device bodies of the product and of the three attention kernels of the gradient of the masked-trajectory loss, shared by
// mtm_grad.hip (DROP = false: the kernels of the eval-mode model) and mtm_dropout.hip (DROP = true: the same code with the keep
// masks of mtm_grad.h, DROPOUT).  With DROP = false nothing of the dropout is compiled in.
#pragma once
#include <stdint.h>

#include "device_util.h"
#include "mtm_grad.h"
#include "philox.h"

namespace m3pc {
namespace {

#if defined(__HIP_DEVICE_COMPILE__)
#define MG_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)
#else
#define MG_MFMA(a, b, c) ((void)(a), (void)(b), (c))
#endif

// ------------------------------------------------------------------------------------------------ the keep masks
// the four words of a quad; bit w of the result: word w >= thr (kept)
__device__ __forceinline__ unsigned int drop_keep4(const DropG& d, uint32_t quad) {
    uint32_t w[4];
    philox4x32_10(quad, d.d0, d.d1, d.c3, d.k0, d.k1, w);
    return (w[0] >= d.thr ? 1u : 0u) | (w[1] >= d.thr ? 2u : 0u) | (w[2] >= d.thr ? 4u : 0u) | (w[3] >= d.thr ? 8u : 0u);
}
// x * k: one rounding, nothing fused into a neighbouring add
__device__ __forceinline__ float drop_apply(bool kept, float x, float scale) { return kept ? __fmul_rn(x, scale) : 0.f; }

// ------------------------------------------------------------------------------------------------ the product
// C[m][n] = sum_k A(m, k) B(k, n) (GemmG, mtm_grad.h)
__device__ __forceinline__ float gelu_grad_exact(float x) {
    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
    const float pdf = 0.39894228040143267794f * expf(-0.5f * x * x);
    return cdf + x * pdf;
}

// One wavefront per 32 x 32 tile of C.  MFMA operand a: lane holds A(m = lane & 31, k = lane >> 5); b: B(k = lane >> 5, n = lane & 31);
// accumulator i is row 8 (i / 4) + 4 (lane >> 5) + i % 4, column lane & 31.  K in ascending blocks of 16: step u of a block multiplies
// k = 8 (u / 4) + u % 4 (lower lane half) and that + 4 (upper half); the operands of the next block are loaded ahead of the eight MFMAs of
// this one, four consecutive k per 16-byte load where the operand is k-contiguous and aligned (vec).
// SPLIT (the dW form, K = rows: few tiles, long K): the four wavefronts of a workgroup share ONE tile, wavefront w taking the k
// blocks w, w + 4, ...; the partial tiles of wavefronts 1, 2, 3 go through LDS and wavefront 0 adds them in that order.
// DROP: the accumulators 4 g .. 4 g + 3 of a lane are the rows 4 q .. 4 q + 3 of one column, one quad of the site: one Philox call.
__device__ __forceinline__ void mg_load8(const GOp& op, const float* base, bool o_ok, int k0, int lh, int K, float* v) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int k = k0 + 8 * h + 4 * lh;
        if (op.vec && o_ok && k + 3 < K) {
            const f32x4 x = *(const f32x4*)(base + k);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * h + j] = x[j];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kk = k + j;
                const bool ok = o_ok && kk < K;
                const long long kr = op.map_k && ok ? rmap(op.map, kk) : (long long)kk;
                v[4 * h + j] = ok ? base[kr * op.s_k] : 0.f;
            }
        }
    }
}

template <bool SPLIT, bool DROP>
__device__ __forceinline__ void mg_gemm_body(const GemmG& p) {
    __shared__ float red[SPLIT ? 3 * 1024 : 1];
    const int lane = threadIdx.x & 63, l31 = lane & 31, lh = lane >> 5, wv = threadIdx.x >> 6;
    const int tiles_n = (p.N + 31) >> 5, tiles_m = (p.M + 31) >> 5;
    const long long w = SPLIT ? (long long)blockIdx.x : (long long)blockIdx.x * 4 + wv;
    if (w >= (long long)tiles_m * tiles_n) return;  // (SPLIT: the grid is the tile count, whole workgroups leave)
    const int tm = (int)(w / tiles_n), tn = (int)(w % tiles_n);
    const int m = 32 * tm + l31, n = 32 * tn + l31;
    const bool m_ok = m < p.M, n_ok = n < p.N;
    const float* pa = p.A.p + (m_ok ? (p.A.map_k ? (long long)m : rmap(p.A.map, m)) * p.A.s_o : 0);
    const float* pb = p.B.p + (n_ok ? (p.B.map_k ? (long long)n : rmap(p.B.map, n)) * p.B.s_o : 0);
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const int kstep = SPLIT ? 64 : 16, kbeg = SPLIT ? 16 * wv : 0;
    float a[8], b[8], a2[8], b2[8];
    if (kbeg < p.K) {
        mg_load8(p.A, pa, m_ok, kbeg, lh, p.K, a);
        mg_load8(p.B, pb, n_ok, kbeg, lh, p.K, b);
    }
    for (int k0 = kbeg; k0 < p.K; k0 += kstep) {
        const bool more = k0 + kstep < p.K;
        if (more) {
            mg_load8(p.A, pa, m_ok, k0 + kstep, lh, p.K, a2);
            mg_load8(p.B, pb, n_ok, k0 + kstep, lh, p.K, b2);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = MG_MFMA(a[u], b[u], acc);
        if (more) {
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] = a2[u], b[u] = b2[u];
        }
    }
    if (SPLIT) {
        if (wv > 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) red[(wv - 1) * 1024 + i * 64 + lane] = acc[i];
        }
        __syncthreads();
        if (wv > 0) return;
#pragma unroll
        for (int w2 = 0; w2 < 3; ++w2)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] += red[w2 * 1024 + i * 64 + lane];
    }
    if (!n_ok) return;
    float add = 0.f;
    if (p.bias) add = p.bias[n];
    if (p.bias2) add += p.bias2[n];
    unsigned int keep = 0xfu;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int mo = 32 * tm + 8 * (i >> 2) + 4 * lh + (i & 3);
        if (DROP && (i & 3) == 0 && mo < p.M) keep = drop_keep4(p.drop, (uint32_t)(mo >> 2) * (uint32_t)p.N + (uint32_t)n);
        if (mo >= p.M) continue;
        const bool kept = (keep >> (i & 3)) & 1u;
        const long long at = rmap(p.cmap, mo) * p.ldc + n;
        float v = acc[i] + add;
        if (p.pos) v += p.pos[(long long)(mo % p.pos_T) * p.N + n];
        if (DROP && !p.gelu_out) v = drop_apply(kept, v, p.drop.scale);
        if (p.res) v += p.res[at];
        if (p.gelu_aux) v *= gelu_grad_exact(p.gelu_aux[at]);
        if (p.accumulate) v += p.C[at];
        p.C[at] = v;
        if (p.gelu_out) p.gelu_out[at] = DROP ? drop_apply(kept, gelu_exact(v), p.drop.scale) : gelu_exact(v);
    }
}

// ------------------------------------------------------------------------------------------------ attention
// DROP, every kernel: the stored P carries "dropped" in its sign bit and the undropped probability in the rest
__device__ __forceinline__ bool att_dropped(float p) { return (__float_as_uint(p) >> 31) != 0u; }

// one wavefront per (b, head, query i): lane owns the keys lane, lane + 64, ...; L <= 256.  DROP: lane q draws the quad of the keys
// 4 q .. 4 q + 3 (ceil(L / 4) <= 64 quads a row) and leaves the four bits in LDS.
template <bool DROP>
__device__ __forceinline__ void mg_attn_fwd_body(const AttG& p) {
    __shared__ float sp[4][MG_ATT_MAX_L];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + wv;
    if (w >= (long long)p.B * p.nh * p.L) return;
    const int i = (int)(w % p.L), hh = (int)((w / p.L) % p.nh), b = (int)(w / ((long long)p.L * p.nh));
    const size_t ld = 3 * (size_t)p.d;
    const float* q = p.QKV + ((size_t)b * p.L + i) * ld + (size_t)hh * p.hd;
    const float* Kb = p.QKV + (size_t)b * p.L * ld + p.d + (size_t)hh * p.hd;
    const float* Vb = Kb + p.d;
    unsigned char* kp = nullptr;
    if constexpr (DROP) {
        __shared__ unsigned char kps[4][MG_ATT_MAX_L];
        kp = kps[wv];
        const int nq = (p.L + 3) >> 2;
        if (lane < nq) {
            const unsigned int k4 = drop_keep4(p.drop, (uint32_t)w * (uint32_t)nq + (uint32_t)lane);
#pragma unroll
            for (int c = 0; c < 4; ++c) kp[4 * lane + c] = (unsigned char)((k4 >> c) & 1u);
        }
    }
    float s[4], mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int j = lane + 64 * c;
        s[c] = -INFINITY;
        if (j < p.L) {
            float a = 0.f;
            for (int e = 0; e < p.hd; ++e) a += (q[e] * p.scale) * Kb[(size_t)j * ld + e];
            s[c] = a;
            mx = fmaxf(mx, a);
        }
    }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        s[c] = lane + 64 * c < p.L ? expf(s[c] - mx) : 0.f;
        sum += s[c];
    }
    sum = wave_sum(sum);
    if (DROP) {  // (the bits of other lanes)
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
    float* Pr = p.P + (((size_t)b * p.nh + hh) * p.L + i) * p.L;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int j = lane + 64 * c;
        if (j < p.L) {
            const float pr = s[c] / sum;
            if (DROP) {
                const bool kept = kp[j] != 0;
                Pr[j] = kept ? pr : -pr;
                sp[wv][j] = drop_apply(kept, pr, p.drop.scale);
            } else {
                Pr[j] = pr;
                sp[wv][j] = pr;
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    for (int e = lane; e < p.hd; e += 64) {
        float a = 0.f;
        for (int j = 0; j < p.L; ++j) a += sp[wv][j] * Vb[(size_t)j * ld + e];
        p.O[((size_t)b * p.L + i) * p.d + (size_t)hh * p.hd + e] = a;
    }
}

// one wavefront per (b, head, key j): out[j][e] = alpha sum_i M[i][j] Z[i][e], queries ascending.  which 0: dV = P^T dO; 1: dK = dS^T Q scale
// DROP (which 0 only): M = P * k
template <bool DROP>
__device__ __forceinline__ void mg_attn_col_body(const AttG& p, int which) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + wv;
    if (w >= (long long)p.B * p.nh * p.L) return;
    const int j = (int)(w % p.L), hh = (int)((w / p.L) % p.nh), b = (int)(w / ((long long)p.L * p.nh));
    const float* Mb = p.P + ((size_t)b * p.nh + hh) * p.L * p.L + j;
    const size_t ldz = which == 0 ? (size_t)p.d : 3 * (size_t)p.d;
    const float* Z = (which == 0 ? p.dO : p.QKV) + (size_t)b * p.L * ldz + (size_t)hh * p.hd;
    const float alpha = which == 0 ? 1.0f : p.scale;
    float* out = p.dQKV + ((size_t)b * p.L + j) * 3 * p.d + (which == 0 ? 2 * p.d : p.d) + (size_t)hh * p.hd;
    for (int e = lane; e < p.hd; e += 64) {
        float a = 0.f;
        for (int i = 0; i < p.L; ++i) {
            float mv = Mb[(size_t)i * p.L];
            if (DROP) mv = drop_apply(!att_dropped(mv), fabsf(mv), p.drop.scale);
            a += mv * Z[(size_t)i * ldz + e];
        }
        out[e] = a * alpha;
    }
}

// one wavefront per (b, head, query i): dP = dO V^T, dS = P (dP - sum_j dP P) over P in place, dQ = dS K scale (keys ascending)
// DROP: dP = (dO V^T) * k, P = |stored P|
template <bool DROP>
__device__ __forceinline__ void mg_attn_row_body(const AttG& p) {
    __shared__ float sp[4][MG_ATT_MAX_L];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + wv;
    if (w >= (long long)p.B * p.nh * p.L) return;
    const int i = (int)(w % p.L), hh = (int)((w / p.L) % p.nh), b = (int)(w / ((long long)p.L * p.nh));
    const size_t ld = 3 * (size_t)p.d;
    const float* dO = p.dO + ((size_t)b * p.L + i) * p.d + (size_t)hh * p.hd;
    const float* Kb = p.QKV + (size_t)b * p.L * ld + p.d + (size_t)hh * p.hd;
    const float* Vb = Kb + p.d;
    float* Pr = p.P + (((size_t)b * p.nh + hh) * p.L + i) * p.L;
    float dp[4], pr[4], dot = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int j = lane + 64 * c;
        dp[c] = 0.f;
        pr[c] = 0.f;
        if (j < p.L) {
            float a = 0.f;
            for (int e = 0; e < p.hd; ++e) a += dO[e] * Vb[(size_t)j * ld + e];
            pr[c] = Pr[j];
            if (DROP) {
                a = drop_apply(!att_dropped(pr[c]), a, p.drop.scale);
                pr[c] = fabsf(pr[c]);
            }
            dp[c] = a;
            dot += a * pr[c];
        }
    }
    dot = wave_sum(dot);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int j = lane + 64 * c;
        if (j < p.L) {
            const float ds = pr[c] * (dp[c] - dot);
            Pr[j] = ds;
            sp[wv][j] = ds;
        }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    for (int e = lane; e < p.hd; e += 64) {
        float a = 0.f;
        for (int j = 0; j < p.L; ++j) a += sp[wv][j] * Kb[(size_t)j * ld + e];
        p.dQKV[((size_t)b * p.L + i) * ld + (size_t)hh * p.hd + e] = a * p.scale;
    }
}

}  // namespace
}  // namespace m3pc
