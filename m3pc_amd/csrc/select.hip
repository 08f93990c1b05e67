// The cross-candidate tail of a plan step (learner.py:318-325) and the top-k used by the fp32 re-score.
// Everything here is one workgroup: N <= 16384 scores live in registers / LDS, reductions are 64-lane
// shuffles + one LDS hop.
#include <atomic>
#include <stdlib.h>
#include <string.h>

#include "device_util.h"
#include "philox.h"

namespace m3pc {

#ifdef M3PC_LAB
thread_local int g_sel_picked = 0;
thread_local unsigned int g_sel_picked_set = 0;
thread_local bool g_sel_force_fallback = false;
#endif

struct ArgMax {
    float v;
    int i;
};
__device__ __forceinline__ ArgMax better(ArgMax a, ArgMax b) {  // larger value, ties -> lower index
    return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
__device__ __forceinline__ ArgMax block_argmax(ArgMax a, float* sv, int* si) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ArgMax b{__shfl_xor(a.v, o), __shfl_xor(a.i, o)};
        a = better(a, b);
    }
    __syncthreads();
    if (lane == 0) {
        sv[wid] = a.v;
        si[wid] = a.i;
    }
    __syncthreads();
    ArgMax r{sv[0], si[0]};
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = better(r, ArgMax{sv[w], si[w]});
    return r;
}
// p = exp(T (E - max E)) / sum;  eval = sum p a0 / sum p;  argmax E;  sample = argmax p / expo
__device__ __forceinline__ void select_body(const SelectP& p, float* sv, int* si) {
    const int tid = threadIdx.x;
    ArgMax am{-INFINITY, 0x7fffffff};
    for (int i = tid; i < p.n; i += 1024) am = better(am, ArgMax{p.er[i], i});
    am = block_argmax(am, sv, si);
    if (tid == 0 && p.argmax) *p.argmax = am.i;
    const float mx = am.v;
    float s = 0.f;
    for (int i = tid; i < p.n; i += 1024) s += expf(__fmul_rn(__fsub_rn(p.er[i], mx), p.temperature));
    const float tot = block_sum(s, sv);
    float ps = 0.f;
    ArgMax sm{-INFINITY, 0x7fffffff};
    for (int i = tid; i < p.n; i += 1024) {
        const float pi = expf(__fmul_rn(__fsub_rn(p.er[i], mx), p.temperature)) / tot;
        if (p.p) p.p[i] = pi;
        ps += pi;
        if (p.expo) sm = better(sm, ArgMax{pi / p.expo[i], i});
    }
    const float psum = block_sum(ps, sv);
    if (p.expo) {
        sm = block_argmax(sm, sv, si);
        if (tid == 0 && p.sample_idx) *p.sample_idx = sm.i;
        if (p.sample_action && tid < p.A) p.sample_action[tid] = p.a0[(long long)sm.i * p.a0_stride + tid];
    }
    if (p.eval_action) {
        for (int a = 0; a < p.A; ++a) {
            float acc = 0.f;
            for (int i = tid; i < p.n; i += 1024) {
                const float pi = expf(__fmul_rn(__fsub_rn(p.er[i], mx), p.temperature)) / tot;
                acc = fmaf(p.a0[(long long)i * p.a0_stride + a], pi, acc);
            }
            const float t = block_sum(acc, sv);
            if (tid == 0) p.eval_action[a] = t / psum;
        }
    }
}
__global__ __launch_bounds__(1024) void select_kernel(SelectP p) {
    __shared__ float sv[16];
    __shared__ int si[16];
    select_body(p, sv, si);
}
void launch_select(const SelectP& p, hipStream_t st) {
    if (p.n <= 0) return;
    M3PC_SEL_PICK(1);
    hipLaunchKernelGGL(select_kernel, dim3(1), dim3(1024), 0, st, p);
}
// select_kernel for E lock-step windows (the fp32 form of m3pc_plan_steps_certified): workgroup w is window w on its rows of the
// (E, n) arrays -- select_body itself, so a window's results are m3pc_select's on its row bit for bit.
__global__ __launch_bounds__(1024) void select_batch_kernel(SelectP p, long long row_stride, long long a0_wstride) {
    __shared__ float sv[16];
    __shared__ int si[16];
    const long long w = blockIdx.x;
    p.er += w * row_stride;
    if (p.a0) p.a0 += w * a0_wstride;
    if (p.expo) p.expo += w * row_stride;
    if (p.p) p.p += w * row_stride;
    if (p.eval_action) p.eval_action += w * p.A;
    if (p.argmax) p.argmax += w;
    if (p.sample_idx) p.sample_idx += w;
    if (p.sample_action) p.sample_action += w * p.A;
    select_body(p, sv, si);
}
void launch_select_batch(const SelectP& p, int E, long long row_stride, long long a0_wstride, hipStream_t st) {
    if (p.n <= 0 || E <= 0) return;
    M3PC_SEL_PICK(2);
    hipLaunchKernelGGL(select_batch_kernel, dim3((unsigned)E), dim3(1024), 0, st, p, row_stride, a0_wstride);
}

// ---------------------------------------------------------------------------------------------- top-k
// Bitonic sort of 64-bit keys {orderable(value), ~index} in LDS (descending), first k indices out.
__device__ __forceinline__ unsigned int orderable(float f) {
    unsigned int u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;  // -0.0 orders as +0.0 (a tie, decided by the index), as in a float compare
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// The multinomial draw of learner.py:324-325 as a race: torch.multinomial(p, 1) = argmax_j p_j / q_j, q ~ Exp(1), and with
// p = softmax(tau (E - max E)) that is argmax_j (tau E_j - log q_j).  race_key is that key for one candidate; the certified
// re-score compares keys built from bf16 scores with keys built from fp32 re-scores (m3pc_topk_race_window / _merge_race).
__device__ __forceinline__ float race_key(float tau, float e, float q) { return __fsub_rn(__fmul_rn(tau, e), logf(q)); }

// What a top-k ranks and where the winners go: value[e] = v[e], or race_key(tau, v[e], expo[e]) when expo is given; the
// element of rank r (descending; ties to the lower index) is written to out[r * out_stride].
struct TopSrc {
    const float* v;
    const float* expo;
    float tau;
    int k;
    int* out;
    int out_stride;
    float* scores_out;  // optional: v[winner] beside its index, same stride (rank-by-counting kernels only)
};
__device__ __forceinline__ float src_value(const TopSrc& s, int e) { return s.expo ? race_key(s.tau, s.v[e], s.expo[e]) : s.v[e]; }

__device__ __forceinline__ void topk_bitonic_body(const float* v, int n, int npow2, int k, int* idx_out, unsigned long long* keys) {
    const int tid = threadIdx.x;
    for (int i = tid; i < npow2; i += 1024)
        keys[i] = i < n ? ((unsigned long long)orderable(v[i]) << 32) | (unsigned int)(~i) : 0ull;
    __syncthreads();
    for (int size = 2; size <= npow2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (npow2 >> 1); t += 1024) {
                const int lo = 2 * t - (t & (stride - 1));
                const int hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const unsigned long long a = keys[lo], b = keys[hi];
                if ((a < b) == desc) {
                    keys[lo] = b;
                    keys[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < k; i += 1024) idx_out[i] = (int)(~(unsigned int)(keys[i] & 0xffffffffull));
}
__global__ __launch_bounds__(1024) void topk_kernel(const float* v, int n, int npow2, int k, int* idx_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];
    topk_bitonic_body(v, n, npow2, k, idx_out, keys);
}
// one workgroup per row of v (E, n): list blockIdx.x of k indices
__global__ __launch_bounds__(1024) void topk_batch_kernel(const float* v, int n, int npow2, int k, int* idx_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];
    topk_bitonic_body(v + (size_t)blockIdx.x * n, n, npow2, k, idx_out + (size_t)blockIdx.x * k, keys);
}
// k <= 64 of n <= 16384 by selection instead of a full sort: every wave extracts the k best of its own 1/16 of the
// values with k rounds of (register-local arg-max, 64-lane butterfly) -- no barrier --, then wave 0 does the same over
// the 16 k survivors.  Same order as the bitonic kernel (descending value, ties to the lower index); ~3x faster
// at n = 1024 and independent of n up to 16384 (the replicated top-k of an 8-GPU run sorts 8192 scores).
// A winner leaves the race by its INDEX (0x7fffffff: the index `better` never prefers), not only by its value: a real score of
// -inf stays a candidate until it has been taken, and is then taken once -- k > #(scores above -inf) lists distinct elements, in
// index order, as the ranking kernels do.
__device__ __forceinline__ void topk_select_body(const TopSrc& src, int n, float* cv, int* ci) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int k = src.k;
    float val[16];
    int idx[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int e = s * 1024 + tid;
        val[s] = e < n ? src_value(src, e) : -INFINITY;
        idx[s] = e < n ? e : 0x7fffffff;
    }
    for (int r = 0; r < k; ++r) {
        ArgMax a{-INFINITY, 0x7fffffff};
#pragma unroll
        for (int s = 0; s < 16; ++s) a = better(a, ArgMax{val[s], idx[s]});
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a = better(a, ArgMax{__shfl_xor(a.v, o), __shfl_xor(a.i, o)});
        if (lane == 0) {
            cv[wid * k + r] = a.v;
            ci[wid * k + r] = a.i;
        }
#pragma unroll
        for (int s = 0; s < 16; ++s)
            if (idx[s] == a.i) {
                val[s] = -INFINITY;
                idx[s] = 0x7fffffff;
            }
    }
    __syncthreads();
    if (wid != 0) return;
    float mv[16];
    int mi[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int c = j * 64 + lane;
        mv[j] = c < 16 * k ? cv[c] : -INFINITY;
        mi[j] = c < 16 * k ? ci[c] : 0x7fffffff;
    }
    for (int r = 0; r < k; ++r) {
        ArgMax a{-INFINITY, 0x7fffffff};
#pragma unroll
        for (int j = 0; j < 16; ++j) a = better(a, ArgMax{mv[j], mi[j]});
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a = better(a, ArgMax{__shfl_xor(a.v, o), __shfl_xor(a.i, o)});
        if (lane == 0) src.out[r * src.out_stride] = a.i;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (mi[j] == a.i) {
                mv[j] = -INFINITY;
                mi[j] = 0x7fffffff;
            }
    }
}
__global__ __launch_bounds__(1024) void topk_select_kernel(TopSrc src, int n) {
    __shared__ float cv[16 * 64];
    __shared__ int ci[16 * 64];
    topk_select_body(src, n, cv, ci);
}
// one workgroup per row of src.v (E, n): list blockIdx.x of src.k entries (out_stride 1)
__global__ __launch_bounds__(1024) void topk_select_batch_kernel(TopSrc src, int n) {
    __shared__ float cv[16 * 64];
    __shared__ int ci[16 * 64];
    src.v += (size_t)blockIdx.x * n;
    src.out += (size_t)blockIdx.x * src.k;
    topk_select_body(src, n, cv, ci);
}

// n <= 2048: rank by counting.  Every element's 64-bit key {orderable(value), ~index} (the bitonic kernel's, so the order
// is the same: descending value, ties to the lower index) is compared with all n keys, read as LDS broadcasts; keys are
// distinct, so rank = #(greater keys) is a permutation and the elements of rank < k write themselves out.  No shuffle
// chains, no rounds: ~5 us at n = 1024 where the k-round selection below takes 33 (16 rounds x 12 dependent shuffles,
// twice).
// Many-block form of the same ranking (n <= 2048): 256 threads per block, thread t of block b ranks element 64 b + (t & 63)
// against a quarter of the keys (t >> 6), the four partial ranks meet in LDS.  16 blocks at n = 1024 instead of one:
// the n^2 / 2 key comparisons spread over 16 CUs (20 us -> a few).
__device__ __forceinline__ void topk_rank_blocks_body(const float* v, int n, int k, int* idx_out, unsigned long long* keys, int (*part)[64]) {
    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
    for (int e = tid; e < 2048; e += 256) keys[e] = e < n ? ((unsigned long long)orderable(v[e]) << 32) | (unsigned int)(~e) : 0ull;
    __syncthreads();
    const int e = blockIdx.x * 64 + lane;
    const unsigned long long mine = e < n ? keys[e] : 0ull;
    const int n4 = (((n + 3) / 4) + 1) & ~1;  // keys per quarter, even (keys past n are 0: never greater than a real key)
    int rank = 0;
    const int j0 = q * n4, j1 = j0 + n4 < 2048 ? j0 + n4 : 2048;
#pragma unroll 8
    for (int j = j0; j < j1; j += 2) {
        const u64x2 kj = *(const u64x2*)&keys[j];
        rank += (kj.x > mine) + (kj.y > mine);
    }
    part[q][lane] = rank;
    __syncthreads();
    if (q == 0 && e < n) {
        rank = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
        if (rank < k) idx_out[rank] = e;
    }
}
__global__ __launch_bounds__(256) void topk_rank_blocks_kernel(const float* v, int n, int k, int* idx_out) {
    __shared__ __attribute__((aligned(16))) unsigned long long keys[2048];
    __shared__ int part[4][64];
    topk_rank_blocks_body(v, n, k, idx_out, keys, part);
}
// the same ranking of row blockIdx.y of v (E, n) into list blockIdx.y
__global__ __launch_bounds__(256) void topk_rank_blocks_batch_kernel(const float* v, int n, int k, int* idx_out) {
    __shared__ __attribute__((aligned(16))) unsigned long long keys[2048];
    __shared__ int part[4][64];
    topk_rank_blocks_body(v + (size_t)blockIdx.y * n, n, k, idx_out + (size_t)blockIdx.y * k, keys, part);
}

// Two rankings in one launch (n <= 2048): blockIdx.y picks the source -- the scores themselves / the race keys.
__global__ __launch_bounds__(256) void topk_rank_blocks2_kernel(TopSrc s0, TopSrc s1, int n) {
    __shared__ __attribute__((aligned(16))) unsigned long long keys[2048];
    __shared__ int part[4][64];
    const TopSrc s = blockIdx.y ? s1 : s0;
    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
    for (int e = tid; e < 2048; e += 256) keys[e] = e < n ? ((unsigned long long)orderable(src_value(s, e)) << 32) | (unsigned int)(~e) : 0ull;
    __syncthreads();
    const int e = blockIdx.x * 64 + lane;
    const unsigned long long mine = e < n ? keys[e] : 0ull;
    const int n4 = (((n + 3) / 4) + 1) & ~1;
    int rank = 0;
    const int j0 = q * n4, j1 = j0 + n4 < 2048 ? j0 + n4 : 2048;
#pragma unroll 8
    for (int j = j0; j < j1; j += 2) {
        const u64x2 kj = *(const u64x2*)&keys[j];
        rank += (kj.x > mine) + (kj.y > mine);
    }
    part[q][lane] = rank;
    __syncthreads();
    if (q == 0 && e < n) {
        rank = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
        if (rank < s.k) {
            s.out[rank * s.out_stride] = e;
            if (s.scores_out) s.scores_out[rank * s.out_stride] = s.v[e];
        }
    }
}

// The same two rankings for 2048 < n <= 16384 (config 3's 4096 candidates, the gathered scores of a candidate-sharded config 4):
// the keys of ALL n elements in dynamic LDS (8 n bytes: 32 KB at 4096, 128 KB at 16384), 64 elements per block ranked by 256
// threads, a quarter of the keys each.  One launch of ~10-20 us where the selection kernel needs k rounds of butterflies in a
// single workgroup (~60 us for the 32 racers) and the 129 best by score a whole bitonic sort.
__device__ __forceinline__ void rank_blocks_dyn_body(const TopSrc& s, int n, int n4, unsigned long long* dkeys, int (*part)[64]) {
    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
    for (int e = tid; e < 4 * n4; e += 256) dkeys[e] = e < n ? ((unsigned long long)orderable(src_value(s, e)) << 32) | (unsigned int)(~e) : 0ull;
    __syncthreads();
    const int e = blockIdx.x * 64 + lane;
    const unsigned long long mine = e < n ? dkeys[e] : 0ull;
    int rank = 0;
    const int j0 = q * n4, j1 = j0 + n4;
#pragma unroll 8
    for (int j = j0; j < j1; j += 2) {
        const u64x2 kj = *(const u64x2*)&dkeys[j];
        rank += (kj.x > mine) + (kj.y > mine);
    }
    part[q][lane] = rank;
    __syncthreads();
    if (q == 0 && e < n) {
        rank = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
        if (rank < s.k) {
            s.out[rank * s.out_stride] = e;
            if (s.scores_out) s.scores_out[rank * s.out_stride] = s.v[e];
        }
    }
}
__global__ __launch_bounds__(256) void topk_rank_blocks2_dyn_kernel(TopSrc s0, TopSrc s1, int n, int n4) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long dkeys[];  // 4 * n4 entries
    __shared__ int part[4][64];
    const TopSrc s = blockIdx.y ? s1 : s0;
    rank_blocks_dyn_body(s, n, n4, dkeys, part);
}
// The two rankings of E windows in one launch (the lock-step batch): blockIdx.z picks the window -- row z of v / expo, list z of
// out / scores_out --, everything else is the kernel above, for every n <= 16384 (keys in dynamic LDS on both sides of 2048: the
// rank of an element is a count of integer key comparisons, so the lists are those of topk_rank_blocks2_kernel too).
__global__ __launch_bounds__(256) void topk_rank_batch_kernel(TopSrc s0, TopSrc s1, int n, int n4, long long v_stride, int list_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long dkeys[];  // 4 * n4 entries
    __shared__ int part[4][64];
    TopSrc s = blockIdx.y ? s1 : s0;
    const long long w = blockIdx.z;
    s.v += w * v_stride;
    if (s.expo) s.expo += w * v_stride;
    s.out += w * list_stride;
    if (s.scores_out) s.scores_out += w * list_stride;
    rank_blocks_dyn_body(s, n, n4, dkeys, part);
}

__global__ __launch_bounds__(1024) void topk_rank_kernel(const float* v, int n, int k, int* idx_out) {
    __shared__ __attribute__((aligned(16))) unsigned long long keys[2048];
    const int tid = threadIdx.x;
    unsigned long long mine[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int e = s * 1024 + tid;
        mine[s] = e < n ? ((unsigned long long)orderable(v[e]) << 32) | (unsigned int)(~e) : 0ull;
        keys[e] = mine[s];
    }
    __syncthreads();
    const int n2 = (n + 1) & ~1;  // (keys past n are 0: never greater than a real key)
    int rank0 = 0, rank1 = 0;
    if (n <= 1024) {
#pragma unroll 8
        for (int j = 0; j < n2; j += 2) {
            const u64x2 kj = *(const u64x2*)&keys[j];
            rank0 += (kj.x > mine[0]) + (kj.y > mine[0]);
        }
    } else {
#pragma unroll 4
        for (int j = 0; j < n2; j += 2) {
            const u64x2 kj = *(const u64x2*)&keys[j];
            rank0 += (kj.x > mine[0]) + (kj.y > mine[0]);
            rank1 += (kj.x > mine[1]) + (kj.y > mine[1]);
        }
    }
    if (tid < n && rank0 < k) idx_out[rank0] = tid;
    if (1024 + tid < n && rank1 < k) idx_out[rank1] = 1024 + tid;
}

void launch_topk(const float* v, int n, int k, int* idx_out, hipStream_t st) {
    if (n <= 0 || k <= 0) return;
    if (n <= 2048 && k <= n) {
        static const bool one_block = M3PC_ENV("M3PC_TOPK_ONE_BLOCK") != nullptr;  // A/B switch
        M3PC_SEL_PICK(one_block ? 12 : 7);
        if (one_block) hipLaunchKernelGGL(topk_rank_kernel, dim3(1), dim3(1024), 0, st, v, n, k, idx_out);
        else hipLaunchKernelGGL(topk_rank_blocks_kernel, dim3((n + 63) / 64), dim3(256), 0, st, v, n, k, idx_out);
        return;
    }
    if (k <= 64 && n <= 16384) {
        M3PC_SEL_PICK(5);
        hipLaunchKernelGGL(topk_select_kernel, dim3(1), dim3(1024), 0, st, TopSrc{v, nullptr, 0.f, k, idx_out, 1, nullptr}, n);
        return;
    }
    int np = 2;
    while (np < n) np <<= 1;
    static bool attr[64] = {};  // (a per-device opt-in)
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev >= 0 && dev < 64 && !attr[dev]) {
        (void)hipFuncSetAttribute((const void*)topk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 16384 * 8);
        attr[dev] = true;
    }
    M3PC_SEL_PICK(3);
    hipLaunchKernelGGL(topk_kernel, dim3(1), dim3(1024), (size_t)np * 8, st, v, n, np, k, idx_out);
}

#ifdef M3PC_LAB
void launch_topk_forced(int variant, const float* v, const float* expo, float tau, int n, int k, int* out, int out_stride, hipStream_t st) {
    if (variant == 1) {
        M3PC_SEL_PICK(12);
        hipLaunchKernelGGL(topk_rank_kernel, dim3(1), dim3(1024), 0, st, v, n, k, out);
    } else if (variant == 2) {
        M3PC_SEL_PICK(7);
        hipLaunchKernelGGL(topk_rank_blocks_kernel, dim3((n + 63) / 64), dim3(256), 0, st, v, n, k, out);
    } else if (variant == 3) {
        M3PC_SEL_PICK(5);
        hipLaunchKernelGGL(topk_select_kernel, dim3(1), dim3(1024), 0, st, TopSrc{v, expo, tau, k, out, out_stride, nullptr}, n);
    } else if (variant == 4) {
        int np = 2;
        while (np < n) np <<= 1;
        (void)hipFuncSetAttribute((const void*)topk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 16384 * 8);
        M3PC_SEL_PICK(3);
        hipLaunchKernelGGL(topk_kernel, dim3(1), dim3(1024), (size_t)np * 8, st, v, n, np, k, out);
    }
}
#endif

// launch_topk for E rows at once (m3pc_refine_plans): the same three regimes with the row as a grid index, so list w is
// launch_topk's of row w (the keys are integers: the order does not depend on who compares them).  No environment switch.
void launch_topk_batch(const float* v, int E, int n, int k, int* idx_out, hipStream_t st) {
    if (E <= 0 || n <= 0 || k <= 0) return;
    if (n <= 2048 && k <= n) {
        M3PC_SEL_PICK(8);
        for (int w0 = 0; w0 < E; w0 += 32768)
            hipLaunchKernelGGL(topk_rank_blocks_batch_kernel, dim3((n + 63) / 64, E - w0 < 32768 ? E - w0 : 32768), dim3(256), 0, st,
                               v + (size_t)w0 * n, n, k, idx_out + (size_t)w0 * k);
        return;
    }
    if (k <= 64 && n <= 16384) {
        M3PC_SEL_PICK(6);
        hipLaunchKernelGGL(topk_select_batch_kernel, dim3(E), dim3(1024), 0, st, TopSrc{v, nullptr, 0.f, k, idx_out, 1, nullptr}, n);
        return;
    }
    int np = 2;
    while (np < n) np <<= 1;
    static bool attr[64] = {};  // (a per-device opt-in)
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev >= 0 && dev < 64 && !attr[dev]) {
        (void)hipFuncSetAttribute((const void*)topk_batch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 16384 * 8);
        attr[dev] = true;
    }
    M3PC_SEL_PICK(4);
    hipLaunchKernelGGL(topk_batch_kernel, dim3(E), dim3(1024), (size_t)np * 8, st, v, n, np, k, idx_out);
}

// > 64 KiB of dynamic LDS for a ranking kernel: state[device] = 0: not asked, 1: granted, 2: refused
static bool rank_lds_fits(const void* kernel, std::atomic<int>* state, size_t lds) {
    if (lds <= 64 * 1024) return true;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    int stt = state[dev].load(std::memory_order_acquire);
    if (stt == 0) {
        stt = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 132 * 1024) == hipSuccess ? 1 : 2;
        if (stt == 2) (void)hipGetLastError();
        state[dev].store(stt, std::memory_order_release);
    }
    return stt == 1;
}

// The two candidate lists of the certified re-score in one buffer (m3pc_topk_race_window): list[rmax + i] = the i-th best
// entry of v (i <= kk - 1), list[rmax - 1 - i] = the i-th best entry by race key (i < rr): the r best racers and the n best
// scorers are the contiguous slice [rmax - r, rmax + n).
bool launch_topk_race(const float* v, const float* expo, float tau, int n, int kk, int rr, int rmax, int* list, float* list_scores,
                      hipStream_t st) {
    if (n <= 0 || kk <= 0) return true;
    const bool one = n <= 16384;  // rank by counting: every element knows its value and its rank -- the scores go out with the ids
    const TopSrc s0{v, nullptr, 0.f, kk, list + rmax, 1, one && list_scores ? list_scores + rmax : nullptr};
    const TopSrc s1{v, expo, tau, rr, list + rmax - 1, -1, one && list_scores ? list_scores + rmax - 1 : nullptr};
    if (n <= 2048 && !M3PC_SEL_FORCE_FALLBACK) {
        M3PC_SEL_PICK(9);
        hipLaunchKernelGGL(topk_rank_blocks2_kernel, dim3((n + 63) / 64, rr > 0 ? 2 : 1), dim3(256), 0, st, s0, s1, n);
        return true;  // (list_scores written)
    }
    if (one && !M3PC_SEL_FORCE_FALLBACK) {  // n <= 16384: the keys in dynamic LDS
        const int n4 = (((n + 3) / 4) + 1) & ~1;
        const size_t lds = (size_t)4 * n4 * sizeof(unsigned long long);
        // > 64 KiB of dynamic LDS is a per-device opt-in, asked for ONCE per device and only when the launch needs it (n > 8192);
        // a refusal is remembered and its error cleared, so that the fallback below is not reported as a failed launch by the
        // caller's hipGetLastError (the same pattern as lds_opt_in in attn_bf16.hip)
        static std::atomic<int> state[64] = {};
        const bool fits = rank_lds_fits((const void*)topk_rank_blocks2_dyn_kernel, state, lds);
        if (fits) {
            M3PC_SEL_PICK(10);
            hipLaunchKernelGGL(topk_rank_blocks2_dyn_kernel, dim3((n + 63) / 64, rr > 0 ? 2 : 1), dim3(256), lds, st, s0, s1, n, n4);
            return true;
        }
    }
    // (the opt-in was refused: the selection kernels, no scores)
    const TopSrc t1{v, expo, tau, rr, list + rmax - 1, -1, nullptr};
    launch_topk(v, n, kk, list + rmax, st);
    if (rr > 0) {
        M3PC_SEL_PICK(5);
        hipLaunchKernelGGL(topk_select_kernel, dim3(1), dim3(1024), 0, st, t1, n);  // (rr <= 64, n <= 16384)
    }
    return false;     // (the caller still has to gather list_scores: launch_window_stats)
}

// launch_topk_race for E windows in one launch (n <= 16384): window w ranks row w of v / expo (row stride v_stride) into list w
// (list_stride >= rmax + kk entries; list_scores in the same layout).  false: the device refused the LDS the keys of n > 8192
// candidates need -- nothing is launched, the caller reports it.
bool launch_topk_race_batch(const float* v, const float* expo, float tau, int E, int n, long long v_stride, int kk, int rr, int rmax,
                            int* list, float* list_scores, int list_stride, hipStream_t st) {
    if (E <= 0 || n <= 0 || kk <= 0) return true;
    if (n > 16384) return false;
    const TopSrc s0{v, nullptr, 0.f, kk, list + rmax, 1, list_scores ? list_scores + rmax : nullptr};
    const TopSrc s1{v, expo, tau, rr, list + rmax - 1, -1, list_scores ? list_scores + rmax - 1 : nullptr};
    const int n4 = (((n + 3) / 4) + 1) & ~1;
    const size_t lds = (size_t)4 * n4 * sizeof(unsigned long long);
    static std::atomic<int> state[64] = {};
    if (!rank_lds_fits((const void*)topk_rank_batch_kernel, state, lds)) return false;
    M3PC_SEL_PICK(11);
    hipLaunchKernelGGL(topk_rank_batch_kernel, dim3((n + 63) / 64, rr > 0 ? 2 : 1, E), dim3(256), lds, st, s0, s1, n, n4, v_stride,
                       list_stride);
    return true;
}

// idx: the kk best entries of v, best first.  n = clamp(#{i < kk: v[idx[i]] >= v[idx[0]] - window}, kmin, kmax) and the
// distance from the best entry to the best one NOT among those n (infinity when there is none).
// Window statistics of the bound-driven re-score: idx = the kk best entries of v (best first).  The raw count of entries
// within `window` of the maximum runs over the WHOLE vector (n_total), so a caller sees when the window holds more than the
// kmax entries it may list (stats[3] > kmax: the listed prefix no longer covers the window).
__global__ __launch_bounds__(256) void window_stats_kernel(const float* v, int n_total, const int* idx, int kk, int kmin, int kmax,
                                                           float window, float* stats, float* host_stats, float seq,
                                                           float* top_scores, int rr) {
    __shared__ int part[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float mx = v[idx[0]];
    int cnt = 0;
    for (int i = tid; i < n_total; i += 256) cnt += v[i] >= mx - window ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) part[wid] = cnt;
    if (top_scores)
        for (int i = tid - rr; i < kk; i += 256) top_scores[i] = v[idx[i]];  // (entries -rr .. -1: the race list in front of idx)
    __syncthreads();
    cnt = part[0] + part[1] + part[2] + part[3];
    int n = cnt < kmin ? kmin : cnt;
    if (n > kmax) n = kmax;
    if (n > kk) n = kk;
    if (tid == 0) {
        const float margin = n < kk ? mx - v[idx[n]] : INFINITY;
        stats[0] = (float)n;
        stats[1] = margin;
        stats[2] = mx;
        stats[3] = (float)cnt;
        if (host_stats) {  // host-mapped (pinned) copy the caller spins on: payload first, then the sequence number
            host_stats[0] = (float)n;
            host_stats[1] = margin;
            host_stats[2] = mx;
            host_stats[3] = (float)cnt;
            __threadfence_system();
            __hip_atomic_store(host_stats + 4, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
void launch_window_stats(const float* v, int n_total, const int* idx, int kk, int kmin, int kmax, float window, float* stats,
                         float* host_stats, float seq, float* top_scores, hipStream_t st, int rr) {
    M3PC_SEL_PICK(13);
    hipLaunchKernelGGL(window_stats_kernel, dim3(1), dim3(256), 0, st, v, n_total, idx, kk, kmin, kmax, window, stats, host_stats, seq,
                       top_scores, rr);
}

// Merge of a bf16 score vector with the fp32 re-scores of the listed candidates (planner: certified re-score).  The list holds
// r race entries (the r best by race key, any order) followed by n score entries (the n best by bf16 score, best first); m = r + n.
//   d_i = b[list[i]] - f[i] over the m listed entries;  c = lower median(d): the common shift of the bf16 scores;
//   out[j] = b[j] - c for every j, then out[list[i]] = f[i] (score entries first, race entries behind them: deterministic when a
//   candidate sits in both parts).
// Arg-max certificate: with |(b_j - f_j) - c| <= delta for every candidate, an un-listed j can only beat the best listed fp32 score
// f* if b_j - c > f* - delta.  need = #{j : b[j] > f* + c - delta} over the WHOLE vector (the score entries are the n largest b, so
// this set is a prefix of the descending order): need <= n certifies that the arg-max of `out` is the fp32 arg-max; otherwise the
// entries n .. need-1 of the order still have to be re-scored.
// Race certificate (expo given): K* = max over the listed entries of race_key(tau, f_i, q_i) is a key the multinomial's winner at
// least reaches; an un-listed j can only win if tau (b_j - c + delta) - log q_j >= K*, i.e. race_key(tau, b_j, q_j) >= K* +
// tau (c - delta).  need_race = the number of such j over the WHOLE vector -- a prefix of the descending race-key order -- so
// need_race <= r certifies that arg-max_j p_j / q_j over `out` is the fp32 draw; otherwise the race entries r .. need_race-1
// still have to be re-scored.
//   stats = {c, max_i |d_i - c|, need, (f* + c - delta) - (largest un-listed b) [inf when everything is listed], -, need_race,
//            K*, K* + tau (c - delta)}   (slot 4 of the host copy carries the sequence number)
__device__ __forceinline__ void rescore_merge_body(const float* b, int n_total, const int* list, int r, int n, const float* list_scores, const float* f, float delta, const float* expo, float tau, float* out, float* stats, float* host_stats, float seq, int nstats) {
    __shared__ float d[1024];
    __shared__ int ids[1024];
    __shared__ float c_sh;
    __shared__ float sv[16], sf[16], sb[16], sk[16];
    __shared__ int sc[16], sr[16];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int m = r + n;
    float kf = -INFINITY;
    if (tid < m) {
        d[tid] = list_scores[tid] - f[tid];
        ids[tid] = list[tid];
        if (expo) kf = race_key(tau, f[tid], expo[ids[tid]]);
    }
    __syncthreads();
    if (tid < m) {
        const float me = d[tid];
        int rank = 0;
        for (int j = 0; j < m; ++j) {
            const float o = d[j];
            rank += (o < me || (o == me && j < tid)) ? 1 : 0;
        }
        if (rank == (m - 1) / 2) c_sh = me;
    }
    __syncthreads();
    const float c = c_sh;
    float dev = tid < m ? fabsf(d[tid] - c) : 0.f;
    float fb = tid < m ? f[tid] : -INFINITY;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        dev = fmaxf(dev, __shfl_xor(dev, o));
        fb = fmaxf(fb, __shfl_xor(fb, o));
        kf = fmaxf(kf, __shfl_xor(kf, o));
    }
    if (lane == 0) {
        sv[wid] = dev;
        sf[wid] = fb;
        sk[wid] = kf;
    }
    __syncthreads();
    float fbest = sf[0], devmax = sv[0], kbest = sk[0];
    for (int w = 1; w < 16; ++w) {
        fbest = fmaxf(fbest, sf[w]);
        devmax = fmaxf(devmax, sv[w]);
        kbest = fmaxf(kbest, sk[w]);
    }
    const float thr = fbest + c - delta;            // on the bf16 scale
    const float thr_r = kbest + tau * (c - delta);  // on the bf16 race-key scale
    int cnt = 0, cnt_r = 0;
    float bout = -INFINITY;  // largest b among the un-listed: everything below the n-th largest b (the score entries are a prefix)
    const float b_last = list_scores[m - 1];
    for (int j = tid; j < n_total; j += 1024) {
        const float v = b[j];
        out[j] = v - c;
        cnt += v > thr ? 1 : 0;
        if (v < b_last) bout = fmaxf(bout, v);
        if (expo) cnt_r += race_key(tau, v, expo[j]) >= thr_r ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
        cnt_r += __shfl_xor(cnt_r, o);
        bout = fmaxf(bout, __shfl_xor(bout, o));
    }
    if (lane == 0) {
        sc[wid] = cnt;
        sr[wid] = cnt_r;
        sb[wid] = bout;
    }
    __syncthreads();
    if (tid >= r && tid < m) out[ids[tid]] = f[tid];
    __syncthreads();
    if (tid < r) out[ids[tid]] = f[tid];
    if (tid == 0) {
        int need = 0, need_r = 0;
        float bo = -INFINITY;
        for (int w = 0; w < 16; ++w) {
            need += sc[w];
            need_r += sr[w];
            bo = fmaxf(bo, sb[w]);
        }
        // (ties with the n-th listed score count as listed above: a tie at the list's edge keeps `need` honest through cnt)
        const float margin = n >= n_total ? INFINITY : thr - bo;
        const float st8[8] = {c, devmax, (float)need, margin, 0.f, (float)need_r, kbest, thr_r};
        for (int i = 0; i < nstats; ++i) stats[i] = st8[i];
        if (host_stats) {
            // all 8 host slots on every merge: a four-statistics merge (no race list) leaves zeros at 5..7 instead of the
            // previous race merge's need_race / K* / threshold on the same slot
            for (int i = 0; i < 8; ++i)
                if (i != 4) host_stats[i] = i < nstats ? st8[i] : 0.f;
            __threadfence_system();
            __hip_atomic_store(host_stats + 4, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
__global__ __launch_bounds__(1024) void rescore_merge_kernel(const float* b, int n_total, const int* list, int r, int n, const float* list_scores, const float* f, float delta, const float* expo, float tau, float* out, float* stats, float* host_stats, float seq, int nstats) {
    rescore_merge_body(b, n_total, list, r, n, list_scores, f, delta, expo, tau, out, stats, host_stats, seq, nstats);
}
// merge + select in one launch (both are one workgroup over the whole vector): the select reads the merged vector the
// workgroup itself has just written (workgroup-scope visibility behind __syncthreads)
__global__ __launch_bounds__(1024) void merge_select_kernel(const float* b, int n_total, const int* list, int r, int n, const float* list_scores, const float* f, float delta, const float* expo, float tau, float* out, float* stats, float* host_stats, float seq, int nstats, SelectP sp) {
    __shared__ float sv[16];
    __shared__ int si[16];
    rescore_merge_body(b, n_total, list, r, n, list_scores, f, delta, expo, tau, out, stats, host_stats, seq, nstats);
    __syncthreads();
    select_body(sp, sv, si);
}
void launch_rescore_merge(const float* b, int n_total, const int* list, int r, int n, const float* list_scores, const float* f,
                          float delta, const float* expo, float tau, float* out, float* stats, float* host_stats, float seq,
                          hipStream_t st) {
    M3PC_SEL_PICK(14);
    hipLaunchKernelGGL(rescore_merge_kernel, dim3(1), dim3(1024), 0, st, b, n_total, list, r, n, list_scores, f, delta, expo, tau, out,
                       stats, host_stats, seq, expo ? 8 : 4);
}
void launch_merge_select(const float* b, int n_total, const int* list, int r, int n, const float* list_scores, const float* f,
                         float delta, const float* expo, float tau, float* out, float* stats, float* host_stats, float seq,
                         const SelectP& sp, hipStream_t st) {
    M3PC_SEL_PICK(15);
    hipLaunchKernelGGL(merge_select_kernel, dim3(1), dim3(1024), 0, st, b, n_total, list, r, n, list_scores, f, delta, expo, tau, out,
                       stats, host_stats, seq, expo ? 8 : 4, sp);
}

// launch_merge_select (or, without `select`, launch_rescore_merge) for up to 64 windows in one launch: workgroup i is window
// w0 + i with its own r / n / delta, its rows of the (E, n_total) arrays, the slice [rmax - r, rmax + n) of its list and its block of
// 8 statistics -- the bodies are those of the one-window kernels, so the results are theirs bit for bit.
__global__ __launch_bounds__(1024) void merge_select_batch_kernel(MergeSelectBatchP P) {
    __shared__ float sv[16];
    __shared__ int si[16];
    const int i = blockIdx.x;
    const long long w = P.w0 + i;
    const int r = P.r[i], n = P.n[i];
    const long long row = w * P.row_stride, lo = w * P.list_stride + P.rmax - r;
    const float* expo = P.expo ? P.expo + row : nullptr;
    float* out = P.out + row;
    rescore_merge_body(P.b + row, P.n_total, P.list + lo, r, n, P.list_scores + lo, P.f + w * P.f_stride + (P.rmax - r - P.f_lo), P.delta[i],
                       P.race ? expo : nullptr, P.tau, out, P.stats + 8 * w, P.host_stats ? P.host_stats + 8 * w : nullptr, P.seq,
                       P.race ? 8 : 4);
    if (!P.select) return;
    __syncthreads();
    SelectP sp;
    sp.er = out;
    sp.a0 = P.a0 ? P.a0 + w * P.a0_wstride : nullptr;
    sp.a0_stride = P.a0_stride;
    sp.n = P.n_total;
    sp.A = P.A;
    sp.temperature = P.tau;
    sp.expo = expo;
    sp.p = P.p ? P.p + row : nullptr;
    sp.eval_action = P.eval_action ? P.eval_action + w * P.A : nullptr;
    sp.argmax = P.argmax ? P.argmax + w : nullptr;
    sp.sample_idx = P.sample_idx ? P.sample_idx + w : nullptr;
    sp.sample_action = P.sample_action ? P.sample_action + w * P.A : nullptr;
    select_body(sp, sv, si);
}
void launch_merge_select_batch(MergeSelectBatchP& P, int E, const int* r, const int* n, const float* delta, hipStream_t st) {
    for (int w0 = 0; w0 < E; w0 += 64) {  // (per-window scalars travel in the kernel arguments: 64 windows per launch)
        const int e = E - w0 < 64 ? E - w0 : 64;
        P.w0 = w0;
        for (int i = 0; i < e; ++i) {
            P.r[i] = r[w0 + i];
            P.n[i] = n[w0 + i];
            P.delta[i] = delta[w0 + i];
        }
        M3PC_SEL_PICK(16);
        hipLaunchKernelGGL(merge_select_batch_kernel, dim3(e), dim3(1024), 0, st, P);
    }
}

// Calibration statistics of the certified re-score (m3pc_calibrate_delta): d_i = b_i - f_i over ALL n <= 16384 candidates (b: the
// low-precision scores, f: their fp32 values), c = the lower median of d -- the element of rank (n - 1) / 2 of the ascending
// order (value, then index: what torch.median returns) --, then max_i |d_i - c| and max_i |f_i|.  One workgroup: every thread
// keeps up to 16 elements in registers and ranks them by counting against all n, which pass through LDS in tiles of 2048
// (broadcast reads, as in topk_rank_kernel; n^2 compares: ~0.3 ms at 16384, beside the ~10 ms fp32 pass that made f).
//   stats (device, 8 floats) = {c, max |d - c|, max |f|, 0, -, 0, 0, 0}; host_stats: the same, payload first, then `seq` into slot 4
//   with system scope (rescore_merge_body's protocol).
__global__ __launch_bounds__(1024) void deviation_stats_kernel(const float* b, const float* f, int n, float* stats, float* host_stats,
                                                               float seq) {
    __shared__ float tile[2048];
    __shared__ float c_sh;
    __shared__ float sv[16], sf[16];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ns = (n + 1023) >> 10;  // elements per thread (uniform)
    float v[16];
    int rank[16];
    float fmx = 0.f;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int e = s * 1024 + tid;
        rank[s] = 0;
        v[s] = 0.f;
        if (e < n) {
            const float fe = f[e];
            v[s] = __fsub_rn(b[e], fe);
            fmx = fmaxf(fmx, fabsf(fe));
        }
    }
    for (int base = 0; base < n; base += 2048) {
        __syncthreads();
        for (int j = tid; j < 2048; j += 1024) {
            const int e = base + j;
            tile[j] = e < n ? __fsub_rn(b[e], f[e]) : 0.f;
        }
        __syncthreads();
        const int m = n - base < 2048 ? n - base : 2048;
        for (int j = 0; j < m; ++j) {
            const float o = tile[j];
            const int je = base + j;
#pragma unroll
            for (int s = 0; s < 16; ++s)
                if (s < ns) rank[s] += (o < v[s] || (o == v[s] && je < s * 1024 + tid)) ? 1 : 0;
        }
    }
    const int mid = (n - 1) / 2;
#pragma unroll
    for (int s = 0; s < 16; ++s)
        if (s * 1024 + tid < n && rank[s] == mid) c_sh = v[s];  // (ranks are a permutation: exactly one writer)
    __syncthreads();
    const float c = c_sh;
    float dev = 0.f;
#pragma unroll
    for (int s = 0; s < 16; ++s)
        if (s * 1024 + tid < n) dev = fmaxf(dev, fabsf(__fsub_rn(v[s], c)));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        dev = fmaxf(dev, __shfl_xor(dev, o));
        fmx = fmaxf(fmx, __shfl_xor(fmx, o));
    }
    if (lane == 0) {
        sv[wid] = dev;
        sf[wid] = fmx;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w) {
            dev = fmaxf(dev, sv[w]);
            fmx = fmaxf(fmx, sf[w]);
        }
        const float st8[8] = {c, dev, fmx, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < 8; ++i) stats[i] = st8[i];
        if (host_stats) {
            for (int i = 0; i < 8; ++i)
                if (i != 4) host_stats[i] = st8[i];
            __threadfence_system();
            __hip_atomic_store(host_stats + 4, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
void launch_deviation_stats(const float* b, const float* f, int n, float* stats, float* host_stats, float seq, hipStream_t st) {
    if (n <= 0 || n > 16384) return;
    M3PC_SEL_PICK(17);
    hipLaunchKernelGGL(deviation_stats_kernel, dim3(1), dim3(1024), 0, st, b, f, n, stats, host_stats, seq);
}

// ---- the eval_action certificate (m3pc_eval_bound; include/m3pc_hip.h states the bound and its claim).  One workgroup over the
// merged vector the select ran on.  p and e are recomputed with select_body's own expressions (same order, so e is its eval_action
// bit for bit); every candidate's membership lives in LDS as 16 bits: not listed / re-scored / the list position of a listed score
// entry that is not re-scored.  Thread t of [n, n_listed) stands for "the score entries up to t re-scored": U is then the un-listed
// candidates (a block_sum over the vector) plus the listed entries t .. n_listed-1 (an inclusive SUFFIX sum over the threads -- sums
// of non-negative terms only, no cancellation where the list holds nearly all the weight), so all bound(n') come out of one scan
// per action component.  Fixed-order reductions: bit-identical from run to run.
// v[t] -> sum_{u >= t} v[u] over the 1024 threads (64-lane shuffles + one LDS hop, fixed order)
__device__ __forceinline__ float block_suffix_sum(float v, float* sv) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float u = __shfl_down(v, o);
        if (lane + o < 64) v += u;
    }
    __syncthreads();
    if (lane == 0) sv[wid] = v;
    __syncthreads();
    float behind = 0.f;
    for (int w = (int)(blockDim.x >> 6) - 1; w > wid; --w) behind += sv[w];
    return v + behind;
}
// v[t] -> sum_{u < t} v[u], the same way from the other end
__device__ __forceinline__ float block_prefix_sum(float v, float* sv) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    __syncthreads();
    if (lane == 63) sv[wid] = v;
    __syncthreads();
    float before = 0.f;
    for (int w = 0; w < wid; ++w) before += sv[w];
    const float ex = __shfl_up(v, 1);
    return (lane ? ex : 0.f) + before;
}
// expm1(eps) S / (1 - (1 - exp(-eps)) P_U) with the denominator as P_L + exp(-eps) P_U (P_L + P_U = 1: sums of non-negative terms,
// where 1 - (1 - exp(-eps)) P_U cancels at a large eps); S, P_L, P_U already divided by the select's sum of p; exactly 0 where S is
__device__ __forceinline__ float eval_bound_of(float em1, float emeps, float S, float PL, float PU) {
    return S > 0.f ? em1 * S / (PL + emeps * PU) : 0.f;
}
// (pos: 16384 entries, sv / si: 16, at_n: 2 floats, at_n_k: one int -- the LDS of the kernel that calls it, so that the one-window
// and the batched kernel run the same expressions in the same order)
__device__ __forceinline__ void eval_bound_body(const float* m, int n_total, const int* list, int r, int n, int n_listed, const float* a0,
                                                long long a0_stride, int A, float tau, float delta, float eval_tol, float* stats,
                                                float* host_stats, float seq, unsigned short* pos, float* sv, int* si, float* at_n,
                                                int* at_n_k_p) {
    int& at_n_k = *at_n_k_p;
    constexpr unsigned short UNLISTED = 0xffffu, RESCORED = 0xfffeu;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (int j = tid; j < n_total; j += 1024) pos[j] = UNLISTED;
    __syncthreads();
    int my_id = -1;  // the listed, not re-scored score entry this thread stands for
    if (tid >= n && tid < n_listed) {
        const int id = list[r + tid];
        if ((unsigned int)id < (unsigned int)n_total) {
            my_id = id;
            pos[id] = (unsigned short)tid;
        }
    }
    __syncthreads();
    if (tid < r + n) {  // (a candidate that sits in both parts, or twice, gets the same mark from every writer)
        const int id = list[tid];
        if ((unsigned int)id < (unsigned int)n_total) pos[id] = RESCORED;
    }
    __syncthreads();
    if (my_id >= 0 && pos[my_id] != (unsigned short)tid) my_id = -1;  // re-scored as a race entry: in L either way, counted once

    // select_body's p and its sums
    ArgMax am{-INFINITY, 0x7fffffff};
    for (int i = tid; i < n_total; i += 1024) am = better(am, ArgMax{m[i], i});
    am = block_argmax(am, sv, si);
    const float mx = am.v;
    float s = 0.f;
    for (int i = tid; i < n_total; i += 1024) s += expf(__fmul_rn(__fsub_rn(m[i], mx), tau));
    const float tot = block_sum(s, sv);
    float pj[16];
    float ps = 0.f, prest = 0.f, pres = 0.f, nu = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int j = q * 1024 + tid;
        pj[q] = 0.f;
        if (j < n_total) {
            pj[q] = expf(__fmul_rn(__fsub_rn(m[j], mx), tau)) / tot;
            ps += pj[q];
            if (pos[j] == UNLISTED) prest += pj[q];
            if (pos[j] == RESCORED) pres += pj[q];
            else nu += 1.f;
        }
    }
    const float psum = block_sum(ps, sv);
    prest = block_sum(prest, sv) / psum;
    pres = block_sum(pres, sv) / psum;
    nu = block_sum(nu, sv);  // (a count <= 16384: exact)
    const float p_me = my_id >= 0 ? expf(__fmul_rn(__fsub_rn(m[my_id], mx), tau)) / tot : 0.f;
    // P_U and P_L with the score entries up to tid re-scored; with all n_listed of them
    const float PU_t = prest + block_suffix_sum(p_me, sv) / psum, PL_t = pres + block_prefix_sum(p_me, sv) / psum;
    const float PL_l = pres + block_sum(p_me, sv) / psum;

    const float eps = fabsf(tau) * delta;
    const float em1 = expm1f(eps), emeps = expf(-eps);
    float b_t = 0.f, b_l = 0.f;  // bound(tid); bound(n_listed)
    int k_t = 0, k_l = 0;
    for (int a = 0; a < A; ++a) {
        float acc = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int j = q * 1024 + tid;
            if (j < n_total) acc = fmaf(a0[(long long)j * a0_stride + a], pj[q], acc);
        }
        const float e = block_sum(acc, sv) / psum;
        float rest = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int j = q * 1024 + tid;
            if (j < n_total && pos[j] == UNLISTED) rest += pj[q] * fabsf(a0[(long long)j * a0_stride + a] - e);
        }
        rest = block_sum(rest, sv) / psum;
        const float c_me = my_id >= 0 ? p_me * fabsf(a0[(long long)my_id * a0_stride + a] - e) : 0.f;
        const float S_t = rest + block_suffix_sum(c_me, sv) / psum;
        const float bt = eval_bound_of(em1, emeps, S_t, PL_t, PU_t), bl = eval_bound_of(em1, emeps, rest, PL_l, prest);
        if (bt > b_t) {
            b_t = bt;
            k_t = a;
        }
        if (bl > b_l) {
            b_l = bl;
            k_l = a;
        }
    }
    // need_eval: the smallest n' of [n, n_listed] whose bound is within the tolerance
    int need = (tid >= n && tid < n_listed && b_t <= eval_tol) ? tid : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int u = __shfl_xor(need, o);
        need = u < need ? u : need;
    }
    __syncthreads();
    if (lane == 0) si[wid] = need;
    if (tid == n && n < n_listed) {
        at_n[0] = b_t;
        at_n[1] = PU_t;
        at_n_k = k_t;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w) need = si[w] < need ? si[w] : need;
        if (need == 0x7fffffff) need = b_l <= eval_tol ? n_listed : n_total;
        const bool all = n >= n_listed;  // nothing listed beyond the re-scored entries: bound(n) is bound(n_listed)
        const float st8[8] = {all ? b_l : at_n[0], (float)need, all ? prest : at_n[1], (float)(all ? k_l : at_n_k), 0.f, eps, b_l, nu};
        for (int i = 0; i < 8; ++i) stats[i] = st8[i];
        if (host_stats) {
            for (int i = 0; i < 8; ++i)
                if (i != 4) host_stats[i] = st8[i];
            __threadfence_system();
            __hip_atomic_store(host_stats + 4, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
__global__ __launch_bounds__(1024) void eval_bound_kernel(const float* m, int n_total, const int* list, int r, int n, int n_listed,
                                                           const float* a0, long long a0_stride, int A, float tau, float delta,
                                                           float eval_tol, float* stats, float* host_stats, float seq) {
    __shared__ unsigned short pos[16384];
    __shared__ float sv[16];
    __shared__ int si[16];
    __shared__ float at_n[2];
    __shared__ int at_n_k;
    eval_bound_body(m, n_total, list, r, n, n_listed, a0, a0_stride, A, tau, delta, eval_tol, stats, host_stats, seq, pos, sv, si, at_n,
                    &at_n_k);
}
void launch_eval_bound(const float* m, int n_total, const int* list, int r, int n, int n_listed, const float* a0, long long a0_stride,
                       int A, float tau, float delta, float eval_tol, float* stats, float* host_stats, float seq, hipStream_t st) {
    if (n_total <= 0 || n_total > 16384 || r < 0 || n < 0 || n > n_listed || r + n_listed > 1024) return;
    M3PC_SEL_PICK(18);
    hipLaunchKernelGGL(eval_bound_kernel, dim3(1), dim3(1024), 0, st, m, n_total, list, r, n, n_listed, a0, a0_stride, A, tau, delta,
                       eval_tol, stats, host_stats, seq);
}
// launch_eval_bound for up to 64 windows in one launch: workgroup i is window w0 + i with its own r / n / delta, row w of the merged
// vectors, the slice of its list from rmax - r on, its first actions and its block of 8 statistics -- the body is the one-window
// kernel's, so the eight floats are its bit for bit.  The pos table is per workgroup: the LDS of the one-window kernel.
__global__ __launch_bounds__(1024) void eval_bound_batch_kernel(EvalBoundBatchP P) {
    __shared__ unsigned short pos[16384];
    __shared__ float sv[16];
    __shared__ int si[16];
    __shared__ float at_n[2];
    __shared__ int at_n_k;
    const int i = blockIdx.x;
    const long long w = P.w0 + i;
    const int r = P.r[i];
    eval_bound_body(P.m + w * P.n_total, P.n_total, P.list + w * P.list_stride + (P.rmax - r), r, P.n[i], P.n_listed,
                    P.a0 + w * P.a0_wstride, P.a0_stride, P.A, P.tau, P.delta[i], P.eval_tol, P.stats + 8 * w,
                    P.host_stats ? P.host_stats + 8 * w : nullptr, P.seq, pos, sv, si, at_n, &at_n_k);
}
void launch_eval_bound_batch(EvalBoundBatchP& P, int E, const int* r, const int* n, const float* delta, hipStream_t st) {
    if (P.n_total <= 0 || P.n_total > 16384) return;
    for (int w = 0; w < E; ++w)  // (the one-window launcher's bounds, for every window, before anything is launched)
        if (r[w] < 0 || r[w] > P.rmax || n[w] < 0 || n[w] > P.n_listed || r[w] + P.n_listed > 1024) return;
    for (int w0 = 0; w0 < E; w0 += 64) {  // (per-window scalars travel in the kernel arguments: 64 windows per launch)
        const int e = E - w0 < 64 ? E - w0 : 64;
        P.w0 = w0;
        for (int i = 0; i < e; ++i) {
            P.r[i] = r[w0 + i];
            P.n[i] = n[w0 + i];
            P.delta[i] = delta[w0 + i];
        }
        M3PC_SEL_PICK(19);
        hipLaunchKernelGGL(eval_bound_batch_kernel, dim3(e), dim3(1024), 0, st, P);
    }
}

__global__ void scatter_kernel(const float* src, const int* index, int n, float* dst, int* index_copy) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        dst[index[i]] = src[i];
        if (index_copy) index_copy[i] = index[i];
    }
}
void launch_scatter(const float* src, const int* index, int n, float* dst, int* index_copy, hipStream_t st) {
    if (n <= 0) return;
    M3PC_SEL_PICK(20);
    hipLaunchKernelGGL(scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, st, src, index, n, dst, index_copy);
}

// cand[w m + i] = sample_actions[w, list_w[lo + i]] (rows of `row` floats) and window_index[w m + i] = w for the slice [lo, lo + m)
// of every window's list: the rows one m3pc_score_actions call re-scores, window-major.  One wave per row; an entry that names no
// candidate (a list slot no ranking wrote) leaves its row untouched.
__global__ __launch_bounds__(64) void gather_listed_kernel(const float* sa, int n_total, int row, const int* list, int list_stride, int lo,
                                                           int m, float* cand, int* window_index) {
    const int o = blockIdx.x, w = o / m, i = o - w * m;
    const int id = list[(long long)w * list_stride + lo + i];
    if (threadIdx.x == 0 && window_index) window_index[o] = w;
    if ((unsigned int)id >= (unsigned int)n_total) return;
    const float* src = sa + ((long long)w * n_total + id) * row;
    float* dst = cand + (long long)o * row;
    for (int c = threadIdx.x; c < row; c += 64) dst[c] = src[c];
}
void launch_gather_listed(const float* sa, int E, int n_total, int row, const int* list, int list_stride, int lo, int m, float* cand,
                          int* window_index, hipStream_t st) {
    if (E <= 0 || m <= 0 || row <= 0) return;
    M3PC_SEL_PICK(21);
    hipLaunchKernelGGL(gather_listed_kernel, dim3((unsigned)(E * m)), dim3(64), 0, st, sa, n_total, row, list, list_stride, lo, m, cand,
                       window_index);
}

// ---- the variates of a plan step from a counter-based generator (m3pc_draw_variates): a value depends on (seed, step, element
// index) alone -- not on the launch geometry, the slice asked for or earlier draws -- so a candidate-sharded rank draws its rows
// of the one-rank array.  Philox4x32-10 (Salmon et al., SC'11): key = (seed lo, seed hi), counter = (block, step lo, step hi,
// array) with array 0 = eps, 1 = expo; block b gives the flat elements 4b .. 4b+3 of its array.  The generator itself: philox.h.
// Box-Muller on two words: u1 = ((wa >> 8) + 1) 2^-24 in (0, 1], u2 = (wb >> 8) 2^-24; z = sqrt(-2 ln u1) (cos 2 pi u2, sin 2 pi u2).
// 2 u2 is exact in fp32, so the angle goes through sincospif unrounded; logf / sqrtf / sincospif are the precise library versions.
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float& z0, float& z1) {
    const float u1 = (float)((wa >> 8) + 1u) * 0x1p-24f;
    const float t2 = (float)(wb >> 8) * 0x1p-23f;
    const float r = sqrtf(-2.f * logf(u1));
    float s, c;
    sincospif(t2, &s, &c);
    z0 = r * c;
    z1 = r * s;
}
// array 0: standard normals; array 1: Exp(1), -ln u with u in (0, 1], and 2^-25 where that is 0 (the select divides by it and the
// race key takes its log).  One thread per Philox block.  g0 / g1: the slice [g0, g1) of the flat array that goes to out[0 .. g1 - g0);
// a block wholly inside the slice is one 16-byte store when g0 and `out` allow it, everything else goes element by element.
__device__ __forceinline__ void variates_body(uint32_t k0, uint32_t k1, uint32_t s0, uint32_t s1, uint32_t array, long long g0,
                                              long long g1, float* __restrict__ out, int vec_ok) {
    const long long b = g0 / 4 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (4 * b >= g1) return;
    uint32_t w[4];
    philox4x32_10((uint32_t)b, s0, s1, array, k0, k1, w);
    float v[4];
    if (array == 0) {
        box_muller(w[0], w[1], v[0], v[1]);
        box_muller(w[2], w[3], v[2], v[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float q = -logf((float)((w[i] >> 8) + 1u) * 0x1p-24f);
            v[i] = q > 0.f ? q : 0x1p-25f;
        }
    }
    const long long e = 4 * b;
    if (vec_ok && e >= g0 && e + 4 <= g1) {
        *reinterpret_cast<float4*>(out + (e - g0)) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (e + i >= g0 && e + i < g1) out[e + i - g0] = v[i];
}
__global__ __launch_bounds__(256) void variates_kernel(uint32_t k0, uint32_t k1, uint32_t s0, uint32_t s1, uint32_t array, long long g0,
                                                       long long g1, float* __restrict__ out, int vec_ok) {
    variates_body(k0, k1, s0, s1, array, g0, g1, out, vec_ok);
}
// The normals of up to 64 windows in one launch: blockIdx.y picks the window -- its step (the generator's counter words) and its
// block of g1 - g0 floats in out.  A value depends on (seed, step, element) alone, so window w gets launch_variates' for steps[w].
struct VariatesBatchP {
    uint32_t s0[64], s1[64];
};
__global__ __launch_bounds__(256) void variates_batch_kernel(uint32_t k0, uint32_t k1, VariatesBatchP sp, long long g0, long long g1,
                                                             float* __restrict__ out, int vec_ok) {
    const int y = blockIdx.y;
    variates_body(k0, k1, sp.s0[y], sp.s1[y], 0u, g0, g1, out + (size_t)y * (size_t)(g1 - g0), vec_ok);
}
void launch_variates(unsigned long long seed, unsigned long long step, int array, long long g0, long long g1, float* out, hipStream_t st) {
    if (g1 <= g0 || !out) return;
    const long long blocks = (g1 + 3) / 4 - g0 / 4;
    const int vec_ok = g0 % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    M3PC_SEL_PICK(22);
    hipLaunchKernelGGL(variates_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, st, (uint32_t)seed, (uint32_t)(seed >> 32),
                       (uint32_t)step, (uint32_t)(step >> 32), (uint32_t)array, g0, g1, out, vec_ok);
}

void launch_variates_batch(unsigned long long seed, const unsigned long long* steps, int E, long long g0, long long g1, float* out,
                           hipStream_t st) {
    if (g1 <= g0 || !out || E <= 0) return;
    const long long blocks = (g1 + 3) / 4 - g0 / 4, len = g1 - g0;
    // (a 16-byte store needs every window's block aligned: len % 4 == 0, or one window)
    const int vec_ok = g0 % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0 && (len % 4 == 0 || E == 1);
    for (int w0 = 0; w0 < E; w0 += 64) {
        const int m = E - w0 < 64 ? E - w0 : 64;
        VariatesBatchP sp;
        memset(&sp, 0, sizeof(sp));
        for (int i = 0; i < m; ++i) {
            sp.s0[i] = (uint32_t)steps[w0 + i];
            sp.s1[i] = (uint32_t)(steps[w0 + i] >> 32);
        }
        M3PC_SEL_PICK(23);
        hipLaunchKernelGGL(variates_batch_kernel, dim3((unsigned)((blocks + 255) / 256), m), dim3(256), 0, st, (uint32_t)seed,
                           (uint32_t)(seed >> 32), sp, g0, g1, out + (size_t)w0 * len, vec_ok);
    }
}

}  // namespace m3pc
