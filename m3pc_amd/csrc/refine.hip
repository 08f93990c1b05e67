// CEM / MPPI refinement of a plan (m3pc_refit_resample, m3pc_refine_plan): the refit of the sampling distribution on the elite
// candidates and the resample from it.  Per iteration the refinement is scoring (m3pc_score_actions' kernels), launch_topk, and
// the two launches below.  Reductions are 64-lane butterflies + one LDS hop summed in a fixed order, no atomics: a result does
// not change from run to run.  m3pc_refine_plans runs the same steps for E lock-step windows: the *_batch kernels below take the window
// as a grid index around the one-window device functions, and the batched resample forms the shifted first distribution.
#include "device_util.h"

namespace m3pc {
namespace {

constexpr int RF_THREADS = 256;  // refit: one workgroup per column
constexpr int RF_HELD = 4;       // elite values a thread keeps in registers between the passes: all of them while k <= 1024

// (an id outside [0, n) would read outside cand / scores: it is clamped, the caller's list is wrong either way)
__device__ __forceinline__ int elite_id(const RefitP& p, int i) {
    const int e = p.elite[i];
    return e < 0 ? 0 : (e >= p.n ? p.n - 1 : e);
}

// f(x_i, E_i) over this thread's elites i = tid, tid + 256, ...: the first RF_HELD from registers, the rest gathered again
template <typename F>
__device__ __forceinline__ void each_elite(const RefitP& p, int c, const float (&xr)[RF_HELD], const float (&er)[RF_HELD], F f) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < RF_HELD; ++j)
        if (tid + j * RF_THREADS < p.k) f(xr[j], er[j]);
    for (int i = tid + RF_HELD * RF_THREADS; i < p.k; i += RF_THREADS) {
        const int e = elite_id(p, i);
        f(p.cand[(size_t)e * p.C + c], p.weighting == 1 ? p.scores[e] : 0.f);
    }
}

// Column c = (t, a) over the k elite rows x_i = cand[elite_i, c]:
//   w_i = u_i / sum u,  u_i = 1 (CEM) or expf(tau (E_i - max E)) (MPPI)
//   mean = x_0 + sum w_i (x_i - x_0)   (= sum w_i x_i; about the column's first elite, so that a column of equal values has
//                                        exactly that value as its mean and exactly 0 as its spread)
//   S = sum w_i (x_i - mean)^2 in a second pass,  D = sum w_i (1 - w_i),  std = max(D > 1e-6 ? sqrt(S / D) : 0, min_std)
__device__ __forceinline__ void refit_body(const RefitP& p, int c, float* sv) {
    const int tid = threadIdx.x;
    const bool mppi = p.weighting == 1;
    float xr[RF_HELD], er[RF_HELD];
#pragma unroll
    for (int j = 0; j < RF_HELD; ++j) {
        const int i = tid + j * RF_THREADS;
        xr[j] = 0.f;
        er[j] = 0.f;
        if (i < p.k) {
            const int e = elite_id(p, i);
            xr[j] = p.cand[(size_t)e * p.C + c];
            if (mppi) er[j] = p.scores[e];
        }
    }
    float mx = 0.f, su = (float)p.k;
    if (mppi) {
        float m = -INFINITY;
        each_elite(p, c, xr, er, [&](float, float E) { m = fmaxf(m, E); });
        mx = block_max(m, sv);
        float s = 0.f;
        each_elite(p, c, xr, er, [&](float, float E) { s += expf(p.tau * (E - mx)); });
        su = block_sum(s, sv);
    }
    auto weight = [&](float E) { return (mppi ? expf(p.tau * (E - mx)) : 1.f) / su; };
    const float x0 = p.cand[(size_t)elite_id(p, 0) * p.C + c];
    float a = 0.f;
    each_elite(p, c, xr, er, [&](float x, float E) { a += weight(E) * (x - x0); });
    const float mean = x0 + block_sum(a, sv);
    float s2 = 0.f, dd = 0.f;
    each_elite(p, c, xr, er, [&](float x, float E) {
        const float w = weight(E), d = x - mean;
        s2 += w * (d * d);
        dd += w * (1.f - w);
    });
    const float S = block_sum(s2, sv);
    const float D = block_sum(dd, sv);
    if (tid == 0) {
        const float sd = D > 1e-6f ? sqrtf(S / D) : 0.f;
        p.mean[c] = mean;
        p.std[c] = fmaxf(sd, p.min_std);
    }
}
__global__ __launch_bounds__(RF_THREADS) void refit_kernel(RefitP p) {
    __shared__ float sv[RF_THREADS / 64];
    refit_body(p, blockIdx.x, sv);
}
// E windows in one launch: blockIdx.y picks the window -- its (n, C) candidates, n scores, k elites, C means and stds --, the
// column's work is refit_body's: a window's mean / std are the one-window launch's bit for bit.
__global__ __launch_bounds__(RF_THREADS) void refit_batch_kernel(RefitP p) {
    __shared__ float sv[RF_THREADS / 64];
    const size_t w = blockIdx.y;
    p.cand += w * p.n * p.C;
    p.elite += w * p.k;
    if (p.scores) p.scores += w * p.n;
    p.mean += w * p.C;
    p.std += w * p.C;
    refit_body(p, blockIdx.x, sv);
}

// element e of the (n, C) block: out = min(1, max(-1, mean_c + std_c * noise)), product and sum rounded separately (what
// torch.clamp(mean + std * noise, -1, 1) computes in fp32).  The first row's threads also write the distribution out (the first
// distribution of a refinement is formed here: tanh of the policy head / the caller's mean, a constant std) and the two actions.
__device__ __forceinline__ float resample_one(const ResampleP& p, int e, float z) {
    const int c = e % p.C;
    const float m = p.mean ? p.mean[c] : tanhf(p.loc[c]);
    const float s = p.std ? p.std[c] : p.std_const;
    const float v = fminf(1.f, fmaxf(-1.f, __fadd_rn(m, __fmul_rn(s, z))));
    if (e < p.C) {
        if (p.mean_out) p.mean_out[c] = m;
        if (p.std_out) p.std_out[c] = s;
        if (e < p.A) {
            if (p.sample_action) p.sample_action[e] = v;
            if (p.eval_action) p.eval_action[e] = m;
        }
    }
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(256) void resample_kernel(ResampleP p) {
    const int stride = gridDim.x * blockDim.x;
    if (VEC) {  // (total % 4 == 0, noise and out 16-byte aligned)
        for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < p.total / 4; q += stride) {
            const float4 z = reinterpret_cast<const float4*>(p.noise)[q];
            float4 o;
            o.x = resample_one(p, 4 * q, z.x);
            o.y = resample_one(p, 4 * q + 1, z.y);
            o.z = resample_one(p, 4 * q + 2, z.z);
            o.w = resample_one(p, 4 * q + 3, z.w);
            reinterpret_cast<float4*>(p.out)[q] = o;
        }
    } else {
        for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < p.total; e += stride) p.out[e] = resample_one(p, e, p.noise[e]);
    }
}

// The resample of E windows: blockIdx.y picks window w0 + y.  Later distributions are rows of mean / std (E, C); the first one is
// formed here per window (row t = c / A): init_mean[w, t + init_offset] while that row is one of the window's init_rows, else tanh
// of its policy head at step T - h + t; std_const.  The arithmetic of an element is resample_one's.
__device__ __forceinline__ float resample_batch_one(const ResampleBatchP& p, int y, size_t w, int e, float z) {
    const int c = e % p.C;
    float m;
    if (p.mean) {
        m = p.mean[w * p.C + c];
    } else {
        const int t = c / p.A + p.init_offset;
        m = p.init_mean && t < p.init_rows[y] ? p.init_mean[(w * p.init_stride + t) * p.A + c % p.A] : tanhf(p.loc[w * p.loc_wstride + c]);
    }
    const float s = p.std ? p.std[w * p.C + c] : p.std_const;
    const float v = fminf(1.f, fmaxf(-1.f, __fadd_rn(m, __fmul_rn(s, z))));
    if (e < p.C) {
        if (p.mean_out) p.mean_out[w * p.C + c] = m;
        if (p.std_out) p.std_out[w * p.C + c] = s;
        if (e < p.A) {
            if (p.sample_action) p.sample_action[w * p.A + e] = v;
            if (p.eval_action) p.eval_action[w * p.A + e] = m;
        }
    }
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(256) void resample_batch_kernel(ResampleBatchP p) {
    const int stride = gridDim.x * blockDim.x, y = blockIdx.y;
    const size_t w = (size_t)p.w0 + y;
    const float* noise = p.noise + w * p.total;
    float* out = p.out + w * p.total;
    if (VEC) {  // (total % 4 == 0, noise and out 16-byte aligned: every window's block is)
        for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < p.total / 4; q += stride) {
            const float4 z = reinterpret_cast<const float4*>(noise)[q];
            float4 o;
            o.x = resample_batch_one(p, y, w, 4 * q, z.x);
            o.y = resample_batch_one(p, y, w, 4 * q + 1, z.y);
            o.z = resample_batch_one(p, y, w, 4 * q + 2, z.z);
            o.w = resample_batch_one(p, y, w, 4 * q + 3, z.w);
            reinterpret_cast<float4*>(out)[q] = o;
        }
    } else {
        for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < p.total; e += stride) out[e] = resample_batch_one(p, y, w, e, noise[e]);
    }
}

__global__ __launch_bounds__(256) void window_index_kernel(int* out, int total, int n) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < total) out[c] = c / n;
}

}  // namespace

void launch_refit(const RefitP& p, hipStream_t st) {
    if (p.C <= 0 || p.k <= 0) return;
    hipLaunchKernelGGL(refit_kernel, dim3(p.C), dim3(RF_THREADS), 0, st, p);
}

void launch_refit_batch(const RefitP& p, int E, hipStream_t st) {
    if (p.C <= 0 || p.k <= 0 || E <= 0) return;
    for (int w0 = 0; w0 < E; w0 += 32768) {  // (far inside the grid's y limit)
        RefitP q = p;
        q.cand += (size_t)w0 * p.n * p.C;
        q.elite += (size_t)w0 * p.k;
        if (q.scores) q.scores += (size_t)w0 * p.n;
        q.mean += (size_t)w0 * p.C;
        q.std += (size_t)w0 * p.C;
        hipLaunchKernelGGL(refit_batch_kernel, dim3(p.C, E - w0 < 32768 ? E - w0 : 32768), dim3(RF_THREADS), 0, st, q);
    }
}

void launch_window_index(int* out, int total, int n, hipStream_t st) {
    if (total <= 0 || n <= 0) return;
    hipLaunchKernelGGL(window_index_kernel, dim3((total + 255) / 256), dim3(256), 0, st, out, total, n);
}

void launch_resample_batch(ResampleBatchP& p, int E, const int* init_rows, hipStream_t st) {
    if (p.total <= 0 || E <= 0) return;
    // a window's block starts w * total elements into noise / out: 16-byte accesses only where that keeps the alignment for EVERY
    // window (total % 4 == 0), not just for window 0
    const bool vec = p.total % 4 == 0 && (reinterpret_cast<uintptr_t>(p.noise) | reinterpret_cast<uintptr_t>(p.out)) % 16 == 0;
    const int work = vec ? p.total / 4 : p.total;
    const int blocks = (work + 255) / 256 < 2048 ? (work + 255) / 256 : 2048;
    for (int w0 = 0; w0 < E; w0 += 64) {
        const int m = E - w0 < 64 ? E - w0 : 64;
        p.w0 = w0;
        for (int i = 0; i < 64; ++i) p.init_rows[i] = i < m && p.init_mean ? (init_rows ? init_rows[w0 + i] : p.init_stride) : 0;
        if (vec) hipLaunchKernelGGL(resample_batch_kernel<true>, dim3(blocks, m), dim3(256), 0, st, p);
        else hipLaunchKernelGGL(resample_batch_kernel<false>, dim3(blocks, m), dim3(256), 0, st, p);
    }
}

void launch_resample(const ResampleP& p, hipStream_t st) {
    if (p.total <= 0) return;
    const bool vec = p.total % 4 == 0 && (reinterpret_cast<uintptr_t>(p.noise) | reinterpret_cast<uintptr_t>(p.out)) % 16 == 0;
    const int work = vec ? p.total / 4 : p.total;
    const int blocks = (work + 255) / 256 < 2048 ? (work + 255) / 256 : 2048;
    if (vec) hipLaunchKernelGGL(resample_kernel<true>, dim3(blocks), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(resample_kernel<false>, dim3(blocks), dim3(256), 0, st, p);
}

}  // namespace m3pc
