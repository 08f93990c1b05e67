// CEM / MPPI refinement of a plan (m3pc_refit_resample, m3pc_refine_plan): the refit of the sampling distribution on the elite
// candidates and the resample from it.  Per iteration the refinement is scoring (m3pc_score_actions' kernels), launch_topk, and
// the two launches below.  Reductions are 64-lane butterflies + one LDS hop summed in a fixed order, no atomics: a result does
// not change from run to run.
#include "kernels.h"

namespace m3pc {
namespace {

constexpr int RF_THREADS = 256;  // refit: one workgroup per column
constexpr int RF_HELD = 4;       // elite values a thread keeps in registers between the passes: all of them while k <= 1024

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wmax(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float block_sum(float v, float* sv) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    v = wsum(v);
    __syncthreads();
    if (lane == 0) sv[wid] = v;
    __syncthreads();
    float t = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sv[w];
    return t;
}
__device__ __forceinline__ float block_max(float v, float* sv) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    v = wmax(v);
    __syncthreads();
    if (lane == 0) sv[wid] = v;
    __syncthreads();
    float t = sv[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) t = fmaxf(t, sv[w]);
    return t;
}

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
__global__ __launch_bounds__(RF_THREADS) void refit_kernel(RefitP p) {
    __shared__ float sv[RF_THREADS / 64];
    const int tid = threadIdx.x, c = blockIdx.x;
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

}  // namespace

void launch_refit(const RefitP& p, hipStream_t st) {
    if (p.C <= 0 || p.k <= 0) return;
    hipLaunchKernelGGL(refit_kernel, dim3(p.C), dim3(RF_THREADS), 0, st, p);
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
