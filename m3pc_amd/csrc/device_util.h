// Device helpers shared by the kernel files: vector and address-space types, wave / block reductions, the row map, the GELUs,
// the counted wait + barrier, and the GEMM epilogue flags.  Everything is __forceinline__: a kernel that is asserted bit-equal
// to another one (split-K reduce against the direct fp32 kernel, fused against unfused LayerNorm tail, ...) runs the same
// function, not a copy of it.
#pragma once
#include "kernels.h"

namespace m3pc {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
typedef const void __attribute__((address_space(1))) * gptr_t;  // global / LDS side of a direct-to-LDS load
typedef void __attribute__((address_space(3))) * lptr_t;
// typed LDS pointers: reads and writes through them are ds_ instructions (through a generic pointer they become flat ones)
typedef char __attribute__((address_space(3))) * lds_c_t;
typedef const char __attribute__((address_space(3))) * lds_cc_t;
typedef const float __attribute__((address_space(3))) * lds_cf32_t;

// ---- reductions: xor butterflies over the 64 lanes; every lane returns the same bits
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// over the workgroup: the wave results through sv (one float per wave), combined left to right by every thread
__device__ __forceinline__ float block_sum(float v, float* sv) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) sv[wid] = v;
    __syncthreads();
    float t = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sv[w];
    return t;
}
// the same two in float64 (mtm_loss.hip: every sum of a loss term): the same butterfly and the same left-to-right combination
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double block_sum_f64(double v, double* sv) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    v = wave_sum_f64(v);
    __syncthreads();
    if (lane == 0) sv[wid] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sv[w];
    return t;
}
__device__ __forceinline__ float block_max(float v, float* sv) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    v = wave_max(v);
    __syncthreads();
    if (lane == 0) sv[wid] = v;
    __syncthreads();
    float t = sv[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) t = fmaxf(t, sv[w]);
    return t;
}

__device__ __forceinline__ int map_row(const RowMap& m, int r) {  // kernels.h: RowMap
    if (m.rpg == 0) return r;
    return (r / m.rpg) * m.gstride + (r % m.rpg) + m.off;
}

// ---- exact-erf GELU.  fp32 arithmetic: libm erff.  bf16 kernels: Abramowitz-Stegun 7.1.26 (|err(erf)| <= 1.5e-7, far below
// bf16 resolution) -- 2 transcendentals + 8 VALU instead of a ~35-instruction erff, which would otherwise make an FFN epilogue
// VALU-bound beside the matrix pipe.
__device__ __forceinline__ float gelu_exact(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_fast(float x) {
    const float ax = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));
    float p = fmaf(t, 1.061405429f, -1.453152027f);
    p = fmaf(t, p, 1.421413741f);
    p = fmaf(t, p, -0.284496736f);
    p = fmaf(t, p, 0.254829592f);
    p *= t;
    const float e = __builtin_amdgcn_exp2f(-ax * ax * 1.44269504088896340736f);
    const float erf_abs = fmaf(-p, e, 1.0f);
    const float hx = 0.5f * x;
    return fmaf(fabsf(hx), erf_abs, hx);  // 0.5x(1+erf(x/sqrt2)) with erf odd
}
// gelu_fast on two values at once: the polynomial runs on v_pk_fma_f32 / v_pk_mul_f32 (two fp32 lanes per instruction), which
// halves its VALU cost; every operation and its order are gelu_fast's, so the results are identical
__device__ __forceinline__ f32x2 gelu_fast2(f32x2 x) {
    const f32x2 one = {1.0f, 1.0f};
    const f32x2 ax = __builtin_elementwise_abs(x) * 0.70710678118654752440f;
    const f32x2 d = __builtin_elementwise_fma((f32x2){0.3275911f, 0.3275911f}, ax, one);
    const f32x2 t = {__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
    f32x2 p = __builtin_elementwise_fma(t, (f32x2){1.061405429f, 1.061405429f}, (f32x2){-1.453152027f, -1.453152027f});
    p = __builtin_elementwise_fma(t, p, (f32x2){1.421413741f, 1.421413741f});
    p = __builtin_elementwise_fma(t, p, (f32x2){-0.284496736f, -0.284496736f});
    p = __builtin_elementwise_fma(t, p, (f32x2){0.254829592f, 0.254829592f});
    p *= t;
    const f32x2 a = -ax * ax * 1.44269504088896340736f;
    const f32x2 e = {__builtin_amdgcn_exp2f(a.x), __builtin_amdgcn_exp2f(a.y)};
    const f32x2 erf_abs = __builtin_elementwise_fma(-p, e, one);
    const f32x2 hx = 0.5f * x;
    return __builtin_elementwise_fma(__builtin_elementwise_abs(hx), erf_abs, hx);
}

// num_records of a buffer resource over b bytes (the field is 32 bits wide)
__device__ __forceinline__ unsigned clamp_bytes(long long b) { return b > 0xfffff000ll ? 0xfffff000u : (unsigned)b; }

// Wait until at most N of this wave's vector-memory operations (LDS-DMA loads among them) are outstanding, then a raw
// s_barrier: a __syncthreads would drain the whole queue.  LGKM: wait for the wave's LDS / scalar operations too.
template <int N, bool LGKM = false>
__device__ __forceinline__ void wait_vmcnt_barrier() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
    if constexpr (LGKM) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}

// ---- GEMM epilogue flags (template parameter of the GEMM kernels).  GE_GELU_EXACT (with GE_GELU): libm erff;
// GE_SPLITK: the block owns a run of k-tiles and writes raw partials to p.ws (gemm.hip, gemm_x3.hip)
enum { GE_GELU = 1, GE_RES = 2, GE_ROWTAB = 4, GE_F32OUT = 8, GE_GELU_EXACT = 16, GE_SPLITK = 1 << 8 };
// the flags of a problem as every launcher forms them; a kernel that differs ors in or masks what it needs
static inline int epi_flags(const GemmP& p) {
    return (p.gelu ? GE_GELU : 0) | (p.res ? GE_RES : 0) | (p.rowtab ? GE_ROWTAB : 0) | (p.Cf ? GE_F32OUT : 0);
}

}  // namespace m3pc
