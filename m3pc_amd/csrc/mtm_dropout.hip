// The kernels of the gradient of the masked-trajectory loss that draw or read keep masks (mtm_grad.h, DROPOUT): the product and the
// three attention kernels of mtm_grad.hip with DROP = true (the bodies of mtm_grad_body.h), dY = dX * k over rows, and the mask
// itself as bytes.  mtm_grad.hip's launchers come here when a launch carries a site (drop.thr != 0).
#include <math.h>
#include <stdint.h>

#include "mtm_grad.h"
#include "mtm_grad_body.h"

namespace m3pc {
namespace {

__global__ __launch_bounds__(256) void mg_gemm_drop_kernel(GemmG p) { mg_gemm_body<false, true>(p); }
__global__ __launch_bounds__(256) void mg_attn_fwd_drop_kernel(AttG p) { mg_attn_fwd_body<true>(p); }
__global__ __launch_bounds__(256) void mg_attn_col_drop_kernel(AttG p) { mg_attn_col_body<true>(p, 0); }
__global__ __launch_bounds__(256) void mg_attn_row_drop_kernel(AttG p) { mg_attn_row_body<true>(p); }

// one thread per (row quad, column): consecutive threads take consecutive columns, so each of the four rows is read and written in
// whole lines, and one Philox call serves the four rows
__global__ __launch_bounds__(256) void mg_drop_rows_kernel(DropRowsG p) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long quads = (long long)((p.R + 3) >> 2) * p.C;
    if (t >= quads) return;
    const int c = (int)(t % p.C), r0 = 4 * (int)(t / p.C);
    const unsigned int k4 = drop_keep4(p.drop, (uint32_t)t);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (r0 + j >= p.R) break;
        const size_t at = (size_t)(r0 + j) * p.C + c;
        p.dY[at] = drop_apply((k4 >> j) & 1u, p.dX[at], p.drop.scale);
    }
}

// the keep bits of one site as bytes.  attn 0: a matrix site of extent (R, C); 1: R attention rows of C keys.  One thread per quad.
__global__ __launch_bounds__(256) void mg_keep_kernel(DropG d, long long R, int C, int attn, unsigned char* keep) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int nq = (C + 3) >> 2;
    const long long quads = attn ? R * nq : ((R + 3) >> 2) * C;
    if (t >= quads) return;
    const unsigned int k4 = drop_keep4(d, (uint32_t)t);
    for (int j = 0; j < 4; ++j) {
        const long long r = attn ? t / nq : 4 * (t / C) + j;
        const int c = attn ? 4 * (int)(t % nq) + j : (int)(t % C);
        if (r < R && c < C) keep[r * C + c] = (unsigned char)((k4 >> j) & 1u);
    }
}

unsigned blocks256(long long n) { return (unsigned)((n + 255) / 256); }
unsigned blocks4(long long n) { return (unsigned)((n + 3) / 4); }

}  // namespace

DropG mg_drop_make(double p, unsigned long long seed, unsigned long long draw) {
    DropG d;
    d.thr = (unsigned int)floor(p * 4294967296.0);  // (p < 1: below 2^32; p < 2^-32 drops nothing)
    d.scale = (float)(1.0 / (1.0 - p));
    d.k0 = (unsigned int)seed;
    d.k1 = (unsigned int)(seed >> 32);
    d.d0 = (unsigned int)draw;
    d.d1 = (unsigned int)(draw >> 32);
    d.c3 = 0;
    return d;
}

void mg_launch_gemm_drop(const GemmG& p, hipStream_t st) {
    const long long tiles = (long long)((p.M + 31) / 32) * ((p.N + 31) / 32);
    M3PC_MG_PICK(16);
    hipLaunchKernelGGL(mg_gemm_drop_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, st, p);
}
void mg_launch_attn_fwd_drop(const AttG& p, hipStream_t st) {
    M3PC_MG_PICK(17);
    hipLaunchKernelGGL(mg_attn_fwd_drop_kernel, dim3(blocks4((long long)p.B * p.nh * p.L)), dim3(256), 0, st, p);
}
void mg_launch_attn_col_drop(const AttG& p, hipStream_t st) {
    M3PC_MG_PICK(18);
    hipLaunchKernelGGL(mg_attn_col_drop_kernel, dim3(blocks4((long long)p.B * p.nh * p.L)), dim3(256), 0, st, p);
}
void mg_launch_attn_row_drop(const AttG& p, hipStream_t st) {
    M3PC_MG_PICK(19);
    hipLaunchKernelGGL(mg_attn_row_drop_kernel, dim3(blocks4((long long)p.B * p.nh * p.L)), dim3(256), 0, st, p);
}
void mg_launch_drop_rows(const DropRowsG& p, hipStream_t st) {
    if (p.R <= 0 || p.C <= 0) return;
    M3PC_MG_PICK(20);
    hipLaunchKernelGGL(mg_drop_rows_kernel, dim3(blocks256((long long)((p.R + 3) / 4) * p.C)), dim3(256), 0, st, p);
}
void mg_launch_keep(const DropG& d, long long R, int C, unsigned char* keep, hipStream_t st) {
    if (R <= 0 || C <= 0) return;
    const int attn = (d.c3 & 0xffu) == MG_DROP_ATTN ? 1 : 0;
    const long long quads = attn ? R * ((C + 3) / 4) : ((R + 3) / 4) * C;
    M3PC_MG_PICK(21);
    hipLaunchKernelGGL(mg_keep_kernel, dim3(blocks256(quads)), dim3(256), 0, st, d, R, C, attn, keep);
}

}  // namespace m3pc
