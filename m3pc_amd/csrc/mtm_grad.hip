// The gradient of the masked-trajectory loss (include/m3pc_hip.h: m3pc_mtm_grad*).  mtm_grad.h states the launches, what the forward
// keeps, the reduction orders, the bytes and the dropout sites.  fp32 only.  The kernels with keep masks: mtm_dropout.hip.
#include <stdint.h>

#include "device_util.h"
#include "iql.h"
#include "mtm_loss.h"
#include "mtm_grad.h"
#include "mtm_grad_body.h"

namespace m3pc {
namespace {

typedef unsigned long long u64;

// ------------------------------------------------------------------------------------------------ the product
// C[m][n] = sum_k A(m, k) B(k, n) (GemmG, mtm_grad.h); the body, with its tiling and its k order: mtm_grad_body.h
template <bool SPLIT>
__global__ __launch_bounds__(256) void mg_gemm_kernel(GemmG p) {
    mg_gemm_body<SPLIT, false>(p);
}

// ------------------------------------------------------------------------------------------------ LayerNorm
__global__ __launch_bounds__(256) void mg_ln_fwd_kernel(LnG p) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= p.rows) return;
    const float* x = p.X + rmap(p.xmap, r) * p.d;
    float s = 0.f;
    for (int c = lane; c < p.d; c += 64) s += x[c];
    const float mean = wave_sum(s) / (float)p.d;
    float v = 0.f;
    for (int c = lane; c < p.d; c += 64) {
        const float t = x[c] - mean;
        v += t * t;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(v) / (float)p.d + 1e-5f);
    for (int c = lane; c < p.d; c += 64) p.Y[(size_t)r * p.d + c] = (x[c] - mean) * rstd * p.g[c] + p.b[c];
    if (lane == 0) {
        p.st[2 * (size_t)r] = mean;
        p.st[2 * (size_t)r + 1] = rstd;
    }
}

// dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma
__global__ __launch_bounds__(256) void mg_ln_bwd_kernel(LnG p) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= p.rows) return;
    const long long xr = rmap(p.xmap, r);
    const float* x = p.X + xr * p.d;
    const float* dy = p.dY + (size_t)r * p.d;
    const float mean = p.st[2 * (size_t)r], rstd = p.st[2 * (size_t)r + 1];
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane; c < p.d; c += 64) {
        const float g = dy[c] * p.g[c];
        s1 += g;
        s2 += g * ((x[c] - mean) * rstd);
    }
    s1 = wave_sum(s1) / (float)p.d;
    s2 = wave_sum(s2) / (float)p.d;
    float* dx = p.dX + xr * p.d;
    for (int c = lane; c < p.d; c += 64) {
        const float g = dy[c] * p.g[c], xh = (x[c] - mean) * rstd;
        const float v = rstd * ((g - s1) - xh * s2);
        dx[c] = p.accumulate ? dx[c] + v : v;
    }
}

// ------------------------------------------------------------------------------------------------ column sums
// the rows (s, j) and the two sums: ColG (mtm_grad.h).  One thread per column and chunk of 64 rows, then one per column over the chunks.
__global__ __launch_bounds__(256) void mg_colsum_kernel(ColG p) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= p.C) return;
    const long long total = (long long)p.nseq * p.n;
    const long long q0 = (long long)blockIdx.y * 64, q1 = q0 + 64 < total ? q0 + 64 : total;
    double a0 = 0.0, a1 = 0.0;
    for (long long q = q0; q < q1; ++q) {
        const int s = (int)(q / p.n), j = (int)(q % p.n);
        if (!((p.sel >> j) & 1ull)) continue;
        const long long br = (long long)s * p.L + p.j0 + j;
        const float dy = p.dY[(p.dy_compact ? q : br) * p.ldy + c];
        a0 += (double)dy;
        if (p.X) {
            const float xh = (p.X[br * p.C + c] - p.st[2 * q]) * p.st[2 * q + 1];
            a1 += (double)(dy * xh);
        }
    }
    p.part[((size_t)blockIdx.y * 2) * p.C + c] = a0;
    p.part[((size_t)blockIdx.y * 2 + 1) * p.C + c] = a1;
}

__global__ __launch_bounds__(256) void mg_colsum_fin_kernel(ColG p) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= p.C) return;
    double a0 = 0.0, a1 = 0.0;
    for (int k = 0; k < p.chunks; ++k) {
        a0 += p.part[((size_t)k * 2) * p.C + c];
        a1 += p.part[((size_t)k * 2 + 1) * p.C + c];
    }
    p.out0[c] = (float)a0;
    if (p.out1) p.out1[c] = (float)a1;
}

// ------------------------------------------------------------------------------------------------ attention
// (the bodies: mtm_grad_body.h)
// one wavefront per (b, head, query i): lane owns the keys lane, lane + 64, ...; L <= 256
__global__ __launch_bounds__(256) void mg_attn_fwd_kernel(AttG p) { mg_attn_fwd_body<false>(p); }

// one wavefront per (b, head, key j): out[j][e] = alpha sum_i M[i][j] Z[i][e], queries ascending.  which 0: dV = P^T dO; 1: dK = dS^T Q scale
__global__ __launch_bounds__(256) void mg_attn_col_kernel(AttG p, int which) { mg_attn_col_body<false>(p, which); }

// one wavefront per (b, head, query i): dP = dO V^T, dS = P (dP - sum_j dP P) over P in place, dQ = dS K scale (keys ascending)
__global__ __launch_bounds__(256) void mg_attn_row_kernel(AttG p) { mg_attn_row_body<false>(p); }

// ------------------------------------------------------------------------------------------------ embedding, gather, scatter
// encoder row j -> (key, timestep): the keys in order, the visible timesteps of each ascending
__device__ __forceinline__ void enc_row_token(const EmbG& p, int j, int* k_out, int* t_out) {
    int k = 0;
    while (k < 3 && j >= p.kept[k]) j -= p.kept[k++];
    u64 m = p.bits[k];
    for (int i = 0; i < j; ++i) m &= m - 1;
    *k_out = k;
    *t_out = __ffsll((long long)m) - 1;
}

__global__ __launch_bounds__(256) void mg_embed_kernel(EmbG p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)p.B * p.Le * p.d) return;
    const int n = (int)(i % p.d), j = (int)((i / p.d) % p.Le), b = (int)(i / ((long long)p.d * p.Le));
    int k, t;
    enc_row_token(p, j, &k, &t);
    const int F = p.feat[k];
    const float* x = p.tok[k] + ((size_t)b * p.T + t) * F;
    const float* w = p.W[k] + (size_t)n * F;
    float a = 0.f;
    for (int f = 0; f < F; ++f) a += x[f] * w[f];
    p.X[i] = ((a + p.bias[k][n]) + p.pdim[k][n]) + p.pos[(size_t)t * p.d + n];
}

// decoder embedding input (b, k, t): the encoder output row of a visible token, the key's mask token of a hidden one
__global__ __launch_bounds__(256) void mg_gather_kernel(EmbG p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)p.B * 4 * p.T * p.d) return;
    const int n = (int)(i % p.d), r = (int)((i / p.d) % (4 * p.T)), b = (int)(i / ((long long)p.d * 4 * p.T));
    const int k = r / p.T, t = r % p.T;
    float v;
    if ((p.bits[k] >> t) & 1ull) {
        const int j = p.eoff[k] + __popcll(p.bits[k] & ((1ull << t) - 1ull));
        v = p.src[((size_t)b * p.Le + j) * p.d + n];
    } else {
        v = p.mtok[k][n];
    }
    p.dst[i] = v;
}

__global__ __launch_bounds__(256) void mg_scatter_kernel(EmbG p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)p.B * p.Le * p.d) return;
    const int n = (int)(i % p.d), j = (int)((i / p.d) % p.Le), b = (int)(i / ((long long)p.d * p.Le));
    int k, t;
    enc_row_token(p, j, &k, &t);
    p.dst[i] = p.src[((size_t)b * 4 * p.T + (size_t)k * p.T + t) * p.d + n];
}

// the visible token rows of key k, compact: out[b kept + i][f] = tok_k[b, t_i][f] (the B operand of the encoder embedding's dW product)
__global__ __launch_bounds__(256) void mg_tokv_kernel(EmbG p, int k, float* out) {
    const int F = p.feat[k], kept = p.kept[k];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)p.B * kept * F) return;
    const int f = (int)(i % F), ii = (int)((i / F) % kept), b = (int)(i / ((long long)F * kept));
    u64 m = p.bits[k];
    for (int q = 0; q < ii; ++q) m &= m - 1;
    const int t = __ffsll((long long)m) - 1;
    out[i] = p.tok[k][((size_t)b * p.T + t) * F + f];
}

// ------------------------------------------------------------------------------------------------ the action head's std, the loss backward
__global__ __launch_bounds__(256) void mg_std_kernel(const float* ls, float* sd, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) sd[i] = expf(-5.0f + 3.5f * (tanhf(ls[i]) + 1.0f));
}

// one thread per (row, feature) of the S + 2 + A head outputs.  The targets, the clipped action and its z are constants.
//   key k != actions in loss_keys:  dpred = 2 (pred - t') / (B T D)
//   actions:  dmu  = [bit] 2 (tanh mu - a) m (1 - tanh^2 mu) / (B T A)  -  hid ((z - mu) / var) / cnt  +  hid er 2 tanh(u) / cnt
//             dstd = - hid ((z - mu)^2 / std^3 - 1 / std) / cnt  +  hid er (2 tanh(u) eps - 1 / std) / cnt      (u = mu + std eps)
//             d log_std-Linear = dstd std 3.5 (1 - tanh^2(ls))
__global__ __launch_bounds__(256) void mg_loss_bwd_kernel(LossBwdG p) {
    const int W = p.S + 2 + p.A;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long rows = (long long)p.batch * p.T;
    if (i >= rows * W) return;
    const int c = (int)(i % W);
    const long long r = i / W;
    const int t = (int)(r % p.T);
    if (c < p.S + 2) {
        const int j = c < p.S ? 0 : c - p.S + 1, k = j == 0 ? M3PC_STATES : j == 1 ? M3PC_REWARDS : M3PC_RETURNS;
        const int D = j == 0 ? p.S : 1, e = j == 0 ? c : 0;
        float g = 0.f;
        if ((p.loss_keys >> k) & 1) {
            const float* tg = p.tgt[k] + r * D;
            float tv = tg[e];
            if (p.flags & M3PC_MTM_NORM_L2) {
                double n2 = 0.0;
                for (int q = 0; q < D; ++q) n2 += (double)(tg[q] * tg[q]);
                tv = tv / sqrtf((float)n2);
            }
            g = 2.0f * (p.pred[j][r * D + e] - tv) / (float)((double)rows * D);
        }
        p.dpred[j][r * D + e] = g;
        return;
    }
    const int e = c - p.S - 2;
    const long long at = r * p.A + e;
    const float mu = p.mu[at], sd = p.sd[at], a = p.tgt[M3PC_ACTIONS][at];
    const bool vis = (p.mask[M3PC_ACTIONS] >> t) & 1ull;
    float dmu = 0.f, dsd = 0.f;
    if (vis) {
        if ((p.loss_keys >> M3PC_ACTIONS) & 1) {
            const float th = tanhf(mu);
            dmu = 2.0f * (th - a) * (1.0f - th * th) / (float)((double)rows * p.A);
        }
    } else {
        const float lo = (float)(-1.0 + 1e-6), hi = (float)(1.0 - 1e-6);
        float ac = a;
        if ((p.flags & M3PC_MTM_CLIP_ACTIONS) && a == a) ac = fminf(fmaxf(a, lo), hi);
        const float z = 0.5f * (log1pf(ac) - log1pf(-ac));
        const float dz = z - mu, var = sd * sd, eps = p.eps[at];
        const float th = tanhf(mu + eps * sd), er = p.entropy_reg_p ? *p.entropy_reg_p : p.entropy_reg;
        dmu = (er * 2.0f * th - dz / var) * p.inv_cnt;
        dsd = (er * (2.0f * th * eps - 1.0f / sd) - (dz * dz / (var * sd) - 1.0f / sd)) * p.inv_cnt;
    }
    const float tl = tanhf(p.ls[at]);
    p.dmu[at] = dmu;
    p.dls[at] = dsd * sd * 3.5f * (1.0f - tl * tl);
}

constexpr size_t al64(size_t n) { return (n + 63) & ~(size_t)63; }

unsigned blocks256(long long n) { return (unsigned)((n + 255) / 256); }
// one wavefront per item, four to a workgroup
unsigned blocks4(long long n) { return (unsigned)((n + 3) / 4); }

}  // namespace

#ifdef M3PC_LAB
thread_local int g_mg_picked = 0;
thread_local unsigned int g_mg_picked_set = 0;
#endif

// ------------------------------------------------------------------------------------------------ the launchers (mtm_grad.h)
void mg_launch_gemm(GemmG& p, hipStream_t st) {
    const long long tiles = (long long)((p.M + 31) / 32) * ((p.N + 31) / 32);
    if (tiles <= 0) return;
    for (GOp* op : {&p.A, &p.B})
        op->vec = op->s_k == 1 && !op->map_k && op->s_o % 4 == 0 && ((uintptr_t)op->p & 15) == 0 ? 1 : 0;
    if (p.drop.thr) return mg_launch_gemm_drop(p, st);  // (mtm_dropout.hip; never with splitk)
    if (p.splitk) {
        M3PC_MG_PICK(2);
        hipLaunchKernelGGL(mg_gemm_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, st, p);
    } else {
        M3PC_MG_PICK(1);
        hipLaunchKernelGGL(mg_gemm_kernel<false>, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, st, p);
    }
}

void mg_launch_ln_fwd(const LnG& p, hipStream_t st) {
    M3PC_MG_PICK(3);
    hipLaunchKernelGGL(mg_ln_fwd_kernel, dim3(blocks4(p.rows)), dim3(256), 0, st, p);
}
void mg_launch_ln_bwd(const LnG& p, hipStream_t st) {
    M3PC_MG_PICK(4);
    hipLaunchKernelGGL(mg_ln_bwd_kernel, dim3(blocks4(p.rows)), dim3(256), 0, st, p);
}

void mg_launch_colsum(ColG& p, double* scratch, hipStream_t st) {
    const long long total = (long long)p.nseq * p.n;
    if (total <= 0) return;  // (the gradient buffers start as zeros)
    p.part = scratch;
    p.chunks = mg_colsum_chunks(total);
    M3PC_MG_PICK(5);
    hipLaunchKernelGGL(mg_colsum_kernel, dim3((p.C + 255) / 256, p.chunks), dim3(256), 0, st, p);
    M3PC_MG_PICK(6);
    hipLaunchKernelGGL(mg_colsum_fin_kernel, dim3((p.C + 255) / 256), dim3(256), 0, st, p);
}

void mg_launch_attn_fwd(const AttG& p, hipStream_t st) {
    if (p.drop.thr) return mg_launch_attn_fwd_drop(p, st);
    M3PC_MG_PICK(7);
    hipLaunchKernelGGL(mg_attn_fwd_kernel, dim3(blocks4((long long)p.B * p.nh * p.L)), dim3(256), 0, st, p);
}
void mg_launch_attn_col(const AttG& p, int which, hipStream_t st) {
    if (p.drop.thr && which == 0) return mg_launch_attn_col_drop(p, st);  // (dK reads dS: the launch without dropout)
    M3PC_MG_PICK(8);
    hipLaunchKernelGGL(mg_attn_col_kernel, dim3(blocks4((long long)p.B * p.nh * p.L)), dim3(256), 0, st, p, which);
}
void mg_launch_attn_row(const AttG& p, hipStream_t st) {
    if (p.drop.thr) return mg_launch_attn_row_drop(p, st);
    M3PC_MG_PICK(9);
    hipLaunchKernelGGL(mg_attn_row_kernel, dim3(blocks4((long long)p.B * p.nh * p.L)), dim3(256), 0, st, p);
}

void mg_launch_embed(const EmbG& p, hipStream_t st) {
    M3PC_MG_PICK(10);
    hipLaunchKernelGGL(mg_embed_kernel, dim3(blocks256((long long)p.B * p.Le * p.d)), dim3(256), 0, st, p);
}
void mg_launch_gather(const EmbG& p, hipStream_t st) {
    M3PC_MG_PICK(11);
    hipLaunchKernelGGL(mg_gather_kernel, dim3(blocks256((long long)p.B * 4 * p.T * p.d)), dim3(256), 0, st, p);
}
void mg_launch_scatter(const EmbG& p, hipStream_t st) {
    M3PC_MG_PICK(12);
    hipLaunchKernelGGL(mg_scatter_kernel, dim3(blocks256((long long)p.B * p.Le * p.d)), dim3(256), 0, st, p);
}
void mg_launch_tokv(const EmbG& p, int k, float* out, hipStream_t st) {
    M3PC_MG_PICK(13);
    hipLaunchKernelGGL(mg_tokv_kernel, dim3(blocks256((long long)p.B * p.kept[k] * p.feat[k])), dim3(256), 0, st, p, k, out);
}

void mg_launch_std(const float* ls, float* sd, long long n, hipStream_t st) {
    M3PC_MG_PICK(14);
    hipLaunchKernelGGL(mg_std_kernel, dim3(blocks256(n)), dim3(256), 0, st, ls, sd, n);
}
void mg_launch_loss_bwd(const LossBwdG& p, hipStream_t st) {
    M3PC_MG_PICK(15);
    hipLaunchKernelGGL(mg_loss_bwd_kernel, dim3(blocks256((long long)p.batch * p.T * (p.S + 2 + p.A))), dim3(256), 0, st, p);
}

}  // namespace m3pc

namespace m3pc {
namespace {

using Obj = struct m3pc_mtm_grad;

// one pass over the buffers: count (base == nullptr) or assign
size_t mg_layout(Obj* g, float* base) {
    const m3pc_handle* h = g->h;
    const size_t B = (size_t)g->max_batch, T = (size_t)h->T, d = (size_t)h->d, ff = (size_t)h->ff, L = 4 * T, R = B * L, RT = B * T;
    const size_t S = (size_t)h->S, A = (size_t)h->A;
    size_t at = 0;
    auto take = [&](float** p, size_t n) {
        if (base) *p = base + at;
        at += al64(n);
    };
    take(&g->grad, g->grad_floats);
    const int nl = h->dm.n_enc_layer + h->dm.n_dec_layer;
    if (base) g->lay.resize(nl);
    Obj::Lay tmp;
    for (int l = 0; l < nl; ++l) {
        Obj::Lay& y = base ? g->lay[l] : tmp;
        take(&y.Xin, R * d);
        take(&y.Hn1, R * d);
        take(&y.QKV, R * 3 * d);
        take(&y.P, R * h->nh * L);
        take(&y.O, R * d);
        take(&y.X1, R * d);
        take(&y.Hn2, R * d);
        take(&y.Fpre, R * ff);
        take(&y.Fact, R * ff);
        take(&y.st1, R * 2);
        take(&y.st2, R * 2);
    }
    take(&g->XencOut, R * d);
    take(&g->EncN, R * d);
    take(&g->st_enc, R * 2);
    take(&g->Zin, R * d);
    take(&g->XdecOut, R * d);
    take(&g->DecN, R * d);
    take(&g->st_dec, R * 2);
    for (int k = 0; k < 4; ++k) take(&g->s.tok[k], RT * h->feat[k]);
    for (int k = 0; k < 3; ++k) take(&g->s.raw[k], RT * h->feat[k]);
    take(&g->s.eps, RT * A);
    const size_t hw[3] = {S, 1, 1};
    for (int j = 0; j < 3; ++j) {
        take(&g->Hh[j], RT * d);
        take(&g->st_h[j], RT * 2);
        take(&g->Hpre[j], RT * d);
        take(&g->Hact[j], RT * d);
        take(&g->pred[j], RT * hw[j]);
        take(&g->dpred[j], RT * hw[j]);
    }
    take(&g->mu, RT * A);
    take(&g->ls, RT * A);
    take(&g->sd, RT * A);
    take(&g->dmu, RT * A);
    take(&g->dls, RT * A);
    take(&g->dX, R * d);
    take(&g->dH, R * d);
    take(&g->dQKV, R * 3 * d);
    take(&g->dF, R * ff);
    take(&g->dO, R * d);
    take(&g->dh1, RT * d);
    take(&g->dh2, RT * d);
    take(&g->rec, M3PC_MTM_LOSS_FLOATS);
    return at;
}

}  // namespace

int mg_ensure(Obj* g) {
    m3pc_handle* h = g->h;
    HIPCHK(hipSetDevice(h->device));
    if (g->ready) return 0;
    const size_t n = mg_layout(g, nullptr);
    if (!g->arena) CHK(dmalloc(&g->arena, n));  // (a call that failed at the second allocation left the first: it is kept, not leaked)
    mg_layout(g, g->arena);
    const size_t RT = (size_t)g->max_batch * h->T, R = 4 * RT;
    const size_t C = (size_t)std::max(3 * h->d, h->ff);
    const size_t n64 = al64(RT) + al64(RT * MTM_LOSS_PART) + mg_colsum_doubles((long long)R, (int)C);  // (no column sum has more rows than R)
    if (!g->arena64) CHK(dmalloc(&g->arena64, n64));
    g->s.raw_returns = g->arena64;
    g->s.part = g->s.raw_returns + al64(RT);
    g->colpart = g->s.part + al64(RT * MTM_LOSS_PART);
    g->ready = true;
    return 0;
}

namespace {

struct Run {
    Obj* g;
    m3pc_handle* h;
    hipStream_t st;
    int B, T, d, ff, Le;
    u64 bits[4];
    int kept[4], eoff[4];
    DropG drop;  // this call's draw (thr == 0: no dropout); c3 is set per site
    // site s of layer li on an (R, C) matrix (s 1, 2, 3) or on the attention probabilities (s 0)
    DropG site(int li, int s) const {
        DropG x = drop;
        x.c3 = (s == 0 ? MG_DROP_ATTN : MG_DROP_MATRIX) | (unsigned int)(4 * li + s) << 8;
        return x;
    }
    float* Wt(const std::string& n) const { return W(h, n).f; }
    float* Gr(const std::string& n) const { return g->grad + g->par[g->idx.at(n)].off; }
};

const RMap NOMAP = {0, 0, 0};

void run_gemm(const Run& r, GemmG& p) { mg_launch_gemm(p, r.st); }
GemmG gemm_zero() {
    GemmG p;
    memset(&p, 0, sizeof(p));
    return p;
}
// C (M, N) = X (M, K) Wt (N, K)^T
GemmG gemm_fwd(const float* X, long long ldx, RMap xmap, const float* Wt, int M, int N, int K, float* C, long long ldc, RMap cmap, const float* bias) {
    GemmG p = gemm_zero();
    p.A = {X, ldx, 1, xmap, 0, 0};
    p.B = {Wt, (long long)K, 1, NOMAP, 0, 0};
    p.C = C;
    p.ldc = ldc;
    p.cmap = cmap;
    p.M = M;
    p.N = N;
    p.K = K;
    p.bias = bias;
    return p;
}
// dX (M, N) = dY (M, K) Wt (K, N)
GemmG gemm_dx(const float* dY, long long ldy, RMap ymap, const float* Wt, int M, int N, int K, float* C, long long ldc, RMap cmap) {
    GemmG p = gemm_zero();
    p.A = {dY, ldy, 1, ymap, 0, 0};
    p.B = {Wt, 1, (long long)N, NOMAP, 0, 0};
    p.C = C;
    p.ldc = ldc;
    p.cmap = cmap;
    p.M = M;
    p.N = N;
    p.K = K;
    return p;
}
// dW (M, N) = dY (rows, M)^T X (rows, N)
GemmG gemm_dw(const float* dY, long long ldy, RMap ymap, const float* X, long long ldx, RMap xmap, int M, int N, int rows, float* C) {
    GemmG p = gemm_zero();
    p.A = {dY, 1, ldy, ymap, 1, 0};
    p.B = {X, 1, ldx, xmap, 1, 0};
    p.splitk = 1;
    p.C = C;
    p.ldc = N;
    p.cmap = NOMAP;
    p.M = M;
    p.N = N;
    p.K = rows;
    return p;
}

void run_ln_fwd(const Run& r, const float* X, RMap xmap, const std::string& name, float* Y, float* st, int rows) {
    LnG p;
    memset(&p, 0, sizeof(p));
    p.X = X;
    p.xmap = xmap;
    p.g = r.Wt(name + ".weight");
    p.b = r.Wt(name + ".bias");
    p.Y = Y;
    p.st = st;
    p.rows = rows;
    p.d = r.d;
    mg_launch_ln_fwd(p, r.st);
}

// sums over the rows (s, j) (ColG) of dY into out0 and, with X / st, of dY xhat into out1
void run_colsum(const Run& r, const float* dY, bool dy_compact, long long ldy, const float* X, const float* st, int nseq, int L, int j0, int n,
                u64 sel, int C, float* out0, float* out1) {
    ColG p;
    memset(&p, 0, sizeof(p));
    p.dY = dY;
    p.dy_compact = dy_compact ? 1 : 0;
    p.ldy = ldy;
    p.X = X;
    p.st = st;
    p.nseq = nseq;
    p.L = L;
    p.j0 = j0;
    p.n = n;
    p.sel = sel;
    p.C = C;
    p.out0 = out0;
    p.out1 = out1;
    mg_launch_colsum(p, r.g->colpart, r.st);
}
void run_colsum_rows(const Run& r, const float* dY, int rows, int C, float* out0) {
    run_colsum(r, dY, false, C, nullptr, nullptr, rows, 1, 0, 1, ~0ull, C, out0, nullptr);
}

// LayerNorm `name` backward over `rows` compact rows of dY: the weight / bias gradients, and dX (rows xmap(r)) = or += the input's
void run_ln_bwd(const Run& r, const float* dY, const float* X, RMap xmap, const float* st, const std::string& name, float* dX, int rows,
                bool accumulate) {
    if (xmap.rpg == 0)
        run_colsum(r, dY, false, r.d, X, st, rows, 1, 0, 1, ~0ull, r.d, r.Gr(name + ".bias"), r.Gr(name + ".weight"));
    else
        run_colsum(r, dY, true, r.d, X, st, rows / xmap.rpg, xmap.gstride, xmap.off, xmap.rpg, ~0ull, r.d, r.Gr(name + ".bias"),
                   r.Gr(name + ".weight"));
    LnG p;
    memset(&p, 0, sizeof(p));
    p.X = X;
    p.xmap = xmap;
    p.g = r.Wt(name + ".weight");
    p.st = const_cast<float*>(st);
    p.dY = dY;
    p.dX = dX;
    p.rows = rows;
    p.d = r.d;
    p.accumulate = accumulate ? 1 : 0;
    mg_launch_ln_bwd(p, r.st);
}

AttG att_params(const Run& r, const Obj::Lay& y, int L, int li) {
    AttG a;
    memset(&a, 0, sizeof(a));
    a.QKV = y.QKV;
    a.P = y.P;
    a.O = y.O;
    a.dO = r.g->dO;
    a.dQKV = r.g->dQKV;
    a.B = r.B;
    a.L = L;
    a.d = r.d;
    a.nh = r.h->nh;
    a.hd = r.h->hd;
    a.scale = 1.0f / sqrtf((float)r.h->hd);
    a.drop = r.site(li, 0);
    return a;
}

// li: the layer's index in g->lay (the dropout sites 4 li + s; mtm_grad.h, DROPOUT)
void block_fwd(const Run& r, const std::string& pfx, const Obj::Lay& y, float* Xout, int L, int li) {
    const int R = r.B * L, d = r.d, ff = r.ff;
    run_ln_fwd(r, y.Xin, NOMAP, pfx + ".norm1", y.Hn1, y.st1, R);
    GemmG p = gemm_fwd(y.Hn1, d, NOMAP, r.Wt(pfx + ".self_attn.in_proj_weight"), R, 3 * d, d, y.QKV, 3 * d, NOMAP, r.Wt(pfx + ".self_attn.in_proj_bias"));
    run_gemm(r, p);
    const AttG a = att_params(r, y, L, li);
    mg_launch_attn_fwd(a, r.st);
    p = gemm_fwd(y.O, d, NOMAP, r.Wt(pfx + ".self_attn.out_proj.weight"), R, d, d, y.X1, d, NOMAP, r.Wt(pfx + ".self_attn.out_proj.bias"));
    p.res = y.Xin;
    p.drop = r.site(li, 1);
    run_gemm(r, p);
    run_ln_fwd(r, y.X1, NOMAP, pfx + ".norm2", y.Hn2, y.st2, R);
    p = gemm_fwd(y.Hn2, d, NOMAP, r.Wt(pfx + ".linear1.weight"), R, ff, d, y.Fpre, ff, NOMAP, r.Wt(pfx + ".linear1.bias"));
    p.gelu_out = y.Fact;
    p.drop = r.site(li, 2);
    run_gemm(r, p);
    p = gemm_fwd(y.Fact, ff, NOMAP, r.Wt(pfx + ".linear2.weight"), R, d, ff, Xout, d, NOMAP, r.Wt(pfx + ".linear2.bias"));
    p.res = y.X1;
    p.drop = r.site(li, 3);
    run_gemm(r, p);
}

// dY = dX * k of site (li, s) over (R, d) rows into `into`; without dropout dX itself
const float* drop_rows(const Run& r, int li, int s, int R, float* into) {
    if (!r.drop.thr) return r.g->dX;
    const DropRowsG p = {r.g->dX, into, R, r.d, r.site(li, s)};
    mg_launch_drop_rows(p, r.st);
    return into;
}

// g->dX: in, the gradient of the block's output; out, of its input
void block_bwd(const Run& r, const std::string& pfx, const Obj::Lay& y, int L, int li) {
    Obj* g = r.g;
    const int R = r.B * L, d = r.d, ff = r.ff;
    const float* dY = drop_rows(r, li, 3, R, g->dO);  // (dO is free until the out_proj dX product below)
    GemmG p = gemm_dx(dY, d, NOMAP, r.Wt(pfx + ".linear2.weight"), R, ff, d, g->dF, ff, NOMAP);
    p.gelu_aux = y.Fpre;
    p.drop = r.site(li, 2);
    run_gemm(r, p);
    p = gemm_dw(dY, d, NOMAP, y.Fact, ff, NOMAP, d, ff, R, r.Gr(pfx + ".linear2.weight"));
    run_gemm(r, p);
    run_colsum_rows(r, dY, R, d, r.Gr(pfx + ".linear2.bias"));
    p = gemm_dx(g->dF, ff, NOMAP, r.Wt(pfx + ".linear1.weight"), R, d, ff, g->dH, d, NOMAP);
    run_gemm(r, p);
    p = gemm_dw(g->dF, ff, NOMAP, y.Hn2, d, NOMAP, ff, d, R, r.Gr(pfx + ".linear1.weight"));
    run_gemm(r, p);
    run_colsum_rows(r, g->dF, R, ff, r.Gr(pfx + ".linear1.bias"));
    run_ln_bwd(r, g->dH, y.X1, NOMAP, y.st2, pfx + ".norm2", g->dX, R, true);
    dY = drop_rows(r, li, 1, R, g->dH);  // (dH is free from the LayerNorm backward above to the Q|K|V dX product below)
    p = gemm_dx(dY, d, NOMAP, r.Wt(pfx + ".self_attn.out_proj.weight"), R, d, d, g->dO, d, NOMAP);
    run_gemm(r, p);
    p = gemm_dw(dY, d, NOMAP, y.O, d, NOMAP, d, d, R, r.Gr(pfx + ".self_attn.out_proj.weight"));
    run_gemm(r, p);
    run_colsum_rows(r, dY, R, d, r.Gr(pfx + ".self_attn.out_proj.bias"));
    const AttG a = att_params(r, y, L, li);
    mg_launch_attn_col(a, 0, r.st);
    mg_launch_attn_row(a, r.st);
    mg_launch_attn_col(a, 1, r.st);
    p = gemm_dx(g->dQKV, 3 * d, NOMAP, r.Wt(pfx + ".self_attn.in_proj_weight"), R, d, 3 * d, g->dH, d, NOMAP);
    run_gemm(r, p);
    p = gemm_dw(g->dQKV, 3 * d, NOMAP, y.Hn1, d, NOMAP, 3 * d, d, R, r.Gr(pfx + ".self_attn.in_proj_weight"));
    run_gemm(r, p);
    run_colsum_rows(r, g->dQKV, R, 3 * d, r.Gr(pfx + ".self_attn.in_proj_bias"));
    run_ln_bwd(r, g->dH, y.Xin, NOMAP, y.st1, pfx + ".norm1", g->dX, R, true);
}

EmbG emb_params(const Run& r) {
    EmbG e;
    memset(&e, 0, sizeof(e));
    for (int k = 0; k < 4; ++k) {
        const std::string kn = KEYN[k];
        e.tok[k] = r.g->s.tok[k];
        e.W[k] = r.Wt("encoder_embed_dict." + kn + ".weight");
        e.bias[k] = r.Wt("encoder_embed_dict." + kn + ".bias");
        e.pdim[k] = r.Wt("encoder_per_dim_encoding." + kn);
        e.mtok[k] = r.Wt("mask_token_dict." + kn);
        e.bits[k] = r.bits[k];
        e.kept[k] = r.kept[k];
        e.eoff[k] = r.eoff[k];
        e.feat[k] = r.h->feat[k];
    }
    e.pos = r.Wt("pos_embed");
    e.B = r.B;
    e.T = r.T;
    e.d = r.d;
    e.Le = r.Le;
    return e;
}

}  // namespace

// everything behind the refusals: the batch is in raw rows, the masks are bits
int mg_run(Obj* g, int batch, const float* states, const float* actions, const float* rewards, const void* returns, int returns_f64,
           const u64 bits[4], const float* eps, float entropy_reg, const float* entropy_reg_p, int flags, int loss_keys, float* record, hipStream_t st) {
    m3pc_handle* h = g->h;
    Run r;
    r.g = g;
    r.h = h;
    r.st = st;
    r.B = batch;
    r.T = h->T;
    r.d = h->d;
    r.ff = h->ff;
    r.Le = 0;
    memset(&r.drop, 0, sizeof(r.drop));
    if (g->drop_p > 0.0) {  // (every refusal lies before this call)
        const DropG dg = mg_drop_make(g->drop_p, g->drop_seed, g->drop_draw);
        if (dg.thr) {  // (p below 2^-32 drops nothing: no launch differs and the draw stays)
            r.drop = dg;
            ++g->drop_draw;
        }
    }
    for (int k = 0; k < 4; ++k) {
        r.bits[k] = bits[k];
        r.kept[k] = __builtin_popcountll(bits[k]);
        r.eoff[k] = r.Le;
        r.Le += r.kept[k];
    }
    const int T = r.T, d = r.d, S = h->S, A = h->A, L4 = 4 * T, RT = batch * T, Rd = batch * L4, Re = batch * r.Le;
    const int nE = h->dm.n_enc_layer, nD = h->dm.n_dec_layer;
    const int HK[3] = {M3PC_STATES, M3PC_REWARDS, M3PC_RETURNS};
    HIPCHK(hipMemsetAsync(g->grad, 0, g->grad_floats * sizeof(float), st));

    // ---------------- forward
    mb_tokenize(h, g->s, batch, states, actions, rewards, returns, returns_f64, st);
    EmbG e = emb_params(r);
    float* enc0 = nE ? g->lay[0].Xin : g->XencOut;
    e.X = enc0;
    mg_launch_embed(e, st);
    for (int l = 0; l < nE; ++l)
        block_fwd(r, "encoder.layers." + std::to_string(l), g->lay[l], l + 1 < nE ? g->lay[l + 1].Xin : g->XencOut, r.Le, l);
    run_ln_fwd(r, g->XencOut, NOMAP, "encoder.norm", g->EncN, g->st_enc, Re);
    e.src = g->EncN;
    e.dst = g->Zin;
    mg_launch_gather(e, st);
    float* dec0 = nD ? g->lay[nE].Xin : g->XdecOut;
    for (int k = 0; k < 4; ++k) {
        const std::string kn = KEYN[k];
        const RMap km = {T, L4, k * T};
        GemmG p = gemm_fwd(g->Zin, d, km, r.Wt("decoder_embed_dict." + kn + ".weight"), RT, d, d, dec0, d, km, r.Wt("decoder_embed_dict." + kn + ".bias"));
        p.bias2 = r.Wt("decoder_per_dim_encoding." + kn);
        p.pos = r.Wt("pos_embed");
        p.pos_T = T;
        run_gemm(r, p);
    }
    for (int l = 0; l < nD; ++l)
        block_fwd(r, "decoder.layers." + std::to_string(l), g->lay[nE + l], l + 1 < nD ? g->lay[nE + l + 1].Xin : g->XdecOut, L4, nE + l);
    run_ln_fwd(r, g->XdecOut, NOMAP, "decoder.norm", g->DecN, g->st_dec, Rd);
    for (int j = 0; j < 3; ++j) {
        const int k = HK[j], F = h->feat[k];
        const std::string hn = std::string("output_head_dict.") + KEYN[k];
        const RMap km = {T, L4, k * T};
        run_ln_fwd(r, g->DecN, km, hn + ".0", g->Hh[j], g->st_h[j], RT);
        GemmG p = gemm_fwd(g->Hh[j], d, NOMAP, r.Wt(hn + ".1.weight"), RT, d, d, g->Hpre[j], d, NOMAP, r.Wt(hn + ".1.bias"));
        p.gelu_out = g->Hact[j];
        run_gemm(r, p);
        p = gemm_fwd(g->Hact[j], d, NOMAP, r.Wt(hn + ".3.weight"), RT, F, d, g->pred[j], F, NOMAP, r.Wt(hn + ".3.bias"));
        run_gemm(r, p);
    }
    const RMap am = {T, L4, M3PC_ACTIONS * T};
    {
        GemmG p = gemm_fwd(g->DecN, d, am, r.Wt("output_head_dict.actions.mu.weight"), RT, A, d, g->mu, A, NOMAP, r.Wt("output_head_dict.actions.mu.bias"));
        run_gemm(r, p);
        p = gemm_fwd(g->DecN, d, am, r.Wt("output_head_dict.actions.log_std.weight"), RT, A, d, g->ls, A, NOMAP, r.Wt("output_head_dict.actions.log_std.bias"));
        run_gemm(r, p);
        mg_launch_std(g->ls, g->sd, (long long)RT * A, st);
    }
    const float* const pred[5] = {g->pred[0], g->pred[1], g->pred[2], g->mu, g->sd};
    // (the optimizer reads the entropy in g->rec: a caller's buffer may be gone by then)
    mb_loss(h, g->s, batch, pred, g->s.tok, bits, eps, entropy_reg, entropy_reg_p, flags, loss_keys, g->rec, st);
    if (record) HIPCHK(hipMemcpyAsync(record, g->rec, M3PC_MTM_LOSS_FLOATS * sizeof(float), hipMemcpyDeviceToDevice, st));
    CHK(check_launch("mtm_grad forward"));

    // ---------------- backward
    {
        LossBwdG p;
        memset(&p, 0, sizeof(p));
        for (int j = 0; j < 3; ++j) {
            p.pred[j] = g->pred[j];
            p.dpred[j] = g->dpred[j];
        }
        p.mu = g->mu;
        p.sd = g->sd;
        p.ls = g->ls;
        p.eps = eps;
        p.dmu = g->dmu;
        p.dls = g->dls;
        for (int k = 0; k < 4; ++k) {
            p.tgt[k] = g->s.tok[k];
            p.mask[k] = bits[k];
        }
        p.batch = batch;
        p.T = T;
        p.S = S;
        p.A = A;
        p.flags = flags;
        p.loss_keys = loss_keys;
        p.entropy_reg = entropy_reg;
        p.entropy_reg_p = entropy_reg_p;
        p.inv_cnt = (float)(1.0 / ((double)batch * (double)(T - r.kept[M3PC_ACTIONS]) * (double)A));
        mg_launch_loss_bwd(p, st);
    }
    float* dDecN = g->dO;
    HIPCHK(hipMemsetAsync(dDecN, 0, (size_t)Rd * d * sizeof(float), st));
    for (int j = 0; j < 3; ++j) {
        const int k = HK[j], F = h->feat[k];
        if (!((loss_keys >> k) & 1)) continue;  // (a key outside loss_keys: its head's gradients stay the zeros they start as)
        const std::string hn = std::string("output_head_dict.") + KEYN[k];
        const RMap km = {T, L4, k * T};
        GemmG p = gemm_dx(g->dpred[j], F, NOMAP, r.Wt(hn + ".3.weight"), RT, d, F, g->dh1, d, NOMAP);
        p.gelu_aux = g->Hpre[j];
        run_gemm(r, p);
        p = gemm_dw(g->dpred[j], F, NOMAP, g->Hact[j], d, NOMAP, F, d, RT, r.Gr(hn + ".3.weight"));
        run_gemm(r, p);
        run_colsum_rows(r, g->dpred[j], RT, F, r.Gr(hn + ".3.bias"));
        p = gemm_dx(g->dh1, d, NOMAP, r.Wt(hn + ".1.weight"), RT, d, d, g->dh2, d, NOMAP);
        run_gemm(r, p);
        p = gemm_dw(g->dh1, d, NOMAP, g->Hh[j], d, NOMAP, d, d, RT, r.Gr(hn + ".1.weight"));
        run_gemm(r, p);
        run_colsum_rows(r, g->dh1, RT, d, r.Gr(hn + ".1.bias"));
        run_ln_bwd(r, g->dh2, g->DecN, km, g->st_h[j], hn + ".0", dDecN, RT, false);
    }
    {
        const std::string hm = "output_head_dict.actions.mu", hl = "output_head_dict.actions.log_std";
        GemmG p = gemm_dx(g->dmu, A, NOMAP, r.Wt(hm + ".weight"), RT, d, A, dDecN, d, am);
        run_gemm(r, p);
        p = gemm_dx(g->dls, A, NOMAP, r.Wt(hl + ".weight"), RT, d, A, dDecN, d, am);
        p.accumulate = 1;
        run_gemm(r, p);
        p = gemm_dw(g->dmu, A, NOMAP, g->DecN, d, am, A, d, RT, r.Gr(hm + ".weight"));
        run_gemm(r, p);
        p = gemm_dw(g->dls, A, NOMAP, g->DecN, d, am, A, d, RT, r.Gr(hl + ".weight"));
        run_gemm(r, p);
        run_colsum_rows(r, g->dmu, RT, A, r.Gr(hm + ".bias"));
        run_colsum_rows(r, g->dls, RT, A, r.Gr(hl + ".bias"));
    }
    run_ln_bwd(r, dDecN, g->XdecOut, NOMAP, g->st_dec, "decoder.norm", g->dX, Rd, false);
    for (int l = nD - 1; l >= 0; --l) block_bwd(r, "decoder.layers." + std::to_string(l), g->lay[nE + l], L4, nE + l);
    for (int k = 0; k < 4; ++k) {  // the decoder embedding: g->dX is the gradient of its output, g->dH becomes that of its input
        const std::string kn = KEYN[k];
        const RMap km = {T, L4, k * T};
        float* gb = r.Gr("decoder_embed_dict." + kn + ".bias");
        run_colsum(r, g->dX, false, d, nullptr, nullptr, batch, L4, k * T, T, ~0ull, d, gb, nullptr);
        HIPCHK(hipMemcpyAsync(r.Gr("decoder_per_dim_encoding." + kn), gb, (size_t)d * sizeof(float), hipMemcpyDeviceToDevice, st));
        GemmG p = gemm_dx(g->dX, d, km, r.Wt("decoder_embed_dict." + kn + ".weight"), RT, d, d, g->dH, d, km);
        run_gemm(r, p);
        p = gemm_dw(g->dX, d, km, g->Zin, d, km, d, d, RT, r.Gr("decoder_embed_dict." + kn + ".weight"));
        run_gemm(r, p);
        const u64 all = T == 64 ? ~0ull : (1ull << T) - 1ull, hidden = ~bits[k] & all;
        if (hidden) run_colsum(r, g->dH, false, d, nullptr, nullptr, batch, L4, k * T, T, hidden, d, r.Gr("mask_token_dict." + kn), nullptr);
    }
    float* dEncN = g->dO;
    e.src = g->dH;
    e.dst = dEncN;
    mg_launch_scatter(e, st);
    run_ln_bwd(r, dEncN, g->XencOut, NOMAP, g->st_enc, "encoder.norm", g->dX, Re, false);
    for (int l = nE - 1; l >= 0; --l) block_bwd(r, "encoder.layers." + std::to_string(l), g->lay[l], r.Le, l);
    for (int k = 0; k < 4; ++k) {
        if (!r.kept[k]) continue;  // (a fully hidden key: exact zeros)
        const std::string kn = KEYN[k];
        float* gb = r.Gr("encoder_embed_dict." + kn + ".bias");
        run_colsum(r, g->dX, false, d, nullptr, nullptr, batch, r.Le, r.eoff[k], r.kept[k], ~0ull, d, gb, nullptr);
        HIPCHK(hipMemcpyAsync(r.Gr("encoder_per_dim_encoding." + kn), gb, (size_t)d * sizeof(float), hipMemcpyDeviceToDevice, st));
        float* tokv = g->dF;  // (scratch: the layers are done with it)
        mg_launch_tokv(e, k, tokv, st);
        const RMap em = {r.kept[k], r.Le, r.eoff[k]};
        GemmG p = gemm_dw(g->dX, d, em, tokv, h->feat[k], NOMAP, d, h->feat[k], batch * r.kept[k], r.Gr("encoder_embed_dict." + kn + ".weight"));
        run_gemm(r, p);
    }
    CHK(check_launch("mtm_grad backward"));
    g->have_grad = true;
    g->consumed = false;
    g->last_loss_keys = loss_keys;
    return 0;
}

// the limits of the keep-mask counters (mtm_grad.h, DROPOUT); nothing to check without dropout.  (With the sizes
// m3pc_mtm_grad_create accepts -- max_batch 4 T max(3 d, ff) <= 2^31, head dim >= 32, L <= 256 -- no site reaches 2^32 quads: the
// second refusal is there for the day those limits move.)
static int mg_drop_check(const struct m3pc_mtm_grad* g, int batch, const char* who) {
    if (!(g->drop_p > 0.0)) return 0;
    const m3pc_handle* h = g->h;
    const int nl = h->dm.n_enc_layer + h->dm.n_dec_layer;
    if (nl > 64) return fail(M3PC_EINVAL, "%s: dropout numbers its sites 4 layer + s in 8 bits, the model has %d layers (> 64)", who, nl);
    const unsigned long long L = 4ull * h->T, R = (unsigned long long)batch * L, lim = 1ull << 32;
    const unsigned long long mq = ((R + 3) / 4) * (unsigned long long)std::max(h->d, h->ff), aq = R * h->nh * ((L + 3) / 4);
    if (mq > lim || aq > lim) return fail(M3PC_EINVAL, "%s: a dropout site of batch %d has more than 2^32 quads (%llu)", who, batch, std::max(mq, aq));
    return 0;
}

int mg_precheck(const struct m3pc_mtm_grad* g, int batch, const unsigned char* const masks[4], int flags, int loss_keys, const char* who,
                u64 bits[4]) {
    CHK(mb_check(g->h->dm, g->max_batch, batch, masks, flags, loss_keys, who, true, bits));
    CHK(mg_drop_check(g, batch, who));
    return mb_state(g->h, who);
}
int mg_precheck_replay(const struct m3pc_mtm_grad* g, m3pc_replay* rb, int batch, int mode, const int* traj_index, const int* start_index,
                       int index_on_device, const unsigned char* const masks[4], int flags, int loss_keys, const char* who, u64 bits[4]) {
    CHK(mb_check(g->h->dm, g->max_batch, batch, masks, flags, loss_keys, who, true, bits));
    CHK(mg_drop_check(g, batch, who));
    CHK(mb_fits(g->h, rb, who));
    CHK(replay_check_segments(rb, batch, mode, traj_index, start_index, index_on_device, who));
    return mb_state(g->h, who);
}

int mg_run_replay(struct m3pc_mtm_grad* g, m3pc_replay* rb, int batch, int mode, const int* traj_index, const int* start_index, int index_on_device,
                  unsigned long long seed, unsigned long long step, const u64 bits[4], const float* eps, float entropy_reg,
                  const float* entropy_reg_p, int flags, int loss_keys, float* record, int* out_traj, int* out_start, hipStream_t st,
                  const char* who) {
    const MtmStage& s = g->s;
    CHK(mb_draw(g->h, s, rb, batch, mode, traj_index, start_index, index_on_device, seed, step, &eps, out_traj, out_start, st, who));
    return mg_run(g, batch, s.raw[0], s.raw[1], s.raw[2], s.raw_returns, 1, bits, eps, entropy_reg, entropy_reg_p, flags, loss_keys, record, st);
}
}  // namespace m3pc

#pragma GCC visibility push(default)
extern "C" {

int m3pc_mtm_grad_create(m3pc_handle* h, int max_batch, struct m3pc_mtm_grad** out) {
    if (!h || !out) return fail(M3PC_EINVAL, "m3pc_mtm_grad_create: null argument");
    if (max_batch < 1) return fail(M3PC_EINVAL, "m3pc_mtm_grad_create: max_batch %d < 1", max_batch);
    if (h->T < 1 || h->T > 64 || h->hd < 1) return fail(M3PC_EINVAL, "m3pc_mtm_grad_create: traj_length %d outside [1, 64]", h->T);
    if ((long long)max_batch * 4 * h->T * std::max(3 * h->d, h->ff) > 0x7fffffffll)
        return fail(M3PC_EINVAL, "m3pc_mtm_grad_create: max_batch %d is too large for these sizes", max_batch);
    Obj* g = new Obj();
    g->h = h;
    g->max_batch = max_batch;
    size_t at = 0;
    for (auto& kv : h->w) {
        if (kv.first == "pos_embed") continue;
        g->idx[kv.first] = (int)g->par.size();
        g->par.push_back({kv.first, kv.second.numel, at});
        at += al64((size_t)kv.second.numel);
    }
    g->grad_floats = at;
    *out = g;
    return 0;
}

int m3pc_mtm_grad_destroy(struct m3pc_mtm_grad* g) {
    if (!g) return 0;
    if (g->arena || g->arena64) {
        (void)hipSetDevice(g->h->device);
        (void)hipDeviceSynchronize();
        if (g->arena) (void)hipFree(g->arena);
        if (g->arena64) (void)hipFree(g->arena64);
    }
    delete g;
    return 0;
}

int m3pc_mtm_grad(struct m3pc_mtm_grad* g, int batch, const float* states, const float* actions, const float* rewards, const void* returns,
                  int returns_f64, const unsigned char* const masks[4], const float* eps, float entropy_reg, int flags, int loss_keys,
                  float* record, void* stream) {
    if (!g || !states || !actions || !rewards || !returns || !masks || !eps) return fail(M3PC_EINVAL, "m3pc_mtm_grad: null argument");
    u64 bits[4];
    CHK(mg_precheck(g, batch, masks, flags, loss_keys, "m3pc_mtm_grad", bits));
    CHK(mg_ensure(g));
    return mg_run(g, batch, states, actions, rewards, returns, returns_f64, bits, eps, entropy_reg, nullptr, flags, loss_keys, record,
                  (hipStream_t)stream);
}

int m3pc_mtm_grad_replay(struct m3pc_mtm_grad* g, m3pc_replay* rb, int batch, int mode, const int* traj_index, const int* start_index,
                         int index_on_device, unsigned long long seed, unsigned long long step, const unsigned char* const masks[4],
                         const float* eps, float entropy_reg, int flags, int loss_keys, float* record, int* out_traj, int* out_start,
                         void* stream) {
    if (!g || !rb || !masks) return fail(M3PC_EINVAL, "m3pc_mtm_grad_replay: null argument");
    const char* who = "m3pc_mtm_grad_replay";
    u64 bits[4];
    CHK(mg_precheck_replay(g, rb, batch, mode, traj_index, start_index, index_on_device, masks, flags, loss_keys, who, bits));
    CHK(mg_ensure(g));
    return mg_run_replay(g, rb, batch, mode, traj_index, start_index, index_on_device, seed, step, bits, eps, entropy_reg, nullptr, flags,
                         loss_keys, record, out_traj, out_start, (hipStream_t)stream, who);
}

int m3pc_mtm_grad_set_dropout(struct m3pc_mtm_grad* g, double p, unsigned long long seed, unsigned long long draw) {
    if (!std::isfinite(p) || p < 0.0 || p >= 1.0) return fail(M3PC_EINVAL, "m3pc_mtm_grad_set_dropout: p %g is not a finite number in [0, 1)", p);
    if (!g) return fail(M3PC_EINVAL, "m3pc_mtm_grad_set_dropout: null g");
    g->drop_p = p;
    g->drop_seed = seed;
    g->drop_draw = draw;
    return 0;
}

int m3pc_mtm_grad_get_dropout(struct m3pc_mtm_grad* g, double* p, unsigned long long* seed, unsigned long long* next_draw) {
    if (!g) return fail(M3PC_EINVAL, "m3pc_mtm_grad_get_dropout: null g");
    if (p) *p = g->drop_p;
    if (seed) *seed = g->drop_seed;
    if (next_draw) *next_draw = g->drop_draw;
    return 0;
}

int m3pc_mtm_grad_export(struct m3pc_mtm_grad* g, const m3pc_named_tensor* tensors, int n, void* stream) {
    if (!g || !tensors || n < 0) return fail(M3PC_EINVAL, "m3pc_mtm_grad_export: null argument");
    auto par = [g](const char* name) {
        auto it = g->idx.find(name);
        return it == g->idx.end() ? nullptr : &g->par[it->second];
    };
    CHK(nt_check(tensors, n, [&](const char* name) { return par(name) ? par(name)->numel : -1ll; }, "m3pc_mtm_grad_export", "parameter"));
    if (!g->have_grad) return fail(M3PC_ESTATE, "m3pc_mtm_grad_export: no gradient call was made");
    HIPCHK(hipSetDevice(g->h->device));
    return nt_copy(tensors, n, true, [&](const char* name) { return g->grad + par(name)->off; }, (hipStream_t)stream);
}

}  // extern "C"
#pragma GCC visibility pop
