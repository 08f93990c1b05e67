// The IQL trainer (include/m3pc_hip.h: m3pc_iql_*): ImplicitQLearning.train (finetune_omtm/model.py:286-308) on the device -- V, the
// TwinQ with its target, and the Gaussian actor, trained from the transition batches of the replay buffer, and the TwinQ handed to
// the planner (m3pc_iql_publish_critic) device to device in the operand order of critic_pack (elementwise.hip).
//
// Every forward pass of train() reads pre-step parameters, so a step is: forwards, output deltas, backwards, updates --
//   1 iql_fwd1_kernel   layer 1 of the seven passes  vf(next_obs) vf(obs) q1t q2t q1 q2 actor     7 x row tiles x hidden / 32 waves
//   2 iql_fwd2_kernel   layer 2                                                                    the same grid
//   3 iql_fwd3_kernel   the output layer (tanh for the actor)                                      7 x row tiles waves
//   4 iql_loss_kernel   adv, the three losses, the output deltas, log_std's gradient and update    one block, a thread per row
//   5 iql_delta_kernel<2>  delta2 = (W3^T delta3) * relu'(h2)  of vf, q1, q2, actor                4 x row tiles x hidden / 32
//   6 iql_delta_kernel<1>  delta1 = (W2^T delta2) * relu'(h1)                                      the same grid
//   7 iql_grad_kernel   dW = delta^T activation (K = batch, ascending rows) and db = delta^T 1 per 32 x 32 tile; Adam, and for q1 /
//                       q2 the soft update of the target with the post-step value, in the epilogue of the wave that owns the tile
// seven launches, no host wait.  The layout is critic_mfma_kernel's: weights are the A operand, data rows the B operand, so a lane
// owns one data row (lane & 31) and accumulator i is output unit 8 (i / 4) + 4 (lane >> 5) + i % 4 of the tile.  Activations live in
// global memory as (pass, row, unit); rows beyond the batch in the last 32-row tile carry zero inputs and zero deltas, so they add
// exact zeros to every gradient.  iql.h states the arithmetic (the Adam order, what is fp64) and holds the parameter structures and the
// launchers every entry point goes through.
#include "device_util.h"
#include "iql.h"

namespace m3pc {
namespace {

__device__ __forceinline__ int train_pass(int t) { return t == 0 ? 1 : t + 3; }  // the forward pass a trained network's backward reads

// feature k of data row `row` of forward pass f: (s - obs_mean) / obs_std, then the action; zero beyond the width and the batch
__device__ __forceinline__ float load_x(const IqlP& p, int f, int in, int row, int k) {
    if (row >= p.B || k >= in) return 0.f;
    if (k < p.S) {
        const float* s = p.pass_next[f] ? p.next_state : p.state;
        return (s[(size_t)row * p.S + k] - p.om[k]) / p.os[k];
    }
    return p.action[(size_t)row * p.A + (k - p.S)];
}

__device__ __forceinline__ void adam_apply(const IqlP& p, int t, float g, float* pp, float* pm, float* pv) {
    float m = *pm, v = *pv;
    m = __fadd_rn(m, __fmul_rn(p.omb1, __fsub_rn(g, m)));
    v = __fadd_rn(__fmul_rn(p.b2, v), __fmul_rn(__fmul_rn(p.omb2, g), g));
    *pm = m;
    *pv = v;
    const double denom = sqrt((double)v) / p.sqrt_bc2 + p.eps;
    *pp = (float)((double)*pp - p.step_size[t] * (double)m / denom);
}

#if defined(__HIP_DEVICE_COMPILE__)
#define IQL_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)
#else
#define IQL_MFMA(a, b, c) ((void)(a), (void)(b), (c))
#endif

// layer 1: h1 = relu(W1 x + b1).  K = the input width padded to a multiple of 32, k pair {2 s, 2 s + 1} per step.
__global__ __launch_bounds__(256) void iql_fwd1_kernel(IqlP p) {
    const int lane = threadIdx.x & 63, l31 = lane & 31, lh = lane >> 5;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int ht = w % p.NT, rt = (w / p.NT) % p.RT, f = w / (p.NT * p.RT);
    if (f >= p.npass) return;
    const NetP n = p.net[p.pass_net[f]];
    const int row = 32 * rt + l31, m = 32 * ht + l31;
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 b = *(const f32x4*)(n.b1 + 32 * ht + 8 * q + 4 * lh);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[4 * q + i] = b[i];
    }
    const int K = (n.in + 31) & ~31;
    for (int s0 = 0; s0 < K / 2; s0 += 8) {  // (operands of eight steps are loaded ahead of their MFMAs)
        float a[8], b[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int k = 2 * (s0 + u) + lh;
            a[u] = k < n.in ? n.W1[(size_t)m * n.in + k] : 0.f;
            b[u] = load_x(p, f, n.in, row, k);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = IQL_MFMA(a[u], b[u], acc);
    }
    float* o = p.h1 + ((size_t)f * p.Bp + row) * p.H + 32 * ht + 4 * lh;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = fmaxf(acc[4 * q + i], 0.f);
        *(f32x4*)(o + 8 * q) = v;
    }
}

// layer 2: h2 = relu(W2 h1 + b2).  Step (g, j) multiplies the k pair {8 g + j, 8 g + 4 + j}, one per lane half, so that a lane
// reads four consecutive k of its weight row and of its data row per load (the pairing of critic_mfma_kernel).
__global__ __launch_bounds__(256) void iql_fwd2_kernel(IqlP p) {
    const int lane = threadIdx.x & 63, l31 = lane & 31, lh = lane >> 5;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int ht = w % p.NT, rt = (w / p.NT) % p.RT, f = w / (p.NT * p.RT);
    if (f >= p.npass) return;
    const NetP n = p.net[p.pass_net[f]];
    const int row = 32 * rt + l31, m = 32 * ht + l31, H = p.H;
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 b = *(const f32x4*)(n.b2 + 32 * ht + 8 * q + 4 * lh);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[4 * q + i] = b[i];
    }
    const float* ap = n.W2 + (size_t)m * H + 4 * lh;
    const float* bp = p.h1 + ((size_t)f * p.Bp + row) * H + 4 * lh;
    for (int g0 = 0; g0 < H / 8; g0 += 4) {  // (hidden / 8 is a multiple of 4: four groups are loaded ahead of their MFMAs)
        f32x4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = *(const f32x4*)(ap + 8 * (g0 + u));
            b[u] = *(const f32x4*)(bp + 8 * (g0 + u));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = IQL_MFMA(a[u][j], b[u][j], acc);
    }
    float* o = p.h2 + ((size_t)f * p.Bp + row) * H + 32 * ht + 4 * lh;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = fmaxf(acc[4 * q + i], 0.f);
        *(f32x4*)(o + 8 * q) = v;
    }
}

// the output layer: out = W3 h2 + b3 on one 32-unit tile (1 or A <= 32 units, the others zero); tanh for the actor
__global__ __launch_bounds__(256) void iql_fwd3_kernel(IqlP p) {
    const int lane = threadIdx.x & 63, l31 = lane & 31, lh = lane >> 5;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int rt = w % p.RT, f = w / p.RT;
    if (f >= p.npass) return;
    const int ni = p.pass_net[f];
    const NetP n = p.net[ni];
    const int row = 32 * rt + l31, H = p.H;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int o = 8 * (i / 4) + 4 * lh + i % 4;
        acc[i] = o < n.out ? n.b3[o] : 0.f;
    }
    const bool on = l31 < n.out;
    const float* ap = n.W3 + (size_t)(on ? l31 : 0) * H + 4 * lh;
    const float* bp = p.h2 + ((size_t)f * p.Bp + row) * H + 4 * lh;
    for (int g0 = 0; g0 < H / 8; g0 += 4) {
        f32x4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = *(const f32x4*)(ap + 8 * (g0 + u));
            b[u] = *(const f32x4*)(bp + 8 * (g0 + u));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = IQL_MFMA(on ? a[u][j] : 0.f, b[u][j], acc);
    }
    float* o = p.out + ((size_t)f * p.Bp + row) * IQL_OUTW + 4 * lh;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = ni == NET_ACTOR ? tanhf(acc[4 * q + i]) : acc[4 * q + i];
        *(f32x4*)(o + 8 * q) = v;
    }
}

// the sum of one value per thread of a 1024-thread block, by a fixed tree: xor butterflies within a wavefront, then the sixteen
// wavefront sums left to right.  Every thread returns the same bits.
__device__ __forceinline__ float iql_block_sum(float v, float* red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < IQL_MAX_BATCH / 64; ++i) s += red[i];
    __syncthreads();
    return s;
}

// Row r of the batch (model.py:228-284): adv = min(q1t, q2t) - v; value loss |tau - 1[adv < 0]| adv^2; targets = r + (1 - done) gamma
// next_v; q loss (mse(q1) + mse(q2)) / 2; actor loss min(exp(beta adv), 100) * -sum_a log N(a; mu, sigma).  The output deltas are the
// derivatives of the three MEANS (1 / batch included).  log_std: its gradient is summed here and its Adam step made here.
__global__ __launch_bounds__(IQL_MAX_BATCH) void iql_loss_kernel(IqlP p) {
    __shared__ float red[IQL_MAX_BATCH / 64];
    const int r = threadIdx.x, Bp = p.Bp;
    const bool on = r < p.B;
    const float inv_b = 1.f / (float)p.B;
    float vl = 0.f, q1l = 0.f, q2l = 0.f, dv = 0.f, dq1 = 0.f, dq2 = 0.f, ea = 0.f;
    if (on) {
        const float* o = p.out + (size_t)r * IQL_OUTW;
        const size_t ps = (size_t)Bp * IQL_OUTW;
        const float next_v = o[0], v = o[ps], qt = fminf(o[2 * ps], o[3 * ps]), q1 = o[4 * ps], q2 = o[5 * ps];
        const float adv = qt - v;
        const float wgt = fabsf(p.expectile - (adv < 0.f ? 1.f : 0.f));
        vl = wgt * adv * adv;
        dv = -2.f * wgt * adv * inv_b;
        const float target = p.reward[r] + (1.f - p.done[r]) * p.gamma * next_v;
        const float e1 = q1 - target, e2 = q2 - target;
        q1l = e1 * e1;
        q2l = e2 * e2;
        dq1 = e1 * inv_b;
        dq2 = e2 * inv_b;
        ea = fminf(expf(p.beta * adv), 100.f);
    }
    if (r < Bp) {
        const float d[3] = {dv, dq1, dq2};
        for (int t = 0; t < 3; ++t) {
            float* o = p.d3 + ((size_t)t * Bp + r) * IQL_OUTW;
            for (int c = 0; c < IQL_OUTW; ++c) o[c] = c == 0 ? d[t] : 0.f;
        }
    }
    float bc = 0.f, my_g = 0.f;
    float* da = p.d3 + ((size_t)NET_ACTOR * Bp + (r < Bp ? r : 0)) * IQL_OUTW;
    for (int a = 0; a < p.A; ++a) {
        const float ls = p.log_std[a];
        const float lsc = fminf(fmaxf(ls, -20.f), 2.f);
        const bool inside = ls >= -20.f && ls <= 2.f;
        const float sigma = expf(lsc), inv_var = 1.f / (sigma * sigma);
        float gls = 0.f, dz = 0.f;
        if (on) {
            const float mu = p.out[((size_t)6 * Bp + r) * IQL_OUTW + a];
            const float diff = p.action[(size_t)r * p.A + a] - mu;
            bc += 0.5f * diff * diff * inv_var + lsc + 0.91893853320467274f;
            const float wgt = ea * inv_b;
            dz = -wgt * diff * inv_var * (1.f - mu * mu);
            gls = inside ? wgt * (1.f - diff * diff * inv_var) : 0.f;
        }
        if (r < Bp) da[a] = dz;
        const float g = iql_block_sum(gls, red);
        if (r == a) my_g = g;
    }
    if (r < Bp)
        for (int a = p.A; a < IQL_OUTW; ++a) da[a] = 0.f;
    const float sv = iql_block_sum(vl, red), s1 = iql_block_sum(q1l, red), s2 = iql_block_sum(q2l, red), sa = iql_block_sum(on ? ea * bc : 0.f, red);
    if (r == 0 && p.losses) {
        p.losses[0] = sv / (float)p.B;
        p.losses[1] = (s1 / (float)p.B + s2 / (float)p.B) * 0.5f;
        p.losses[2] = sa / (float)p.B;
    }
    if (r < p.A) adam_apply(p, NET_ACTOR, my_g, p.log_std + r, p.ls_m + r, p.ls_v + r);
}

// L = 2: delta2 = (W3^T delta3) * relu'(h2), K = the output width (8 for one output, 32 for the actor's A <= 32);
// L = 1: delta1 = (W2^T delta2) * relu'(h1), K = hidden.  The A operand W[k][m] is read with consecutive lanes on consecutive m.
template <int L>
__global__ __launch_bounds__(256) void iql_delta_kernel(IqlP p) {
    const int lane = threadIdx.x & 63, l31 = lane & 31, lh = lane >> 5;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int ht = w % p.NT, rt = (w / p.NT) % p.RT, t = w / (p.NT * p.RT);
    if (t >= IQL_NETS) return;
    const NetP n = p.net[t];
    const int f = train_pass(t), row = 32 * rt + l31, m = 32 * ht + l31, H = p.H;
    const int K = L == 2 ? (n.out > 8 ? 32 : 8) : H;
    const int kmax = L == 2 ? n.out : H;
    const float* W = L == 2 ? n.W3 : n.W2;
    const float* bp = L == 2 ? p.d3 + ((size_t)t * p.Bp + row) * IQL_OUTW + 4 * lh : p.d2 + ((size_t)t * p.Bp + row) * H + 4 * lh;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int g = 0; g < K / 8; ++g) {
        const f32x4 b = *(const f32x4*)(bp + 8 * g);
        float a[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = 8 * g + 4 * lh + j;
            a[j] = k < kmax ? W[(size_t)k * H + m] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = IQL_MFMA(a[j], b[j], acc);
    }
    const float* act = (L == 2 ? p.h2 : p.h1) + ((size_t)f * p.Bp + row) * H + 32 * ht + 4 * lh;
    float* o = (L == 2 ? p.d2 : p.d1) + ((size_t)t * p.Bp + row) * H + 32 * ht + 4 * lh;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 hv = *(const f32x4*)(act + 8 * q);
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = hv[i] > 0.f ? acc[4 * q + i] : 0.f;
        *(f32x4*)(o + 8 * q) = v;
    }
}

// One wavefront per 32 x 32 tile of one gradient: dW[m][n] = sum over the rows of the batch, ascending, two per MFMA, of
// delta[row][m] * activation[row][n]; the tile behind the last column tile is the bias gradient: its "activation" is 1 in column
// (row / 2) % 32 and 0 elsewhere, so that column n sums every 32nd row pair in ascending order and the 32 columns are then added by a
// fixed butterfly -- two short levels instead of one chain as long as the batch, which a sum of same-signed terms needs.  The epilogue is
// the update: Adam on the element, then for q1 / q2 target <- (1 - tau) target + tau q with the post-step q (model.py:257-260).
__global__ __launch_bounds__(256) void iql_grad_kernel(IqlP p) {
    const int lane = threadIdx.x & 63, l31 = lane & 31, lh = lane >> 5;
    int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int NT = p.NT, H = p.H;
    int t = 0, c1 = 0, c2 = 0, NI = 0;
    for (; t < IQL_NETS; ++t) {
        NI = (p.net[t].in + 31) / 32;
        c1 = NT * (NI + 1);
        c2 = NT * (NT + 1);
        const int c = c1 + c2 + NT + 1;
        if (w < c) break;
        w -= c;
    }
    if (t >= IQL_NETS) return;
    const NetP n = p.net[t], am = p.am[t], av = p.av[t];
    const int f = train_pass(t);
    int layer, mt, nt, Mdim, Ndim, ldd;
    bool bias;
    const float* delta;
    if (w < c1) {
        layer = 1, mt = w / (NI + 1), nt = w % (NI + 1), bias = nt == NI, Mdim = H, Ndim = n.in, ldd = H;
        delta = p.d1 + (size_t)t * p.Bp * H;
    } else if (w < c1 + c2) {
        w -= c1;
        layer = 2, mt = w / (NT + 1), nt = w % (NT + 1), bias = nt == NT, Mdim = H, Ndim = H, ldd = H;
        delta = p.d2 + (size_t)t * p.Bp * H;
    } else {
        w -= c1 + c2;
        layer = 3, mt = 0, nt = w, bias = nt == NT, Mdim = n.out, Ndim = H, ldd = IQL_OUTW;
        delta = p.d3 + (size_t)t * p.Bp * IQL_OUTW;
    }
    const int col = 32 * nt + l31;
    const float* act = (layer == 2 ? p.h1 : p.h2) + (size_t)f * p.Bp * H;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const float* dp = delta + 32 * mt + l31;
    for (int s0 = 0; s0 < p.Bp / 2; s0 += 8) {  // (Bp / 2 is a multiple of 16: eight steps are loaded ahead of their MFMAs)
        float a[8], b[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int k = 2 * (s0 + u) + lh;
            a[u] = dp[(size_t)k * ldd];
            if (bias) b[u] = ((k >> 1) & 31) == l31 ? 1.f : 0.f;
            else if (layer == 1) b[u] = load_x(p, f, n.in, k, col);
            else b[u] = act[(size_t)k * H + col];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = IQL_MFMA(a[u], b[u], acc);
    }
    float *W, *mW, *vW, *tW = nullptr;
    if (layer == 1) W = bias ? n.b1 : n.W1, mW = bias ? am.b1 : am.W1, vW = bias ? av.b1 : av.W1;
    else if (layer == 2) W = bias ? n.b2 : n.W2, mW = bias ? am.b2 : am.W2, vW = bias ? av.b2 : av.W2;
    else W = bias ? n.b3 : n.W3, mW = bias ? am.b3 : am.W3, vW = bias ? av.b3 : av.W3;
    if (t == NET_Q1 || t == NET_Q2) {
        const NetP tn = p.net[t + 3];
        if (layer == 1) tW = bias ? tn.b1 : tn.W1;
        else if (layer == 2) tW = bias ? tn.b2 : tn.W2;
        else tW = bias ? tn.b3 : tn.W3;
    }
    if (bias) {  // the 32 partial sums of a unit, left to right by a fixed butterfly (offsets < 32 stay within a lane half)
#pragma unroll
        for (int i = 0; i < 16; ++i)
#pragma unroll
            for (int off = 16; off >= 1; off >>= 1) acc[i] += __shfl_xor(acc[i], off);
    }
    if (bias ? l31 != 0 : col >= Ndim) return;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int m = 32 * mt + 8 * (i / 4) + 4 * lh + i % 4;
        if (m >= Mdim) continue;
        const size_t x = bias ? (size_t)m : (size_t)m * Ndim + col;
        adam_apply(p, t, acc[i], W + x, mW + x, vW + x);
        if (tW) tW[x] = __fadd_rn(__fmul_rn(p.omt, tW[x]), __fmul_rn(p.tau, W[x]));
    }
}

// m3pc_iql_evaluate: what the forward kernels left in `out` (pass 0, and pass 1 for the twin) -> the caller's rows
__global__ __launch_bounds__(256) void iql_eval_out_kernel(const float* out, int Bp, int rows, int twin, int width, float* dst) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= rows * width) return;
    const int r = x / width, c = x % width;
    float v = out[(size_t)r * IQL_OUTW + c];
    if (twin) v = fminf(v, out[((size_t)Bp + r) * IQL_OUTW + c]);
    dst[x] = v;
}

__global__ __launch_bounds__(256) void iql_copy_kernel(float* dst, const float* src, long long n) {
    for (long long x = (long long)blockIdx.x * 256 + threadIdx.x; x < n; x += (long long)gridDim.x * 256) dst[x] = src[x];
}

__global__ __launch_bounds__(256) void iql_publish_kernel(PublishP p) {
    const int H = p.H, SA = p.SA, NT = H / 32, NG = H / 8;
    const long long s0 = (long long)SA * H, s1 = s0 + H, s2 = s1 + (long long)H * H, s3 = s2 + H, s4 = s3 + H, s5 = s4 + 1,
                    s6 = s5 + p.n_w1f, s7 = s6 + p.n_w2f, per = s7 + p.S;
    for (long long x = (long long)blockIdx.x * 256 + threadIdx.x; x < 2 * per; x += (long long)gridDim.x * 256) {
        const int qn = (int)(x / per);
        const long long y = x - qn * per;
        const NetP& n = p.q[qn];
        if (y < s0) {
            const int fe = (int)(y / H), c = (int)(y % H);
            p.W1T[qn][y] = n.W1[(size_t)c * SA + fe];
        } else if (y < s1) {
            p.b1[qn][y - s0] = n.b1[y - s0];
        } else if (y < s2) {
            const int k = (int)((y - s1) / H), c = (int)((y - s1) % H);
            p.W2T[qn][y - s1] = n.W2[(size_t)c * H + k];
        } else if (y < s3) {
            p.b2[qn][y - s2] = n.b2[y - s2];
        } else if (y < s4) {
            p.W3[qn][y - s3] = n.W3[y - s3];
        } else if (y < s5) {
            p.b3[qn][0] = n.b3[0];
        } else if (y < s6) {
            const long long z = y - s5;
            const int j = (int)(z & 3), lane = (int)((z >> 2) & 63), g = (int)((z >> 8) & 3), tt = (int)(z >> 10);
            const int fe = 2 * (4 * g + j) + (lane >> 5);
            p.W1F[qn][z] = fe < SA ? n.W1[(size_t)(32 * tt + (lane & 31)) * SA + fe] : 0.f;
        } else if (y < s7) {
            const long long z = y - s6;
            float v = 0.f;
            if (z < (long long)NT * NG * 256) {
                const int j = (int)(z & 3), lane = (int)((z >> 2) & 63);
                const int g = (int)((z >> 8) % NG), u = (int)((z >> 8) / NG);
                v = n.W2[(size_t)(32 * u + (lane & 31)) * H + 8 * g + 4 * (lane >> 5) + j];
            }
            p.W2F[qn][z] = v;
        } else if (qn == 0) {
            p.c_om[y - s7] = p.om[y - s7];
        } else {
            p.c_os[y - s7] = p.os[y - s7];
        }
    }
}

}  // namespace

#ifdef M3PC_LAB
thread_local int g_iql_picked = 0;
thread_local unsigned int g_iql_picked_set = 0;
#endif

void iql_launch_fwd(const IqlP& p, int layer, hipStream_t st) {
    const dim3 blk(256);
    if (layer == 1) {
        M3PC_IQL_PICK(1);
        hipLaunchKernelGGL(iql_fwd1_kernel, dim3((p.npass * p.RT * p.NT + 3) / 4), blk, 0, st, p);
    } else if (layer == 2) {
        M3PC_IQL_PICK(2);
        hipLaunchKernelGGL(iql_fwd2_kernel, dim3((p.npass * p.RT * p.NT + 3) / 4), blk, 0, st, p);
    } else {
        M3PC_IQL_PICK(3);
        hipLaunchKernelGGL(iql_fwd3_kernel, dim3((p.npass * p.RT + 3) / 4), blk, 0, st, p);
    }
}
void iql_launch_loss(const IqlP& p, hipStream_t st) {
    M3PC_IQL_PICK(4);
    hipLaunchKernelGGL(iql_loss_kernel, dim3(1), dim3(IQL_MAX_BATCH), 0, st, p);
}
void iql_launch_delta(const IqlP& p, int L, hipStream_t st) {
    const dim3 grid((IQL_NETS * p.RT * p.NT + 3) / 4), blk(256);
    if (L == 2) {
        M3PC_IQL_PICK(5);
        hipLaunchKernelGGL(iql_delta_kernel<2>, grid, blk, 0, st, p);
    } else {
        M3PC_IQL_PICK(6);
        hipLaunchKernelGGL(iql_delta_kernel<1>, grid, blk, 0, st, p);
    }
}
void iql_launch_grad(const IqlP& p, hipStream_t st) {
    M3PC_IQL_PICK(7);
    hipLaunchKernelGGL(iql_grad_kernel, dim3((iql_grad_tiles(p) + 3) / 4), dim3(256), 0, st, p);
}
void iql_launch_eval_out(const float* out, int Bp, int rows, int twin, int width, float* dst, hipStream_t st) {
    M3PC_IQL_PICK(8);
    hipLaunchKernelGGL(iql_eval_out_kernel, dim3((rows * width + 255) / 256), dim3(256), 0, st, out, Bp, rows, twin, width, dst);
}
void iql_launch_copy(float* dst, const float* src, long long n, hipStream_t st) {
    M3PC_IQL_PICK(9);
    hipLaunchKernelGGL(iql_copy_kernel, dim3(iql_copy_blocks(n)), dim3(256), 0, st, dst, src, n);
}
void iql_launch_publish(const PublishP& p, hipStream_t st) {
    M3PC_IQL_PICK(10);
    hipLaunchKernelGGL(iql_publish_kernel, dim3(iql_copy_blocks(iql_publish_total(p))), dim3(256), 0, st, p);
}
}  // namespace m3pc

// One trainer.  Device storage is allocated (and the Adam moments zeroed, in stream order) by the first call that enqueues work:
// m3pc_iql_create itself makes no HIP call.
struct m3pc_iql {
    int device = 0, S = 0, A = 0, H = 0;
    struct Off {
        size_t W1, b1, W2, b2, W3, b3;
        int in, out;
    } off[IQL_NETS];             // offsets of a trained network's tensors within a bank, floats, each a multiple of 4
    size_t off_log_std = 0, bank_floats = 0, tbank_floats = 0;
    float* bank[3] = {nullptr, nullptr, nullptr};  // parameters, Adam exp_avg, Adam exp_avg_sq of vf | q1 | q2 | actor | log_std
    float* tbank = nullptr;      // q_target: q1 | q2, laid out as in a bank
    float *om = nullptr, *os = nullptr;
    float *h1 = nullptr, *h2 = nullptr, *out = nullptr, *d3 = nullptr, *d2 = nullptr, *d1 = nullptr;
    float *bs = nullptr, *ba = nullptr, *br = nullptr, *bs2 = nullptr, *bd = nullptr;  // the batch m3pc_iql_train draws
    bool ready = false, norm_set = false;
    bool loaded[4] = {false, false, false, false};  // M3PC_IQL_QF, _Q_TARGET, _VF, _ACTOR
    long long total_it = 0;      // ImplicitQLearning.total_it: the steps made so far (the host's mirror)
    m3pc::StagePool pool;
};

namespace {

size_t round4(size_t x) { return (x + 3) & ~(size_t)3; }

int iql_ensure(m3pc_iql* q, hipStream_t st) {
    HIPCHK(hipSetDevice(q->device));
    if (q->ready) return 0;
    for (int b = 0; b < 3; ++b) CHK(dmalloc(&q->bank[b], q->bank_floats));
    CHK(dmalloc(&q->tbank, q->tbank_floats));
    CHK(dmalloc(&q->om, 64));
    CHK(dmalloc(&q->os, 64));
    const size_t Bp = IQL_MAX_BATCH, H = (size_t)q->H;
    CHK(dmalloc(&q->h1, IQL_PASSES * Bp * H));
    CHK(dmalloc(&q->h2, IQL_PASSES * Bp * H));
    CHK(dmalloc(&q->out, IQL_PASSES * Bp * IQL_OUTW));
    CHK(dmalloc(&q->d3, IQL_NETS * Bp * IQL_OUTW));
    CHK(dmalloc(&q->d2, IQL_NETS * Bp * H));
    CHK(dmalloc(&q->d1, IQL_NETS * Bp * H));
    CHK(dmalloc(&q->bs, Bp * q->S));
    CHK(dmalloc(&q->ba, Bp * q->A));
    CHK(dmalloc(&q->br, Bp));
    CHK(dmalloc(&q->bs2, Bp * q->S));
    CHK(dmalloc(&q->bd, Bp));
    for (int b = 0; b < 3; ++b) HIPCHK(hipMemsetAsync(q->bank[b], 0, q->bank_floats * sizeof(float), st));
    HIPCHK(hipMemsetAsync(q->tbank, 0, q->tbank_floats * sizeof(float), st));
    q->ready = true;
    return 0;
}

NetP net_at(const m3pc_iql* q, float* base, int t, size_t rebase) {
    const auto& o = q->off[t];
    NetP n;
    n.W1 = base + (o.W1 - rebase);
    n.b1 = base + (o.b1 - rebase);
    n.W2 = base + (o.W2 - rebase);
    n.b2 = base + (o.b2 - rebase);
    n.W3 = base + (o.W3 - rebase);
    n.b3 = base + (o.b3 - rebase);
    n.in = o.in;
    n.out = o.out;
    return n;
}

IqlP iql_params(const m3pc_iql* q) {
    IqlP p;
    memset(&p, 0, sizeof(p));
    for (int t = 0; t < IQL_NETS; ++t) {
        p.net[t] = net_at(q, q->bank[0], t, 0);
        p.am[t] = net_at(q, q->bank[1], t, 0);
        p.av[t] = net_at(q, q->bank[2], t, 0);
    }
    p.net[NET_Q1T] = net_at(q, q->tbank, NET_Q1, q->off[NET_Q1].W1);
    p.net[NET_Q2T] = net_at(q, q->tbank, NET_Q2, q->off[NET_Q1].W1);
    p.log_std = q->bank[0] + q->off_log_std;
    p.ls_m = q->bank[1] + q->off_log_std;
    p.ls_v = q->bank[2] + q->off_log_std;
    p.om = q->om;
    p.os = q->os;
    p.h1 = q->h1;
    p.h2 = q->h2;
    p.out = q->out;
    p.d3 = q->d3;
    p.d2 = q->d2;
    p.d1 = q->d1;
    p.H = q->H;
    p.NT = q->H / 32;
    p.S = q->S;
    p.A = q->A;
    return p;
}

// the tensors of a part, by their state_dict names (model.py:146-191, :107-133): the bank (3 = the target) and the offset within it
struct Entry {
    std::string name;
    int bank;
    size_t off;
    long long numel;
};
std::vector<Entry> part_entries(const m3pc_iql* q, int part) {
    static const char* FIELD[6] = {"net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias"};
    std::vector<Entry> e;
    int group, b;  // group: 0 qf, 1 vf, 2 actor; b: bank, or 3 = the target
    if (part == M3PC_IQL_QF) group = 0, b = 0;
    else if (part == M3PC_IQL_Q_TARGET) group = 0, b = 3;
    else if (part == M3PC_IQL_VF) group = 1, b = 0;
    else if (part == M3PC_IQL_ACTOR) group = 2, b = 0;
    else {
        group = (part - M3PC_IQL_QF_ADAM_M) / 2;
        b = 1 + (part - M3PC_IQL_QF_ADAM_M) % 2;
    }
    const size_t rebase = b == 3 ? q->off[NET_Q1].W1 : 0;
    auto add = [&](const char* prefix, int t) {
        const auto& o = q->off[t];
        const size_t at[6] = {o.W1, o.b1, o.W2, o.b2, o.W3, o.b3};
        const long long H = q->H;
        const long long num[6] = {H * o.in, H, H * H, H, (long long)o.out * H, o.out};
        for (int i = 0; i < 6; ++i) e.push_back({std::string(prefix) + FIELD[i], b, at[i] - rebase, num[i]});
    };
    if (group == 0) {
        add("q1.", NET_Q1);
        add("q2.", NET_Q2);
    } else if (group == 1) {
        add("v.", NET_V);
    } else {
        add("net.", NET_ACTOR);
        e.push_back({"log_std", b, q->off_log_std, q->A});
    }
    return e;
}
float* entry_dev(const m3pc_iql* q, const Entry& e) { return (e.bank == 3 ? q->tbank : q->bank[e.bank]) + e.off; }  // (behind iql_ensure)

int find_named(const m3pc_named_tensor* list, int n, const std::string& name) {
    for (int i = 0; i < n; ++i)
        if (list[i].name && name == list[i].name) return i;
    return -1;
}

bool finite_nonneg(double v) { return v >= 0.0 && v <= 1.7976931348623157e308; }

int check_args(const m3pc_iql_args* a, const char* who) {
    if (!finite_nonneg(a->v_lr) || !finite_nonneg(a->q_lr) || !finite_nonneg(a->actor_lr))
        return fail(M3PC_EINVAL, "%s: a learning rate is negative or not finite", who);
    if (!(a->expectile > 0.0 && a->expectile < 1.0)) return fail(M3PC_EINVAL, "%s: expectile outside (0, 1)", who);
    if (!(a->beta >= -1.7976931348623157e308 && a->beta <= 1.7976931348623157e308)) return fail(M3PC_EINVAL, "%s: beta is not finite", who);
    if (!finite_nonneg(a->discount)) return fail(M3PC_EINVAL, "%s: the discount must be finite and >= 0", who);
    if (!(a->tau >= 0.0 && a->tau <= 1.0)) return fail(M3PC_EINVAL, "%s: tau outside [0, 1]", who);
    if (a->actor_t_max < 1) return fail(M3PC_EINVAL, "%s: actor_t_max %lld < 1", who, a->actor_t_max);
    if (a->flags != 0) return fail(M3PC_EINVAL, "%s: flags %d must be 0", who, a->flags);
    return 0;
}

int check_trainable(const m3pc_iql* q, const char* who) {
    static const char* NAME[4] = {"qf", "q_target", "vf", "actor"};
    for (int i = 0; i < 4; ++i)
        if (!q->loaded[i]) return fail(M3PC_ESTATE, "%s: %s is not loaded", who, NAME[i]);
    if (!q->norm_set) return fail(M3PC_ESTATE, "%s: obs_mean / obs_std are not loaded", who);
    return 0;
}

// one step on a device batch: seven launches
int iql_step(m3pc_iql* q, const m3pc_iql_args* a, int batch, const float* state, const float* action, const float* reward,
             const float* next_state, const float* done, float* losses, hipStream_t st) {
    IqlP p = iql_params(q);
    iql_set_rows(p, batch);
    p.state = state;
    p.action = action;
    p.reward = reward;
    p.next_state = next_state;
    p.done = done;
    p.losses = losses;
    p.npass = IQL_PASSES;
    const int nets[IQL_PASSES] = {NET_V, NET_V, NET_Q1T, NET_Q2T, NET_Q1, NET_Q2, NET_ACTOR};
    for (int f = 0; f < IQL_PASSES; ++f) p.pass_net[f] = nets[f], p.pass_next[f] = f == 0;
    p.expectile = (float)a->expectile;
    p.beta = (float)a->beta;
    p.gamma = (float)a->discount;
    p.omt = (float)(1.0 - a->tau);
    p.tau = (float)a->tau;
    p.omb1 = (float)(1.0 - 0.9);
    p.b2 = (float)0.999;
    p.omb2 = (float)(1.0 - 0.999);
    const double k = (double)q->total_it, t = k + 1.0;
    const double bc1 = 1.0 - pow(0.9, t), bc2 = 1.0 - pow(0.999, t);
    const double actor_lr = a->actor_lr * 0.5 * (1.0 + cos(3.14159265358979323846 * k / (double)a->actor_t_max));
    p.step_size[NET_V] = a->v_lr / bc1;
    p.step_size[NET_Q1] = p.step_size[NET_Q2] = a->q_lr / bc1;
    p.step_size[NET_ACTOR] = actor_lr / bc1;
    p.sqrt_bc2 = sqrt(bc2);
    p.eps = 1e-8;
    for (int layer = 1; layer <= 3; ++layer) iql_launch_fwd(p, layer, st);
    iql_launch_loss(p, st);
    iql_launch_delta(p, 2, st);
    iql_launch_delta(p, 1, st);
    iql_launch_grad(p, st);
    CHK(check_launch("iql_train_step"));
    q->total_it += 1;
    return 0;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int m3pc_iql_create(m3pc_handle* h, int hidden, m3pc_iql** out) {
    if (!h || !out) return fail(M3PC_EINVAL, "null argument");
    const int S = h->dm.state_dim, A = h->dm.action_dim;
    if (hidden != 64 && hidden != 128 && hidden != 256) return fail(M3PC_EINVAL, "m3pc_iql_create: hidden %d is none of 64, 128, 256", hidden);
    if (S < 1 || A < 1 || A > 32 || S + A > 64)
        return fail(M3PC_EINVAL, "m3pc_iql_create: state_dim %d / action_dim %d outside the covered sizes (A <= 32, S + A <= 64)", S, A);
    m3pc_iql* q = new m3pc_iql();
    q->device = h->device;
    q->S = S;
    q->A = A;
    q->H = hidden;
    size_t at = 0;
    const size_t H = (size_t)hidden;
    for (int t = 0; t < IQL_NETS; ++t) {
        auto& o = q->off[t];
        o.in = (t == NET_Q1 || t == NET_Q2) ? S + A : S;
        o.out = t == NET_ACTOR ? A : 1;
        o.W1 = at, at = round4(at + H * o.in);
        o.b1 = at, at = round4(at + H);
        o.W2 = at, at = round4(at + H * H);
        o.b2 = at, at = round4(at + H);
        o.W3 = at, at = round4(at + (size_t)o.out * H);
        o.b3 = at, at = round4(at + o.out);
    }
    q->off_log_std = at;
    q->bank_floats = round4(at + A);
    q->tbank_floats = q->off[NET_ACTOR].W1 - q->off[NET_Q1].W1;
    *out = q;
    return 0;
}

int m3pc_iql_destroy(m3pc_iql* q) {
    if (!q) return 0;
    if (q->ready || !q->pool.stages.empty()) {
        (void)hipSetDevice(q->device);
        (void)hipDeviceSynchronize();
        for (void* b : {(void*)q->bank[0], (void*)q->bank[1], (void*)q->bank[2], (void*)q->tbank, (void*)q->om, (void*)q->os, (void*)q->h1,
                        (void*)q->h2, (void*)q->out, (void*)q->d3, (void*)q->d2, (void*)q->d1, (void*)q->bs, (void*)q->ba, (void*)q->br,
                        (void*)q->bs2, (void*)q->bd})
            if (b) (void)hipFree(b);
        q->pool.destroy();
    }
    delete q;
    return 0;
}

int m3pc_iql_load(m3pc_iql* q, int part, const m3pc_named_tensor* tensors, int n, const float* obs_mean, const float* obs_std, void* stream) {
    if (!q || !tensors) return fail(M3PC_EINVAL, "null argument");
    if (part < M3PC_IQL_QF || part > M3PC_IQL_ACTOR_ADAM_V) return fail(M3PC_EINVAL, "m3pc_iql_load: part %d is no M3PC_IQL_* part", part);
    if ((obs_mean == nullptr) != (obs_std == nullptr)) return fail(M3PC_EINVAL, "m3pc_iql_load: obs_mean and obs_std come together (one of them is null)");
    const std::vector<Entry> ent = part_entries(q, part);
    std::vector<int> at(ent.size());
    for (size_t i = 0; i < ent.size(); ++i) {
        at[i] = find_named(tensors, n, ent[i].name);
        if (at[i] < 0) return fail(M3PC_EINVAL, "m3pc_iql_load: the state_dict is missing '%s'", ent[i].name.c_str());
        const m3pc_named_tensor& t = tensors[at[i]];
        if (!t.data) return fail(M3PC_EINVAL, "m3pc_iql_load: '%s' has no data", ent[i].name.c_str());
        if (t.numel != ent[i].numel)
            return fail(M3PC_EINVAL, "m3pc_iql_load: '%s' has %lld elements, expected %lld", ent[i].name.c_str(), t.numel, ent[i].numel);
    }
    hipStream_t st = (hipStream_t)stream;
    CHK(iql_ensure(q, st));
    auto abandon = [&](int rc) {  // (copies already enqueued still read their blocks: record the events before giving them back)
        (void)q->pool.release(st);
        return rc;
    };
    for (size_t i = 0; i < ent.size(); ++i) {
        const m3pc_named_tensor& t = tensors[at[i]];
        const void* src = t.data;
        if (!t.on_device)
            if (int rc = q->pool.stage(t.data, (size_t)t.numel * sizeof(float), &src, "m3pc_iql")) return abandon(rc);
        iql_launch_copy(entry_dev(q, ent[i]), (const float*)src, t.numel, st);
    }
    if (obs_mean) {
        const void *m = nullptr, *s = nullptr;
        int rc = q->pool.stage(obs_mean, (size_t)q->S * sizeof(float), &m, "m3pc_iql");
        if (!rc) rc = q->pool.stage(obs_std, (size_t)q->S * sizeof(float), &s, "m3pc_iql");
        if (rc) return abandon(rc);
        iql_launch_copy(q->om, (const float*)m, (long long)q->S, st);
        iql_launch_copy(q->os, (const float*)s, (long long)q->S, st);
        q->norm_set = true;
    }
    const int rc = check_launch("iql_load");
    const int rr = q->pool.release(st);
    if (rc || rr) return rc ? rc : rr;
    if (part <= M3PC_IQL_ACTOR) q->loaded[part] = true;
    return 0;
}

int m3pc_iql_export(m3pc_iql* q, int part, const m3pc_named_tensor* tensors, int n, void* stream) {
    if (!q || !tensors) return fail(M3PC_EINVAL, "null argument");
    if (part < M3PC_IQL_QF || part > M3PC_IQL_ACTOR_ADAM_V) return fail(M3PC_EINVAL, "m3pc_iql_export: part %d is no M3PC_IQL_* part", part);
    const std::vector<Entry> ent = part_entries(q, part);
    std::vector<int> at(ent.size());
    for (size_t i = 0; i < ent.size(); ++i) {
        at[i] = find_named(tensors, n, ent[i].name);
        if (at[i] < 0) return fail(M3PC_EINVAL, "m3pc_iql_export: no room was given for '%s'", ent[i].name.c_str());
        const m3pc_named_tensor& t = tensors[at[i]];
        if (!t.data) return fail(M3PC_EINVAL, "m3pc_iql_export: '%s' has no data", ent[i].name.c_str());
        if (t.numel != ent[i].numel)
            return fail(M3PC_EINVAL, "m3pc_iql_export: '%s' has %lld elements, expected %lld", ent[i].name.c_str(), t.numel, ent[i].numel);
    }
    if (part <= M3PC_IQL_ACTOR && !q->loaded[part]) return fail(M3PC_ESTATE, "m3pc_iql_export: part %d is not loaded", part);
    hipStream_t st = (hipStream_t)stream;
    CHK(iql_ensure(q, st));
    for (size_t i = 0; i < ent.size(); ++i) {
        const m3pc_named_tensor& t = tensors[at[i]];
        float* dst = const_cast<float*>(t.data);
        if (t.on_device) iql_launch_copy(dst, (const float*)entry_dev(q, ent[i]), t.numel, st);
        else HIPCHK(hipMemcpyAsync(dst, entry_dev(q, ent[i]), (size_t)t.numel * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    return check_launch("iql_export");
}

int m3pc_iql_set_step(m3pc_iql* q, long long total_it) {
    if (!q) return fail(M3PC_EINVAL, "null argument");
    if (total_it < 0) return fail(M3PC_EINVAL, "m3pc_iql_set_step: total_it %lld < 0", total_it);
    q->total_it = total_it;
    return 0;
}

int m3pc_iql_get_step(m3pc_iql* q, long long* total_it) {
    if (!q || !total_it) return fail(M3PC_EINVAL, "null argument");
    *total_it = q->total_it;
    return 0;
}

int m3pc_iql_train_step(m3pc_iql* q, const m3pc_iql_args* args, int batch, const float* state, const float* action, const float* reward,
                        const float* next_state, const float* done, float* losses, void* stream) {
    if (!q || !args || !state || !action || !reward || !next_state || !done) return fail(M3PC_EINVAL, "null argument");
    if (batch < 1 || batch > IQL_MAX_BATCH) return fail(M3PC_EINVAL, "m3pc_iql_train_step: batch %d outside [1, %d]", batch, IQL_MAX_BATCH);
    CHK(check_args(args, "m3pc_iql_train_step"));
    CHK(check_trainable(q, "m3pc_iql_train_step"));
    hipStream_t st = (hipStream_t)stream;
    CHK(iql_ensure(q, st));
    return iql_step(q, args, batch, state, action, reward, next_state, done, losses, st);
}

int m3pc_iql_train(m3pc_iql* q, const m3pc_iql_args* args, m3pc_replay* rb, int n_steps, int batch, int n_online, unsigned long long seed,
                   unsigned long long step, float* losses, void* stream) {
    if (!q || !args || !rb) return fail(M3PC_EINVAL, "null argument");
    if (n_steps < 1) return fail(M3PC_EINVAL, "m3pc_iql_train: n_steps %d < 1", n_steps);
    if (batch < 1 || batch > IQL_MAX_BATCH) return fail(M3PC_EINVAL, "m3pc_iql_train: batch %d outside [1, %d]", batch, IQL_MAX_BATCH);
    CHK(check_args(args, "m3pc_iql_train"));
    int S = 0, A = 0, device = 0;
    replay_sizes(rb, &S, &A, &device);
    if (S != q->S || A != q->A || device != q->device)
        return fail(M3PC_EINVAL, "m3pc_iql_train: the buffer (S %d, A %d, device %d) does not fit the trainer (%d, %d, %d)", S, A, device, q->S, q->A,
                    q->device);
    CHK(check_trainable(q, "m3pc_iql_train"));
    // what m3pc_replay_sample_transitions would refuse, here before any HIP call (the counts are the host's mirrors)
    if (n_online < 0 || n_online > batch) return fail(M3PC_EINVAL, "m3pc_iql_train: n_online %d outside [0, batch=%d]", n_online, batch);
    int held_off = 0, held_on = 0;
    CHK(m3pc_replay_counts(rb, nullptr, &held_off, &held_on));
    if (n_online > 0 && held_on == 0) return fail(M3PC_ESTATE, "m3pc_iql_train: the online ring is empty");
    if (batch - n_online > 0 && held_off == 0) return fail(M3PC_ESTATE, "m3pc_iql_train: the offline ring is empty");
    if (n_online > held_on) return fail(M3PC_EINVAL, "m3pc_iql_train: %d rows asked of the online ring, which holds %d", n_online, held_on);
    if (batch - n_online > held_off)
        return fail(M3PC_EINVAL, "m3pc_iql_train: %d rows asked of the offline ring, which holds %d", batch - n_online, held_off);
    hipStream_t st = (hipStream_t)stream;
    CHK(iql_ensure(q, st));
    for (int k = 0; k < n_steps; ++k) {
        CHK(m3pc_replay_sample_transitions(rb, batch, n_online, nullptr, 0, seed, step + (unsigned long long)k, q->bs, q->ba, q->br, q->bs2, q->bd,
                                           nullptr, stream));
        CHK(iql_step(q, args, batch, q->bs, q->ba, q->br, q->bs2, q->bd, losses ? losses + 3 * (size_t)k : nullptr, st));
    }
    return 0;
}

int m3pc_iql_publish_critic(m3pc_iql* q, m3pc_handle* h, void* stream) {
    if (!q || !h) return fail(M3PC_EINVAL, "null argument");
    if (h->dm.critic_hidden != q->H || h->dm.state_dim != q->S || h->dm.action_dim != q->A || h->device != q->device)
        return fail(M3PC_EINVAL, "m3pc_iql_publish_critic: the handle (S %d, A %d, critic_hidden %d, device %d) does not fit the trainer (%d, %d, %d, %d)",
                    h->dm.state_dim, h->dm.action_dim, h->dm.critic_hidden, h->device, q->S, q->A, q->H, q->device);
    if (!q->loaded[M3PC_IQL_QF]) return fail(M3PC_ESTATE, "m3pc_iql_publish_critic: qf is not loaded");
    if (!q->norm_set) return fail(M3PC_ESTATE, "m3pc_iql_publish_critic: obs_mean / obs_std are not loaded");
    hipStream_t st = (hipStream_t)stream;
    CHK(iql_ensure(q, st));
    PublishP p;
    memset(&p, 0, sizeof(p));
    for (int i = 0; i < 2; ++i) {
        p.q[i] = net_at(q, q->bank[0], NET_Q1 + i, 0);
        p.W1T[i] = h->cW1T[i];
        p.b1[i] = h->cb1[i];
        p.W2T[i] = h->cW2T[i];
        p.b2[i] = h->cb2[i];
        p.W3[i] = h->cW3[i];
        p.b3[i] = h->cb3[i];
        p.W1F[i] = h->cW1F[i];
        p.W2F[i] = h->cW2F[i];
    }
    p.om = q->om;
    p.os = q->os;
    p.c_om = h->c_om;
    p.c_os = h->c_os;
    p.S = q->S;
    p.SA = q->S + q->A;
    p.H = q->H;
    const bool packed = h->cW1F[0] != nullptr;
    p.n_w1f = packed ? (long long)critic_w1f_floats(q->H) : 0;
    p.n_w2f = packed ? (long long)critic_w2f_floats(q->H) : 0;
    iql_launch_publish(p, st);
    CHK(check_launch("iql_publish_critic"));
    h->critic_set = true;
    return 0;
}

int m3pc_iql_evaluate(m3pc_iql* q, int which, const float* states, const float* actions, int rows, float* out, void* stream) {
    if (!q || !states || !out) return fail(M3PC_EINVAL, "null argument");
    if (which < M3PC_IQL_Q_MIN || which > M3PC_IQL_ACTOR_MEAN) return fail(M3PC_EINVAL, "m3pc_iql_evaluate: which %d is no M3PC_IQL_* output", which);
    const bool twin = which == M3PC_IQL_Q_MIN || which == M3PC_IQL_Q_TARGET_MIN;
    if (twin && !actions) return fail(M3PC_EINVAL, "null argument");
    if (rows < 1) return fail(M3PC_EINVAL, "m3pc_iql_evaluate: rows %d < 1", rows);
    const int part = which == M3PC_IQL_Q_MIN ? M3PC_IQL_QF : which == M3PC_IQL_Q_TARGET_MIN ? M3PC_IQL_Q_TARGET : which == M3PC_IQL_V ? M3PC_IQL_VF : M3PC_IQL_ACTOR;
    if (!q->loaded[part]) return fail(M3PC_ESTATE, "m3pc_iql_evaluate: part %d is not loaded", part);
    if (!q->norm_set) return fail(M3PC_ESTATE, "m3pc_iql_evaluate: obs_mean / obs_std are not loaded");
    hipStream_t st = (hipStream_t)stream;
    CHK(iql_ensure(q, st));
    IqlP p = iql_params(q);
    p.npass = twin ? 2 : 1;
    p.pass_net[0] = which == M3PC_IQL_Q_MIN ? NET_Q1 : which == M3PC_IQL_Q_TARGET_MIN ? NET_Q1T : which == M3PC_IQL_V ? NET_V : NET_ACTOR;
    p.pass_net[1] = which == M3PC_IQL_Q_MIN ? NET_Q2 : NET_Q2T;
    const int width = which == M3PC_IQL_ACTOR_MEAN ? q->A : 1;
    for (int r0 = 0; r0 < rows; r0 += IQL_MAX_BATCH) {
        const int nr = rows - r0 < IQL_MAX_BATCH ? rows - r0 : IQL_MAX_BATCH;
        iql_set_rows(p, nr);
        p.state = states + (size_t)r0 * q->S;
        p.action = actions ? actions + (size_t)r0 * q->A : nullptr;
        for (int layer = 1; layer <= 3; ++layer) iql_launch_fwd(p, layer, st);
        iql_launch_eval_out(p.out, p.Bp, nr, twin ? 1 : 0, width, out + (size_t)r0 * width, st);
    }
    return check_launch("iql_evaluate");
}

}  // extern "C"
#pragma GCC visibility pop
