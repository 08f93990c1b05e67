// The IQL trainer (include/m3pc_hip.h: m3pc_iql_*): ImplicitQLearning.train of finetune_omtm/model.py:286-308 on the device.
// Shared between iql.hip (the kernels, their launchers and the C ABI), replay.hip (which tells the trainer what a buffer holds) and,
// in the lab build, m3pc_debug.hip (the hooks that run each kernel alone through the launchers below).
//
// ARITHMETIC.  fp32 throughout; every matrix product is a chain of v_mfma_f32_32x32x2_f32 (exact fp32 fma per term) owned by ONE
// wavefront per 32 x 32 output tile, which walks its K dimension in a fixed order: no split-K, no floating-point atomics, and the
// bias gradients, the log_std gradient and the three loss means are summed by fixed trees.  A step is bit-identical from run to run.
//
// ADAM is torch.optim.Adam's (betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad) in this order per element, with
// b1 = (float)0.9, 1 - b1 = (float)(1.0 - 0.9), b2 = (float)0.999, 1 - b2 = (float)(1.0 - 0.999):
//     m <- m + (1 - b1) (g - m)                        fp32: one subtraction, one product, one sum
//     v <- b2 v + ((1 - b2) g) g                        fp32: three products, one sum
//     p <- p - (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// The two moment recurrences are fp32.  The parameter expression is evaluated in that order in FP64 from the fp32 moments and
// rounded to fp32 once: lr / (1 - b1^t) and sqrt(1 - b2^t) are computed by the host in double and passed as launch scalars, and
// an fp32 evaluation of the quotient would add up to three roundings of the update to the half ulp of the result -- visible where
// the update is larger than the parameter (small biases at t = 1).  The actor's rate at 0-based step k is lr (1 + cos(pi k /
// T_max)) / 2, the closed form of CosineAnnealingLR (model.py:219) with eta_min = 0; torch's recursive form agrees with it to
// rounding (a few ulp of the rate after 10^6 steps).  The host mirrors the step count: no entry point reads the device.
#pragma once
#include "stage.h"

struct m3pc_replay;
namespace m3pc {
// what a replay buffer was created with (replay.hip)
void replay_sizes(const m3pc_replay* rb, int* S, int* A, int* device);

// ------------------------------------------------------------------------------------------------ parameter structures
// (iql.hip holds the kernels; iql_step, the other entry points and the lab hooks of m3pc_debug.hip fill these and go through the
// launchers below)
constexpr int IQL_MAX_BATCH = 1024, IQL_PASSES = 7, IQL_OUTW = 32, IQL_NETS = 4;
constexpr int NET_V = 0, NET_Q1 = 1, NET_Q2 = 2, NET_ACTOR = 3, NET_Q1T = 4, NET_Q2T = 5;

struct NetP {
    float *W1, *b1, *W2, *b2, *W3, *b3;  // torch layout: (H, in) (H) (H, H) (H) (out, H) (out)
    int in, out;
};

struct IqlP {
    NetP net[6];                // NET_*: parameters
    NetP am[IQL_NETS], av[IQL_NETS];  // Adam moments of the four trained networks
    float *log_std, *ls_m, *ls_v;
    const float *om, *os;       // obs_mean, obs_std (S)
    const float *state, *action, *reward, *next_state, *done;
    float *h1, *h2;             // (pass, Bp, H) activations after ReLU
    float* out;                 // (pass, Bp, 32) network outputs
    float *d3, *d2, *d1;        // (net, Bp, 32) (net, Bp, H) (net, Bp, H) deltas of the trained networks
    float* losses;              // optional: value_loss, q_loss, actor_loss
    int B, Bp, RT, H, NT, S, A;
    int npass, pass_net[IQL_PASSES], pass_next[IQL_PASSES];  // a forward pass: its network; 1 = it reads next_state
    float expectile, beta, gamma, omt, tau;
    float omb1, b2, omb2;       // Adam: 1 - beta1, beta2, 1 - beta2
    double step_size[IQL_NETS], sqrt_bc2, eps;
};

// m3pc_iql_publish_critic: q1 / q2 into the planner's critic buffers -- the transposed copies and plain vectors the scalar critic
// kernel reads, and (n_w1f != 0) the MFMA operand streams of critic_pack (elementwise.hip), index for index.
struct PublishP {
    NetP q[2];
    float *W1T[2], *b1[2], *W2T[2], *b2[2], *W3[2], *b3[2], *W1F[2], *W2F[2];
    const float *om, *os;
    float *c_om, *c_os;
    int S, SA, H;
    long long n_w1f, n_w2f;  // critic_w1f_floats / critic_w2f_floats, or 0
};

// lab build: the id of the iql.hip kernel the calling thread launched last and the set of ids launched since the set was last
// cleared -- include/m3pc_hip_debug.h, "IQL-trainer kernel ids"; the product build records nothing
#ifdef M3PC_LAB
extern thread_local int g_iql_picked;
extern thread_local unsigned int g_iql_picked_set;
#define M3PC_IQL_PICK(id) (::m3pc::g_iql_picked = (id), ::m3pc::g_iql_picked_set |= 1u << (id))
#else
#define M3PC_IQL_PICK(id) ((void)0)
#endif

// ------------------------------------------------------------------------------------------------ launchers
// The grid geometry, the tile count of the gradient grid and the block count of the copies exist here once.
// B, and with it the padded row count Bp (whole 32-row tiles) and the row tiles RT
inline void iql_set_rows(IqlP& p, int rows) {
    p.B = rows;
    p.Bp = (rows + 31) & ~31;
    p.RT = p.Bp / 32;
}
// the 32 x 32 tiles of iql_grad_kernel: per trained network NT (NI + 1) of layer 1, NT (NT + 1) of layer 2 and NT + 1 of layer 3
// (the "+ 1" is the bias tile), NI = ceil(in / 32)
inline int iql_grad_tiles(const IqlP& p) {
    int tiles = 0;
    for (int t = 0; t < IQL_NETS; ++t) tiles += p.NT * ((p.net[t].in + 31) / 32 + 1) + p.NT * (p.NT + 1) + p.NT + 1;
    return tiles;
}
inline int iql_copy_blocks(long long n) { return (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024); }
// the elements iql_publish_kernel writes
inline long long iql_publish_total(const PublishP& p) {
    return 2 * ((long long)p.SA * p.H + (long long)p.H * p.H + 3 * p.H + 1 + p.n_w1f + p.n_w2f + p.S);
}
void iql_launch_fwd(const IqlP& p, int layer, hipStream_t st);  // layer 1, 2, 3: iql_fwd1 / 2 / 3_kernel over p.npass passes
void iql_launch_loss(const IqlP& p, hipStream_t st);
void iql_launch_delta(const IqlP& p, int L, hipStream_t st);    // L 2, 1: iql_delta_kernel<L>
void iql_launch_grad(const IqlP& p, hipStream_t st);
void iql_launch_eval_out(const float* out, int Bp, int rows, int twin, int width, float* dst, hipStream_t st);
void iql_launch_copy(float* dst, const float* src, long long n, hipStream_t st);
void iql_launch_publish(const PublishP& p, hipStream_t st);
}  // namespace m3pc
