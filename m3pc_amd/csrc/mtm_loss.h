// The masked-trajectory loss (include/m3pc_hip.h: m3pc_mtm_loss*): the forward half of Learner.compute_mtm_loss
// (finetune_omtm/learner.py:419-504) and of omtm.forward_loss (omtm/models/mtm_model.py:440-532) on the device.
// Shared between mtm_loss.hip (the kernels and the C ABI), replay.hip (what a buffer holds) and m3pc.hip (the handle's end).
//
// LAUNCHES.  Two, behind the forward's: mtm_loss_rows_kernel (one wavefront per row (b, t): the elementwise terms in fp32, their sum
// over the row's features in float64 -> six doubles per row in a scratch block) and mtm_loss_reduce_kernel (ONE workgroup of 256
// threads: thread i adds the rows i, i + 256, ... in that order, then the 64-lane butterfly and the four wave results left to right;
// the masks and the counts enter here).  No floating-point atomics, and the second stage never looks at the first one's grid: a call
// is bit-identical from run to run and for any number of rows beyond `batch`.
//
// ARITHMETIC.  Per element in fp32, in the order the reference's expressions are written (the build has -ffp-contract=off):
//   states / rewards / returns:  t' = t / sqrtf(sum_d t^2) with M3PC_MTM_NORM_L2 (the sum of the fp32 squares in float64, rounded to
//                                fp32 once), else t;  raw = (pred - t')^2
//   actions:                     raw = (tanhf(mu) - a)^2
//   Normal(mu, std).log_prob(x): ((-((x - mu)^2)) / (2 (std std)) - logf(std)) - (float)log(sqrt(2 pi))
//   log|det J|(x):               2 ((float)log 2 - x - softplus(-2 x)),  softplus(y) = y > 20 ? y : log1pf(expf(y))
//   likelihood:                  a' = clip(a, (float)(-1 + 1e-6), (float)(1 - 1e-6)) with M3PC_MTM_CLIP_ACTIONS, else a;
//                                z = 0.5 (log1pf(a') - log1pf(-a'));  lp = log_prob(z) - log|det J|(z)
//   entropy:                     u = mu + eps std;  lq = log_prob(u) - log|det J|(u)      (the cached pre-tanh value: no atanh)
// Every sum is float64.  The twelve per-key numbers, entropy, nll and total are formed in float64 from the sums and the counts and
// rounded to fp32 once.  raw * m and raw * (1 - m) of the reference are s m and s (1 - m) on the row sum s: m is 0 or 1 per row, raw
// >= 0 or NaN, so the product is 0, s or NaN exactly where the reference's is.  lp and lq are SELECTED by the action mask (the
// reference indexes, it does not multiply): a NaN at a visible timestep stays out.  A zero count divides as IEEE does.
//
// THE RECORD, M3PC_MTM_LOSS_FLOATS floats: [3 k + 0] loss_k, [3 k + 1] masked_loss_k, [3 k + 2] masked_c_loss_k for k = M3PC_STATES,
// _ACTIONS, _REWARDS, _RETURNS ([4] and [5], the masked variants of the actions, which do not exist, are 0); [12] entropy; [13] nll;
// [14] total.
#pragma once
#include "m3pc_internal.h"

struct m3pc_replay;
namespace m3pc {

constexpr int MTM_LOSS_PART = 6;  // doubles per row in the scratch block: states, rewards, returns, actions, sum lp, sum lq

struct MtmLossP {
    const float *pred[3];   // states (rows, S), rewards (rows,), returns (rows,)
    const float *mu, *sd;   // (rows, A)
    const float *tgt[4];    // tokenised targets in key order
    const float* eps;       // (rows, A)
    unsigned long long mask[4];  // bit t of mask[k]: token t of key k is visible
    int batch, T, S, A, flags, loss_keys;
    float entropy_reg;
    const float* entropy_reg_p;  // optional device scalar read in place of entropy_reg (the trainer's temperature, mtm_opt.h)
    double* part;           // (rows, MTM_LOSS_PART)
    float* record;
};
void launch_mtm_loss(const MtmLossP& p, hipStream_t st);

// replay.hip: what a buffer was created with, and the refusals of m3pc_replay_sample_segments that need no HIP call
int replay_segment_length(const m3pc_replay* rb);
int replay_check_segments(m3pc_replay* rb, int batch, int mode, const int* traj_index, const int* start_index, int index_on_device,
                          const char* who);
// m3pc.hip calls it from m3pc_destroy
void mtm_loss_free(m3pc_handle* h);

}  // namespace m3pc
