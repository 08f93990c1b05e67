// The IQL trainer (include/m3pc_hip.h: m3pc_iql_*): ImplicitQLearning.train of finetune_omtm/model.py:286-308 on the device.
// Shared between iql.hip (the kernels and the C ABI) and replay.hip (which tells the trainer what a buffer holds).
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
}  // namespace m3pc
