// The optimizers of the masked-trajectory model (include/m3pc_hip.h: m3pc_mtm_opt_*, m3pc_mtm_train*): what Learner.mtm_update
// (finetune_omtm/learner.py:506-538) does behind loss.backward() -- AdamW over every parameter (omtm.configure_optimizers,
// mtm_model.py:779-841), the LambdaLR schedule and the Adam step of the float64 log_temperature -- on the device, applied to the
// handle's own fp32 weights, with every derived weight form refreshed behind it (derive_weights, m3pc.hip).
// Shared between mtm_opt.hip (the kernels, their launchers and the C ABI) and, in the lab build, m3pc_debug.hip.
//
// LAUNCHES of one step: mo_adamw_kernel (ONE launch over all parameters) and mo_temperature_kernel (one thread); behind the last
// step of a call the packs of derive_weights for the tensors that moved.  No stream synchronise, no host wait, no copy from host memory:
// the learning rate travels as a kernel argument, the bias corrections are derived on the device from the per-tensor step counts.
//
// SEGMENT TABLE.  One MoSeg per parameter, built at create, device-resident.  A block table maps workgroup b to (segment, chunk):
// every workgroup owns MO_CHUNK consecutive elements of ONE tensor, so no block assumes that a tensor ends where a block does and
// a tensor of one element costs one (mostly idle) workgroup.  A thread owns four consecutive elements: one 16-byte access per
// array where the four bases are 16-byte aligned and the four elements exist, else element by element (the tail, a misaligned base).
//
// INACTIVE TENSORS.  A tensor of the output head of a key outside loss_keys has no gradient in the reference (.grad = None) and
// torch's AdamW skips it: no decay, no moment update, no step.  Its workgroups leave at once: weight, moments, bf16 copies and step
// count keep their bits.  A tensor whose gradient is all zeros is NOT inactive.
//
// STEP COUNTS are per tensor (torch's state['step']), int64 on the device in two arrays the launches alternate between: a launch
// reads `steps_in`, and the workgroup of a tensor's chunk 0 writes `steps_out` (t + 1, or t for an inactive tensor).  No workgroup
// reads what another writes.
//
// ARITHMETIC per element of an active tensor, t = its step count + 1, g its gradient, with the fp32 constants
// omb1 = (float)(1 - beta1), b2 = (float)beta2, omb2 = (float)(1 - beta2) and explicit-rounding intrinsics (no contraction):
//     m <- m + omb1 (g - m)                             fp32: one subtraction, one product, one sum      (adam_apply, iql.hip)
//     v <- b2 v + (omb2 g) g                            fp32: three products, one sum
//   then in float64, from the fp32 m and v just stored:
//     bc1 = 1 - beta1^t;  bc2 = 1 - beta2^t             pow() of the device's float64 library
//     q   = p (1 - lr_t wd)                             decaying tensors only; else q = p.   lr_t: a launch scalar (double)
//     p  <- (float)( q - (lr_t / bc1) m / (sqrt(v) / sqrt(bc2) + eps) )                      rounded to fp32 ONCE
// and for a GEMM weight (write_bf16) the same thread writes hi = bf16(p), lo = bf16(p - (float)hi), round-to-nearest-even: the
// bits of launch_f32_split_bf16 (gemm_x3.hip) on the new p.
// The decay and the step are ONE float64 expression: torch rounds p (1 - lr wd) to fp32 before the step and evaluates the quotient
// in fp32, which costs up to four more roundings at the half ulp of p; the float64 restatement of tests/mtm_opt_ref.py is the
// common reference.  With g = 0 and m = v = 0 the quotient is 0 / eps = 0 and p <- (float)(p (1 - lr_t wd)) exactly.
//
// SCHEDULE (host, m3pc_mtm_lr): lr_t = learning_rate * lambda(s) at scheduler count s (LambdaLR):
//     warmup_steps == 0:  0.5 (1 + cos(s / num_train_steps * pi))                                          learner.py:50-51
//     warmup_steps  > 0:  s < warmup ? s / warmup : 0.5 (1 + cos((s - warmup) / (num_train_steps - warmup) * pi))   train.py:889-899
//
// TEMPERATURE (mo_temperature_kernel, one thread, float64 as the reference's log_temperature): with the entropy of the gradient
// call's device record (record[12], an fp32 value) and t = temp_step + 1, torch.optim.Adam's order:
//     g = exp(log_t) (entropy - target_entropy)
//     m <- m + (g - m) (1 - b1);   v <- v b2 + ((1 - b2) g) g
//     log_t <- log_t - ((lr / (1 - b1^t)) m) / (sqrt(v) / sqrt(1 - b2^t) + eps)
// It writes log_t, m, v, the count, (float)exp(log_t) for the next gradient call (LossBwdG::entropy_reg_p) and the three doubles
// of train_record {lr_t used, exp(log_t), log_t}.
//
// DETERMINISM.  Nothing is reduced: every element is written by one thread from values only that thread reads.  No atomics.  A
// step is bit-identical from run to run.
//
// BYTES per element and step: 16 read (p, g, m, v), 12 written (p, m, v), + 4 written for a GEMM weight (hi, lo).
#pragma once
#include "m3pc_internal.h"

namespace m3pc {

constexpr int MO_CHUNK = 2048;  // elements of one tensor a workgroup of 256 threads owns: two groups of four per thread

struct MoSeg {
    float* p;            // the fp32 weight (Tensor::f)
    bf16_t* b;           // Tensor::b (hi at [0, numel), lo behind it), or null
    long long g_off;     // in the gradient arena
    long long s_off;     // in the two moment arenas
    long long numel;
    int decay;
    int head_key;        // the loss key whose output head the tensor belongs to, or -1: active whatever loss_keys is
};

struct MoAdamP {
    const MoSeg* seg;
    const int2* blk;     // (n_blocks): segment, chunk
    int n_blocks;
    const float* grad;
    float *exp_avg, *exp_avg_sq;
    const long long* steps_in;
    long long* steps_out;
    int loss_keys, write_bf16;
    double lr_t, wd, beta1, beta2, eps;
    float omb1, b2, omb2;
};

struct MoTempP {
    double* state;        // log_t, exp_avg, exp_avg_sq, step count
    float* temp_f;        // (float)exp(log_t)
    const float* record;  // the gradient call's record: [12] entropy
    double* train_record; // optional: lr_t, exp(log_t), log_t
    double lr_t, target_entropy, lr, beta1, beta2, eps;
};

// the block table of a segment list: (segment, chunk) per workgroup, segments in order
inline void mo_block_table(const long long* numel, int n, std::vector<int2>& out) {
    out.clear();
    for (int s = 0; s < n; ++s)
        for (long long c = 0; c * MO_CHUNK < numel[s]; ++c) out.push_back(make_int2(s, (int)c));
}
void mo_launch_adamw(const MoAdamP& p, hipStream_t st);
void mo_launch_temperature(const MoTempP& p, hipStream_t st);
}  // namespace m3pc
