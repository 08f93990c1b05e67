/*
 * m3pc_hip.h -- C ABI of libm3pc_hip.so, the MI355X (gfx950) implementation of the m3pc
 * test-time MPC plan step.
 *
 * The reference (wkh923/m3pc) is pure Python/PyTorch and has no native interface; the entry
 * points below are what a ctypes binding for its hot path binds (INTEGRATION.md shows the
 * stub).  Each function names the reference code it replaces (paths relative to the
 * reference root).
 *
 * Conventions
 *   - every function returns 0 on success, a negative M3PC_E* code on failure;
 *     m3pc_last_error() returns a thread-local message for the last failure.
 *   - "device" pointers are HIP device pointers owned by the caller (e.g. tensor.data_ptr());
 *     they must stay alive until the stream has been synchronised.  "host" pointers are
 *     ordinary process memory and are consumed before the call returns.
 *   - `stream` is a hipStream_t passed as void* (0 = default stream).  Calls enqueue work on
 *     it and return without synchronising unless documented otherwise.
 *   - one handle per (process, device); a handle is not re-entrant: calls are made from one host thread
 *     at a time.  Work enqueued by DIFFERENT calls may overlap on the device only as documented at
 *     "Pipelined plan steps" below.
 *   - all tensors are dense row-major fp32 unless stated otherwise.
 *   - the library reads no environment variable (A/B switches and kernel-level hooks live in the
 *     lab build libm3pc_hip_lab.so only, declared in m3pc_hip_debug.h).
 *
 * Pipelined plan steps.  A rollout over independent windows (the reference's loops plan one window per
 * call: replay_buffer.py:204-232, learner.py:645-741) may keep several plan steps in flight: each step
 * owns one of M3PC_SLOTS step slots (m3pc_plan_args::slot: the policy head and returns tokens of its
 * policy pass), and the handle holds three workspaces -- the candidate workspace (m3pc_candidate_pass,
 * m3pc_plan_step_batch's candidate pass, m3pc_forward, m3pc_mtm_loss and m3pc_mtm_loss_replay (their forward), m3pc_score_actions of
 * more than max_rescore candidates or in bf16), the policy workspace (m3pc_policy_pass, m3pc_plan_step_batch's policy pass) and
 * the re-score workspace (m3pc_rescore* / fp32 m3pc_score_actions of <= max_rescore candidates).  Calls
 * that use the SAME workspace must be ordered on the device (same stream, or events); calls on different
 * workspaces may run on different streams at
 * the same time.  ABI v5: there are TWO policy workspaces and TWO re-score workspaces, picked by the parity of the step slot
 * (slot & 1): the policy passes / re-scores of two steps whose slots differ in parity may run on two streams at the same time.  m3pc_amd/planner.py (plan_async) is the reference user: candidate passes back to back
 * on the caller's stream, the policy passes and the re-scores of the neighbouring steps on two more.
 */
#ifndef M3PC_HIP_H
#define M3PC_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history.  Added within v7 (new symbols and structures only; nothing existing changed): m3pc_plan_step_certified,
 * m3pc_calibrate_delta, m3pc_cert_args, m3pc_cert_record; then m3pc_plan_step_certified_begin / _end, m3pc_set_step_streams and
 * m3pc_draw_variates; then m3pc_refit_resample, m3pc_refine_plan and m3pc_refine_args (CEM / MPPI refinement); then
 * m3pc_plan_steps_certified (a lock-step batch of certified steps); then m3pc_eval_bound, m3pc_plan_step_certified_eval and
 * m3pc_eval_record (the eval_action certificate); then m3pc_plan_step_certified_eval_begin / _eval_end and
 * m3pc_plan_steps_certified_eval (that certificate in the pipelined and the lock-step step); then m3pc_refine_plans (the
 * refinement of a lock-step batch of windows, with a shifted warm start); then m3pc_episodes_create / _destroy / _reset / _observe /
 * _record / _windows / _values / _export and the opaque m3pc_episodes (the episode store); then m3pc_replay_create / _destroy / _append /
 * _append_transitions / _push_episodes / _sample_segments / _sample_transitions / _values_up_bound / _counts / _path_lengths and the
 * opaque m3pc_replay (the replay buffer); then m3pc_iql_create / _destroy / _load / _export / _set_step / _get_step / _train_step / _train /
 * _publish_critic / _evaluate, m3pc_iql_args and the opaque m3pc_iql (the IQL trainer); then m3pc_mtm_loss_terms, m3pc_mtm_loss and
 * m3pc_mtm_loss_replay (the masked-trajectory loss); then m3pc_mtm_grad_create / _destroy / m3pc_mtm_grad / _replay / _export and
 * the opaque struct m3pc_mtm_grad (its gradient); then m3pc_mtm_opt_create / _destroy / _decays / _step / _export / _load / _get_state /
 * _set_state, m3pc_mtm_lr, m3pc_mtm_train_step, m3pc_mtm_train, m3pc_mtm_weights_export, m3pc_mtm_opt_args, m3pc_mtm_opt_state and
 * the opaque struct m3pc_mtm_opt (its optimizers).  v7: M3PC_PREC_BF16X3, a third precision of the candidate pass, accepted wherever a precision is taken
 * (m3pc_forward, m3pc_candidate_pass, m3pc_plan_step[_batch], m3pc_score_actions, m3pc_goal_step_batch, m3pc_profile_read); no new
 * entry point and no structure change.  v6 (round 6): no new entry point and no structure change; m3pc_rescore_merge now writes all 8 floats of its
 * host_stats block (slots 5..7 as zeros: a reader of the 8-float layout never sees an earlier race merge's values), so a caller
 * that passed the 5-float block of m3pc_topk_window must pass 8.  Inside the library: a bf16 candidate pass carries its residual
 * stream between the encoder layers in bf16 and runs the output heads' last Linear on bf16 hidden rows (scores move within the
 * bf16 deviation the certified re-score is calibrated on; fp32 passes are unchanged).  v5 (round 5): m3pc_topk_race_window, m3pc_rescore_merge_race, m3pc_merge_race_select (the certified multinomial
 * draw of the bf16 plan step); M3PC_PLAN_PRUNED_POLICY; m3pc_profile_enable(h, 3); the handle holds two chain workspaces per kind,
 * picked by the parity of m3pc_plan_args::slot.  v4: m3pc_goal_step_batch, m3pc_dims::max_goal_batch.  v3: M3PC_PLAN_DEFER_JOIN,
 * m3pc_candidate_join.  No structure changed layout in v5. */
#define M3PC_ABI_VERSION 7

#define M3PC_OK 0
#define M3PC_EINVAL (-1)   /* bad argument / shape mismatch            */
#define M3PC_ESTATE (-2)   /* weights / tokenizer / critic not loaded  */
#define M3PC_EHIP (-3)     /* HIP runtime error                        */
#define M3PC_ENOMEM (-4)   /* workspace too small for the request      */

/* modality order everywhere: the reference's dict insertion order
 * states, actions, rewards, returns (finetune_omtm/learner.py:348-366; mtm_model.py:625,676) */
#define M3PC_STATES 0
#define M3PC_ACTIONS 1
#define M3PC_REWARDS 2
#define M3PC_RETURNS 3

/* plan_guidance modes (finetune_omtm/learner.py:389-407) */
#define M3PC_MODE_RTG 0     /* rtg_guiding            learner.py:271-327 */
#define M3PC_MODE_CRITIC 1  /* critic_lambda_guiding  learner.py:211-268 */
#define M3PC_MODE_NOISE 2   /* noise_adding_lambda    learner.py:142-208 */

/* arithmetic of the batched candidate pass */
#define M3PC_PREC_FP32 0  /* fp32 operands, f32 MFMA (v_mfma_f32_32x32x2_f32), fp32 accumulate */
#define M3PC_PREC_BF16 1  /* bf16 operands, bf16 MFMA (v_mfma_f32_32x32x16_bf16), fp32 accumulate,
                             fp32 residual stream / LayerNorm / softmax */
#define M3PC_PREC_BF16X3 2 /* split bf16: the fp32 pass (fp32 activations, residual stream, attention, LayerNorm, heads) with its
                              weight GEMMs (K >= 32) as x = hi + lo, hi = bf16(x), lo = bf16(x - hi) (round to nearest even) for both
                              operands and a.w = a_hi.w_hi + a_hi.w_lo + a_lo.w_hi: three v_mfma_f32_32x32x16_bf16 per k-step into
                              one fp32 accumulator (relative error ~2^-16 per product) */

typedef struct m3pc_handle m3pc_handle;

/* static sizes of one planner instance: omtmConfig + data_shapes + traj_length
 * (mtm_model.py:200-221, 324-344; finetune_omtm/config.yaml:5,29-34) */
typedef struct m3pc_dims {
    int state_dim;      /* S */
    int action_dim;     /* A */
    int traj_length;    /* T  (cfg.traj_length == model max_len) */
    int n_embd;         /* d, multiple of 64 */
    int n_head;
    int n_enc_layer;
    int n_dec_layer;
    int max_candidates; /* largest n_count a plan_step call will use on this device */
    int max_batch;      /* largest B for m3pc_forward */
    int critic_hidden;  /* TwinQ hidden width (256), 0 = no critic */
    int max_rescore;    /* largest n of m3pc_rescore* / fp32 m3pc_score_actions that runs in the re-score
                           workspace (beside a candidate pass); 0 = 64 */
    int max_goal_batch; /* largest batch of m3pc_goal_step_batch (zero-shot windows per call); 0 = none.  ABI v4 */
} m3pc_dims;

/* step slots of a handle (see "Pipelined plan steps") */
#define M3PC_SLOTS 4

/* one entry of a state_dict: fp32, contiguous, torch layout */
typedef struct m3pc_named_tensor {
    const char* name;   /* e.g. "encoder.layers.0.self_attn.in_proj_weight" */
    const float* data;
    long long numel;
    int on_device;      /* 0: host pointer, 1: device pointer */
} m3pc_named_tensor;

typedef struct m3pc_plan_args {
    int mode;          /* M3PC_MODE_*                                                        */
    int precision;     /* M3PC_PREC_* for the candidate pass (the policy pass is always fp32) */
    int horizon;       /* effective h of this step (learner.py:342-345)                      */
    int n_total;       /* cfg.action_samples: leading dimension of eps                       */
    int n_begin;       /* first candidate scored by this call (candidate sharding)           */
    int n_count;       /* number of candidates scored by this call                           */
    double lmbda;      /* TD(lambda) mixing, python float in the reference (learner.py:313-316) */
    double discount;   /* gamma (learner.py:307-309)                                         */
    double rtg;        /* return-to-go written into every returns slot (learner.py:368-385)  */
    int slot;          /* step slot in [0, M3PC_SLOTS) holding this step's policy pass           */
    int returns_f64;   /* dtype of `returns`: 0 float32, 1 float64                               */
    const void* returns; /* optional device (T,) raw returns row of the window (what
                          trajectory["returns"] holds, learner.py:272-293); NULL: `rtg` everywhere */
    int flags;         /* M3PC_PLAN_* bits (m3pc_candidate_pass); 0 = none                       */
    int window;        /* m3pc_candidate_pass behind m3pc_policy_pass_batch: which of the slot's windows
                          this step plans (0 after a single-window m3pc_policy_pass)                */
} m3pc_plan_args;

/* m3pc_plan_args::flags.  M3PC_PLAN_DEFER_JOIN (m3pc_candidate_pass only): a large bf16 pass runs its candidate
 * parts on the caller's stream and on streams of the handle; by default the caller's stream waits for all of them
 * before the call returns to it (outputs complete in stream order).  With this bit it does not: the outputs of the
 * parts that ran elsewhere are complete only behind m3pc_candidate_join(h, slot, stream), and the caller's stream is
 * free to start the next step's first part while the last part of this one still runs (no idle tail per step). */
#define M3PC_PLAN_DEFER_JOIN 1
/* M3PC_PLAN_PRUNED_POLICY (m3pc_policy_pass only, with loc == std == NULL): the policy head is computed at the h action tokens
 * t >= T - h alone -- the rows a plan step samples its candidates from (learner.py:285-287 reads sample((N,))[:, 0, T-h:]) -- through
 * the exactly pruned decoder (those tokens are masked under the rcbc mask: shared query rows and masked-token K|V from the plan
 * tables, the kept tokens alone through decoder-embed / K|V, out-proj / FFN / actor head on h rows instead of 4T).  Rows t < T - h of
 * the slot's loc / std (what m3pc_candidate_pass copies out) are zero.  Same arithmetic per computed row up to fp32 re-association. */
#define M3PC_PLAN_PRUNED_POLICY 2
/* M3PC_PLAN_INPUTS_READY (m3pc_plan_step_certified_begin only): the window -- states, actions, rewards, the returns row -- is
 * complete already in the order of the slot's chain stream (written before the stream's earlier work was enqueued and since
 * synchronised, or copied on that chain stream: m3pc_set_step_streams), so the policy pass does not wait for the caller's stream,
 * that is for the candidate pass of the step before, and runs beside it.  eps and expo are read on the caller's stream and behind
 * it: they need no more than stream order either way.  The caller then also orders the chain streams behind whatever other entry
 * point used the handle last. */
#define M3PC_PLAN_INPUTS_READY 4

const char* m3pc_last_error(void);
int m3pc_abi_version(void);

/* Learner.__init__'s model construction (learner.py:32-36): allocates handle, weight arena and
 * workspace on `device`.  Synchronous. */
int m3pc_create(const m3pc_dims* dims, int device, m3pc_handle** out);
int m3pc_destroy(m3pc_handle* h);

/* omtm.load_state_dict (learner.py:33-35): tensors by state_dict name.
 * Unknown names are ignored.  The FIRST call must bring every required name; later calls may bring any
 * subset -- fine-tuning updates the weights between rollouts (finetune.py:306) -- and re-derive only what
 * depends on the tensors that came: their bf16 copies, the packed fragment streams of the layers they
 * belong to, the embedding tables, and (decoder-side tensors only) the cached mask-pattern tables.
 * Synchronous (the tensors may be released when the call returns). */
int m3pc_load_weights(m3pc_handle* h, const m3pc_named_tensor* tensors, int n, void* stream);
/* what the last m3pc_load_weights did: out4 = {tensors copied, fused-layer-tail streams re-packed,
 * fused-decoder-input streams re-packed, 1 if the cached decoder tables were invalidated} */
int m3pc_load_stats(m3pc_handle* h, long long* out4);

/* ContinuousTokenizer(mean, std, stats, normalize) (tokenizers/continuous.py:31-62):
 * host arrays of `dim` floats. */
int m3pc_set_tokenizer(m3pc_handle* h, int key, const float* mean, const float* std, int dim, int normalize);

/* TwinQ weights (finetune_omtm/model.py:146-171): "q1.net.0.weight" ... "q2.net.4.bias",
 * plus the observation mean / std attributes (host, state_dim floats each). */
int m3pc_set_critic(m3pc_handle* h, const m3pc_named_tensor* tensors, int n, const float* obs_mean,
                    const float* obs_std, void* stream);

/* ContinuousTokenizer.encode / decode (tokenizers/continuous.py:68-94) on device rows:
 * out = (in - mean) / std   resp.  out = in * std + mean  (identity when normalize == 0).
 * `in_f64` != 0: the input rows are float64 and are normalised in float64 before the cast
 * (the reference's behaviour for `returns`, learner.py:371-374). */
int m3pc_tokenize(m3pc_handle* h, int key, const void* in, int in_f64, float* out, long long rows, void* stream);
int m3pc_detokenize(m3pc_handle* h, int key, const float* in, float* out, long long rows, void* stream);

/* omtm.forward (mtm_model.py:593-607) for one token per timestep and modality.
 *   tokens[k]  device (B,T,D_k) tokenised inputs
 *   masks[k]   host   (T,) 0/1 bytes, shared by the batch (mtm_model.py:572-575)
 *   out_*      device, may be NULL to skip a head:
 *              out_states (B,T,S), out_rewards (B,T,1), out_returns (B,T,1)   raw head outputs
 *              out_mu / out_std (B,T,A)     DiagGaussianActor loc / std (mtm_model.py:313-321)
 */
int m3pc_forward(m3pc_handle* h, int batch, const float* const tokens[4], const unsigned char* const masks[4],
                 float* out_states, float* out_rewards, float* out_returns, float* out_mu, float* out_std,
                 int precision, void* stream);

/* Zero-shot goal reaching: both forwards of action_piid_sample (zeroshot_omtm/learner.py:151-261) in one call, on RAW
 * (un-normalised) windows -- the tokenizer is applied inside, as in m3pc_plan_step:
 *   path inference under the pi mask (zeroshot_omtm/masks.py:72-91) -> the de-tokenised predicted observations over the
 *   window rows [0, idx] and [idx+2, T-2] (learner.py:240-246) -> inverse dynamics under the fid mask (masks.py:30-47).
 *   batch      E independent windows (<= max_batch); states (E,T,S), actions (E,T,A), rewards (E,T,1) device
 *   rtg        host (E,) return-to-go per window, written into every returns slot (learner.py:205-223)
 *   masks_*    host (T,) 0/1 bytes per modality, as m3pc_forward;  idx = T - h
 *   inferred       device out (E,T,S): the de-tokenised states head of the first forward
 *   window_states  device out (E,T,S): the observation rows the second forward saw
 *   out_mu/out_std device out (E,T,A): DiagGaussianActor loc / std of the second forward (mtm_model.py:313-321)
 * fp32; runs in the policy workspace and uses step slot 0. */
int m3pc_goal_step(m3pc_handle* h, int batch, const float* states, const float* actions, const float* rewards,
                   const double* rtg, const unsigned char* const masks_pi[4], const unsigned char* const masks_fid[4],
                   int idx, float* inferred, float* window_states, float* out_mu, float* out_std, void* stream);

/* m3pc_goal_step for MANY windows per call (BASELINE config 5: 64 environments x 1024 = 8192 windows per GPU), exactly
 * pruned to what the reference reads of the two forwards and run in the arithmetic of the candidate pass:
 *   path inference (pi mask, zeroshot_omtm/masks.py:72-91): the states head is read at the window rows t <= idx and
 *   idx+2 <= t <= T-2 only (zeroshot_omtm/learner.py:240-246) -- those decoder tokens are the queries of the decoder layer;
 *   inverse dynamics (fid mask, masks.py:30-47): the action distribution is read at token idx only (learner.py:250-256) --
 *   ONE query per window.  Un-read decoder rows are never computed; read rows are computed as in m3pc_goal_step.
 *   Neither mask keeps a rewards or returns token, so those rows of the window (and the return-to-go) never enter the
 *   arithmetic: the call takes states and actions only.
 *   batch      E independent windows (<= max_goal_batch): states (E,T,S), actions (E,T,A) device, RAW (un-normalised)
 *   idx        T - h; the masks are built inside (plan tables cached per idx)
 *   goal_mode  M3PC_GOAL_PIID: action_piid_sample (learner.py:151-261), both forwards;
 *              M3PC_GOAL_ID:   action_id_sample (learner.py:60-149), one forward under the gid mask (masks.py:50-69)
 *   precision  M3PC_PREC_BF16: bf16 MFMA kernels of the candidate pass (fused layer tails); M3PC_PREC_FP32: fp32 MFMA;
 *              M3PC_PREC_BF16X3: the fp32 pass with split-bf16 weight GEMMs (see M3PC_PREC_BF16X3).
 *              Either way a window's result does not depend on which other windows share the call, as long as the
 *              batch sizes fall in the same kernel regime (environment sharding: no collective).  fp32: bit-identical at any
 *              batch size.  bf16: bit-identical between calls of the same regime; the regime boundaries are >= 2048 windows
 *              (the call runs as two parts on two streams), >= 12288 token rows per pass (fused layer tails; below: the
 *              split / GEMM forms), >= 64 windows (two short windows per attention tile) and >= 1024 (window, head) items
 *              (pipelined attention) -- a remainder shard that crosses one agrees with the unsharded call to the bf16
 *              tolerance (|d loc| <= 3e-2), not bit for bit; shard evenly, or use fp32, where bits must match.
 *   window_states  device out (E,T,S), optional: the observation rows the inverse-dynamics forward saw
 *   out_mu/out_std device out (E,A): DiagGaussianActor loc / std at token idx (mtm_model.py:313-321)
 * Runs in the candidate workspace. */
#define M3PC_GOAL_PIID 0
#define M3PC_GOAL_ID 1
int m3pc_goal_step_batch(m3pc_handle* h, int batch, const float* states, const float* actions, int idx, int goal_mode,
                         int precision, float* window_states, float* out_mu, float* out_std, void* stream);

/* The two halves of m3pc_plan_step as calls of their own, for pipelined callers:
 *   m3pc_policy_pass     learner.py:278-284: returns tokens + return-conditioned policy (batch 1, rcbc
 *                        mask, fp32) -> loc / std of the slot (and the caller's copies, optional).  Policy
 *                        workspace.
 *   m3pc_candidate_pass  learner.py:285-316: candidates from the slot's policy head and eps, batched
 *                        forward under the fd mask, TD(lambda) scores.  Candidate workspace.  Arguments as
 *                        m3pc_plan_step. */
int m3pc_policy_pass(m3pc_handle* h, const m3pc_plan_args* args, const float* states, const float* actions,
                     const float* rewards, float* loc, float* std, void* stream);
int m3pc_candidate_pass(m3pc_handle* h, const m3pc_plan_args* args, const float* states, const float* actions,
                        const float* rewards, const float* eps, float* loc, float* std, float* sample_actions,
                        float* expect_return, float* pred_rewards, float* pred_boot, void* stream);
/* The policy passes of E independent windows as ONE pass at batch E (learner.py:278-284 per window; several
 * environments step together: replay_buffer.py:204-232 per environment): states (E,T,S), actions (E,T,A), rewards (E,T,1)
 * device, rtg host (E,).  The slot then holds E policy heads; m3pc_candidate_pass plans window w of them with
 * m3pc_plan_args::window = w and that window's rows of states / actions / rewards.  loc / std: optional (E,T,A) out.
 * args: mode, horizon, slot are read.  E <= max_batch.  The few-row fp32 kernels choose their tiling by the row count, so
 * a window's policy head agrees with the single-window pass to fp32 rounding, not bit for bit. */
int m3pc_policy_pass_batch(m3pc_handle* h, const m3pc_plan_args* args, int n_windows, const float* states,
                           const float* actions, const float* rewards, const double* rtg, float* loc, float* std,
                           void* stream);
/* Orders `stream` behind every part of the last m3pc_candidate_pass(M3PC_PLAN_DEFER_JOIN) of step slot `slot`
 * (no-op when that pass joined by itself or ran in one part).  The consumer of a step's scores -- the re-score +
 * select of learner.py:318-325 -- calls it on its own stream. */
int m3pc_candidate_join(m3pc_handle* h, int slot, void* stream);

/* One MPC plan step up to (not including) the cross-candidate select:
 * rtg_guiding / critic_lambda_guiding / noise_adding_lambda (learner.py:142-316).
 *   states/actions/rewards   device (T,S) (T,A) (T,1): the raw (un-normalised) window assembled by
 *                            action_sample (learner.py:348-366), future rows zero
 *   eps       device standard normals: (n_total,T,A) for RTG/CRITIC -- the reference draws
 *             dist.sample((N,)) over every timestep (learner.py:285-287) -- or (n_total,h,A)
 *             for NOISE (learner.py:157-163)
 *   loc,std   device out (T,A), optional: the policy pass distribution
 *   sample_actions  device out (n_count,h,A): candidates [n_begin, n_begin+n_count)
 *   expect_return   device out (n_count,): TD(lambda) scores BEFORE the max shift
 *   pred_rewards, pred_boot  device out (n_count,h), optional: decoded predicted rewards and
 *             the bootstrap term (1000 x predicted return, or min(q1,q2))
 */
int m3pc_plan_step(m3pc_handle* h, const m3pc_plan_args* args, const float* states, const float* actions,
                   const float* rewards, const float* eps, float* loc, float* std, float* sample_actions,
                   float* expect_return, float* pred_rewards, float* pred_boot, void* stream);

/* Score caller-supplied candidate action sequences: learner.py:288-316 (from the overwrite of the window's future actions
 * on), without the policy pass and without sampling.  Serves the fp32 re-score of batched plans, CEM-style refinement
 * (sequence_dataset.py:919-1000) and any caller that brings its own candidates.
 *   n_windows E >= 1 history windows: states (E,T,S), actions (E,T,A), rewards (E,T,1) device, raw (un-normalised)
 *   cand            device (n_count,h,A): the candidates' actions of the last h steps (rows < T-h come from the window)
 *   window_index    device (n_count,) int32: the window each candidate continues; NULL = all window 0 (E == 1)
 *   args            mode (RTG or CRITIC scoring), precision, horizon, n_count, lmbda, discount are read
 *   expect_return   device out (n_count,); pred_rewards / pred_boot device out (n_count,h), optional */
int m3pc_score_actions(m3pc_handle* h, const m3pc_plan_args* args, int n_windows, const float* states,
                       const float* actions, const float* rewards, const float* cand, const int* window_index,
                       float* expect_return, float* pred_rewards, float* pred_boot, void* stream);

/* m3pc_plan_step for E independent windows in one pass of the kernels (the counterpart of a rollout loop that steps E
 * environments: replay_buffer.py:204-232 / learner.py:681-691 plan one window per call): policy pass at batch E,
 * args->n_total candidates per window, one candidate pass over all E * n_total rows.  All windows share the horizon.
 *   states (E,T,S), actions (E,T,A), rewards (E,T,1) device;  rtg host (E,) doubles
 *   eps device (E, n_total, T, A) [RTG/CRITIC] or (E, n_total, h, A) [NOISE];  window_index device (E*n_total,) int32 = c / n_total
 *   loc, std device out (E,T,A), optional;  sample_actions device out (E*n_total,h,A);  expect_return device out (E*n_total,) */
int m3pc_plan_step_batch(m3pc_handle* h, const m3pc_plan_args* args, int n_windows, const float* states,
                         const float* actions, const float* rewards, const double* rtg, const float* eps,
                         const int* window_index, float* loc, float* std, float* sample_actions, float* expect_return,
                         void* stream);

/* fp32 re-scoring of an arbitrary subset of the candidates of the plan step that owns args->slot
 * (its policy-pass loc/std are reused; same window, eps and args as that call, args->precision ignored).
 * Runs in the re-score workspace when n <= max_rescore, else in the candidate workspace.
 * Used after a bf16 candidate pass to make the reported arg-max independent of bf16 rounding: the same
 * learner.py:288-316 arithmetic, restricted to rows `index`.
 *   index           device (n,) int32 candidate ids in [0, n_total)
 *   sample_actions  device out (n,h,A), optional
 *   expect_return   device out (n,) */
int m3pc_rescore(m3pc_handle* h, const m3pc_plan_args* args, const float* states, const float* actions,
                 const float* rewards, const float* eps, const int* index, int n, float* sample_actions,
                 float* expect_return, void* stream);

/* m3pc_rescore of the k best entries of a full score vector, written back in place:
 *   expect_return  device in/out (n_total,): scores of ALL candidates (after the all-gather when
 *                  sharded); its k largest entries are replaced by their fp32 re-scores
 *   topk_index     device out (k,) int32, optional: the re-scored candidate ids, best first */
int m3pc_rescore_topk(m3pc_handle* h, const m3pc_plan_args* args, const float* states, const float* actions,
                      const float* rewards, const float* eps, float* expect_return, int k, int* topk_index,
                      void* stream);

/* Bound-driven re-score set (the arg-max of learner.py:318-325 must not depend on bf16 rounding): if every bf16 score is
 * within delta of its fp32 value up to a common shift, the fp32 arg-max lies among the candidates whose bf16 score is
 * within window = 2 delta of the bf16 maximum.  Finds the kmax + 1 best entries of expect_return (descending; ties to the
 * lower index) and n = clamp(#{E_i >= max E - window}, kmin, kmax).
 *   topk_index  device out (kmax + 1,) int32
 *   stats       device out float[4]: {n, max E - (best E not among the n) [inf if none], max E, the count over ALL n_total
 *               entries, unclamped: > kmax means the listed prefix does not cover the window}
 *   top_scores  device out (kmax + 1,), optional: expect_return[topk_index[i]] (kept for m3pc_rescore_merge)
 *   host_stats  optional: host-mapped (pinned) float[5] the kernel also writes -- the four stats, then `seq` into [4] with
 *               system scope; a caller that spins on host_stats[4] == seq reads n without a stream synchronisation */
int m3pc_topk_window(m3pc_handle* h, const float* expect_return, int n_total, int kmax, int kmin, float window,
                     int* topk_index, float* stats, float* top_scores, float* host_stats, float seq, void* stream);
/* The score vector the select runs on after a partial fp32 re-score, and the certificate that the partial re-score was
 * enough.  bf16 scores and their fp32 values differ by a common shift c plus a bounded deviation, so un-re-scored entries
 * are brought onto the fp32 scale before they meet the re-scored ones in one softmax / arg-max (learner.py:318-325):
 *   index / top_scores / top_rescored: the n best candidates by bf16 score (best first: m3pc_topk_window), their bf16
 *   scores and their fp32 re-scores (m3pc_rescore)
 *   c = lower median over the n listed entries of (top_scores[i] - top_rescored[i])
 *   merged[j] = scores[j] - c for all j < n_total;  merged[index[i]] = top_rescored[i]
 *   With |(bf16_j - fp32_j) - c| <= delta for every candidate, an un-listed j can hold the fp32 arg-max only if
 *   scores[j] > f* + c - delta (f* = the best re-scored fp32 score).  need = #{j : scores[j] > f* + c - delta}: need <= n
 *   certifies arg-max(merged) = the fp32 arg-max; otherwise re-score entries n .. need-1 of the order and merge again
 *   (need can only shrink).
 *   stats device out float[4] = {c, max_i |top_scores[i] - top_rescored[i] - c|, need, threshold - best un-listed score};
 *   host_stats / seq as for m3pc_topk_window, except that host_stats must hold 8 floats here: slots 5..7 are written as zeros,
 *   so that a reader of the 8-float layout of m3pc_rescore_merge_race never sees an earlier race merge's values on the same
 *   buffer.  `merged` may alias `scores`. */
int m3pc_rescore_merge(m3pc_handle* h, const float* scores, int n_total, const int* index, int n, const float* top_scores,
                       const float* top_rescored, float delta, float* merged, float* stats, float* host_stats, float seq,
                       void* stream);
/* The SAMPLED action of a plan step (learner.py:324-325: sample_action = a0[torch.multinomial(p, 1)], the action every online
 * rollout step executes, replay_buffer.py:206-216) must not depend on bf16 rounding either.  torch.multinomial(p, 1) is
 * arg-max_j p_j / q_j with q ~ Exp(1) (m3pc_select), and with p = softmax(temperature (E - max E)) that is the race
 * arg-max_j (temperature E_j - log q_j).  An un-re-scored candidate's key is off by at most temperature * delta, so only
 * candidates whose bf16 key comes within 2 temperature delta of the best can win: ABI v5 lists them, re-scores them beside the
 * best-by-score candidates and certifies the draw as m3pc_rescore_merge certifies the arg-max.
 *
 * m3pc_topk_race_window: m3pc_topk_window (window = 0) plus the rmax best candidates by race key, both in ONE list of
 * rmax + kmax + 1 entries laid out for contiguous slices:
 *   list[rmax + i]      the i-th best candidate by score (i <= kmax), best first
 *   list[rmax - 1 - i]  the i-th best candidate by race key temperature * E_j - log expo_j (i < rmax)
 * so "the r best racers and the n best scorers" is list[rmax - r .. rmax + n): one m3pc_rescore call, one merge.
 *   expo         device (n_total,) the Exp(1) variates m3pc_select will draw with
 *   list_scores  device out (rmax + kmax + 1,), optional: expect_return[list[i]]
 *   stats / host_stats / seq as m3pc_topk_window (of the score part); stats may be NULL (one launch fewer up to 2048 candidates:
 *   the ranking kernel writes list_scores itself).  rmax <= min(64, n_total). */
int m3pc_topk_race_window(m3pc_handle* h, const float* expect_return, const float* expo, float temperature, int n_total, int kmax,
                          int kmin, int rmax, int* list, float* stats, float* list_scores, float* host_stats, float seq, void* stream);
/* m3pc_rescore_merge over such a list: `list` = r race entries followed by n score entries (a slice of the list above),
 * list_scores / list_rescored their bf16 scores and fp32 re-scores.  The shift c, the deviation, merged[] and the arg-max
 * certificate (need) are m3pc_rescore_merge's over all r + n entries.  Race certificate: K* = max over the listed entries of
 * (temperature * rescored_i - log expo_i); need_race = #{j : temperature * scores[j] - log expo[j] >= K* + temperature (c - delta)}
 * over the whole vector: need_race <= r certifies that the draw arg-max_j merged-p_j / expo_j is the fp32 draw; otherwise re-score
 * the race entries r .. need_race-1 and merge again.
 *   stats device out float[8] = {c, deviation, need, margin, -, need_race, K*, K* + temperature (c - delta)}; the host copy
 *   carries `seq` in slot 4 (host_stats must hold 8 floats).  r + n <= 1024. */
int m3pc_rescore_merge_race(m3pc_handle* h, const float* scores, const float* expo, float temperature, int n_total, const int* list,
                            int r, int n, const float* list_scores, const float* list_rescored, float delta, float* merged,
                            float* stats, float* host_stats, float seq, void* stream);
/* m3pc_rescore_merge_race followed by m3pc_select on the merged vector (with the same expo / temperature), in ONE launch: both are
 * one workgroup over the whole vector, and the re-score's tail is a chain of dependent launches.  The certificate's statistics
 * reach host_stats before the select part runs.  Arguments as the two calls.
 * Contract: scores and list_rescored hold no NaN (m3pc_select's contract applies to the merged vector the select part reads). */
int m3pc_merge_race_select(m3pc_handle* h, const float* scores, const float* expo, float temperature, int n_total, const int* list,
                           int r, int n, const float* list_scores, const float* list_rescored, float delta, float* merged,
                           float* stats, float* host_stats, float seq, const float* a0, long long a0_stride, float* p,
                           float* eval_action, int* argmax, int* sample_idx, float* sample_action, void* stream);
/* m3pc_rescore of the n listed candidates (device int32 ids), written back into the full score vector in place. */
int m3pc_rescore_listed(m3pc_handle* h, const m3pc_plan_args* args, const float* states, const float* actions,
                        const float* rewards, const float* eps, const int* index, int n, float* expect_return,
                        void* stream);

/* The cross-candidate tail (learner.py:318-325) over all N candidates (after an all-gather when
 * sharded): p = softmax(temperature * (E - max E)), eval_action = sum p*a0 / sum p, argmax E, and the
 * multinomial draw sample_action = a0[multinomial(p, 1)].
 *   a0 device (n, A) rows with stride a0_stride floats (sample_actions[:,0,:] => stride h*A)
 *   expo      device (n,) Exp(1) variates, optional.  torch.multinomial(p, 1) is argmax(p / q) with
 *             q = empty_like(p).exponential_(1) drawn from the caller's generator; passing that q
 *             here reproduces torch's draw without its dozen tiny launches.
 *   p device out (n,), eval_action device out (A,), argmax device out (1,),
 *   sample_idx device out (1,), sample_action device out (A,) -- each optional
 * Contract: expect_return holds no NaN.  A NaN score is never picked by the arg-max or by the race; a vector of NaN alone leaves
 * 0x7fffffff as the index, and sample_action would be gathered from there.  The caller keeps NaN out; +-inf scores are ordered. */
int m3pc_select(m3pc_handle* h, const float* expect_return, const float* a0, long long a0_stride, int n,
                float temperature, const float* expo, float* p, float* eval_action, int* argmax,
                int* sample_idx, float* sample_action, void* stream);

/* The CERTIFIED plan step as one call: learner.py:278-325 with the candidate pass in bf16 / split bf16 and both returned actions
 * -- the arg-max behind eval_action (learner.py:318-323) and the multinomial draw behind sample_action (learner.py:324-325) --
 * following the fp32 path's decisions.  It is the protocol of m3pc_amd/certificate.py (resolve) for a serial step, made of the
 * calls above in the same order, all on `stream`:
 *   m3pc_policy_pass (honours M3PC_PLAN_PRUNED_POLICY) -> m3pc_candidate_pass in args->precision -> m3pc_topk_race_window
 *   (m3pc_topk_window when rmax == 0) -> m3pc_rescore of list[rmax - rfirst .. rmax + kmin) -> m3pc_merge_race_select -> read the
 *   certificates (need, need_race) -> while one asks for more: raise delta (grow_delta), m3pc_rescore of the score entries up to
 *   `need` (<= kmax) / of the race entries up to `need_race` (<= rmax), merge + select again.
 *   Window set (need > kmax, need <= 1024 - 32): the `need` best candidates by low-precision score (descending, ties to the lower
 *   index: m3pc_topk_window's order) are listed in place of the score entries and re-scored in chunks of max_rescore.
 *   Everything (a larger window set, an exhausted race list, or a window set whose certificate still asks for more): one fp32
 *   m3pc_candidate_pass in the candidate workspace, stream-ordered, no device-wide synchronisation; the select then runs on fp32
 *   scores alone (record: everything = 1, n_rescored = n_total).
 * args->precision == M3PC_PREC_FP32: m3pc_plan_step + m3pc_select, record {certified = 1, everything = 1, n_rescored = n_total};
 * m3pc_cert_args is then read for its temperature only.  One rank: n_begin == 0 and n_count == n_total (<= 16384), else
 * M3PC_EINVAL.  Bad kmin / kmax / rfirst / rmax and null required pointers return M3PC_EINVAL before any HIP call.
 *   expo            device (n_total,) the Exp(1) variates of the draw (m3pc_select)
 *   loc, std        device out (T,A), optional;  sample_actions device out (n_total,h,A)
 *   scores_low      device out (n_total,): the candidate pass's scores
 *   merged          device out (n_total,): the vector the select ran on (m3pc_rescore_merge)
 *   list            device out (rmax + 1024,) int32, optional: the final lists -- the n_race re-scored race entries in front of
 *                   list[rmax], the n_rescored re-scored score entries from list[rmax] on (not after `everything`)
 *   p, eval_action, argmax, sample_idx, sample_action   device out, each optional, as m3pc_select
 *   record          host out, valid on return; every device output is complete in stream order
 * The certificates are read from a pinned host-mapped block the handle owns per step slot (the host_stats / seq mechanism of
 * m3pc_rescore_merge): the host spins on the sequence number for at most 10 s, then synchronises `stream` once and reads the
 * device copy; M3PC_EHIP if that fails too.  The host blocks until the LAST certificate of the step has been read. */
typedef struct m3pc_cert_args {
    float temperature;   /* cfg.temperature (learner.py:319) */
    float delta;         /* bound on |(low - fp32) - shift| going in (m3pc_calibrate_delta) */
    int grow_delta;      /* 1: raise delta to 1.5 x the deviation this step's re-scored set shows; 0: delta is fixed */
    int kmin, kmax;      /* first-pass / listed score entries; 1 <= kmin <= min(kmax, n_total), kmax + rmax <= 1023 */
    int rfirst, rmax;    /* first-pass / listed race entries; 1 <= rfirst <= rmax <= min(64, n_total), or rmax == rfirst == 0:
                            the arg-max certificate only (the draw is then a near-winner of the fp32 draw) */
} m3pc_cert_args;

typedef struct m3pc_cert_record {
    int n_rescored, n_race;            /* score / race entries re-scored in fp32 at the end */
    int need_first, need_race_first;   /* what the FIRST certificates asked for */
    int saturated, everything, certified, rounds;  /* window set taken / fp32 scores for every candidate / the step ended on
                                                      satisfied certificates (it cannot end otherwise) / merges issued */
    float delta, shift, deviation, margin;  /* delta coming out (>= going in); the LAST merge's common shift, largest deviation
                                               from it, and margin of the arg-max threshold over the best un-listed score */
} m3pc_cert_record;

int m3pc_plan_step_certified(m3pc_handle* h, const m3pc_plan_args* args, const m3pc_cert_args* cert, const float* states,
                             const float* actions, const float* rewards, const float* eps, const float* expo, float* loc, float* std,
                             float* sample_actions, float* scores_low, float* merged, int* list, float* p, float* eval_action,
                             int* argmax, int* sample_idx, float* sample_action, m3pc_cert_record* record, void* stream);

/* The THIRD certificate: eval_action (learner.py:318-323), the softmax-weighted mean of the first actions over ALL candidates and
 * what every eval=True call returns.  Candidates that were not re-scored enter it with shift-corrected low-precision scores; under
 * the model the other two certificates rest on -- every un-re-scored merged score is within delta of its fp32 value -- the
 * deviation of eval_action from the fp32 step's is bounded per step.  After the last merge, with m the merged vector, L the
 * re-scored candidates (race and score entries: m_j = f_j there), U all others, tau the temperature, eps = tau delta,
 * p = softmax(tau (m - max m)) and e = sum_j p_j a0_j the eval_action the select produced, for every action component k:
 *     S_k = sum_{j in U} p_j |a0_jk - e_k|      P_U = sum_{j in U} p_j
 *     B_k = expm1(eps) S_k / (1 - (1 - exp(-eps)) P_U)      eval_bound = max_k B_k
 * Claim: if |m_j - f_j| <= delta on U, then |e_k - e32_k| <= B_k, e32 being the select on fp32 scores.  (The fp32 weights are
 * w_j r_j with r_j in [exp(-eps), exp(eps)] on U and 1 on L; sum_j w_j (a_j - e) = 0 gives
 * e32 - e = sum_U w_j (r_j - 1)(a_j - e) / sum_j w_j r_j; the numerator is at most expm1(eps) sum_U w_j |a_j - e|, the denominator
 * at least W (1 - (1 - exp(-eps)) P_U).)  delta is calibrated, not proven (m3pc_calibrate_delta): the bound inherits the measured
 * exceedance rate of the other two certificates.
 * need_eval: the score list holds n_listed entries (best low-precision score first), the first n of them re-scored.  bound(n'),
 * n <= n' <= n_listed, is the formula on the CURRENT m and e with the score entries n .. n'-1 moved from U to L (an entry that is a
 * re-scored race entry too is in L either way and counts once); it does not increase with n'.  need_eval = the smallest n' with
 * bound(n') <= eval_tol, or n_total when even bound(n_listed) exceeds it (the list cannot reach the tolerance).
 *
 * m3pc_eval_bound: the certificate as a call (one launch of one workgroup; fixed-order reductions: bit-identical from run to run).
 *   merged     device (n_total,): the vector the select ran on;  a0 device (n_total, A) rows of stride a0_stride floats
 *   list       device int32: r re-scored race entries, then n_listed score entries -- the layout m3pc_rescore_merge_race takes, with
 *              the listed but un-re-scored score entries behind the n re-scored ones.  An id outside [0, n_total) is ignored.
 *   eval_tol   > 0; +inf: report only (need_eval = n)
 *   stats      device out float[8] = {eval_bound = bound(n), need_eval, P_U, the k that attains eval_bound, -, eps, bound(n_listed),
 *              |U|};  host_stats / seq: optional host-mapped float[8] copy closed by `seq` in slot 4, as m3pc_rescore_merge
 * M3PC_EINVAL before any HIP call: a null required pointer (h, merged, list, a0, stats), eval_tol <= 0 or NaN, delta < 0 or NaN,
 * n_total outside [1, 16384], A outside [1, 1024], r < 0, r + n_listed > 1024, n outside [0, n_listed].  The temperature enters as
 * |temperature|. */
int m3pc_eval_bound(m3pc_handle* h, const float* merged, int n_total, const int* list, int r, int n, int n_listed, const float* a0,
                    long long a0_stride, int A, float temperature, float delta, float eval_tol, float* stats, float* host_stats,
                    float seq, void* stream);

/* m3pc_plan_step_certified with the eval_action certificate as a third one beside `need` and `need_race`: the same step, and once
 * the arg-max and race certificates are satisfied and nothing is to be redone, m3pc_eval_bound runs behind the last merge + select
 * (list = the re-scored race entries and the kmax listed score entries, delta = the bound as it stands) and reports into a second
 * host-mapped block of the step slot (allocated at the first such call; the bounded wait of m3pc_plan_step_certified).
 *   need_eval > n_rescored, need_eval <= kmax: m3pc_rescore of the score entries up to need_eval, merge + select again, all three
 *   certificates read again (grow_delta may raise delta and ask again); n_rescored strictly grows, so the loop ends.
 *   need_eval = n_total (the list cannot reach eval_tol; also behind a window set, whose list is wholly re-scored): the existing
 *   every-candidate-in-fp32 path; records: everything = 1, eval_bound = 0, eval_certified = 1.
 *   args->precision == M3PC_PREC_FP32: erec = {0, 0, 0, 0, 1}.
 *   eval_tol = +inf: ONE bound launch, no extension -- every output buffer and every field of `record` is bit for bit what
 *   m3pc_plan_step_certified gives on the same inputs.
 * Which tier reaches a tolerance: at a nearly flat softmax (rtg guidance, temperature 0.01) bf16's delta leaves a bound of ~3e-2
 * that no list lowers to 1e-3 -- the tier that certifies eval_action there is M3PC_PREC_BF16X3 (bound ~6e-5 with nothing extra
 * re-scored); where the list holds a good share of the softmax weight (few candidates, peaked scores) a few dozen fp32 rows
 * tighten a bf16 step's bound.  DESIGN.md section 5 has the measured table.
 * Refusals: those of m3pc_plan_step_certified, plus erec == NULL and eval_tol <= 0 or NaN (M3PC_EINVAL, before any HIP call), plus
 * M3PC_ESTATE while a pipelined step is begun.
 * The same certificate in the pipelined step: m3pc_plan_step_certified_eval_begin / _eval_end below; in a lock-step batch:
 * m3pc_plan_steps_certified_eval.  This call keeps its launch sequence. */
typedef struct m3pc_eval_record {
    float eval_bound;      /* the LAST bound: |eval_action - fp32 eval_action| <= eval_bound under the delta model; 0 after `everything` */
    int need_eval_first;   /* what the FIRST eval certificate asked for (n_total: the list could not reach eval_tol) */
    int n_eval;            /* score entries re-scored because THIS certificate asked, beyond what the other two asked for */
    int eval_rounds;       /* bound launches */
    int eval_certified;    /* eval_bound <= eval_tol at the end */
} m3pc_eval_record;

int m3pc_plan_step_certified_eval(m3pc_handle* h, const m3pc_plan_args* args, const m3pc_cert_args* cert, const float* states,
                                  const float* actions, const float* rewards, const float* eps, const float* expo, float* loc,
                                  float* std, float* sample_actions, float* scores_low, float* merged, int* list, float* p,
                                  float* eval_action, int* argmax, int* sample_idx, float* sample_action, m3pc_cert_record* record,
                                  float eval_tol, m3pc_eval_record* erec, void* stream);

/* Pipelined certified steps: m3pc_plan_step_certified in two halves, so that a host keeps up to M3PC_SLOTS steps in flight (the
 * rate of m3pc_amd/planner.py's plan_async, from the library alone).  _begin enqueues and returns: it reads nothing from the device
 * and never waits on it.  _end resolves the step begun in `slot`.  For the same inputs the two calls produce exactly what
 * m3pc_plan_step_certified produces -- every output buffer and every field of the record, bit for bit -- at any depth
 * 1..M3PC_SLOTS, with the _ends in any order, in every regime of the certificate and for every precision.
 *   Schedule (planner.py's default: alternate chain streams, tail stream, deferred join).  The policy pass of the step in slot s
 *   goes to chain stream s & 1, behind `stream` as it stands at _begin (M3PC_PLAN_INPUTS_READY: without waiting for it).  The candidate pass goes to `stream` behind it, with
 *   M3PC_PLAN_DEFER_JOIN; `stream` carries nothing else of the step, so consecutive steps' candidate passes run back to back.  The
 *   step's tail -- m3pc_candidate_join, lists, first fp32 re-score, merge + certificates + select -- runs on the chain stream and is
 *   enqueued behind the policy pass of the next _begin that uses that chain stream, or by _end if it is still pending then.
 *   _end reads the certificates (the bounded wait of m3pc_plan_step_certified, the only host wait), enqueues on the chain stream
 *   what they ask for, orders `stream` behind the step's last kernel and fills the record.  What a slow path runs in the
 *   candidate workspace (a re-score of more than max_rescore candidates, the fp32 pass over every candidate) is ordered by events
 *   behind every candidate pass enqueued so far, and later candidate passes behind it: no device-wide synchronisation.
 *   Buffers.  The window, eps and expo must be complete in `stream` order at _begin; they and every output buffer must stay
 *   untouched until _end of the slot has returned.  The outputs are complete in the order of _end's `stream`.
 *   State.  _begin on a slot whose step has not been ended, _end on a slot with no begun step, and m3pc_plan_step_certified /
 *   m3pc_calibrate_delta / m3pc_set_step_streams with any step begun return M3PC_ESTATE.  Bad arguments (the checks of
 *   m3pc_plan_step_certified) return M3PC_EINVAL and leave the handle usable.  Every OTHER compute entry point of the handle is
 *   called with no step begun, and on a stream that the next _begin's `stream` is ordered behind (what HipPlanner._drain /
 *   _mark_main enforce in Python).  m3pc_destroy drains.
 *   Adaptive state (delta going in, kmin, rfirst) stays the caller's, per _begin; the record of _end carries what it folds back.
 * m3pc_set_step_streams (optional): the two chain streams (slot parity 0 / 1).  Not called, or NULLs: the handle creates two
 * non-blocking streams of its own at the first _begin.  A process that already owns such a pair (m3pc_amd/planner.py) passes it,
 * so that the process stays within the device's four hardware queues. */
int m3pc_set_step_streams(m3pc_handle* h, void* chain0, void* chain1);
int m3pc_plan_step_certified_begin(m3pc_handle* h, const m3pc_plan_args* args, const m3pc_cert_args* cert, const float* states,
                                   const float* actions, const float* rewards, const float* eps, const float* expo, float* loc,
                                   float* std, float* sample_actions, float* scores_low, float* merged, int* list, float* p,
                                   float* eval_action, int* argmax, int* sample_idx, float* sample_action, void* stream);
int m3pc_plan_step_certified_end(m3pc_handle* h, int slot, m3pc_cert_record* record, void* stream);

/* m3pc_plan_step_certified_eval in two halves: schedule, buffers and state rules are those of _begin / _end above.  For the same
 * inputs the pair produces exactly what m3pc_plan_step_certified_eval produces -- every output buffer, every field of `record` and
 * every field of `erec`, bit for bit -- at any depth 1..M3PC_SLOTS, with the _ends in any order, with plain and eval steps mixed in
 * flight, in every regime of the certificates and for every precision (M3PC_PREC_FP32: erec = {0, 0, 0, 0, 1}).
 *   No second host wait in the common case.  When the step's tail is enqueued, m3pc_eval_bound goes out on the chain stream right
 *   behind the first merge + select, for the state that pass assumes (r = rfirst, n = kmin, n_listed = min(kmax, n_total), delta as
 *   it came in), into the slot's second host-mapped block.  _eval_end reads the two certificates; if they ask for nothing -- no
 *   further merge was issued, delta is unchanged -- that launch IS the serial call's bound launch (same kernel, same inputs, same
 *   bits) and its statistics are taken.  Otherwise it is dropped, and the bound is launched behind the last merge and waited for
 *   as in the serial call.  What the bound asks for is re-scored in _eval_end on the chain stream, like every other extension.
 *   erec->eval_rounds counts the bounds the loop read: a dropped launch is not one.
 *   Mixing.  m3pc_plan_step_certified_end on a slot begun with _eval_begin resolves the two certificates only (the block written in
 *   advance is ignored).  _eval_end on a slot begun with m3pc_plan_step_certified_begin returns M3PC_ESTATE and leaves the step
 *   begun.  eval_tol <= 0 or NaN, and erec == NULL, return M3PC_EINVAL before any HIP call.  m3pc_plan_step_certified_eval with a
 *   step begun returns M3PC_ESTATE.  No new streams, no device-wide synchronisation, the bounded wait of the other certificates.
 * examples/pipelined_eval.c is a complete host. */
int m3pc_plan_step_certified_eval_begin(m3pc_handle* h, const m3pc_plan_args* args, const m3pc_cert_args* cert, const float* states,
                                        const float* actions, const float* rewards, const float* eps, const float* expo, float* loc,
                                        float* std, float* sample_actions, float* scores_low, float* merged, int* list, float* p,
                                        float* eval_action, int* argmax, int* sample_idx, float* sample_action, float eval_tol,
                                        void* stream);
int m3pc_plan_step_certified_eval_end(m3pc_handle* h, int slot, m3pc_cert_record* record, m3pc_eval_record* erec, void* stream);

/* A LOCK-STEP BATCH of certified plan steps as one call: E = n_windows environments that step together (replay_buffer.py:204-232 per
 * environment), all windows sharing one effective horizon.  It is the protocol of m3pc_amd/lockstep.py (action_sample_batch(lockstep=True))
 * restated in C, everything on `stream`, in the serial form (there is no _begin / _end split of this call):
 *   1. m3pc_policy_pass_batch into args->slot (args->flags, args->window and args->rtg are ignored; rtg comes per window)
 *   2. E x m3pc_candidate_pass (window = w, that window's rows, M3PC_PLAN_DEFER_JOIN) in args->precision, one m3pc_candidate_join
 *   3. the lists of m3pc_topk_race_window (m3pc_topk_window when rmax == 0) of all windows in ONE launch
 *   4. list[rmax - rfirst .. rmax + kmin) of every window gathered window-major, with the window index beside it
 *   5. ONE fp32 m3pc_score_actions over those E (rfirst + kmin) rows (RTG scoring for M3PC_MODE_RTG, else CRITIC scoring)
 *   6. merge + certificates + select of all windows in ONE launch, each window's statistics to a host-mapped block of its own
 *   7. ONE bounded wait for the E sequence numbers (at most 10 s, then one synchronisation of `stream` and the device copies)
 *   8. per window, in ascending order, the loop of m3pc_plan_step_certified on the window's certificates.  Its fp32 re-scores are
 *      m3pc_score_actions calls with n_windows = 1 on the window's own rows, over gathered slices of its list in chunks of max_rescore
 *      (score entries up to `need`, race entries up to `need_race`, the window set); its merges are the one-window
 *      m3pc_merge_race_select (m3pc_rescore_merge + m3pc_select when rmax == 0) on the window's rows and host block.  Everything: ONE
 *      fp32 m3pc_score_actions over all n_total candidates of the window, the best entry merged with itself at delta 0, the select.
 * delta across windows: every window's first merge runs under cert->delta.  With grow_delta a window that raises the bound raises it
 * for every LATER window, and such a window is first merged and selected again under the raised bound, before its certificate is
 * read.  records[w].delta is the bound coming out of window w -- records[E-1].delta is what the caller folds back -- and
 * records[w].rounds counts the merges issued for window w (the batched launch counts as one).
 * args->precision == M3PC_PREC_FP32: fp32 candidate passes, merged = a copy of scores_low, the selects of all windows in one launch
 * (m3pc_select's results per window, bit for bit), records {certified = 1, everything = 1, n_rescored = n_total}; cert is read for
 * its temperature only.
 * A window's results are those of the lock-step Python path for the same inputs, bit for bit.  They are NOT the bits of
 * m3pc_plan_step_certified on that window alone: the few-row fp32 kernels choose their tiling by the row count (see
 * m3pc_policy_pass_batch), so the two agree to fp32 rounding.
 *   states (E,T,S), actions (E,T,A), rewards (E,T,1) device;  rtg host (E,)
 *   eps       device (E,n_total,T,A) for RTG / CRITIC, (E,n_total,h,A) for NOISE;  expo device (E,n_total)
 *   loc, std  device out (E,T,A), optional;  sample_actions device out (E,n_total,h,A)
 *   scores_low, merged   device out (E,n_total)
 *   list      device out (E, rmax + 1024) int32, optional: per window the final lists, as m3pc_plan_step_certified's
 *   p (E,n_total), eval_action (E,A), argmax (E,), sample_idx (E,), sample_action (E,A)   device out, each optional
 *   records   host out (E,), valid on return; every device output is complete in stream order
 * Refused before any HIP call: null required pointers, n_windows < 1, args->returns != NULL (the batched policy pass takes rtg only)
 * and every check of m3pc_plan_step_certified (M3PC_EINVAL); then n_windows > max_batch (M3PC_EINVAL), a pipelined step begun
 * (M3PC_ESTATE), CRITIC / NOISE without critic weights (M3PC_ESTATE), and a first pass of more than max(max_candidates, max_rescore)
 * rows, E (rfirst + kmin) (M3PC_ENOMEM).  The per-window buffers (lists, statistics, host blocks, gathered rows) are sized by
 * m3pc_dims::max_batch and allocated at the first call.  Between calls the handle is in the state m3pc_plan_step_certified leaves. */
int m3pc_plan_steps_certified(m3pc_handle* h, const m3pc_plan_args* args, const m3pc_cert_args* cert, int n_windows,
                              const float* states, const float* actions, const float* rewards, const double* rtg,
                              const float* eps, const float* expo, float* loc, float* std, float* sample_actions,
                              float* scores_low, float* merged, int* list, float* p, float* eval_action, int* argmax,
                              int* sample_idx, float* sample_action, m3pc_cert_record* records, void* stream);

/* m3pc_plan_steps_certified with the eval_action certificate per window (erecs: host out (E,)).  Steps 1-7 are unchanged; behind
 * the batched merge of step 6 ONE launch bounds every window (m3pc_eval_bound per window: r = rfirst, n = kmin, delta = cert->delta)
 * into a second host-mapped block per window; step 8 runs the loop of m3pc_plan_step_certified_eval per window.  A window that
 * issued no merge beyond the batched one (records[w].rounds == 1, which also means no earlier window raised delta) takes its block;
 * any other window launches m3pc_eval_bound behind its last merge and waits.  Extensions are the window's own re-scores and merges;
 * a raised delta travels to later windows as in m3pc_plan_steps_certified.
 *   eval_tol = +inf: every output buffer and every record is bit for bit m3pc_plan_steps_certified's.
 *   erecs[w].eval_bound is bit for bit a stand-alone m3pc_eval_bound on the returned merged row, lists and records[w].
 *   M3PC_PREC_FP32: erecs[w] = {0, 0, 0, 0, 1}.
 * Refusals: those of m3pc_plan_steps_certified, plus erecs == NULL and eval_tol <= 0 or NaN (M3PC_EINVAL, before any HIP call).
 * The Python lock-step protocol (m3pc_amd/lockstep.py) has no eval form. */
int m3pc_plan_steps_certified_eval(m3pc_handle* h, const m3pc_plan_args* args, const m3pc_cert_args* cert, int n_windows,
                                   const float* states, const float* actions, const float* rewards, const double* rtg,
                                   const float* eps, const float* expo, float* loc, float* std, float* sample_actions,
                                   float* scores_low, float* merged, int* list, float* p, float* eval_action, int* argmax,
                                   int* sample_idx, float* sample_action, m3pc_cert_record* records, float eval_tol,
                                   m3pc_eval_record* erecs, void* stream);

/* The variates of a plan step, for a host without a generator of its own: eps device out (n_count, row_elems) standard normals =
 * rows [n_begin, n_begin + n_count) of the (n_total, row_elems) array of (seed, step); expo device out (n_count,) Exp(1) (never 0),
 * the same rows of the (n_total,) array.  Either may be NULL.  row_elems = T * A (RTG / CRITIC) or h * A (NOISE).
 * Counter-based: a value depends on (seed, step, element index) only -- not on n_begin / n_count, the launch geometry or earlier
 * draws -- so a candidate-sharded rank draws its slice of the one-rank array.  Philox4x32-10, key = (seed lo, seed hi), counter =
 * (block, step lo, step hi, array), array 0 = eps, 1 = expo; block b gives the flat elements 4b .. 4b+3.  Normals: words (w0, w1)
 * and (w2, w3) through Box-Muller, u1 = ((wa >> 8) + 1) 2^-24, u2 = (wb >> 8) 2^-24, z = sqrt(-2 ln u1) (cos 2 pi u2, sin 2 pi u2).
 * Exponentials: -ln(((w >> 8) + 1) 2^-24), and 2^-25 where that is 0.  It is NOT torch's generator stream. */
int m3pc_draw_variates(m3pc_handle* h, unsigned long long seed, unsigned long long step, int n_begin, int n_count, int row_elems,
                       float* eps, float* expo, void* stream);

/* delta of the certified step from ONE full fp32 candidate pass over the candidates of the step that owns args->slot (its
 * policy pass is reused; the pass runs in the candidate workspace): d = scores_low - fp32, c = the lower median of d (the
 * element torch.median returns), *delta_out = max(factor * max|d - c|, 1e-6 * max|fp32|, 1e-30).  A caller keeps the maximum
 * over the first steps behind a weight load (m3pc_amd/planner.py: 16 windows, factor 1.6).  n_total <= 16384, one rank;
 * stream-ordered, with one bounded read of the host-mapped statistics at the end (as above). */
int m3pc_calibrate_delta(m3pc_handle* h, const m3pc_plan_args* args, const float* states, const float* actions, const float* rewards,
                         const float* eps, const float* scores_low, float factor, float* delta_out, void* stream);

/* Iterative refinement of a plan: cross-entropy (CEM) or softmax-weighted (MPPI) refits of a per-(step, action) Gaussian over the
 * last h actions, warm-startable from the previous plan -- the algorithm of the legacy sample_action_cem
 * (research/omtm/datasets/sequence_dataset.py:919-1000: noisy copies of the policy mean, score, keep top_k, refit, resample, clamp to
 * [-1, 1]) on this model's plan step, as m3pc_amd/goal.py (cem_guiding) states it.
 *
 * The refit, per column c = (t, a) of the h * A columns, over the k elite rows x_i = cand[elite_i, c]:
 *   weights  M3PC_REFINE_CEM:  w_i = 1 / k
 *            M3PC_REFINE_MPPI: u_i = expf(temperature * (E[elite_i] - max_i E[elite_i])), w_i = u_i / sum u
 *   mean_c = sum w_i x_i;  S_c = sum w_i (x_i - mean_c)^2 (a second pass over the values);  D = sum w_i (1 - w_i)
 *   std_c  = max(D > 1e-6 ? sqrt(S_c / D) : 0, min_std)
 * With equal weights that is torch.std's unbiased estimate (0 at k = 1); with MPPI weights the reliability-weighted unbiased
 * variance.  A column whose elites are all equal has exactly that value as its mean and exactly 0 in front of the floor.
 * The resample: out[j, c] = min(1, max(-1, mean_c + std_c * noise[j, c])), product and sum rounded separately in fp32 (bit for bit
 * torch.clamp(mean + std * noise, -1, 1)).  Both kernels reduce in a fixed order without atomics: results are bit-identical from
 * run to run. */
#define M3PC_REFINE_CEM 0
#define M3PC_REFINE_MPPI 1
#define M3PC_REFINE_MAX_ITER 16
typedef struct m3pc_refine_args {   /* 4-byte fields only, in this order */
    int iterations;      /* 1 .. M3PC_REFINE_MAX_ITER */
    int top_k;           /* elites per iteration, 1 .. n_total */
    int weighting;       /* M3PC_REFINE_* */
    float temperature;   /* MPPI only; finite, >= 0 */
    float init_std;      /* finite, >= 0 */
    float min_std;       /* floor of every refit std; finite, >= 0 */
    unsigned int seed_lo, seed_hi, step_lo, step_hi;  /* generator coordinates, read when noise == NULL */
} m3pc_refine_args;

/* One refit (+ optional resample) as a call of its own, for a host that runs its own loop.  Needs a handle (for A and the device),
 * no weights.
 *   cand     device (n, horizon, A);  elites device (k,) int32: distinct ids in [0, n), any order (an id outside is clamped)
 *   scores   device (n,): read for M3PC_REFINE_MPPI only (NULL allowed for M3PC_REFINE_CEM)
 *   mean, std  device out (horizon, A)
 *   noise    device (n, horizon, A) and cand_out device out (n, horizon, A): both given (refit, then resample) or both NULL
 *            (refit only).  cand_out may alias cand.
 * n <= 16384, 1 <= k <= n, 1 <= horizon <= T; bad arguments return M3PC_EINVAL before any HIP call. */
int m3pc_refit_resample(m3pc_handle* h, const float* cand, int n, int horizon, const float* scores, const int* elites, int k,
                        int weighting, float temperature, float min_std, const float* noise, float* mean, float* std,
                        float* cand_out, void* stream);

/* The whole refinement as one call, all on `stream`; nothing is read back to the host, the host never waits:
 *   1. m3pc_policy_pass for `args` (honours M3PC_PLAN_PRUNED_POLICY, args->returns, rtg): the slot's policy head and returns tokens
 *   2. mean[0] = init_mean if given (device (h, A): the warm start, e.g. the previous call's final mean), else tanh of the policy
 *      loc over the last h steps;  std[0] = init_std
 *   3. candidates = resample(mean[0], std[0], noise[0])
 *   4. for it = 0 .. iterations-1: scores[it] = the candidates' TD(lambda) scores in args->precision (m3pc_score_actions: RTG or
 *      CRITIC scoring, one window);  elites[it] = their top_k (descending, ties to the lower index);  refit into mean[it+1],
 *      std[it+1];  candidates = resample(mean[it+1], std[it+1], noise[it+1])
 *   5. sample_action = candidates[0, 0, :], eval_action = mean[iterations][0, :]
 * One rank: n_begin == 0, n_count == n_total <= min(max_candidates, 16384).  args->flags: M3PC_PLAN_PRUNED_POLICY or 0 (anything else: M3PC_EINVAL).
 *   mean, std    device out (iterations + 1, h, A)
 *   candidates   device out (n_total, h, A): the live buffer of the loop; on return the candidates of the last resample
 *   scores       device out (iterations, n_total), optional;  elites device out (iterations, top_k) int32, optional
 *   noise        device (iterations + 1, n_total, h, A) standard normals, or NULL: the library draws them -- exactly what
 *                m3pc_draw_variates(seed, step, 0, (iterations + 1) * n_total, h * A, eps, NULL) yields
 *   sample_action, eval_action   device out (A,), each optional
 * In M3PC_PREC_BF16 the elite set of an iteration is the bf16 ranking's; M3PC_PREC_BF16X3 and M3PC_PREC_FP32 are the modes whose
 * elite sets follow fp32 scores (no certificate covers the elite boundary).
 * Bad arguments (the one-rank checks of m3pc_plan_step_certified; iterations, top_k, weighting, temperature, init_std, min_std;
 * a mode other than RTG / CRITIC; null required pointers) return M3PC_EINVAL before any HIP call.  M3PC_ESTATE while a pipelined
 * certified step is begun, and for CRITIC scoring without critic weights, before anything is enqueued.  Runs in the workspaces of m3pc_policy_pass and m3pc_score_actions, under their ordering rules. */
int m3pc_refine_plan(m3pc_handle* h, const m3pc_plan_args* args, const m3pc_refine_args* refine, const float* states,
                     const float* actions, const float* rewards, const float* init_mean, const float* noise,
                     float* mean, float* std, float* candidates, float* scores, int* elites,
                     float* sample_action, float* eval_action, void* stream);

/* m3pc_refine_plan for E windows that step together, as ONE call: every launch of the loop takes the batch as a grid dimension, so
 * an iteration is one scoring pass over the E * n_total rows (window_index[c] = c / n_total, kept in the handle), one top-k, one refit
 * and one resample, whatever E is.  All on `stream`; nothing is read back, the host never waits.
 *   1. m3pc_policy_pass_batch into args->slot (rtg per window; args->rtg is ignored)
 *   2. mean[0] of window w, row t (the receding-horizon warm start: the previous plan, shifted):
 *        init_mean[w, t + init_offset]   when init_mean is given and t + init_offset < init_rows[w],
 *        tanh(policy loc[w, T - h + t])  otherwise  (init_rows[w] = 0: a cold start)
 *      std[0] = init_std.  A closed loop passes the last call's final mean with init_offset = 1: with the same horizon the last
 *      row comes from the policy head; while the effective horizon shrinks by one per step (the first T steps of an episode)
 *      init_rows[w] = h + 1 and nothing is filled.
 *   3. candidates = resample(mean[0], std[0], noise[0]);  4. iterations x (score, top_k, refit, resample) as m3pc_refine_plan;
 *   5. sample_action[w] = candidates[w, 0, 0, :], eval_action[w] = mean[iterations][w][0, :]
 * For the same inputs a window's top-k, refit and resample are the one-window kernels' bit for bit; its policy head and scores agree
 * with m3pc_refine_plan's to fp32 rounding (the few-row kernels tile by the row count), so the elite sets agree where the boundary
 * is clear.
 *   states (E,T,S), actions (E,T,A), rewards (E,T,1) device;  rtg host (E,)
 *   init_mean   device (E, init_stride, A) or NULL (all cold);  init_rows host (E,), each in [0, init_stride], NULL = init_stride for
 *               every window;  init_offset >= 0
 *   noise       device (iterations + 1, E, n_total, h, A), or NULL: the library draws -- window w gets what m3pc_refine_plan uses for
 *               (seed, steps[w]);  steps host (E,), NULL = refine step + w
 *   mean, std   device out (iterations + 1, E, h, A);  candidates device out (E, n_total, h, A)
 *   scores      device out (iterations, E, n_total), optional;  elites device out (iterations, E, top_k) int32, optional
 *   sample_action, eval_action   device out (E, A), each optional
 * Refused before any HIP call: every check of m3pc_refine_plan; n_windows < 1, args->returns != NULL, args->flags != 0, init_mean
 * with init_stride < 1, an init_rows[w] outside [0, init_stride], init_offset < 0 (M3PC_EINVAL); n_windows > max_batch or
 * n_windows * n_total > max_candidates (M3PC_ENOMEM); a pipelined step begun, CRITIC scoring without critic weights (M3PC_ESTATE).
 * Where it pays: the batch call shares the policy chain and the short launches of an iteration among the windows, but its scoring
 * pass gives up the first-layer sharing of history rows that a one-window m3pc_score_actions has.  Measured at E = 8 against eight
 * m3pc_refine_plan calls (DESIGN.md section 5 "Refinement", tools/refine_batch_ab.py): 0.40 (bf16) / 0.81 (fp32) of their time at the
 * shipped shape (N = 625, H = 4, T = 8), 0.92 at the headline shape (N = 1024, H = 16, T = 32) -- no crossover up to there; the gain
 * shrinks as scoring takes over the call, so beyond the headline's rows per window measure before relying on either. */
int m3pc_refine_plans(m3pc_handle* h, const m3pc_plan_args* args, const m3pc_refine_args* refine, int n_windows,
                      const float* states, const float* actions, const float* rewards, const double* rtg,
                      const float* init_mean, int init_stride, const int* init_rows, int init_offset,
                      const float* noise, const unsigned long long* steps,
                      float* mean, float* std, float* candidates, float* scores, int* elites,
                      float* sample_action, float* eval_action, void* stream);

/* THE EPISODE STORE: the rollout histories of n_envs environments on the device, and their windows assembled there.  It replaces the
 * episode buffer every caller of the reference keeps on the host -- current_trajectory of ReplayBuffer.online_rollout
 * (finetune_omtm/replay_buffer.py:189-243) and of Learner.evaluate_plan (learner.py:660-700), and the way-point buffer of the zero-shot
 * rollout (zeroshot_omtm/learner.py:515-603) -- together with the window rules of action_sample (finetune_omtm/learner.py:342-366) and
 * action_piid_sample (zeroshot_omtm/learner.py:164-223), which a host would otherwise restate.
 *   Storage, fp32, one array per key, so that a trajectory is three contiguous blocks: obs (n_envs, max_steps, S), act (n_envs,
 *   max_steps, A), rew (n_envs, max_steps), and int32 path_length (n_envs) with a host mirror.  The host makes every call that changes a
 *   path length, so the mirror is always what the calls made so far leave behind and no entry point reads the device.
 *   A store is created on a handle, from which it takes S, A, T and the device; it needs no weights and does not refer to the handle
 *   afterwards.  m3pc_episodes_create makes no HIP call: the storage is allocated, and zeroed in stream order, by the first call that
 *   enqueues work.  A store is not re-entrant; its calls are ordered on the device by the caller (one stream, or events).
 *   Everything is stream-ordered: no entry point waits for the device or synchronises it (m3pc_episodes_destroy drains).  Host
 *   arguments -- env_ids always; observations, actions, rewards and tables when on_device == 0 -- are consumed before the call returns:
 *   they are copied into pinned, device-visible blocks of the store that the kernels read directly.  A block is used again once the work
 *   that read it has run; while none is free another is allocated, so the host never waits, however many ids a call brings.
 *   env_ids: host int32 (n,), or NULL for the environments 0 .. n-1.
 *   Kernels: gathers and scatters over a flat element index, coalesced across a row's features for any row width; no atomics; the one
 *   reduction (values) runs in a fixed order: results are bit-identical from run to run.
 * Refused with M3PC_EINVAL before any HIP call: null required pointers, n_envs < 1, max_steps < T, n outside [1, n_envs], an id outside
 * [0, n_envs) or repeated within one call, a mode other than M3PC_WINDOW_*, horizon outside [1, T], clip_min > clip_max (or a NaN
 * among them), a non-finite or negative discount, env outside [0, n_envs).  Refused with M3PC_ESTATE, with nothing written and no path
 * length changed: observe, record or windows on an environment whose path_length == max_steps -- a full episode is a refusal, never an
 * out-of-range access (the window of such an episode would take store row max_steps). */
typedef struct m3pc_episodes m3pc_episodes;
#define M3PC_WINDOW_PLAN 0  /* action_sample:      finetune_omtm/learner.py:342-366 */
#define M3PC_WINDOW_GOAL 1  /* action_piid_sample: zeroshot_omtm/learner.py:164-223 */
int m3pc_episodes_create(m3pc_handle* h, int n_envs, int max_steps, m3pc_episodes** out);
int m3pc_episodes_destroy(m3pc_episodes* ep);
/* The start of an episode (replay_buffer.py:189-203, learner.py:660-674: fresh zero arrays, path_length 0): the three blocks of every
 * listed environment zeroed, its path length 0.  obs_table, optional: (n, max_steps, S), one table per listed environment, float32 or
 * float64 (table_f64; rounded as NumPy's assignment into a float32 array rounds), host or device (on_device): the observation block
 * starts out as this table -- the held way-points of the zero-shot rollout (zeroshot_omtm/learner.py:515-539). */
int m3pc_episodes_reset(m3pc_episodes* ep, const int* env_ids, int n, const void* obs_table, int table_f64, int on_device, void* stream);
/* current_trajectory["observations"][timestep] = observation (replay_buffer.py:206, learner.py:683): obs[e, path_length[e], :] = row i
 * of obs (n, S), float32 or float64 (obs_f64), host or device (on_device).  The path length stays. */
int m3pc_episodes_observe(m3pc_episodes* ep, const int* env_ids, int n, const void* obs, int obs_f64, int on_device, void* stream);
/* action = np.clip(action, clip_min, clip_max); current_trajectory["actions"][timestep] = action; ["rewards"][timestep] = reward;
 * path_length += 1 (replay_buffer.py:213-229, learner.py:690-697): act[e, path_length[e], :] = min(max(a, clip_min), clip_max) with the
 * bits of np.clip (NaN stays, the sign of a zero is kept), rew[e, path_length[e]] = r, then path_length[e] += 1.
 * actions (n, A), rewards (n,) float32, both host or both device (on_device). */
int m3pc_episodes_record(m3pc_episodes* ep, const int* env_ids, int n, const float* actions, const float* rewards, float clip_min,
                         float clip_max, int on_device, void* stream);
/* The windows of n environments: states (n,T,S), actions (n,T,A), rewards (n,T,1) device out -- the layouts m3pc_plan_steps_certified,
 * m3pc_refine_plans, m3pc_policy_pass_batch and m3pc_goal_step_batch take, so the output feeds them with no copy in between.
 * With end = path_length[e] and H = horizon:  h = H if end + H >= T else T - end;  hl = T - h + 1;  lo = end - hl + 1.
 *   M3PC_WINDOW_PLAN (finetune_omtm/learner.py:342-366): rows t < hl of all three keys are store rows lo + t -- row `end` of act / rew is
 *   whatever the store holds there, zero after a reset; the reference copies it too --, rows t >= hl are zero.
 *   M3PC_WINDOW_GOAL (zeroshot_omtm/learner.py:164-223): actions and rewards as above; states[t] = obs[lo + t] for t < smart =
 *   T - max(0, end + h - max_steps) -- the future rows are way-points -- and zero behind; max_steps stands where the reference has the
 *   literal 1000.
 * horizons, optional: host out (n,), the effective h of every window, from the mirror -- valid on return; windows that go into one
 * batched call share it. */
int m3pc_episodes_windows(m3pc_episodes* ep, const int* env_ids, int n, int mode, int horizon, float* states, float* actions, float* rewards,
                          int* horizons, void* stream);
/* The discounted values ReplayBuffer.online_rollout hands to update_buffer (replay_buffer.py:234-243, discounts: :70), M = max_steps:
 *   V[t] = sum_{j=0}^{M-t-2} rew[t+1+j] discount^j, formed in float64 by the reverse recurrence V[t] = rew[t+1] + discount V[t+1],
 *   V[M-1] = 0, stored as float32;  use_avg != 0: the stored value is fp32(fp64(fp32(V[t])) / (M - t)).
 * values: device out (n, max_steps).  One thread per environment. */
int m3pc_episodes_values(m3pc_episodes* ep, const int* env_ids, int n, double discount, int use_avg, float* values, void* stream);
/* One environment's blocks -- obs (max_steps, S), act (max_steps, A), rew (max_steps), each optional -- copied to caller buffers on the
 * device (on_device != 0) or on the host (complete once the stream has been synchronised), and its path length (host out, optional,
 * from the mirror: valid on return).  What new_trajectories carries out of online_rollout (replay_buffer.py:245-250). */
int m3pc_episodes_export(m3pc_episodes* ep, int env, float* obs, float* act, float* rew, int* path_length, int on_device, void* stream);

/* THE REPLAY BUFFER: ReplayBuffer of finetune_omtm/replay_buffer.py on the device -- what the episodes of the store are handed to, and
 * where the training batches of the fine-tuning loop (finetune_omtm/finetune.py:281-310) come from, as device arrays a training loop on
 * the same GPU reads in place.
 *   Storage.  A trajectory ring of traj_capacity slots: obs (C, max_steps, S), act (C, max_steps, A), rew (C, max_steps) float32, val (C,
 *   max_steps) FLOAT64 (values_segmented is float64 in the reference, and traj_sample returns "returns" as float64), int32 path_length (C).
 *   Two transition rings, M3PC_REPLAY_OFFLINE and M3PC_REPLAY_ONLINE, each of its own capacity: state (cap, S), action (cap, A), reward,
 *   next_state (cap, S), done, float32 -- deque(maxlen=...) of :101-102.  A capacity of 0 leaves that part out.  In every ring logical
 *   index 0 is the oldest entry and logical index i is physical slot (head + i) % capacity; every index of this interface is logical.
 *   A buffer is created on a handle, from which it takes S, A and the device; it needs no weights and does not refer to the handle
 *   afterwards.  m3pc_replay_create makes no HIP call: the storage is allocated by the first call that enqueues work.  A buffer is not
 *   re-entrant; its calls are ordered on the device by the caller (one stream, or events).  Everything is stream-ordered: no entry point
 *   waits for the device (m3pc_replay_destroy drains).  Host arguments are consumed before the call returns, through the pinned,
 *   device-visible staging blocks the episode store uses.  The host mirrors counts, ring heads and path lengths -- it makes every call
 *   that changes one -- so validation and the readers (m3pc_replay_counts, m3pc_replay_path_lengths) never read the device.
 *   Kernels: gathers and scatters with consecutive lanes on consecutive features of a row; no atomics; every reduction in a fixed order:
 *   results are bit-identical from run to run.
 *   THE LIBRARY'S DRAWS come from the generator of m3pc_draw_variates, Philox4x32-10 with key = (seed lo, seed hi) and counter = (block,
 *   step lo, step hi, array): a draw depends on (seed, step, row) alone.  All index arithmetic is exact integer arithmetic.
 *     Segments, array 2: row j takes the words w0 .. w3 of block j.
 *       M3PC_REPLAY_UNIFORM: trajectory i = (w0 * count) >> 32.
 *       M3PC_REPLAY_LENGTH (in proportion to path length, np.random.choice(p = path_lengths / sum) of :330-332): r = (w0 * sum) >> 32 with
 *       sum = the sum of the held path lengths, then the i with cum[i] <= r < cum[i+1], cum the int64 exclusive scan of the path lengths
 *       in logical order (made on the device, in a fixed order, when the ring has changed since the last scan).
 *       start = (w2 * (path_length[i] - segment_length + 1)) >> 32 (np.random.randint(0, len - L + 1) of :345-347).
 *       A multiply-shift (w * n) >> 32 takes each of n values with probability within 2^-32 of 1/n: a relative bias of at most n / 2^32.
 *     Transitions, distinct within a ring (random.sample of :371-381 draws without replacement): row j of a ring's rows takes logical
 *     index pi(j), pi a keyed bijection of [0, n), n = the ring's count: for n = 1, pi(0) = 0; else with b = ceil(log2 n), half =
 *     ceil(b / 2), mask = 2^half - 1 and the four round keys k0 .. k3 = the words of Philox block 0, array 3 (online ring) or 4 (offline
 *     ring), x = j is taken through   (l, r) = (x >> half, x & mask);  four times, for k = k0 .. k3:  (l, r) = (r, l ^ ((((r + k) mod 2^32)
 *     * 0x9E3779B1 mod 2^32) >> (32 - half)));  x = (l << half) | r   -- a balanced Feistel network, a bijection of [0, 2^(2 half)) --
 *     again and again until x < n (cycle walking: a bijection of [0, n); the domain is smaller than 4 n).  O(1) per row, no scratch.
 *     This does not reproduce NumPy's or Python's Mersenne streams, and nothing can: a caller who needs the reference's exact batches
 *     passes its indices.  tests/replay_ref.py restates the draws bit for bit.
 * Refused with M3PC_EINVAL before any HIP call: null required pointers; a capacity < 0; max_steps < 1; segment_length outside [1,
 * max_steps]; n outside [1, capacity] (append, append_transitions) or [1, n_envs] (push_episodes); a path length < segment_length or >
 * max_steps; a ring other than M3PC_REPLAY_OFFLINE / _ONLINE; a store of other sizes or another device; an id outside [0, n_envs) or
 * repeated; a non-finite or negative discount; batch < 1; a mode other than M3PC_REPLAY_UNIFORM / _LENGTH; one of traj_index /
 * start_index without the other; a host index out of range; n_online outside [0, batch]; more rows asked of a ring than it holds.
 * Refused with M3PC_ESTATE: sampling, or values_up_bound, on a part that holds nothing. */
typedef struct m3pc_replay m3pc_replay;
#define M3PC_REPLAY_UNIFORM 0  /* select_mode "uniform": replay_buffer.py:320-326 */
#define M3PC_REPLAY_LENGTH 1   /* select_mode "prob":    replay_buffer.py:328-332 */
#define M3PC_REPLAY_OFFLINE 0  /* offline_trans_buffer,  replay_buffer.py:101 */
#define M3PC_REPLAY_ONLINE 1   /* online_trans_buffer,   replay_buffer.py:102 */
int m3pc_replay_create(m3pc_handle* h, int traj_capacity, int max_steps, int segment_length, int offline_capacity, int online_capacity,
                       m3pc_replay** out);
int m3pc_replay_destroy(m3pc_replay* rb);
/* update_buffer (replay_buffer.py:272-310) on caller arrays, and the first fill (:129-160): n trajectories -- obs (n, max_steps, S), act
 * (n, max_steps, A), rew (n, max_steps) float32, val (n, max_steps) float64, host or device (on_device, one flag for the four), lens (n,)
 * int32 ALWAYS on the host (the mirror) -- are appended at the tail in order; when the ring is full the oldest leave (:288-304: drop the
 * first n, append the n new).  All max_steps rows are copied.  The reference does not filter an episode shorter than traj_length, which
 * later makes np.random.randint(0, <= 0) raise in traj_sample; here such an entry is refused, with nothing written. */
int m3pc_replay_append(m3pc_replay* rb, int n, const float* obs, const float* act, const float* rew, const double* val, const int* lens,
                       int on_device, void* stream);
/* The offline fill (replay_buffer.py:108-125), or online_trans_buffer.append (:223-227) for a caller without a store: n transitions --
 * state (n, S), action (n, A), reward (n,), next_state (n, S), done (n,) float32, host or device -- appended to ring `which`. */
int m3pc_replay_append_transitions(m3pc_replay* rb, int which, int n, const float* state, const float* action, const float* reward,
                                   const float* next_state, const float* done, int on_device, void* stream);
/* The end of online_rollout (replay_buffer.py:223-251) for the episodes of a store, device to device, in one launch.  For the listed
 * environments (env_ids host int32 (n,), or NULL for 0 .. n-1), in order:
 *   an episode with path_length >= segment_length is appended to the trajectory ring as m3pc_replay_append would: the three blocks and
 *   the path length as m3pc_episodes_export gives them, and the values of :234-243 computed in the same pass by the recurrence of
 *   m3pc_episodes_values -- V[t] = rew[t+1] + discount V[t+1] in float64, rounded to float32 (the assignment of :238), then widened; with
 *   use_avg the stored value is (double)(float)V[t] / (max_steps - t), NOT rounded again: a float32 array divided by an int64 array is a
 *   float64 array in NumPy (:240-242; m3pc_episodes_values rounds this quotient to float32, the buffer must not).  A shorter episode
 *   is skipped as a trajectory (online_rollout's "too short");
 *   the transitions (obs[t], act[t], rew[t], obs[t+1], 0), t < path_length, of EVERY listed episode are appended to the online ring
 *   (:223-227 appends them whatever becomes of the trajectory).  final_obs, optional, (n, S) float32, host or device (final_on_device):
 *   row i is the next state of episode i's last transition; without it that transition is left out (the store never holds row
 *   path_length of a full episode).
 * taken, optional host out: the number of trajectories appended, from the mirrors -- valid on return.  The store is only read. */
int m3pc_replay_push_episodes(m3pc_replay* rb, m3pc_episodes* ep, const int* env_ids, int n, double discount, int use_avg, const float* final_obs,
                              int final_on_device, int* taken, void* stream);
/* traj_sample (replay_buffer.py:312-366): states (batch, L, S), actions (batch, L, A), rewards (batch, L, 1) float32 and returns (batch,
 * L, 1) float64 -- or float32, the float64 value rounded, when returns_f32 != 0 -- device out, L = segment_length; row j is rows start ..
 * start + L - 1 of trajectory i.  (i, start) per row: traj_index / start_index, both (batch,) int32 on the host (checked) or the device
 * (index_on_device; clamped into range, so that no index leads out of the storage), or, when both are NULL, drawn by the library from
 * (seed, step) by `mode` (above); mode is checked either way.  out_traj / out_start, optional device out (batch,) int32: the pair of every
 * row.  At most two launches: the gather, and the scan in front of it when M3PC_REPLAY_LENGTH draws from a ring that has changed. */
int m3pc_replay_sample_segments(m3pc_replay* rb, int batch, int mode, const int* traj_index, const int* start_index, int index_on_device,
                                unsigned long long seed, unsigned long long step, float* states, float* actions, float* rewards, void* returns,
                                int returns_f32, int* out_traj, int* out_start, void* stream);
/* trans_sample (replay_buffer.py:368-420): state (batch, S), action (batch, A), reward (batch, 1), next_state (batch, S), done (batch, 1)
 * float32 device out; rows [0, n_online) from the online ring, the other batch - n_online from the offline ring (the order of :375-382).
 * index, (batch,) int32 host (checked) or device (clamped): the logical index of every row within its ring; NULL: drawn by the library,
 * distinct within each ring (above).  out_index, optional device out (batch,).  One launch. */
int m3pc_replay_sample_transitions(m3pc_replay* rb, int batch, int n_online, const int* index, int index_on_device, unsigned long long seed,
                                   unsigned long long step, float* state, float* action, float* reward, float* next_state, float* done, int* out_index,
                                   void* stream);
/* values_up_bound (replay_buffer.py:161, :310): out (max_steps,) float64 device, the maximum over the held trajectories of every value
 * column, all max_steps rows -- the episode_rtg_ref evaluate_plan is called with (finetune.py:373-377). */
int m3pc_replay_values_up_bound(m3pc_replay* rb, double* out, void* stream);
/* The mirrors (host out, each optional; no HIP call): the number of held trajectories, offline and online transitions. */
int m3pc_replay_counts(m3pc_replay* rb, int* trajectories, int* offline, int* online);
/* path_lengths (replay_buffer.py:133, :288) in logical order: host out, the first `count` of `capacity` entries; no HIP call. */
int m3pc_replay_path_lengths(m3pc_replay* rb, int* path_lengths, int capacity);

/* THE IQL TRAINER: ImplicitQLearning of finetune_omtm/model.py:194-334 on the device -- the two updates of the fine-tuning loop that
 * learner.critic_update(buffer.trans_sample()) makes (finetune_omtm/finetune.py:281-310): V (model.py:174-191), the TwinQ with its target
 * (:146-171, :213) and the Gaussian actor (:107-133), all MLPs [in, hidden, hidden, out] with ReLU, states normalised with (s - obs_mean) /
 * obs_std -- trained from the transition batches of the replay buffer, and the TwinQ handed to the planner without the host.
 *   Sizes.  hidden 64, 128 or 256; S + A <= 64, A <= 32 (input features are padded to a multiple of 32); 1 <= batch <= 1024.
 *   (m3pc_create itself takes state_dim <= 32 today; the trainer's own rule is the wider one.)
 *   A trainer is created on a handle, from which it takes S, A and the device; it does not refer to the handle afterwards.
 *   m3pc_iql_create makes no HIP call: storage is allocated, and the Adam moments zeroed, by the first call that enqueues work.  A trainer
 *   is not re-entrant; its calls are ordered on the device by the caller.  Everything is stream-ordered and no entry point waits for the
 *   device (m3pc_iql_destroy drains): host tensors given to m3pc_iql_load are consumed before it returns, through pinned staging blocks;
 *   host tensors m3pc_iql_export writes are complete once the stream has passed the call -- give it pinned (page-locked) memory: a copy
 *   into pageable host memory is one the runtime may make the calling thread wait for.  The host mirrors the step count.
 *   ONE STEP is train() (model.py:286-308), in which every forward pass reads pre-step parameters:
 *     next_v = vf(next_obs);  adv = min(q1_target, q2_target)(obs, act) - vf(obs);  value_loss = mean(|expectile - 1[adv < 0]| adv^2)   (:59-60, :228-240)
 *     targets = r + (1 - done) discount next_v;  q_loss = (mse(q1, targets) + mse(q2, targets)) / 2                                    (:251-253)
 *     actor_loss = mean(min(exp(beta adv), 100) * -sum_A log N(act; tanh(net(obs)), exp(clamp(log_std, -20, 2))))                       (:269-279)
 *     Adam on vf, qf and the actor (torch.optim.Adam defaults; the actor's rate follows CosineAnnealingLR(actor_t_max), :219), then
 *     q_target <- (1 - tau) q_target + tau qf with the POST-step qf (:22-24, :257-260), each product rounded to fp32, then the sum.
 *   Seven launches per step; fp32 on v_mfma_f32_32x32x2_f32 (every product an exact fp32 fma); one wavefront owns an output tile and sums
 *   its K dimension in a fixed order, no atomics: a step is bit-identical from run to run.  m3pc_amd/csrc/iql.h states the order of the
 *   Adam arithmetic and what of it is fp64.
 *   Tensors go by the reference's state_dict names, per part (m3pc_named_tensor; any other name in the list is ignored):
 *     M3PC_IQL_QF, _Q_TARGET, _QF_ADAM_M, _QF_ADAM_V     "q1.net.0.weight" (hidden, S+A) ".0.bias" ".2.weight" ".2.bias" ".4.weight" (1, hidden) ".4.bias", and "q2. ..."
 *     M3PC_IQL_VF, _VF_ADAM_M, _VF_ADAM_V                "v.net.0.weight" (hidden, S) ... "v.net.4.bias"
 *     M3PC_IQL_ACTOR, _ACTOR_ADAM_M, _ACTOR_ADAM_V       "net.net.0.weight" (hidden, S) ... "net.net.4.weight" (A, hidden) "net.net.4.bias" (A), "log_std" (A)
 *   _ADAM_M / _ADAM_V are exp_avg / exp_avg_sq of torch.optim.Adam's state, zero until loaded.
 * Refused with M3PC_EINVAL before any HIP call: null required pointers; sizes outside the covered set (create); a part or an output that
 * is none of the macros; a missing or mis-shaped tensor; one of obs_mean / obs_std without the other; total_it < 0; batch outside [1,
 * 1024]; n_steps < 1; rows < 1; a non-finite or negative rate or discount; expectile outside (0, 1); a non-finite beta; tau outside [0, 1];
 * actor_t_max < 1; flags != 0; a replay buffer or a handle of other sizes or another device.  Refused with M3PC_ESTATE: training before
 * qf, q_target, vf, the actor and obs_mean / obs_std are loaded; publishing, evaluating or exporting a network that is not loaded.  The
 * refusals of m3pc_replay_sample_transitions apply to m3pc_iql_train. */
typedef struct m3pc_iql m3pc_iql;
#define M3PC_IQL_QF 0
#define M3PC_IQL_Q_TARGET 1
#define M3PC_IQL_VF 2
#define M3PC_IQL_ACTOR 3
#define M3PC_IQL_QF_ADAM_M 4
#define M3PC_IQL_QF_ADAM_V 5
#define M3PC_IQL_VF_ADAM_M 6
#define M3PC_IQL_VF_ADAM_V 7
#define M3PC_IQL_ACTOR_ADAM_M 8
#define M3PC_IQL_ACTOR_ADAM_V 9
/* m3pc_iql_evaluate: which output */
#define M3PC_IQL_Q_MIN 0         /* TwinQ.forward, model.py:170-171 */
#define M3PC_IQL_Q_TARGET_MIN 1  /* the same of q_target */
#define M3PC_IQL_V 2             /* ValueFunction.forward, :189-191 */
#define M3PC_IQL_ACTOR_MEAN 3    /* GaussianPolicy.forward(...).mean, :129-133: what act() returns in evaluation (:135-143) */
typedef struct m3pc_iql_args {
    double v_lr, q_lr, actor_lr; /* the three optimizers' rates; the actor's is the base rate of its cosine schedule */
    double expectile;            /* iql_tau, model.py:204 */
    double beta;                 /* :205 */
    double discount;             /* :207 */
    double tau;                  /* the target's soft-update rate, :208 */
    long long actor_t_max;       /* max_steps, :206 / :219 */
    int flags;                   /* must be 0 */
} m3pc_iql_args;
int m3pc_iql_create(m3pc_handle* h, int hidden, m3pc_iql** out);
int m3pc_iql_destroy(m3pc_iql* iql);
/* load_state_dict (model.py:322-334), one part per call: every tensor of the part must be in the list (its on_device says where it
 * lives).  obs_mean / obs_std, host (S,), both or neither: the normalisation all networks share.  Loading M3PC_IQL_QF does NOT copy it
 * into the target (:325 is the caller's second call with M3PC_IQL_Q_TARGET). */
int m3pc_iql_load(m3pc_iql* iql, int part, const m3pc_named_tensor* tensors, int n, const float* obs_mean, const float* obs_std, void* stream);
/* state_dict (:310-320), one part per call: every tensor of the part is written to the `data` of the entry of its name (host or device
 * by its on_device; written although the field is declared const). */
int m3pc_iql_export(m3pc_iql* iql, int part, const m3pc_named_tensor* tensors, int n, void* stream);
/* total_it (:225, :334): the number of steps made, which sets Adam's bias corrections and the actor's rate of the next step */
int m3pc_iql_set_step(m3pc_iql* iql, long long total_it);
int m3pc_iql_get_step(m3pc_iql* iql, long long* total_it);
/* train(batch) (:286-308).  state (batch, S), action (batch, A), reward (batch, 1), next_state (batch, S), done (batch, 1): float32 device
 * arrays, what m3pc_replay_sample_transitions writes.  losses, optional device out (3,): value_loss, q_loss, actor_loss. */
int m3pc_iql_train_step(m3pc_iql* iql, const m3pc_iql_args* args, int batch, const float* state, const float* action, const float* reward,
                        const float* next_state, const float* done, float* losses, void* stream);
/* n_steps steps in one call (finetune.py:288-290, v_iter_per_mtm of them per iteration): step k trains on the batch the buffer draws for
 * (seed, step + k) with n_online rows from the online ring; losses, optional device out (n_steps, 3).  Per step the bits are those of
 * m3pc_replay_sample_transitions followed by m3pc_iql_train_step. */
int m3pc_iql_train(m3pc_iql* iql, const m3pc_iql_args* args, m3pc_replay* rb, int n_steps, int batch, int n_online, unsigned long long seed,
                   unsigned long long step, float* losses, void* stream);
/* What m3pc_set_critic does with qf's state_dict, device to device in one launch: q1 / q2 in the operand order of the handle's critic
 * kernels, obs_mean / obs_std, and the handle's critic counts as set.  The handle was created with critic_hidden == hidden. */
int m3pc_iql_publish_critic(m3pc_iql* iql, m3pc_handle* h, void* stream);
/* states (rows, S), actions (rows, A; unused, may be NULL, for M3PC_IQL_V and _ACTOR_MEAN) device -> out (rows,) or (rows, A) device. */
int m3pc_iql_evaluate(m3pc_iql* iql, int which, const float* states, const float* actions, int rows, float* out, void* stream);

/* THE MASKED-TRAJECTORY LOSS: the forward half of Learner.compute_mtm_loss (finetune_omtm/learner.py:419-504; what mtm_update trains on,
 * :506-538, and what finetune.py:346-370 logs as eval/loss*) and of omtm.forward_loss (omtm/models/mtm_model.py:440-532), for one token
 * per timestep and modality and continuous heads.  Per call, with m_k the (T,) mask of key k (1 = visible to the encoder), n_vis its
 * sum, raw = (pred - target)^2 per element:
 *   targets      the tokenised batch; with M3PC_MTM_NORM_L2 the target row of every key but the actions is divided by its l2 norm
 *                (mtm_model.py:481-482; for the two scalar keys that is t / |t|: the sign, NaN at 0)
 *   per key k != actions:   loss_k = mean of raw;  masked_c_loss_k = sum over b, t, d of raw m / n_vis / B;  masked_loss_k = the same with
 *                1 - m and T - n_vis.  The divisor is the token count alone, as in the reference; a zero count divides as IEEE does.
 *   actions      loss = mean over (b, t, a) of (tanh(mu) - target)^2 m_t; no masked variants
 *   likelihood   a = the target actions, clipped to [(float)(-1 + 1e-6), (float)(1 - 1e-6)] with M3PC_MTM_CLIP_ACTIONS (learner.py:490);
 *                z = 0.5 (log1p(a) - log1p(-a));  lp = Normal(mu, std).log_prob(z) - 2 (log 2 - z - softplus(-2 z));
 *                log_likelihood = mean of lp over b, the timesteps whose action mask is 0, and a (a MEAN over the action dimension: the
 *                reference's sum(axis=2) runs over the length-1 token axis); NaN when no timestep is hidden
 *   entropy      u = mu + std eps;  lq = Normal(mu, std).log_prob(u) - 2 (log 2 - u - softplus(-2 u));  entropy = mean of -lq over the same set
 *   total        = sum of loss_k over the keys whose bit (1 << M3PC_STATES ...) is set in loss_keys, minus (log_likelihood + entropy_reg entropy)
 * The two reference forms are two settings: fine-tuning (learner.py:419-504) is flags = M3PC_MTM_CLIP_ACTIONS with loss_keys = the keys up
 * to and including the first key that is not the actions in the batch's key order -- its lines 488-504 sit INSIDE the key loop, so it
 * returns after `states` for the order traj_sample produces: loss_keys = 1; pretraining (mtm_model.py:440-532, norm "l2", loss_keys None)
 * is flags = M3PC_MTM_NORM_L2 with loss_keys = 15.  All twelve per-key numbers are computed either way.
 *   record       device out, M3PC_MTM_LOSS_FLOATS floats: [3 k] loss_k, [3 k + 1] masked_loss_k, [3 k + 2] masked_c_loss_k for k = M3PC_STATES,
 *                _ACTIONS, _REWARDS, _RETURNS ([4] and [5], which have no meaning, are 0); [12] entropy; [13] nll = -log_likelihood; [14] total
 *   masks        host, four (T,) arrays of 0/1 bytes, as m3pc_forward;  eps device (batch, T, A) standard normals;  entropy_reg = exp(log_temperature)
 * Elementwise terms are fp32 in the reference's operation order; every sum is float64 in a fixed tree (per-row sums to a scratch block, then
 * one workgroup), no atomics: a call is bit-identical from run to run and does not depend on rows beyond `batch`.  Two launches behind the
 * forward's (m3pc_amd/csrc/mtm_loss.h).  Stream-ordered; no entry point waits for the device (the first call allocates the scratch).
 * Refused with M3PC_EINVAL before any HIP call: null required pointers; batch outside [1, max_batch]; a mask byte other than 0 / 1; unknown
 * flag bits; loss_keys outside [0, 15]; a precision that is none; a replay buffer whose S, A, device or segment_length != T do not fit the
 * handle; the refusals of m3pc_replay_sample_segments.  Refused with M3PC_ESTATE: weights or tokenizers not loaded (m3pc_mtm_loss, _replay). */
#define M3PC_MTM_LOSS_FLOATS 15
#define M3PC_MTM_NORM_L2 1        /* mtm_model.py:481-482 */
#define M3PC_MTM_CLIP_ACTIONS 2   /* learner.py:490 */
/* The loss on caller-supplied predictions -- pred_states (batch, T, S), pred_rewards / pred_returns (batch, T, 1), mu / std (batch, T, A):
 * what m3pc_forward writes -- and tokenised targets[k] (batch, T, D_k), all device.  Needs no weights. */
int m3pc_mtm_loss_terms(m3pc_handle* h, int batch, const float* pred_states, const float* pred_rewards, const float* pred_returns,
                        const float* mu, const float* std, const float* const targets[4], const unsigned char* const masks[4],
                        const float* eps, float entropy_reg, int flags, int loss_keys, float* record, void* stream);
/* One call on a RAW batch -- states (batch, T, S), actions (batch, T, A), rewards (batch, T, 1) float32, returns (batch, T, 1) float32 or,
 * with returns_f64, float64: what m3pc_replay_sample_segments writes: m3pc_tokenize of the four, omtm.forward under the masks in
 * `precision` (m3pc_forward; in the candidate workspace, which it leaves as m3pc_forward does), then the loss on its heads.  out_*,
 * optional device out: the five head outputs, shaped as m3pc_forward's. */
int m3pc_mtm_loss(m3pc_handle* h, int batch, const float* states, const float* actions, const float* rewards, const void* returns,
                  int returns_f64, const unsigned char* const masks[4], const float* eps, float entropy_reg, int flags, int loss_keys,
                  int precision, float* record, float* out_states, float* out_rewards, float* out_returns, float* out_mu, float* out_std,
                  void* stream);
/* The same on the batch the buffer draws at (seed, step, mode), or at the caller's indices: batch ... step, out_traj and out_start are the
 * arguments of m3pc_replay_sample_segments, with its semantics; the rows are gathered into the handle's scratch (returns float64) and never
 * cross the host.  eps: device (batch, T, A), or NULL: array 0 of the generator of m3pc_draw_variates at the same (seed, step), elements
 * [0, batch T A).  rb was created on this handle's sizes with segment_length == T. */
int m3pc_mtm_loss_replay(m3pc_handle* h, m3pc_replay* rb, int batch, int mode, const int* traj_index, const int* start_index,
                         int index_on_device, unsigned long long seed, unsigned long long step, const unsigned char* const masks[4],
                         const float* eps, float entropy_reg, int flags, int loss_keys, int precision, float* record, int* out_traj,
                         int* out_start, void* stream);

/* THE GRADIENT OF THE MASKED-TRAJECTORY LOSS: the forward above and loss.backward() of Learner.mtm_update (finetune_omtm/learner.py:506-538)
 * through the whole model -- loss terms, heads, decoder blocks, decoder embedding and mask tokens, encoder blocks, encoder embedding --
 * in one call: a raw batch in, one gradient tensor per parameter out, under the reference's state_dict names.  The optimizers stay the
 * caller's, or the library's (m3pc_mtm_opt_* below).  The gradient is that of `total`, record[14] as defined above for the given flags and loss_keys, with respect to every tensor
 * of the model's state_dict except the buffer pos_embed.  Held constant: the tokenised targets (the l2-normalised ones too), the clipped
 * action and its z, entropy_reg, the masks.  eps is the caller's; u = mu + std eps is differentiated through mu and std (rsample), and std
 * = exp(-5 + 3.5 (tanh(.) + 1)) through the log_std Linear.
 *   dropout      the model is the eval-mode one until m3pc_mtm_grad_set_dropout(g, p, seed, draw) with p > 0 switches on the four dropout
 *                sites of every nn.TransformerEncoderLayer(norm_first=True) of the training-mode model (the shipped configs train with
 *                dropout 0.1): the attention probabilities, dropout1 behind out_proj, the feed-forward's dropout behind the GELU and
 *                dropout2 behind linear2; the embeddings and the output heads have none.  An element is kept iff its word of the
 *                library's Philox4x32-10 stream is >= floor(p 2^32), and a kept element is multiplied by (float)(1 / (1 - p)); the stream
 *                is a pure function of (seed, draw, site, element) -- THE LIBRARY'S OWN, NOT TORCH'S (counter layout, sites and the
 *                arithmetic order: m3pc_amd/csrc/mtm_grad.h).  Every gradient call -- m3pc_mtm_grad, m3pc_mtm_grad_replay,
 *                m3pc_mtm_train_step and each step of m3pc_mtm_train -- uses the object's current draw and then advances it by one; a
 *                refused call does not.  n steps of one m3pc_mtm_train use the draws d .. d + n - 1 and equal n single calls bit for
 *                bit.  The record, and the entropy the temperature step reads, come from the dropped forward (the reference's
 *                train/loss).  m3pc_mtm_loss* stays the eval-mode loss.  p == 0 switches dropout off: no launch differs from an object
 *                that never had it set; a p below 2^-32 has threshold 0 and is treated the same (nothing drops, the draw does not
 *                advance).  _set / _get_dropout are host-only: no HIP call, no wait; the outputs of _get are optional.
 *                Refused with M3PC_EINVAL: a null g; p not finite or outside [0, 1); and, by the gradient calls while p > 0, a model of
 *                more than 64 layers or a batch whose largest site has more than 2^32 groups of four elements.
 *   A key outside loss_keys contributes nothing: with loss_keys = 1 the rewards and returns heads get exact zeros (the reference leaves
 *   .grad = None there).  Structural zeros are exact zeros: the mask token of a fully visible key; the encoder embedding and the
 *   encoder_per_dim_encoding of a fully hidden key.  When total is NaN (no hidden action timestep, an l2 norm of 0) the call returns
 *   M3PC_OK and the gradients are unspecified.
 *   weights      the object reads the fp32 weights and the tokenizers of the handle it was created on at the time of each call: after
 *                m3pc_load_weights the next call differentiates the new weights.  The handle must outlive the object.
 *   workspace    the object never writes to the handle and leaves the candidate workspace alone.  It owns the activations its forward
 *                saves and one gradient buffer per parameter.  _create makes no HIP call; the first enqueueing call allocates
 *                max_batch x the bytes per batch element, with L = 4 T, n = n_enc_layer + n_dec_layer, d = embed_dim, ff = 4 d:
 *                  4 [ n L (8 d + 2 ff + 4 + n_head L) + L (12 d + ff + 4) + T (11 d + 4 S + 8 A + 13) ] + 56 T  bytes
 *                (rounded up per buffer to 256 bytes), plus once the gradients (the parameters' bytes) and the column-sum partials,
 *                2 (max_batch L / 64 + 2) max(3 d, ff) doubles.
 *   precision    fp32 only: the products on v_mfma_f32_32x32x2_f32, one wavefront per 32 x 32 output tile, K in ascending order (the
 *                weight gradients: four wavefronts per tile, each a fixed quarter of the k blocks, added in a fixed order);
 *                column sums in float64 in a fixed order.  No floating-point atomics: a call is bit-identical from run to run and does
 *                not depend on rows beyond `batch` or on what an earlier call left in the workspace (m3pc_amd/csrc/mtm_grad.h).
 *   record       optional device out, the M3PC_MTM_LOSS_FLOATS floats of m3pc_mtm_loss, from the forward this call runs.
 *   export       each listed gradient is written in the torch layout of its parameter to the entry's `data` (host or device by its
 *                on_device; written although the field is declared const).  Gradients are those of the last gradient call.
 *   replay form  the sampling arguments and semantics of m3pc_mtm_loss_replay; per call the bits of m3pc_replay_sample_segments followed
 *                by m3pc_mtm_grad.
 * Stream-ordered; no entry point waits for the device (_destroy drains).  Refused with M3PC_EINVAL before any HIP call: what m3pc_mtm_loss
 * refuses, with max_batch the object's; max_batch < 1 (create); masks that keep no token (as m3pc_forward); an export name that is not a
 * parameter (pos_embed included); an export numel that does not fit the parameter.  Refused with M3PC_ESTATE: weights or tokenizers not
 * loaded; export before any gradient call. */
struct m3pc_mtm_grad; /* (no typedef: the name is the gradient call's; say `struct m3pc_mtm_grad`) */
int m3pc_mtm_grad_create(m3pc_handle* h, int max_batch, struct m3pc_mtm_grad** out);
int m3pc_mtm_grad_destroy(struct m3pc_mtm_grad* g);
int m3pc_mtm_grad(struct m3pc_mtm_grad* g, int batch, const float* states, const float* actions, const float* rewards, const void* returns,
                  int returns_f64, const unsigned char* const masks[4], const float* eps, float entropy_reg, int flags, int loss_keys,
                  float* record, void* stream);
int m3pc_mtm_grad_replay(struct m3pc_mtm_grad* g, m3pc_replay* rb, int batch, int mode, const int* traj_index, const int* start_index,
                         int index_on_device, unsigned long long seed, unsigned long long step, const unsigned char* const masks[4],
                         const float* eps, float entropy_reg, int flags, int loss_keys, float* record, int* out_traj, int* out_start,
                         void* stream);
int m3pc_mtm_grad_export(struct m3pc_mtm_grad* g, const m3pc_named_tensor* tensors, int n, void* stream);
int m3pc_mtm_grad_set_dropout(struct m3pc_mtm_grad* g, double p, unsigned long long seed, unsigned long long draw);
int m3pc_mtm_grad_get_dropout(struct m3pc_mtm_grad* g, double* p, unsigned long long* seed, unsigned long long* next_draw);

/* THE OPTIMIZERS OF THE MASKED-TRAJECTORY MODEL: what Learner.mtm_update (finetune_omtm/learner.py:506-538) does behind loss.backward(),
 * on the device and on the HANDLE'S OWN WEIGHTS -- AdamW over every parameter in the two groups of omtm.configure_optimizers
 * (mtm_model.py:779-841), the LambdaLR schedule, and the Adam step of the float64 log_temperature on exp(log_t) (entropy - target_entropy)
 * with the gradient call's entropy.  A step moves the fp32 weights of the handle the gradient object was created on and re-derives
 * every form the passes read (what m3pc_load_weights derives) behind it: the next plan step runs on the trained weights, and nothing
 * crosses the host.  Arithmetic order, launches and determinism: m3pc_amd/csrc/mtm_opt.h.
 *   inactive     the output-head tensors of a key outside loss_keys have no gradient in the reference and torch's AdamW skips them: their
 *                weights, moments, bf16 copies and step counts keep their bits.  Step counts are per tensor.  An all-zero gradient IS stepped.
 *   schedule     the step made at scheduler count s uses lr = learning_rate * lambda(s) (m3pc_mtm_lr: what scheduler.get_last_lr()[0]
 *                shows before the step); warmup_steps == 0: 0.5 (1 + cos(s / num_train_steps * pi)); warmup_steps > 0: s / warmup_steps
 *                below it, then 0.5 (1 + cos((s - warmup_steps) / (num_train_steps - warmup_steps) * pi)).
 *   _step        applies the gradients and the entropy of g's last gradient call under that call's loss_keys, once.
 *   _train_step  m3pc_mtm_grad with entropy_reg read from the device temperature, then _step.  record: optional device out, the
 *                M3PC_MTM_LOSS_FLOATS floats; train_record: optional DEVICE out, 3 doubles {lr used, temperature after, log_temperature after}.
 *   _train       n_steps such steps on the segments rb draws at (seed, step0 + i) as m3pc_mtm_grad_replay draws them, eps library-drawn;
 *                masks: 4 n_steps host rows (step i: masks[4 i + key]); records (n_steps, 15) floats and train_records (n_steps, 3) doubles,
 *                optional device out.  The bf16 copies and the derived forms are written behind the last step only; weights, moments
 *                and records are bit-identical to n_steps single calls.
 *   _export/_load  which = 1: exp_avg, 2: exp_avg_sq, in the torch layout of the parameter (host or device by on_device); steps: optional
 *                HOST array, one count per listed tensor (a call that passes it waits for the stream).  m3pc_mtm_weights_export: the handle's fp32 weights.
 *   _get/_set_state  synchronous (they wait for the device).  temperature: out only, the float the next gradient call reads.
 * _create makes no HIP call; the first enqueueing call allocates two moment arenas of the parameters' size (zeroed) and the tables.  The
 * gradient object must outlive the optimizer.  The stepping entries wait for nothing and copy nothing from host memory per step; they
 * order themselves behind deferred candidate parts as m3pc_load_weights does, and invalidate what it invalidates.
 * Refused with M3PC_EINVAL before any HIP call, the argument named in m3pc_last_error: a null argument; hyper-parameters out of range
 * (negative or non-finite rates, betas outside [0, 1), eps <= 0, num_train_steps < 1, warmup_steps outside [0, num_train_steps)); what
 * m3pc_mtm_grad / m3pc_mtm_grad_replay refuse; n_steps < 1; a name that is not a parameter, a numel that does not fit, `which` not 1 or 2.
 * Refused with M3PC_ESTATE: _step without a gradient call or twice on one; a stepping entry while a pipelined certified step is between
 * _begin and _end on the handle; weights or tokenizers not loaded. */
typedef struct m3pc_mtm_opt_args {
    double learning_rate, weight_decay, beta1, beta2, eps; /* AdamW: the reference uses betas (0.9, 0.999), eps 1e-8 */
    long long num_train_steps, warmup_steps;
    double temp_learning_rate, temp_beta1, temp_beta2, temp_eps; /* the reference: 1e-4, 0.9, 0.999, 1e-8 */
    double target_entropy;
    double init_log_temperature;
} m3pc_mtm_opt_args;
typedef struct m3pc_mtm_opt_state {
    long long sched_step, temp_step;
    double log_temperature, temp_exp_avg, temp_exp_avg_sq;
    double temperature;
} m3pc_mtm_opt_state;
struct m3pc_mtm_opt;
int m3pc_mtm_opt_create(struct m3pc_mtm_grad* g, const m3pc_mtm_opt_args* args, struct m3pc_mtm_opt** out);
int m3pc_mtm_opt_destroy(struct m3pc_mtm_opt* opt);
int m3pc_mtm_lr(const m3pc_mtm_opt_args* args, long long sched_step, double* lr);
int m3pc_mtm_opt_decays(struct m3pc_mtm_opt* opt, const char* name, int* decays);
int m3pc_mtm_opt_step(struct m3pc_mtm_opt* opt, void* stream);
int m3pc_mtm_train_step(struct m3pc_mtm_opt* opt, int batch, const float* states, const float* actions, const float* rewards, const void* returns,
                        int returns_f64, const unsigned char* const masks[4], const float* eps, int flags, int loss_keys, float* record,
                        double* train_record, void* stream);
int m3pc_mtm_train(struct m3pc_mtm_opt* opt, m3pc_replay* rb, int n_steps, int batch, int mode, unsigned long long seed, unsigned long long step0,
                   const unsigned char* const* masks, int flags, int loss_keys, float* records, double* train_records, void* stream);
int m3pc_mtm_opt_export(struct m3pc_mtm_opt* opt, int which, const m3pc_named_tensor* tensors, int n, long long* steps, void* stream);
int m3pc_mtm_opt_load(struct m3pc_mtm_opt* opt, int which, const m3pc_named_tensor* tensors, int n, const long long* steps, void* stream);
int m3pc_mtm_weights_export(m3pc_handle* h, const m3pc_named_tensor* tensors, int n, void* stream);
int m3pc_mtm_opt_get_state(struct m3pc_mtm_opt* opt, m3pc_mtm_opt_state* out);
int m3pc_mtm_opt_set_state(struct m3pc_mtm_opt* opt, const m3pc_mtm_opt_state* in);

/* kernel-level timing of the last plan_step for bench.py / profiling: when enabled the library
 * brackets the MFMA launches with hipEvents on the stream they run on.  enable = 2: in addition the two candidate
 * halves of a plan step (normally overlapped on two streams) run one after the other on `stream`, so that a
 * bracket holds that launch alone.  enable = 3: that ordering WITHOUT the event brackets (for an external kernel trace
 * of every launch alone on the chip: rocprofv3 -- python3 bench.py --depth 0 --serial-halves). */
int m3pc_profile_enable(m3pc_handle* h, int enable);
/* sums since the last reset over the MFMA launches of one arithmetic (precision = M3PC_PREC_*, or -1 for
 * all) or over the fused layer-tail launches alone (M3PC_PROF_LAYER_TAIL: the dominant kernel, block_fused.hip):
 * launches, milliseconds between the bracketing events, flops (2*M*N*K per product) */
#define M3PC_PROF_LAYER_TAIL 16
int m3pc_profile_read(m3pc_handle* h, int precision, long long* launches, double* gemm_ms, double* gemm_flops,
                      int reset);

#ifdef __cplusplus
}
#endif
#endif /* M3PC_HIP_H */
