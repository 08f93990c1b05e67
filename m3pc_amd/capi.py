"""ctypes binding of libm3pc_hip.so (C ABI: include/m3pc_hip.h).

``import torch`` happens first on purpose: the library's DT_NEEDED ``libamdhip64.so.7`` then resolves to
the HIP runtime torch already loaded, so device pointers and streams are shared with PyTorch-ROCm.
The HIP extension is mandatory: if the shared object is missing this module raises -- there is no CPU
fallback anywhere in ``m3pc_amd``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence

import torch  # noqa: F401  (must precede the CDLL below)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("M3PC_LIB") or os.path.join(_HERE, "libm3pc_hip.so")  # (M3PC_LIB: tools/ point at the lab build)

STATES, ACTIONS, REWARDS, RETURNS = 0, 1, 2, 3
KEYS = ("states", "actions", "rewards", "returns")
MODE_RTG, MODE_CRITIC, MODE_NOISE = 0, 1, 2
PREC_FP32, PREC_BF16, PREC_BF16X3 = 0, 1, 2  # M3PC_PREC_*: BF16X3 is the fp32 pass with split-bf16 weight GEMMs (3 bf16 MFMAs)
PRECISIONS = {"fp32": PREC_FP32, "bf16": PREC_BF16, "bf16x3": PREC_BF16X3}
LOW_PRECISION = (PREC_BF16, PREC_BF16X3)  # candidate passes whose scores the certified fp32 re-score follows
PROF_LAYER_TAIL = 16  # m3pc_profile_read: the fused layer-tail launches only
ABI_VERSION = 7
GOAL_PIID, GOAL_ID = 0, 1  # m3pc_goal_step_batch goal_mode
SLOTS = 4  # M3PC_SLOTS: plan steps in flight per handle


def precision_code(name: str) -> int:
    """M3PC_PREC_* of a precision name ("fp32", "bf16", "bf16x3"); ValueError for anything else."""
    if name not in PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {name!r}")
    return PRECISIONS[name]

EXPORTS = (
    "m3pc_last_error", "m3pc_abi_version", "m3pc_create", "m3pc_destroy", "m3pc_load_weights", "m3pc_load_stats",
    "m3pc_set_tokenizer", "m3pc_set_critic", "m3pc_tokenize", "m3pc_detokenize", "m3pc_forward", "m3pc_goal_step",
    "m3pc_goal_step_batch",
    "m3pc_policy_pass", "m3pc_candidate_pass", "m3pc_candidate_join", "m3pc_policy_pass_batch",
    "m3pc_plan_step", "m3pc_plan_step_batch", "m3pc_score_actions", "m3pc_rescore", "m3pc_rescore_topk", "m3pc_topk_window",
    "m3pc_rescore_listed", "m3pc_rescore_merge", "m3pc_topk_race_window", "m3pc_rescore_merge_race", "m3pc_merge_race_select", "m3pc_select",
    "m3pc_profile_enable",
    "m3pc_profile_read",
    "m3pc_plan_step_certified", "m3pc_calibrate_delta",
    "m3pc_set_step_streams", "m3pc_plan_step_certified_begin", "m3pc_plan_step_certified_end", "m3pc_draw_variates",
    "m3pc_refit_resample", "m3pc_refine_plan",
    "m3pc_plan_steps_certified",
    "m3pc_eval_bound", "m3pc_plan_step_certified_eval",
    "m3pc_plan_step_certified_eval_begin", "m3pc_plan_step_certified_eval_end", "m3pc_plan_steps_certified_eval",
    "m3pc_refine_plans",
    "m3pc_episodes_create", "m3pc_episodes_destroy", "m3pc_episodes_reset", "m3pc_episodes_observe", "m3pc_episodes_record",
    "m3pc_episodes_windows", "m3pc_episodes_values", "m3pc_episodes_export",
    "m3pc_replay_create", "m3pc_replay_destroy", "m3pc_replay_append", "m3pc_replay_append_transitions", "m3pc_replay_push_episodes",
    "m3pc_replay_sample_segments", "m3pc_replay_sample_transitions", "m3pc_replay_values_up_bound", "m3pc_replay_counts",
    "m3pc_replay_path_lengths",
    "m3pc_iql_create", "m3pc_iql_destroy", "m3pc_iql_load", "m3pc_iql_export", "m3pc_iql_set_step", "m3pc_iql_get_step",
    "m3pc_iql_train_step", "m3pc_iql_train", "m3pc_iql_publish_critic", "m3pc_iql_evaluate",
    "m3pc_mtm_loss_terms", "m3pc_mtm_loss", "m3pc_mtm_loss_replay",
    "m3pc_mtm_grad_create", "m3pc_mtm_grad_destroy", "m3pc_mtm_grad", "m3pc_mtm_grad_replay", "m3pc_mtm_grad_export",
    "m3pc_mtm_grad_set_dropout", "m3pc_mtm_grad_get_dropout",
    "m3pc_mtm_opt_create", "m3pc_mtm_opt_destroy", "m3pc_mtm_lr", "m3pc_mtm_opt_decays", "m3pc_mtm_opt_step", "m3pc_mtm_train_step",
    "m3pc_mtm_train", "m3pc_mtm_opt_export", "m3pc_mtm_opt_load", "m3pc_mtm_weights_export", "m3pc_mtm_opt_get_state",
    "m3pc_mtm_opt_set_state",
)


class Dims(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "state_dim", "action_dim", "traj_length", "n_embd", "n_head", "n_enc_layer", "n_dec_layer",
        "max_candidates", "max_batch", "critic_hidden", "max_rescore", "max_goal_batch")]


class NamedTensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("numel", C.c_longlong), ("on_device", C.c_int)]


class MtmOptArgs(C.Structure):
    """m3pc_mtm_opt_args; the defaults are the reference's (learner.py:42-58; torch's AdamW / Adam eps)."""
    _fields_ = [("learning_rate", C.c_double), ("weight_decay", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("num_train_steps", C.c_longlong), ("warmup_steps", C.c_longlong), ("temp_learning_rate", C.c_double),
                ("temp_beta1", C.c_double), ("temp_beta2", C.c_double), ("temp_eps", C.c_double), ("target_entropy", C.c_double),
                ("init_log_temperature", C.c_double)]

    @classmethod
    def make(cls, learning_rate, weight_decay, num_train_steps, target_entropy, init_log_temperature, beta1=0.9, beta2=0.999, eps=1e-8,
             warmup_steps=0, temp_learning_rate=1e-4, temp_beta1=0.9, temp_beta2=0.999, temp_eps=1e-8):
        return cls(float(learning_rate), float(weight_decay), float(beta1), float(beta2), float(eps), int(num_train_steps), int(warmup_steps),
                   float(temp_learning_rate), float(temp_beta1), float(temp_beta2), float(temp_eps), float(target_entropy),
                   float(init_log_temperature))


class MtmOptState(C.Structure):
    _fields_ = [("sched_step", C.c_longlong), ("temp_step", C.c_longlong), ("log_temperature", C.c_double), ("temp_exp_avg", C.c_double),
                ("temp_exp_avg_sq", C.c_double), ("temperature", C.c_double)]


class PlanArgs(C.Structure):
    _fields_ = [("mode", C.c_int), ("precision", C.c_int), ("horizon", C.c_int), ("n_total", C.c_int),
                ("n_begin", C.c_int), ("n_count", C.c_int), ("lmbda", C.c_double), ("discount", C.c_double),
                ("rtg", C.c_double), ("slot", C.c_int), ("returns_f64", C.c_int), ("returns", C.c_void_p),
                ("flags", C.c_int), ("window", C.c_int)]


class CertArgs(C.Structure):
    """m3pc_cert_args: what ``m3pc_plan_step_certified`` takes of the certified re-score's state."""
    _fields_ = [("temperature", C.c_float), ("delta", C.c_float), ("grow_delta", C.c_int), ("kmin", C.c_int), ("kmax", C.c_int),
                ("rfirst", C.c_int), ("rmax", C.c_int)]


class CertRecord(C.Structure):
    """m3pc_cert_record: what the certified step re-scored and what its certificates said."""
    _fields_ = [("n_rescored", C.c_int), ("n_race", C.c_int), ("need_first", C.c_int), ("need_race_first", C.c_int),
                ("saturated", C.c_int), ("everything", C.c_int), ("certified", C.c_int), ("rounds", C.c_int),
                ("delta", C.c_float), ("shift", C.c_float), ("deviation", C.c_float), ("margin", C.c_float)]


class EvalRecord(C.Structure):
    """m3pc_eval_record: what the eval_action certificate of ``m3pc_plan_step_certified_eval`` bounded and asked for."""
    _fields_ = [("eval_bound", C.c_float), ("need_eval_first", C.c_int), ("n_eval", C.c_int), ("eval_rounds", C.c_int),
                ("eval_certified", C.c_int)]


class RefineArgs(C.Structure):
    """m3pc_refine_args: the refinement loop of ``m3pc_refine_plan`` (seed / step: read when the library draws the noise)."""
    _fields_ = [("iterations", C.c_int), ("top_k", C.c_int), ("weighting", C.c_int), ("temperature", C.c_float),
                ("init_std", C.c_float), ("min_std", C.c_float), ("seed_lo", C.c_uint), ("seed_hi", C.c_uint),
                ("step_lo", C.c_uint), ("step_hi", C.c_uint)]


class IqlArgs(C.Structure):
    """m3pc_iql_args: the hyper-parameters of one IQL step (``m3pc_iql_train_step`` / ``m3pc_iql_train``)."""
    _fields_ = [("v_lr", C.c_double), ("q_lr", C.c_double), ("actor_lr", C.c_double), ("expectile", C.c_double), ("beta", C.c_double),
                ("discount", C.c_double), ("tau", C.c_double), ("actor_t_max", C.c_longlong), ("flags", C.c_int)]


REFINE_CEM, REFINE_MPPI = 0, 1  # M3PC_REFINE_*
REFINE_MAX_ITER = 16
REFINE_WEIGHTINGS = {"cem": REFINE_CEM, "mppi": REFINE_MPPI}

PLAN_DEFER_JOIN = 1
PLAN_PRUNED_POLICY = 2
PLAN_INPUTS_READY = 4
WINDOW_PLAN, WINDOW_GOAL = 0, 1  # M3PC_WINDOW_*: the window rule of m3pc_episodes_windows
REPLAY_UNIFORM, REPLAY_LENGTH = 0, 1  # M3PC_REPLAY_*: how m3pc_replay_sample_segments draws a trajectory
REPLAY_OFFLINE, REPLAY_ONLINE = 0, 1  # M3PC_REPLAY_*: the two transition rings
# M3PC_IQL_*: the parts of m3pc_iql_load / _export, and the outputs of m3pc_iql_evaluate
(IQL_QF, IQL_Q_TARGET, IQL_VF, IQL_ACTOR, IQL_QF_ADAM_M, IQL_QF_ADAM_V, IQL_VF_ADAM_M, IQL_VF_ADAM_V, IQL_ACTOR_ADAM_M,
 IQL_ACTOR_ADAM_V) = range(10)
IQL_Q_MIN, IQL_Q_TARGET_MIN, IQL_V, IQL_ACTOR_MEAN = range(4)
# the masked-trajectory loss (m3pc_mtm_loss*): the record's length, the flags, and the two reference forms as (flags, loss_keys)
MTM_LOSS_FLOATS = 15
MTM_NORM_L2, MTM_CLIP_ACTIONS = 1, 2
MTM_ENTROPY, MTM_NLL, MTM_TOTAL = 12, 13, 14  # record slots behind the 4 x (loss, masked_loss, masked_c_loss)


class M3pcError(RuntimeError):
    pass


_lib = None


def load_library(path: Optional[str] = None):
    """dlopen the library (no GPU needed) and declare the prototypes."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise M3pcError(f"{p} not found: build it with `python -m m3pc_amd.build` "
                        "(m3pc_amd has no fallback path without its HIP library)")
    lib = C.CDLL(p)
    vp, i, ll, f, d = C.c_void_p, C.c_int, C.c_longlong, C.c_float, C.c_double
    lib.m3pc_last_error.restype = C.c_char_p
    lib.m3pc_last_error.argtypes = []
    lib.m3pc_abi_version.restype = i
    protos = {
        "m3pc_create": [C.POINTER(Dims), i, C.POINTER(vp)],
        "m3pc_destroy": [vp],
        "m3pc_load_weights": [vp, C.POINTER(NamedTensor), i, vp],
        "m3pc_load_stats": [vp, C.POINTER(ll)],
        "m3pc_set_tokenizer": [vp, i, C.POINTER(f), C.POINTER(f), i, i],
        "m3pc_set_critic": [vp, C.POINTER(NamedTensor), i, C.POINTER(f), C.POINTER(f), vp],
        "m3pc_tokenize": [vp, i, vp, i, vp, ll, vp],
        "m3pc_detokenize": [vp, i, vp, vp, ll, vp],
        "m3pc_forward": [vp, i, C.POINTER(vp), C.POINTER(vp), vp, vp, vp, vp, vp, i, vp],
        "m3pc_goal_step": [vp, i, vp, vp, vp, C.POINTER(d), C.POINTER(vp), C.POINTER(vp), i, vp, vp, vp, vp, vp],
        "m3pc_goal_step_batch": [vp, i, vp, vp, i, i, i, vp, vp, vp, vp],
        "m3pc_policy_pass": [vp, C.POINTER(PlanArgs), vp, vp, vp, vp, vp, vp],
        "m3pc_candidate_pass": [vp, C.POINTER(PlanArgs), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "m3pc_candidate_join": [vp, i, vp],
        "m3pc_policy_pass_batch": [vp, C.POINTER(PlanArgs), i, vp, vp, vp, C.POINTER(d), vp, vp, vp],
        "m3pc_plan_step": [vp, C.POINTER(PlanArgs), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "m3pc_plan_step_batch": [vp, C.POINTER(PlanArgs), i, vp, vp, vp, C.POINTER(d), vp, vp, vp, vp, vp, vp, vp],
        "m3pc_score_actions": [vp, C.POINTER(PlanArgs), i, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "m3pc_rescore": [vp, C.POINTER(PlanArgs), vp, vp, vp, vp, vp, i, vp, vp, vp],
        "m3pc_rescore_topk": [vp, C.POINTER(PlanArgs), vp, vp, vp, vp, vp, i, vp, vp],
        "m3pc_topk_window": [vp, vp, i, i, i, f, vp, vp, vp, vp, f, vp],
        "m3pc_rescore_merge": [vp, vp, i, vp, i, vp, vp, f, vp, vp, vp, f, vp],
        "m3pc_topk_race_window": [vp, vp, vp, f, i, i, i, i, vp, vp, vp, vp, f, vp],
        "m3pc_rescore_merge_race": [vp, vp, vp, f, i, vp, i, i, vp, vp, f, vp, vp, vp, f, vp],
        "m3pc_merge_race_select": [vp, vp, vp, f, i, vp, i, i, vp, vp, f, vp, vp, vp, f, vp, ll, vp, vp, vp, vp, vp, vp],
        "m3pc_rescore_listed": [vp, C.POINTER(PlanArgs), vp, vp, vp, vp, vp, i, vp, vp],
        "m3pc_select": [vp, vp, vp, ll, i, f, vp, vp, vp, vp, vp, vp, vp],
        "m3pc_plan_step_certified": [vp, C.POINTER(PlanArgs), C.POINTER(CertArgs), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                     vp, vp, vp, C.POINTER(CertRecord), vp],
        "m3pc_plan_steps_certified": [vp, C.POINTER(PlanArgs), C.POINTER(CertArgs), i, vp, vp, vp, C.POINTER(d), vp, vp, vp, vp, vp, vp,
                                      vp, vp, vp, vp, vp, vp, vp, C.POINTER(CertRecord), vp],
        "m3pc_eval_bound": [vp, vp, i, vp, i, i, i, vp, ll, i, f, f, f, vp, vp, f, vp],
        "m3pc_plan_step_certified_eval": [vp, C.POINTER(PlanArgs), C.POINTER(CertArgs), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                          vp, vp, vp, vp, C.POINTER(CertRecord), f, C.POINTER(EvalRecord), vp],
        "m3pc_calibrate_delta": [vp, C.POINTER(PlanArgs), vp, vp, vp, vp, vp, f, C.POINTER(f), vp],
        "m3pc_set_step_streams": [vp, vp, vp],
        "m3pc_plan_step_certified_begin": [vp, C.POINTER(PlanArgs), C.POINTER(CertArgs), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                           vp, vp, vp, vp, vp, vp],
        "m3pc_plan_step_certified_end": [vp, i, C.POINTER(CertRecord), vp],
        "m3pc_plan_step_certified_eval_begin": [vp, C.POINTER(PlanArgs), C.POINTER(CertArgs), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                vp, vp, vp, vp, vp, f, vp],
        "m3pc_plan_step_certified_eval_end": [vp, i, C.POINTER(CertRecord), C.POINTER(EvalRecord), vp],
        "m3pc_plan_steps_certified_eval": [vp, C.POINTER(PlanArgs), C.POINTER(CertArgs), i, vp, vp, vp, C.POINTER(d), vp, vp, vp, vp, vp,
                                           vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(CertRecord), f, C.POINTER(EvalRecord), vp],
        "m3pc_draw_variates": [vp, C.c_ulonglong, C.c_ulonglong, i, i, i, vp, vp, vp],
        "m3pc_refit_resample": [vp, vp, i, i, vp, vp, i, i, f, f, vp, vp, vp, vp, vp],
        "m3pc_refine_plan": [vp, C.POINTER(PlanArgs), C.POINTER(RefineArgs), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "m3pc_refine_plans": [vp, C.POINTER(PlanArgs), C.POINTER(RefineArgs), i, vp, vp, vp, C.POINTER(d), vp, i, C.POINTER(i), i, vp,
                              C.POINTER(C.c_ulonglong), vp, vp, vp, vp, vp, vp, vp, vp],
        "m3pc_episodes_create": [vp, i, i, C.POINTER(vp)],
        "m3pc_episodes_destroy": [vp],
        "m3pc_episodes_reset": [vp, C.POINTER(i), i, vp, i, i, vp],
        "m3pc_episodes_observe": [vp, C.POINTER(i), i, vp, i, i, vp],
        "m3pc_episodes_record": [vp, C.POINTER(i), i, vp, vp, f, f, i, vp],
        "m3pc_episodes_windows": [vp, C.POINTER(i), i, i, i, vp, vp, vp, C.POINTER(i), vp],
        "m3pc_episodes_values": [vp, C.POINTER(i), i, d, i, vp, vp],
        "m3pc_episodes_export": [vp, i, vp, vp, vp, C.POINTER(i), i, vp],
        "m3pc_replay_create": [vp, i, i, i, i, i, C.POINTER(vp)],
        "m3pc_replay_destroy": [vp],
        "m3pc_replay_append": [vp, i, vp, vp, vp, vp, C.POINTER(i), i, vp],
        "m3pc_replay_append_transitions": [vp, i, i, vp, vp, vp, vp, vp, i, vp],
        "m3pc_replay_push_episodes": [vp, vp, C.POINTER(i), i, d, i, vp, i, C.POINTER(i), vp],
        "m3pc_replay_sample_segments": [vp, i, i, vp, vp, i, C.c_ulonglong, C.c_ulonglong, vp, vp, vp, vp, i, vp, vp, vp],
        "m3pc_replay_sample_transitions": [vp, i, i, vp, i, C.c_ulonglong, C.c_ulonglong, vp, vp, vp, vp, vp, vp, vp],
        "m3pc_replay_values_up_bound": [vp, vp, vp],
        "m3pc_replay_counts": [vp, C.POINTER(i), C.POINTER(i), C.POINTER(i)],
        "m3pc_replay_path_lengths": [vp, C.POINTER(i), i],
        "m3pc_iql_create": [vp, i, C.POINTER(vp)],
        "m3pc_iql_destroy": [vp],
        "m3pc_iql_load": [vp, i, C.POINTER(NamedTensor), i, C.POINTER(f), C.POINTER(f), vp],
        "m3pc_iql_export": [vp, i, C.POINTER(NamedTensor), i, vp],
        "m3pc_iql_set_step": [vp, ll],
        "m3pc_iql_get_step": [vp, C.POINTER(ll)],
        "m3pc_iql_train_step": [vp, C.POINTER(IqlArgs), i, vp, vp, vp, vp, vp, vp, vp],
        "m3pc_iql_train": [vp, C.POINTER(IqlArgs), vp, i, i, i, C.c_ulonglong, C.c_ulonglong, vp, vp],
        "m3pc_iql_publish_critic": [vp, vp, vp],
        "m3pc_iql_evaluate": [vp, i, vp, vp, i, vp, vp],
        "m3pc_mtm_loss_terms": [vp, i, vp, vp, vp, vp, vp, C.POINTER(vp), C.POINTER(vp), vp, f, i, i, vp, vp],
        "m3pc_mtm_loss": [vp, i, vp, vp, vp, vp, i, C.POINTER(vp), vp, f, i, i, i, vp, vp, vp, vp, vp, vp, vp],
        "m3pc_mtm_loss_replay": [vp, vp, i, i, vp, vp, i, C.c_ulonglong, C.c_ulonglong, C.POINTER(vp), vp, f, i, i, i, vp, vp, vp, vp],
        "m3pc_mtm_grad_create": [vp, i, C.POINTER(vp)],
        "m3pc_mtm_grad_destroy": [vp],
        "m3pc_mtm_grad": [vp, i, vp, vp, vp, vp, i, C.POINTER(vp), vp, f, i, i, vp, vp],
        "m3pc_mtm_grad_replay": [vp, vp, i, i, vp, vp, i, C.c_ulonglong, C.c_ulonglong, C.POINTER(vp), vp, f, i, i, vp, vp, vp, vp],
        "m3pc_mtm_grad_export": [vp, C.POINTER(NamedTensor), i, vp],
        "m3pc_mtm_grad_set_dropout": [vp, C.c_double, C.c_ulonglong, C.c_ulonglong],
        "m3pc_mtm_grad_get_dropout": [vp, C.POINTER(C.c_double), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)],
        "m3pc_mtm_opt_create": [vp, C.POINTER(MtmOptArgs), C.POINTER(vp)],
        "m3pc_mtm_opt_destroy": [vp],
        "m3pc_mtm_lr": [C.POINTER(MtmOptArgs), ll, C.POINTER(d)],
        "m3pc_mtm_opt_decays": [vp, C.c_char_p, C.POINTER(i)],
        "m3pc_mtm_opt_step": [vp, vp],
        "m3pc_mtm_train_step": [vp, i, vp, vp, vp, vp, i, C.POINTER(vp), vp, i, i, vp, vp, vp],
        "m3pc_mtm_train": [vp, vp, i, i, i, C.c_ulonglong, C.c_ulonglong, C.POINTER(vp), i, i, vp, vp, vp],
        "m3pc_mtm_opt_export": [vp, i, C.POINTER(NamedTensor), i, C.POINTER(ll), vp],
        "m3pc_mtm_opt_load": [vp, i, C.POINTER(NamedTensor), i, C.POINTER(ll), vp],
        "m3pc_mtm_weights_export": [vp, C.POINTER(NamedTensor), i, vp],
        "m3pc_mtm_opt_get_state": [vp, C.POINTER(MtmOptState)],
        "m3pc_mtm_opt_set_state": [vp, C.POINTER(MtmOptState)],
        "m3pc_profile_enable": [vp, i],
        "m3pc_profile_read": [vp, i, C.POINTER(ll), C.POINTER(d), C.POINTER(d), i],
    }
    for name, args in protos.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = i
    if lib.m3pc_abi_version() != ABI_VERSION:
        raise M3pcError(f"ABI mismatch: library {lib.m3pc_abi_version()} vs binding {ABI_VERSION}")
    if path is None:
        _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        raise M3pcError(f"m3pc error {rc}: {load_library().m3pc_last_error().decode()}")


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _named(sd: Dict[str, torch.Tensor]):
    """state_dict -> (NamedTensor array, keep-alive list).  Tensors are made fp32-contiguous."""
    keep = []
    arr = (NamedTensor * len(sd))()
    for j, (k, v) in enumerate(sd.items()):
        t = v.detach().to(torch.float32).contiguous()
        nb = k.encode()
        keep.append((t, nb))
        arr[j] = NamedTensor(nb, t.data_ptr(), t.numel(), 1 if t.is_cuda else 0)
    return arr, keep


class HostStats:
    """A pinned, host-mapped float buffer a kernel writes its statistics to, followed (system scope, release) by a sequence
    number at [4]: the host reads them by spinning on the sequence number -- visible a few microseconds after the kernel
    ends, where a blocking device-to-host copy costs tens -- without synchronising a stream."""

    def __init__(self):
        self.buf = torch.zeros(8, dtype=torch.float32).pin_memory()
        self.np = self.buf.numpy()
        self.seq = 0

    def next_seq(self) -> float:
        self.seq = self.seq % 1000000 + 1
        return float(self.seq)

    def ready(self, seq: float) -> bool:
        return self.np[4] == seq

    def read(self):
        """[0..3] the four statistics every kernel writes; [4..6] = slots 5..7 of the buffer (m3pc_rescore_merge_race: need_race,
        the best listed race key, its threshold; zero for the kernels that write four)."""
        hs = self.np
        return [float(hs[0]), float(hs[1]), float(hs[2]), float(hs[3]), float(hs[5]), float(hs[6]), float(hs[7])]

    def wait(self, seq: float, fallback: Optional[torch.Tensor] = None, timeout: float = 10.0):
        import time as _t
        hs = self.np
        t0 = _t.perf_counter()
        spins = 0
        while hs[4] != seq:
            spins += 1
            if (spins & 1023) == 0 and _t.perf_counter() - t0 > timeout:  # never hang on the mapped buffer
                if fallback is not None:
                    # the device copy of the statistics is written on another stream than the current one: order behind
                    # everything on the device before reading it (this path is taken when the mapped buffer misbehaved)
                    torch.cuda.synchronize(fallback.device)
                    fb = [float(x) for x in fallback.cpu()]
                    return fb[:4] + (fb[5:8] if len(fb) >= 8 else [0.0, 0.0, 0.0])
                raise M3pcError("timed out waiting for kernel statistics in host-mapped memory")
        return self.read()


class Handle:
    """RAII wrapper of one m3pc_handle (one per process and GPU)."""

    def __init__(self, state_dim, action_dim, traj_length, n_embd=512, n_head=4, n_enc_layer=2, n_dec_layer=1,
                 max_candidates=1024, max_batch=1, critic_hidden=256, device: int = 0, max_rescore: int = 64,
                 max_goal_batch: int = 0):
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise M3pcError("no HIP device visible: m3pc_amd runs only on a GPU (there is no CPU path)")
        self.device = torch.device("cuda", device)
        self.dims = Dims(state_dim, action_dim, traj_length, n_embd, n_head, n_enc_layer, n_dec_layer,
                         max_candidates, max_batch, critic_hidden, max(int(max_rescore), 1), max(int(max_goal_batch), 0))
        self.max_rescore = max(int(max_rescore), 1)
        self.max_goal_batch = max(int(max_goal_batch), 0)
        self._h = C.c_void_p()
        torch.cuda.init()
        with torch.cuda.device(self.device):
            check(self.lib.m3pc_create(C.byref(self.dims), device, C.byref(self._h)))
        self.T, self.S, self.A = traj_length, state_dim, action_dim

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.m3pc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- setup -------------------------------------------------------------------------------------
    def load_weights(self, state_dict: Dict[str, torch.Tensor]):
        """All tensors (first call) or any subset of them (later calls: only what depends on them is re-derived)."""
        arr, keep = _named(state_dict)
        check(self.lib.m3pc_load_weights(self._h, arr, len(state_dict), _stream(self.device)))
        del keep

    def load_stats(self):
        """{tensors, tail_streams, kv_streams, tables_invalidated} of the last ``load_weights``."""
        out = (C.c_longlong * 4)()
        check(self.lib.m3pc_load_stats(self._h, out))
        return dict(tensors=out[0], tail_streams=out[1], kv_streams=out[2], tables_invalidated=bool(out[3]))

    def set_tokenizer(self, key: int, mean, std, normalize: bool):
        m = torch.as_tensor(mean, dtype=torch.float32).contiguous().cpu().reshape(-1)
        s = torch.as_tensor(std, dtype=torch.float32).contiguous().cpu().reshape(-1)
        fp = C.POINTER(C.c_float)
        check(self.lib.m3pc_set_tokenizer(self._h, key, C.cast(m.data_ptr(), fp), C.cast(s.data_ptr(), fp),
                                          m.numel(), int(bool(normalize))))

    def set_critic(self, q_state_dict: Dict[str, torch.Tensor], obs_mean, obs_std):
        arr, keep = _named(q_state_dict)
        m = torch.as_tensor(obs_mean, dtype=torch.float32).contiguous().cpu().reshape(-1)
        s = torch.as_tensor(obs_std, dtype=torch.float32).contiguous().cpu().reshape(-1)
        fp = C.POINTER(C.c_float)
        check(self.lib.m3pc_set_critic(self._h, arr, len(q_state_dict), C.cast(m.data_ptr(), fp),
                                       C.cast(s.data_ptr(), fp), _stream(self.device)))
        del keep

    # -- tokenizer ---------------------------------------------------------------------------------
    def tokenize(self, key: int, x: torch.Tensor) -> torch.Tensor:
        assert x.is_cuda and x.dtype in (torch.float32, torch.float64)
        x = x.contiguous()
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        rows = x.numel() // x.shape[-1]
        check(self.lib.m3pc_tokenize(self._h, key, _ptr(x), int(x.dtype == torch.float64), _ptr(out), rows,
                                     _stream(self.device)))
        return out

    def detokenize(self, key: int, y: torch.Tensor) -> torch.Tensor:
        y = y.contiguous()
        out = torch.empty_like(y)
        check(self.lib.m3pc_detokenize(self._h, key, _ptr(y), _ptr(out), y.numel() // y.shape[-1],
                                       _stream(self.device)))
        return out

    # -- model -------------------------------------------------------------------------------------
    def forward(self, tokens: Sequence[Optional[torch.Tensor]], masks: Sequence, want=KEYS, precision=PREC_FP32):
        """tokens[k]: (B,T,D_k) fp32 cuda; masks[k]: (T,) 0/1.  Returns dict of raw head outputs;
        'actions' -> (mu, std)."""
        B = next(t.shape[0] for t in tokens if t is not None)
        toks = [None if t is None else t.to(torch.float32).contiguous() for t in tokens]
        tp = (C.c_void_p * 4)(*[None if t is None else t.data_ptr() for t in toks])
        mb = [bytes(bytearray(int(v != 0) for v in m)) for m in masks]
        mbuf = [C.create_string_buffer(b, len(b)) for b in mb]
        mp = (C.c_void_p * 4)(*[C.addressof(b) for b in mbuf])
        dev = self.device
        feat = (self.S, self.A, 1, 1)
        out = {}
        for k, name in enumerate(KEYS):
            if name in want and k != ACTIONS:
                out[name] = torch.empty((B, self.T, feat[k]), dtype=torch.float32, device=dev)
        mu = sd = None
        if "actions" in want:
            mu = torch.empty((B, self.T, self.A), dtype=torch.float32, device=dev)
            sd = torch.empty_like(mu)
            out["actions"] = (mu, sd)
        check(self.lib.m3pc_forward(self._h, B, tp, mp, _ptr(out.get("states")), _ptr(out.get("rewards")),
                                    _ptr(out.get("returns")), _ptr(mu), _ptr(sd), precision, _stream(dev)))
        return out

    @staticmethod
    def _mask_ptrs(masks):
        mb = [bytes(bytearray(int(v != 0) for v in m)) for m in masks]
        mbuf = [C.create_string_buffer(b, len(b)) for b in mb]
        return (C.c_void_p * 4)(*[C.addressof(b) for b in mbuf]), mbuf

    # -- the masked-trajectory loss ------------------------------------------------------------------
    def mtm_loss_terms(self, preds, targets, masks, eps, entropy_reg: float, flags: int, loss_keys: int, batch: Optional[int] = None,
                       record: Optional[torch.Tensor] = None) -> torch.Tensor:
        """m3pc_mtm_loss_terms: preds = (states, rewards, returns, mu, std) and the four tokenised targets, (B,T,D) fp32 cuda; masks:
        four (T,) 0/1 rows; eps (B,T,A).  Returns the device record (``MTM_LOSS_FLOATS`` floats); nothing is read back."""
        p = [self._f32(t) for t in preds]
        tg = [self._f32(t) for t in targets]
        e = self._f32(eps)
        B = int(p[0].shape[0] if batch is None else batch)
        rec = torch.empty(MTM_LOSS_FLOATS, dtype=torch.float32, device=self.device) if record is None else record
        tp = (C.c_void_p * 4)(*[t.data_ptr() for t in tg])
        mp, keep = self._mask_ptrs(masks)
        check(self.lib.m3pc_mtm_loss_terms(self._h, B, *[_ptr(t) for t in p], tp, mp, _ptr(e), float(entropy_reg), int(flags), int(loss_keys),
                                           _ptr(rec), _stream(self.device)))
        return rec

    def mtm_loss(self, states, actions, rewards, returns, masks, eps, entropy_reg: float, flags: int, loss_keys: int,
                 precision: int = PREC_FP32, want_heads: bool = False):
        """m3pc_mtm_loss on a raw batch (returns float32 or float64): tokenise, forward under the masks, the loss.  Returns the device
        record, and with ``want_heads`` the five head outputs (states, rewards, returns, mu, std) behind it."""
        s, a, r = (self._f32(t) for t in (states, actions, rewards))
        v = returns.contiguous() if returns.dtype == torch.float64 else self._f32(returns)
        e = self._f32(eps)
        B = int(s.shape[0])
        f32 = dict(dtype=torch.float32, device=self.device)
        rec = torch.empty(MTM_LOSS_FLOATS, **f32)
        heads = [torch.empty((B, self.T, w), **f32) for w in (self.S, 1, 1, self.A, self.A)] if want_heads else [None] * 5
        mp, keep = self._mask_ptrs(masks)
        check(self.lib.m3pc_mtm_loss(self._h, B, _ptr(s), _ptr(a), _ptr(r), _ptr(v), int(v.dtype == torch.float64), mp, _ptr(e),
                                     float(entropy_reg), int(flags), int(loss_keys), int(precision), _ptr(rec), *[_ptr(t) for t in heads],
                                     _stream(self.device)))
        return (rec, heads) if want_heads else rec

    def goal_step(self, states, actions, rewards, rtg, masks_pi, masks_fid, idx: int):
        """Both forwards of the zero-shot piid call on raw windows: states (E,T,S), actions (E,T,A), rewards (E,T,1) fp32 cuda,
        rtg (E,) floats.  Returns (mu, std) (E,T,A) of the inverse-dynamics forward, the de-tokenised inferred states (E,T,S) and
        the observation rows the second forward saw (E,T,S)."""
        E = states.shape[0]
        f32 = dict(dtype=torch.float32, device=self.device)
        ins = [self._f32(t) for t in (states, actions, rewards)]
        inferred = torch.empty((E, self.T, self.S), **f32)
        window = torch.empty((E, self.T, self.S), **f32)
        mu = torch.empty((E, self.T, self.A), **f32)
        sd = torch.empty_like(mu)
        rt = (C.c_double * E)(*[float(v) for v in rtg])
        pi, keep1 = self._mask_ptrs(masks_pi)
        fid, keep2 = self._mask_ptrs(masks_fid)
        check(self.lib.m3pc_goal_step(self._h, E, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), rt, pi, fid, int(idx), _ptr(inferred),
                                      _ptr(window), _ptr(mu), _ptr(sd), _stream(self.device)))
        return mu, sd, inferred, window

    def goal_step_batch(self, states, actions, idx: int, goal_mode: int = GOAL_PIID, precision: int = PREC_BF16,
                        want_window: bool = False, out=None):
        """The zero-shot call for many windows, exactly pruned (m3pc_goal_step_batch): states (E,T,S), actions (E,T,A) raw fp32
        cuda.  Returns (mu, std) (E,A) of the action token at ``idx`` [and the observation rows (E,T,S) the inverse-dynamics
        forward saw].  ``out``: optional preallocated (mu, std)."""
        E = states.shape[0]
        f32 = dict(dtype=torch.float32, device=self.device)
        s, a = self._f32(states), self._f32(actions)
        assert s.shape == (E, self.T, self.S) and a.shape == (E, self.T, self.A)
        mu, sd = out if out is not None else (torch.empty((E, self.A), **f32), torch.empty((E, self.A), **f32))
        window = torch.empty((E, self.T, self.S), **f32) if want_window else None
        check(self.lib.m3pc_goal_step_batch(self._h, E, _ptr(s), _ptr(a), int(idx), int(goal_mode), int(precision), _ptr(window),
                                            _ptr(mu), _ptr(sd), _stream(self.device)))
        return (mu, sd, window) if want_window else (mu, sd)

    # -- plan step ---------------------------------------------------------------------------------
    @staticmethod
    def _f32(t):
        return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.to(torch.float32).contiguous()

    def _args(self, mode, precision, horizon, n_total, n_begin, n_count, lmbda, discount, rtg, slot=0, returns=None):
        a = PlanArgs(mode, precision, horizon, n_total, n_begin, n_count, lmbda, discount, rtg, slot, 0, None, 0, 0)
        if returns is not None:
            assert returns.is_cuda and returns.is_contiguous() and returns.numel() == self.T
            assert returns.dtype in (torch.float32, torch.float64)
            a.returns_f64 = int(returns.dtype == torch.float64)
            a.returns = returns.data_ptr()
        return a

    def policy_pass(self, mode: int, states, actions, rewards, horizon: int, rtg: float, slot: int = 0, returns=None,
                    loc=None, std=None, pruned: bool = False):
        """PASS 1 of a plan step on the current stream (chain workspace): leaves the policy head in ``slot``.
        returns: optional (T,) device row of raw returns (float32 / float64) instead of the constant ``rtg``.
        pruned (with loc = std = None): the head at the h action tokens the candidates are sampled from only, through the
        exactly pruned decoder (M3PC_PLAN_PRUNED_POLICY); rows t < T - h of the slot's loc / std are zero."""
        args = self._args(mode, PREC_FP32, horizon, 1, 0, 1, 0.0, 0.0, rtg, slot, returns)
        if pruned and loc is None and std is None:
            args.flags = PLAN_PRUNED_POLICY
        check(self.lib.m3pc_policy_pass(self._h, C.byref(args), _ptr(self._f32(states)), _ptr(self._f32(actions)),
                                        _ptr(self._f32(rewards)), _ptr(loc), _ptr(std), _stream(self.device)))

    def candidate_pass(self, mode: int, states, actions, rewards, eps, horizon: int, lmbda: float, discount: float,
                       n_total: int, n_begin: int = 0, n_count: Optional[int] = None, precision: int = PREC_FP32, slot: int = 0,
                       want_debug: bool = False, out=None, defer_join: bool = False, window: int = 0):
        """Candidates + PASS 2 + scores of a plan step on the current stream (candidate workspace) from ``slot``'s policy
        head.  ``out``: optional dict of preallocated loc / std / sample_actions / expect_return.  ``defer_join``: the
        current stream does not wait for the parts of the pass that run on the handle's own streams; the consumer of the
        scores calls ``candidate_join(slot)`` on its stream (M3PC_PLAN_DEFER_JOIN)."""
        n_count = n_total - n_begin if n_count is None else n_count
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        out = out or {}
        loc = out.get("loc")
        std = out.get("std")
        if loc is None:
            loc = torch.empty((self.T, self.A), **f32)
            std = torch.empty((self.T, self.A), **f32)
        acts = out.get("sample_actions")
        if acts is None:
            acts = torch.empty((n_count, horizon, self.A), **f32)
        er = out.get("expect_return")
        if er is None:
            er = torch.empty((n_count,), **f32)
        pr = torch.empty((n_count, horizon), **f32) if want_debug else None
        pb = torch.empty((n_count, horizon), **f32) if want_debug else None
        args = self._args(mode, precision, horizon, n_total, n_begin, n_count, lmbda, discount, 0.0, slot)
        args.flags = PLAN_DEFER_JOIN if defer_join else 0
        args.window = int(window)  # which of the slot's policy heads (policy_pass_batch)
        ins = [self._f32(t) for t in (states, actions, rewards, eps)]
        check(self.lib.m3pc_candidate_pass(self._h, C.byref(args), _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), _ptr(ins[3]),
                                           _ptr(loc), _ptr(std), _ptr(acts), _ptr(er), _ptr(pr), _ptr(pb), _stream(dev)))
        res = dict(loc=loc, std=std, sample_actions=acts, expect_return=er)
        if want_debug:
            res["pred_rewards"], res["pred_boot"] = pr, pb
        return res

    def policy_pass_batch(self, mode: int, states, actions, rewards, horizon: int, rtg, slot: int = 0, loc=None, std=None):
        """PASS 1 of E windows as one pass at batch E (policy workspace): states (E,T,S), actions (E,T,A), rewards (E,T,1),
        rtg (E,) floats.  Leaves E policy heads in ``slot``: ``candidate_pass(..., slot=slot, window=w)`` plans window w."""
        E = states.shape[0]
        args = self._args(mode, PREC_FP32, horizon, 1, 0, 1, 0.0, 0.0, 0.0, slot)
        rt = (C.c_double * E)(*[float(v) for v in rtg])
        check(self.lib.m3pc_policy_pass_batch(self._h, C.byref(args), E, _ptr(self._f32(states)), _ptr(self._f32(actions)),
                                              _ptr(self._f32(rewards)), rt, _ptr(loc), _ptr(std), _stream(self.device)))

    def candidate_join(self, slot: int):
        """Order the current stream behind every part of ``slot``'s last candidate pass enqueued with ``defer_join``."""
        check(self.lib.m3pc_candidate_join(self._h, int(slot), _stream(self.device)))

    def plan_step(self, mode: int, states, actions, rewards, eps, horizon: int, rtg: float, lmbda: float,
                  discount: float, n_total: int, n_begin: int = 0, n_count: Optional[int] = None,
                  precision: int = PREC_FP32, want_debug: bool = False, slot: int = 0, returns=None):
        n_count = n_total - n_begin if n_count is None else n_count
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        loc = torch.empty((self.T, self.A), **f32)
        std = torch.empty((self.T, self.A), **f32)
        acts = torch.empty((n_count, horizon, self.A), **f32)
        er = torch.empty((n_count,), **f32)
        pr = torch.empty((n_count, horizon), **f32) if want_debug else None
        pb = torch.empty((n_count, horizon), **f32) if want_debug else None
        args = self._args(mode, precision, horizon, n_total, n_begin, n_count, lmbda, discount, rtg, slot, returns)
        ins = [self._f32(t) for t in (states, actions, rewards, eps)]
        check(self.lib.m3pc_plan_step(self._h, C.byref(args), _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), _ptr(ins[3]),
                                      _ptr(loc), _ptr(std), _ptr(acts), _ptr(er), _ptr(pr), _ptr(pb), _stream(dev)))
        res = dict(loc=loc, std=std, sample_actions=acts, expect_return=er)
        if want_debug:
            res["pred_rewards"], res["pred_boot"] = pr, pb
        return res

    def plan_step_certified(self, mode: int, states, actions, rewards, eps, expo, horizon: int, rtg: float, lmbda: float,
                            discount: float, n_total: int, temperature: float, delta: float = 0.0, grow_delta: bool = False,
                            kmin: int = 8, kmax: int = 128, rfirst: int = 2, rmax: int = 32, precision: int = PREC_BF16,
                            slot: int = 0, returns=None, pruned: bool = False, eval_tol: Optional[float] = None):
        """One certified plan step in ONE library call (m3pc_plan_step_certified): policy pass, candidate pass in ``precision``,
        lists, fp32 re-scores, certificates and select on the current stream.  Returns (res, record): ``res`` holds loc, std,
        sample_actions, expect_return_low, expect_return (the merged vector), list (rmax + 1024 int32: race entries in front of
        ``rmax``, score entries behind) and sel = (p, eval_action, argmax, sample_idx, sample_action); ``record`` is the
        ``CertRecord`` of the step.  The host has read the step's last certificate when the call returns; the tensors are
        complete in stream order.  eval_tol (``plan_step_certified_eval``): the call is m3pc_plan_step_certified_eval and the return
        value (res, record, eval_record)."""
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        loc = torch.empty((self.T, self.A), **f32)
        std = torch.empty((self.T, self.A), **f32)
        acts = torch.empty((n_total, horizon, self.A), **f32)
        low = torch.empty((n_total,), **f32)
        merged = torch.empty((n_total,), **f32)
        lst = torch.empty((int(rmax) + 1024,), dtype=torch.int32, device=dev)
        sel = self.select_buffers(n_total)
        args = self._args(mode, precision, horizon, n_total, 0, n_total, lmbda, discount, rtg, slot, returns)
        args.flags = PLAN_PRUNED_POLICY if pruned else 0
        cert = CertArgs(float(temperature), float(delta), int(bool(grow_delta)), int(kmin), int(kmax), int(rfirst), int(rmax))
        rec = CertRecord()
        ins = [self._f32(t) for t in (states, actions, rewards, eps)]
        assert expo.numel() == n_total and expo.dtype == torch.float32 and expo.is_contiguous()
        res = dict(loc=loc, std=std, sample_actions=acts, expect_return_low=low, expect_return=merged, list=lst, sel=sel)
        if eval_tol is not None:
            erec = EvalRecord()
            check(self.lib.m3pc_plan_step_certified_eval(self._h, C.byref(args), C.byref(cert), _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]),
                                                         _ptr(ins[3]), _ptr(expo), _ptr(loc), _ptr(std), _ptr(acts), _ptr(low),
                                                         _ptr(merged), _ptr(lst), *[_ptr(t) for t in sel], C.byref(rec),
                                                         float(eval_tol), C.byref(erec), _stream(dev)))
            return res, rec, erec
        check(self.lib.m3pc_plan_step_certified(self._h, C.byref(args), C.byref(cert), _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]),
                                                _ptr(ins[3]), _ptr(expo), _ptr(loc), _ptr(std), _ptr(acts), _ptr(low), _ptr(merged),
                                                _ptr(lst), *[_ptr(t) for t in sel], C.byref(rec), _stream(dev)))
        return res, rec

    def plan_step_certified_eval(self, mode: int, states, actions, rewards, eps, expo, horizon: int, rtg: float, lmbda: float,
                                 discount: float, n_total: int, temperature: float, eval_tol: float = float("inf"), **kw):
        """``plan_step_certified`` with the eval_action certificate (m3pc_plan_step_certified_eval): the step re-scores score entries
        until |eval_action - the fp32 step's| <= eval_tol under the delta model, or scores every candidate in fp32 when its list
        cannot reach that.  eval_tol = inf: report only.  Returns (res, record, eval_record); keywords as ``plan_step_certified``."""
        return self.plan_step_certified(mode, states, actions, rewards, eps, expo, horizon, rtg, lmbda, discount, n_total, temperature,
                                        eval_tol=float(eval_tol), **kw)

    def eval_bound(self, merged: torch.Tensor, lst: torch.Tensor, r: int, n: int, n_listed: int, a0: torch.Tensor, temperature: float,
                   delta: float, eval_tol: float = float("inf"), stats: Optional[torch.Tensor] = None, host_stats=None, seq: float = 0.0):
        """The eval_action certificate on a merged vector (m3pc_eval_bound): lst = r re-scored race entries, then n_listed score
        entries of which the first n are re-scored; a0: (N, A) view (may be strided).  Returns the device stats (8 floats) =
        [eval_bound, need_eval, P_U, arg-max component, -, eps, bound(n_listed), |U|]."""
        nt = merged.numel()
        assert merged.is_contiguous() and merged.dtype == torch.float32 and lst.dtype == torch.int32 and lst.is_contiguous()
        assert a0.shape[0] == nt and a0.stride(-1) == 1 and a0.dtype == torch.float32 and lst.numel() >= r + n_listed
        if stats is None:
            stats = torch.empty((8,), dtype=torch.float32, device=self.device)
        assert stats.numel() >= 8
        check(self.lib.m3pc_eval_bound(self._h, _ptr(merged), nt, _ptr(lst), int(r), int(n), int(n_listed), _ptr(a0), a0.stride(0),
                                       a0.shape[1], float(temperature), float(delta), float(eval_tol), _ptr(stats),
                                       None if host_stats is None else C.c_void_p(host_stats.data_ptr()), float(seq),
                                       _stream(self.device)))
        return stats

    def plan_steps_certified(self, mode: int, states, actions, rewards, rtg, eps, expo, horizon: int, lmbda: float, discount: float,
                             n_total: int, temperature: float, delta: float = 0.0, grow_delta: bool = False, kmin: int = 8,
                             kmax: int = 128, rfirst: int = 2, rmax: int = 32, precision: int = PREC_BF16, slot: int = 0,
                             want_policy: bool = True, want_list: bool = True, want_p: bool = True, out=None,
                             eval_tol: Optional[float] = None):
        """A lock-step batch of certified plan steps in ONE library call (m3pc_plan_steps_certified) on the current stream: states
        (E,T,S), actions (E,T,A), rewards (E,T,1), rtg (E,) floats, eps (E, n_total, T|h, A), expo (E, n_total).  Returns (res,
        records): ``res`` holds loc / std (E,T,A), sample_actions (E,n_total,h,A), expect_return_low and expect_return (the merged
        vectors, (E,n_total)), list (E, rmax + 1024) int32 and sel = (p (E,n_total), eval_action (E,A), argmax (E,), sample_idx (E,),
        sample_action (E,A)); ``records`` is the list of the windows' ``CertRecord``.  want_policy / want_list / want_p = False: the
        optional loc + std / list / p are passed as NULL (``None`` in ``res``).  ``out``: optional preallocated contiguous outputs
        by name (loc, std, sample_actions, expect_return_low, expect_return, list, p, eval_action, argmax, sample_idx,
        sample_action).  The host has read every window's last certificate when the call returns; the tensors are complete in
        stream order.  eval_tol: the call is m3pc_plan_steps_certified_eval (the eval_action certificate per window) and the return
        value (res, records, eval_records)."""
        dev, T, A = self.device, self.T, self.A
        ins = [self._f32(t) for t in (states, actions, rewards, eps, expo)]
        E = int(ins[0].shape[0])
        assert ins[0].shape == (E, T, self.S) and ins[1].shape == (E, T, A) and ins[2].numel() == E * T
        assert ins[3].numel() == E * n_total * (horizon if mode == MODE_NOISE else T) * A and ins[4].numel() == E * n_total
        rt = [float(v) for v in rtg]
        assert len(rt) == E
        shapes = dict(loc=(E, T, A), std=(E, T, A), sample_actions=(E, n_total, horizon, A), expect_return_low=(E, n_total),
                      expect_return=(E, n_total), list=(E, int(rmax) + 1024), p=(E, n_total), eval_action=(E, A), argmax=(E,),
                      sample_idx=(E,), sample_action=(E, A))
        skip = (() if want_policy else ("loc", "std")) + (() if want_list else ("list",)) + (() if want_p else ("p",))
        o = {}
        for name, shape in shapes.items():
            dtype = torch.int32 if name in ("list", "argmax", "sample_idx") else torch.float32
            t = None
            if name not in skip:
                t = (out or {}).get(name)
                if t is None:
                    t = torch.empty(shape, dtype=dtype, device=dev)
                assert t.is_cuda and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == shape, name
            o[name] = t
        loc, std, acts, low, merged, lst = (o[k] for k in ("loc", "std", "sample_actions", "expect_return_low", "expect_return", "list"))
        sel = tuple(o[k] for k in ("p", "eval_action", "argmax", "sample_idx", "sample_action"))
        args = self._args(mode, precision, horizon, n_total, 0, n_total, lmbda, discount, 0.0, slot)
        cert = CertArgs(float(temperature), float(delta), int(bool(grow_delta)), int(kmin), int(kmax), int(rfirst), int(rmax))
        recs = (CertRecord * E)()
        res = dict(loc=loc, std=std, sample_actions=acts, expect_return_low=low, expect_return=merged, list=lst, sel=sel)
        if eval_tol is not None:
            erecs = (EvalRecord * E)()
            check(self.lib.m3pc_plan_steps_certified_eval(self._h, C.byref(args), C.byref(cert), E, _ptr(ins[0]), _ptr(ins[1]),
                                                          _ptr(ins[2]), (C.c_double * E)(*rt), _ptr(ins[3]), _ptr(ins[4]), _ptr(loc),
                                                          _ptr(std), _ptr(acts), _ptr(low), _ptr(merged), _ptr(lst),
                                                          *[_ptr(t) for t in sel], recs, float(eval_tol), erecs, _stream(dev)))
            return res, list(recs), list(erecs)
        check(self.lib.m3pc_plan_steps_certified(self._h, C.byref(args), C.byref(cert), E, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]),
                                                 (C.c_double * E)(*rt), _ptr(ins[3]), _ptr(ins[4]), _ptr(loc), _ptr(std), _ptr(acts),
                                                 _ptr(low), _ptr(merged), _ptr(lst), *[_ptr(t) for t in sel], recs, _stream(dev)))
        return res, list(recs)

    def set_step_streams(self, chain0: Optional["torch.cuda.Stream"], chain1: Optional["torch.cuda.Stream"]):
        """The two chain streams of the pipelined certified steps (m3pc_set_step_streams); None, None: the handle's own."""
        self._step_streams = (chain0, chain1)  # (kept alive as long as the handle uses them)
        check(self.lib.m3pc_set_step_streams(self._h, C.c_void_p(chain0.cuda_stream) if chain0 is not None else None,
                                             C.c_void_p(chain1.cuda_stream) if chain1 is not None else None))

    def plan_step_certified_begin(self, mode: int, states, actions, rewards, eps, expo, horizon: int, rtg: float, lmbda: float,
                                  discount: float, n_total: int, temperature: float, delta: float = 0.0, grow_delta: bool = False,
                                  kmin: int = 8, kmax: int = 128, rfirst: int = 2, rmax: int = 32, precision: int = PREC_BF16,
                                  slot: int = 0, returns=None, pruned: bool = False, inputs_ready: bool = False,
                                  eval_tol: Optional[float] = None):
        """The enqueueing half of ``plan_step_certified`` (m3pc_plan_step_certified_begin): arguments as there, on the current
        stream; nothing is read from the device.  Returns the step's ``res`` dict -- the same tensors, complete only behind
        ``plan_step_certified_end(slot)``; it also keeps the inputs alive.  states / actions / rewards / eps / expo must be fp32,
        contiguous and left untouched until the step has been ended.  inputs_ready: the window (states, actions, rewards) is
        complete already in the order of the slot's chain stream (M3PC_PLAN_INPUTS_READY): the policy pass does not wait for the
        current stream.  eval_tol: the call is m3pc_plan_step_certified_eval_begin -- the step carries the eval_action certificate
        and is resolved by ``plan_step_certified_end(slot, eval=True)``."""
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        loc = torch.empty((self.T, self.A), **f32)
        std = torch.empty((self.T, self.A), **f32)
        acts = torch.empty((n_total, horizon, self.A), **f32)
        low = torch.empty((n_total,), **f32)
        merged = torch.empty((n_total,), **f32)
        lst = torch.empty((int(rmax) + 1024,), dtype=torch.int32, device=dev)
        sel = self.select_buffers(n_total)
        args = self._args(mode, precision, horizon, n_total, 0, n_total, lmbda, discount, rtg, slot, returns)
        args.flags = (PLAN_PRUNED_POLICY if pruned else 0) | (PLAN_INPUTS_READY if inputs_ready else 0)
        cert = CertArgs(float(temperature), float(delta), int(bool(grow_delta)), int(kmin), int(kmax), int(rfirst), int(rmax))
        ins = [self._f32(t) for t in (states, actions, rewards, eps)]
        assert expo.numel() == n_total and expo.dtype == torch.float32 and expo.is_contiguous()
        if eval_tol is not None:
            check(self.lib.m3pc_plan_step_certified_eval_begin(self._h, C.byref(args), C.byref(cert), _ptr(ins[0]), _ptr(ins[1]),
                                                               _ptr(ins[2]), _ptr(ins[3]), _ptr(expo), _ptr(loc), _ptr(std), _ptr(acts),
                                                               _ptr(low), _ptr(merged), _ptr(lst), *[_ptr(t) for t in sel],
                                                               float(eval_tol), _stream(dev)))
        else:
            check(self.lib.m3pc_plan_step_certified_begin(self._h, C.byref(args), C.byref(cert), _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]),
                                                          _ptr(ins[3]), _ptr(expo), _ptr(loc), _ptr(std), _ptr(acts), _ptr(low),
                                                          _ptr(merged), _ptr(lst), *[_ptr(t) for t in sel], _stream(dev)))
        return dict(loc=loc, std=std, sample_actions=acts, expect_return_low=low, expect_return=merged, list=lst, sel=sel,
                    keep=(ins, expo, returns))

    def plan_step_certified_end(self, slot: int, eval: bool = False):
        """Resolve the step begun in ``slot`` (m3pc_plan_step_certified_end): its outputs are complete in the order of the current
        stream when the call returns; -> the step's ``CertRecord``.  eval: m3pc_plan_step_certified_eval_end, for a step begun with
        an ``eval_tol``; -> (record, eval_record)."""
        rec = CertRecord()
        if eval:
            erec = EvalRecord()
            check(self.lib.m3pc_plan_step_certified_eval_end(self._h, int(slot), C.byref(rec), C.byref(erec), _stream(self.device)))
            return rec, erec
        check(self.lib.m3pc_plan_step_certified_end(self._h, int(slot), C.byref(rec), _stream(self.device)))
        return rec

    def draw_variates(self, seed: int, step: int, n_total: int, row_elems: int, n_begin: int = 0, n_count: Optional[int] = None,
                      eps: Optional[torch.Tensor] = None, expo: Optional[torch.Tensor] = None, want_eps: bool = True,
                      want_expo: bool = True):
        """Rows [n_begin, n_begin + n_count) of the step's (n_total, row_elems) standard normals and (n_total,) Exp(1) variates
        from the library's counter-based generator (m3pc_draw_variates), on the current stream.  ``eps`` / ``expo``: optional
        contiguous fp32 device buffers of (at least) n_count * row_elems / n_count elements to draw into.  -> (eps, expo)."""
        n_count = n_total - n_begin if n_count is None else n_count
        if eps is None and want_eps:
            eps = torch.empty((n_count, row_elems), dtype=torch.float32, device=self.device)
        if expo is None and want_expo:
            expo = torch.empty((n_count,), dtype=torch.float32, device=self.device)
        for t, n in ((eps, n_count * row_elems), (expo, n_count)):
            assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= n)
        check(self.lib.m3pc_draw_variates(self._h, int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), int(n_begin), int(n_count),
                                          int(row_elems), _ptr(eps), _ptr(expo), _stream(self.device)))
        return eps, expo

    def refit_resample(self, cand: torch.Tensor, elites: torch.Tensor, scores: Optional[torch.Tensor] = None,
                       weighting: int = REFINE_CEM, temperature: float = 0.0, min_std: float = 0.0,
                       noise: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
        """One CEM / MPPI refit of cand (n,h,A) on the rows ``elites`` (k,) int32 (m3pc_refit_resample), on the current stream:
        -> (mean (h,A), std (h,A)), and with ``noise`` (n,h,A) also the resampled candidates clamp(mean + std * noise, -1, 1)
        (``out``: the buffer they go to; may be ``cand`` itself).  scores (n,): needed for REFINE_MPPI.  Needs no weights."""
        assert cand.is_cuda and cand.dtype == torch.float32 and cand.is_contiguous() and cand.dim() == 3 and cand.shape[2] == self.A
        assert elites.is_cuda and elites.dtype == torch.int32 and elites.is_contiguous()
        n, hz = int(cand.shape[0]), int(cand.shape[1])
        f32 = dict(dtype=torch.float32, device=self.device)
        mean = torch.empty((hz, self.A), **f32)
        std = torch.empty((hz, self.A), **f32)
        if scores is not None:
            assert scores.is_cuda and scores.dtype == torch.float32 and scores.is_contiguous() and scores.numel() == n
        if noise is not None:
            assert noise.is_cuda and noise.dtype == torch.float32 and noise.is_contiguous() and noise.numel() == cand.numel()
            out = torch.empty_like(cand) if out is None else out
            assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == cand.numel()
        else:
            out = None
        check(self.lib.m3pc_refit_resample(self._h, _ptr(cand), n, hz, _ptr(scores), _ptr(elites), int(elites.numel()), int(weighting),
                                           float(temperature), float(min_std), _ptr(noise), _ptr(mean), _ptr(std), _ptr(out),
                                           _stream(self.device)))
        return (mean, std) if noise is None else (mean, std, out)

    def refine_plan(self, mode: int, states, actions, rewards, horizon: int, rtg: float, lmbda: float, discount: float, n_total: int,
                    iterations: int = 2, top_k: int = 128, weighting: int = REFINE_CEM, temperature: float = 0.0,
                    init_std: float = 0.1, min_std: float = 0.0, noise: Optional[torch.Tensor] = None, seed: int = 0, step: int = 0,
                    init_mean: Optional[torch.Tensor] = None, precision: int = PREC_FP32, slot: int = 0, returns=None,
                    pruned: bool = False, out: Optional[Dict[str, torch.Tensor]] = None, want_trace: bool = True,
                    want_actions: bool = True):
        """The whole CEM / MPPI refinement of a plan in ONE library call on the current stream (m3pc_refine_plan): policy pass,
        then ``iterations`` x (score the candidates in ``precision``, top_k, refit, resample).  noise: (iterations+1, n_total, h, A)
        normals, or None: the library draws them from (seed, step) -- ``draw_variates(seed, step, (iterations+1) * n_total, h * A)``.
        init_mean (h,A): the warm start (else tanh of the policy loc).  ``out``: optional preallocated outputs by name.
        -> dict: mean, std (iterations+1,h,A), candidates (n_total,h,A), scores (iterations,n_total), elites (iterations,top_k)
        int32, sample_action (1,A), eval_action (A,).  want_trace=False: no scores / elites (the call's optional outputs are
        passed as NULL: scratch of the handle stands in); want_actions=False: no sample_action / eval_action."""
        dev, A, it, n, hz, k = self.device, self.A, int(iterations), int(n_total), int(horizon), int(top_k)
        shapes = dict(mean=(it + 1, hz, A), std=(it + 1, hz, A), candidates=(n, hz, A), scores=(it, n), elites=(it, k),
                      sample_action=(1, A), eval_action=(A,))
        res = {}
        skip = (() if want_trace else ("scores", "elites")) + (() if want_actions else ("sample_action", "eval_action"))
        for name, shape in shapes.items():
            if name in skip:
                continue
            shape = tuple(max(v, 0) for v in shape)  # (a bad size is the library's to refuse)
            dtype = torch.int32 if name == "elites" else torch.float32
            t = (out or {}).get(name)
            if t is None:
                t = torch.empty(shape, dtype=dtype, device=dev)
            assert t.is_cuda and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == shape, name
            res[name] = t
        if noise is not None:
            assert noise.is_cuda and noise.dtype == torch.float32 and noise.is_contiguous() and noise.numel() == (it + 1) * n * hz * A
        if init_mean is not None:
            init_mean = self._f32(init_mean)
            assert init_mean.is_cuda and init_mean.numel() == hz * A
        args = self._args(mode, precision, hz, n, 0, n, lmbda, discount, rtg, slot, returns)
        args.flags = PLAN_PRUNED_POLICY if pruned else 0
        seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
        ref = RefineArgs(it, k, int(weighting), float(temperature), float(init_std), float(min_std), seed & 0xFFFFFFFF, seed >> 32,
                         step & 0xFFFFFFFF, step >> 32)
        ins = [self._f32(t) for t in (states, actions, rewards)]
        check(self.lib.m3pc_refine_plan(self._h, C.byref(args), C.byref(ref), _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), _ptr(init_mean),
                                        _ptr(noise), _ptr(res["mean"]), _ptr(res["std"]), _ptr(res["candidates"]), _ptr(res.get("scores")),
                                        _ptr(res.get("elites")), _ptr(res.get("sample_action")), _ptr(res.get("eval_action")), _stream(dev)))
        return res

    def refine_plans(self, mode: int, states, actions, rewards, horizon: int, rtg, lmbda: float, discount: float, n_total: int,
                     iterations: int = 2, top_k: int = 128, weighting: int = REFINE_CEM, temperature: float = 0.0,
                     init_std: float = 0.1, min_std: float = 0.0, noise: Optional[torch.Tensor] = None, seed: int = 0, step: int = 0,
                     steps=None, init_mean: Optional[torch.Tensor] = None, init_rows=None, init_offset: int = 0,
                     precision: int = PREC_FP32, slot: int = 0, out: Optional[Dict[str, torch.Tensor]] = None,
                     want_trace: bool = True, want_actions: bool = True):
        """``refine_plan`` for E windows that step together, in ONE library call on the current stream (m3pc_refine_plans): states
        (E,T,S), actions (E,T,A), rewards (E,T,1), rtg (E,) floats.  noise: (iterations+1, E, n_total, h, A) normals, or None: the
        library draws window w's from (seed, steps[w]) -- ``steps`` (E,) ints, default ``step + w``.  init_mean (E, init_stride, A):
        the warm start; row t of window w's first mean is init_mean[w, t + init_offset] while t + init_offset < init_rows[w]
        (default: init_stride), else tanh of the window's policy loc; init_rows[w] = 0: a cold start.
        -> dict: mean, std (iterations+1,E,h,A), candidates (E,n_total,h,A), scores (iterations,E,n_total), elites
        (iterations,E,top_k) int32, sample_action, eval_action (E,A).  want_trace / want_actions / out: as ``refine_plan``."""
        dev, A, it, n, hz, k = self.device, self.A, int(iterations), int(n_total), int(horizon), int(top_k)
        ins = [self._f32(t) for t in (states, actions, rewards)]
        E = int(ins[0].shape[0]) if ins[0].dim() == 3 else 0
        assert ins[0].shape == (E, self.T, self.S) and ins[1].shape == (E, self.T, A) and ins[2].numel() == E * self.T
        rt = [float(v) for v in rtg]
        assert len(rt) == E
        shapes = dict(mean=(it + 1, E, hz, A), std=(it + 1, E, hz, A), candidates=(E, n, hz, A), scores=(it, E, n), elites=(it, E, k),
                      sample_action=(E, A), eval_action=(E, A))
        res = {}
        skip = (() if want_trace else ("scores", "elites")) + (() if want_actions else ("sample_action", "eval_action"))
        for name, shape in shapes.items():
            if name in skip:
                continue
            shape = tuple(max(v, 0) for v in shape)  # (a bad size is the library's to refuse)
            dtype = torch.int32 if name == "elites" else torch.float32
            t = (out or {}).get(name)
            if t is None:
                t = torch.empty(shape, dtype=dtype, device=dev)
            assert t.is_cuda and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == shape, name
            res[name] = t
        if noise is not None:
            assert noise.is_cuda and noise.dtype == torch.float32 and noise.is_contiguous() and noise.numel() == (it + 1) * E * n * hz * A
        stride, rows = 0, None
        if init_mean is not None:
            init_mean = self._f32(init_mean)
            assert init_mean.is_cuda and init_mean.dim() == 3 and init_mean.shape[0] == E and init_mean.shape[2] == A
            stride = int(init_mean.shape[1])
            if init_rows is not None:
                assert len(init_rows) == E
                rows = (C.c_int * max(E, 1))(*[int(v) for v in init_rows])
        stp = None
        if steps is not None:
            assert len(steps) == E
            stp = (C.c_ulonglong * max(E, 1))(*[int(v) & (2 ** 64 - 1) for v in steps])
        args = self._args(mode, precision, hz, n, 0, n, lmbda, discount, 0.0, slot)
        seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
        ref = RefineArgs(it, k, int(weighting), float(temperature), float(init_std), float(min_std), seed & 0xFFFFFFFF, seed >> 32,
                         step & 0xFFFFFFFF, step >> 32)
        check(self.lib.m3pc_refine_plans(self._h, C.byref(args), C.byref(ref), E, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]),
                                         (C.c_double * max(E, 1))(*rt), _ptr(init_mean), stride, rows, int(init_offset), _ptr(noise), stp,
                                         _ptr(res["mean"]), _ptr(res["std"]), _ptr(res["candidates"]), _ptr(res.get("scores")),
                                         _ptr(res.get("elites")), _ptr(res.get("sample_action")), _ptr(res.get("eval_action")),
                                         _stream(dev)))
        return res

    def calibrate_delta(self, mode: int, states, actions, rewards, eps, scores_low: torch.Tensor, horizon: int, lmbda: float,
                        discount: float, n_total: int, factor: float = 1.6, slot: int = 0) -> float:
        """delta of the certified step from one full fp32 candidate pass over the candidates of the step that owns ``slot``
        (m3pc_calibrate_delta): max(factor x the largest deviation of (scores_low - fp32) from its lower median, 1e-6 x the
        largest |fp32 score|, 1e-30).  Blocks until the statistics are on the host."""
        assert scores_low.numel() == n_total and scores_low.dtype == torch.float32 and scores_low.is_contiguous()
        args = self._args(mode, PREC_FP32, horizon, n_total, 0, n_total, lmbda, discount, 0.0, slot)
        ins = [self._f32(t) for t in (states, actions, rewards, eps)]
        out = C.c_float()
        check(self.lib.m3pc_calibrate_delta(self._h, C.byref(args), _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), _ptr(ins[3]),
                                            _ptr(scores_low), float(factor), C.byref(out), _stream(self.device)))
        return float(out.value)

    def plan_step_batch(self, mode: int, states, actions, rewards, rtg, eps, horizon: int, lmbda: float, discount: float,
                        n_total: int, precision: int = PREC_FP32, slot: int = 0):
        """E windows x n_total candidates in one pass: states (E,T,S), actions (E,T,A), rewards (E,T,1), rtg (E,) floats,
        eps (E, n_total, T|h, A).  Returns expect_return (E, n_total), sample_actions (E, n_total, h, A), loc/std (E,T,A)."""
        E = states.shape[0]
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        loc = torch.empty((E, self.T, self.A), **f32)
        std = torch.empty((E, self.T, self.A), **f32)
        acts = torch.empty((E, n_total, horizon, self.A), **f32)
        er = torch.empty((E, n_total), **f32)
        widx = torch.arange(E, dtype=torch.int32, device=dev).repeat_interleave(n_total).contiguous()
        args = self._args(mode, precision, horizon, n_total, 0, n_total, lmbda, discount, 0.0, slot)
        ins = [self._f32(t) for t in (states, actions, rewards, eps)]
        assert ins[3].numel() == E * n_total * (horizon if mode == MODE_NOISE else self.T) * self.A
        rt = (C.c_double * E)(*[float(v) for v in rtg])
        check(self.lib.m3pc_plan_step_batch(self._h, C.byref(args), E, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), rt, _ptr(ins[3]),
                                            _ptr(widx), _ptr(loc), _ptr(std), _ptr(acts), _ptr(er), _stream(dev)))
        return dict(loc=loc, std=std, sample_actions=acts, expect_return=er, window_index=widx)

    def score_actions(self, mode: int, states, actions, rewards, cand: torch.Tensor, window_index: Optional[torch.Tensor],
                      horizon: int, lmbda: float, discount: float, precision: int = PREC_FP32, want_debug: bool = False,
                      slot: int = 0):
        """TD(lambda) scores of caller-supplied candidates cand (n,h,A); states/actions/rewards (E,T,.) or (T,.) windows,
        window_index (n,) int32 (None: one window).  slot: whose returns tokens (and, for few-row fp32 calls, which of the two
        chain workspaces: slot & 1) the pass uses."""
        dev = self.device
        n = cand.shape[0]
        ins = [self._f32(t) for t in (states, actions, rewards, cand)]
        E = 1 if ins[0].dim() == 2 else ins[0].shape[0]
        er = torch.empty((n,), dtype=torch.float32, device=dev)
        pr = torch.empty((n, horizon), dtype=torch.float32, device=dev) if want_debug else None
        pb = torch.empty((n, horizon), dtype=torch.float32, device=dev) if want_debug else None
        wi = None if window_index is None else window_index.to(torch.int32).contiguous()
        args = self._args(mode, precision, horizon, n, 0, n, lmbda, discount, 0.0, slot)
        check(self.lib.m3pc_score_actions(self._h, C.byref(args), E, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), _ptr(ins[3]),
                                          _ptr(wi), _ptr(er), _ptr(pr), _ptr(pb), _stream(dev)))
        return (er, pr, pb) if want_debug else er

    def rescore(self, mode: int, states, actions, rewards, eps, index: torch.Tensor, horizon: int, rtg: float,
                lmbda: float, discount: float, n_total: int, slot: int = 0, out: Optional[torch.Tensor] = None, want_actions: bool = True):
        """fp32 scores (and candidates) of rows ``index`` (int32 cuda) of the plan step that owns ``slot``.
        ``out``: optional (n,) fp32 destination of the scores (a slice of a larger buffer is fine)."""
        n = index.numel()
        dev = self.device
        acts = torch.empty((n, horizon, self.A), dtype=torch.float32, device=dev) if want_actions else None
        er = out if out is not None else torch.empty((n,), dtype=torch.float32, device=dev)
        assert er.numel() == n and er.is_contiguous() and er.dtype == torch.float32
        args = self._args(mode, PREC_FP32, horizon, n_total, 0, n, lmbda, discount, rtg, slot)
        ins = [self._f32(t) for t in (states, actions, rewards, eps)]
        assert index.dtype == torch.int32 and index.is_contiguous()
        check(self.lib.m3pc_rescore(self._h, C.byref(args), _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), _ptr(ins[3]),
                                    _ptr(index), n, _ptr(acts), _ptr(er), _stream(dev)))
        return er, acts

    def rescore_topk(self, mode: int, states, actions, rewards, eps, expect_return: torch.Tensor, k: int,
                     horizon: int, rtg: float, lmbda: float, discount: float, slot: int = 0):
        """Replace the k largest entries of ``expect_return`` (all N candidates, contiguous fp32 cuda) by
        their fp32 re-scores, in place.  Returns the re-scored candidate ids (k,) int32."""
        n = expect_return.numel()
        assert expect_return.is_contiguous() and expect_return.dtype == torch.float32
        top = torch.empty((k,), dtype=torch.int32, device=self.device)
        args = self._args(mode, PREC_FP32, horizon, n, 0, n, lmbda, discount, rtg, slot)
        ins = [self._f32(t) for t in (states, actions, rewards, eps)]
        check(self.lib.m3pc_rescore_topk(self._h, C.byref(args), _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]),
                                         _ptr(ins[3]), _ptr(expect_return), k, _ptr(top), _stream(self.device)))
        return top

    def topk_window(self, expect_return: torch.Tensor, kmax: int, kmin: int, window: float, top: Optional[torch.Tensor] = None,
                    stats: Optional[torch.Tensor] = None, top_scores: Optional[torch.Tensor] = None, host_stats=None, seq: float = 0.0):
        """The kmax + 1 best candidates (ids, best first) and stats = [n, margin to the best one outside the n, max, raw
        count over the whole vector] where n = clamp(#{E >= max E - window}, kmin, kmax).  Both stay on the device.
        top_scores: optional (kmax + 1,) buffer receiving the listed scores; host_stats: optional pinned float tensor (>= 5)
        the kernel also writes, followed by ``seq`` (see ``HostStats``)."""
        n = expect_return.numel()
        assert expect_return.is_contiguous() and expect_return.dtype == torch.float32
        if top is None:
            top = torch.empty((kmax + 1,), dtype=torch.int32, device=self.device)
        if stats is None:
            stats = torch.empty((4,), dtype=torch.float32, device=self.device)
        check(self.lib.m3pc_topk_window(self._h, _ptr(expect_return), n, kmax, kmin, float(window), _ptr(top), _ptr(stats),
                                        _ptr(top_scores), None if host_stats is None else C.c_void_p(host_stats.data_ptr()),
                                        float(seq), _stream(self.device)))
        return top, stats

    def topk_window_issue(self, expect_return: torch.Tensor, kmax: int, kmin: int, window: float):
        """``topk_window`` with its statistics also written to a pinned, host-mapped buffer followed by a sequence number.
        Returns (top ids on the device, ticket for ``topk_window_wait``); one ticket outstanding at a time."""
        if not hasattr(self, "_hs"):
            self._hs = HostStats()
        seq = self._hs.next_seq()
        top, stats = self.topk_window(expect_return, kmax, kmin, window, host_stats=self._hs.buf, seq=seq)
        return top, (seq, stats)

    def topk_window_wait(self, ticket):
        """The statistics of ``topk_window_issue`` on the host without a stream synchronisation.
        [n, margin_outside, max, raw count] as python floats."""
        seq, stats = ticket
        return self._hs.wait(seq, stats)

    def topk_window_host(self, expect_return: torch.Tensor, kmax: int, kmin: int, window: float):
        """``topk_window_issue`` + ``topk_window_wait``: (top ids on the device, statistics on the host)."""
        top, ticket = self.topk_window_issue(expect_return, kmax, kmin, window)
        return top, self.topk_window_wait(ticket)

    def rescore_listed(self, mode: int, states, actions, rewards, eps, expect_return: torch.Tensor, index: torch.Tensor,
                       horizon: int, rtg: float, lmbda: float, discount: float, slot: int = 0):
        """Replace the entries ``index`` (int32 cuda) of ``expect_return`` by their fp32 re-scores, in place."""
        n = expect_return.numel()
        assert index.dtype == torch.int32 and index.is_contiguous() and expect_return.is_contiguous()
        args = self._args(mode, PREC_FP32, horizon, n, 0, n, lmbda, discount, rtg, slot)
        ins = [self._f32(t) for t in (states, actions, rewards, eps)]
        check(self.lib.m3pc_rescore_listed(self._h, C.byref(args), _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), _ptr(ins[3]),
                                           _ptr(index), index.numel(), _ptr(expect_return), _stream(self.device)))

    def rescore_merge(self, scores: torch.Tensor, index: torch.Tensor, n: int, top_scores: torch.Tensor, top_rescored: torch.Tensor,
                      delta: float = 0.0, merged: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None, host_stats=None,
                      seq: float = 0.0):
        """merged = scores - median(top_scores[:n] - top_rescored[:n]), entries index[:n] replaced by top_rescored[:n];
        stats = [shift, largest deviation from it, need = #{scores > best fp32 + shift - delta}, margin].  See m3pc_rescore_merge."""
        assert scores.is_contiguous() and scores.dtype == torch.float32 and index.dtype == torch.int32
        if merged is None:
            merged = torch.empty_like(scores)
        if stats is None:
            stats = torch.empty((4,), dtype=torch.float32, device=self.device)
        check(self.lib.m3pc_rescore_merge(self._h, _ptr(scores), scores.numel(), _ptr(index), int(n), _ptr(top_scores),
                                          _ptr(top_rescored), float(delta), _ptr(merged), _ptr(stats),
                                          None if host_stats is None else C.c_void_p(host_stats.data_ptr()), float(seq),
                                          _stream(self.device)))
        return merged, stats

    def topk_race_window(self, expect_return: torch.Tensor, expo: torch.Tensor, temperature: float, kmax: int, kmin: int, rmax: int,
                         lst: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None,
                         list_scores: Optional[torch.Tensor] = None, want_stats: bool = True):
        """``topk_window`` plus the rmax best candidates by race key temperature * E - log expo (the multinomial draw's race),
        in one list: lst[rmax + i] = i-th best by score (i <= kmax), lst[rmax - 1 - i] = i-th best racer.  Returns (lst, stats)."""
        n = expect_return.numel()
        assert expect_return.is_contiguous() and expect_return.dtype == torch.float32
        assert expo.is_contiguous() and expo.dtype == torch.float32 and expo.numel() == n
        if lst is None:
            lst = torch.empty((rmax + kmax + 1,), dtype=torch.int32, device=self.device)
        if stats is None and want_stats:
            stats = torch.empty((4,), dtype=torch.float32, device=self.device)
        assert lst.numel() >= rmax + min(kmax + 1, n)
        check(self.lib.m3pc_topk_race_window(self._h, _ptr(expect_return), _ptr(expo), float(temperature), n, int(kmax), int(kmin),
                                             int(rmax), _ptr(lst), _ptr(stats), _ptr(list_scores), None, 0.0, _stream(self.device)))
        return lst, stats

    def rescore_merge_race(self, scores: torch.Tensor, expo: torch.Tensor, temperature: float, lst: torch.Tensor, r: int, n: int,
                           list_scores: torch.Tensor, list_rescored: torch.Tensor, delta: float = 0.0,
                           merged: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None, host_stats=None, seq: float = 0.0):
        """``rescore_merge`` over r race entries followed by n score entries (lst / list_scores / list_rescored start at the first
        race entry); stats (8 floats) = [shift, deviation, need, margin, -, need_race, best listed race key, its threshold]."""
        assert scores.is_contiguous() and scores.dtype == torch.float32 and lst.dtype == torch.int32
        assert lst.numel() >= r + n and list_scores.numel() >= r + n and list_rescored.numel() >= r + n
        if merged is None:
            merged = torch.empty_like(scores)
        if stats is None:
            stats = torch.empty((8,), dtype=torch.float32, device=self.device)
        assert stats.numel() >= 8
        check(self.lib.m3pc_rescore_merge_race(self._h, _ptr(scores), _ptr(expo), float(temperature), scores.numel(), _ptr(lst), int(r),
                                               int(n), _ptr(list_scores), _ptr(list_rescored), float(delta), _ptr(merged), _ptr(stats),
                                               None if host_stats is None else C.c_void_p(host_stats.data_ptr()), float(seq),
                                               _stream(self.device)))
        return merged, stats

    def merge_race_select(self, scores: torch.Tensor, expo: torch.Tensor, temperature: float, lst: torch.Tensor, r: int, n: int,
                          list_scores: torch.Tensor, list_rescored: torch.Tensor, a0: torch.Tensor, delta: float = 0.0,
                          merged: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None, host_stats=None, seq: float = 0.0,
                          out=None):
        """``rescore_merge_race`` + ``select`` on the merged vector in one launch.  Returns (merged, stats, (p, eval_action, argmax,
        sample_idx, sample_action))."""
        nt = scores.numel()
        assert scores.is_contiguous() and scores.dtype == torch.float32 and lst.dtype == torch.int32
        assert lst.numel() >= r + n and list_scores.numel() >= r + n and list_rescored.numel() >= r + n
        assert a0.shape[0] == nt and a0.stride(-1) == 1 and expo.numel() == nt and expo.is_contiguous()
        if merged is None:
            merged = torch.empty_like(scores)
        if stats is None:
            stats = torch.empty((8,), dtype=torch.float32, device=self.device)
        p, ev, am, si, sa = out if out is not None else self.select_buffers(nt)
        check(self.lib.m3pc_merge_race_select(self._h, _ptr(scores), _ptr(expo), float(temperature), nt, _ptr(lst), int(r), int(n),
                                              _ptr(list_scores), _ptr(list_rescored), float(delta), _ptr(merged), _ptr(stats),
                                              None if host_stats is None else C.c_void_p(host_stats.data_ptr()), float(seq),
                                              _ptr(a0), a0.stride(0), _ptr(p), _ptr(ev), _ptr(am), _ptr(si), _ptr(sa),
                                              _stream(self.device)))
        return merged, stats, (p, ev, am, si, sa)

    def select_buffers(self, n: int):
        """Output tensors of ``select`` (p, eval_action, argmax, sample_idx, sample_action), allocated on the current stream."""
        dev = self.device
        return (torch.empty((n,), dtype=torch.float32, device=dev), torch.empty((self.A,), dtype=torch.float32, device=dev),
                torch.empty((1,), dtype=torch.int32, device=dev), torch.empty((1,), dtype=torch.int32, device=dev),
                torch.empty((1, self.A), dtype=torch.float32, device=dev))

    def select(self, expect_return: torch.Tensor, a0: torch.Tensor, temperature: float,
               expo: Optional[torch.Tensor] = None, out=None):
        """a0: (N, A) view (may be a strided slice sample_actions[:, 0]).  Returns (p, eval_action, argmax)
        and, when ``expo`` (N Exp(1) variates) is given, also (sample_idx, sample_action (1, A)).
        out: optional ``select_buffers(n)`` tuple to write into."""
        n = expect_return.numel()
        assert a0.shape[0] == n and a0.stride(-1) == 1
        p, ev, am, si, sa = out if out is not None else self.select_buffers(n)
        if expo is None:
            si = sa = None
        else:
            assert expo.numel() == n and expo.dtype == torch.float32 and expo.is_contiguous()
        check(self.lib.m3pc_select(self._h, _ptr(expect_return.contiguous()), _ptr(a0), a0.stride(0), n,
                                   float(temperature), _ptr(expo), _ptr(p), _ptr(ev), _ptr(am), _ptr(si), _ptr(sa),
                                   _stream(self.device)))
        if expo is None:
            return p, ev, am
        return p, ev, am, si, sa

    # -- profiling ---------------------------------------------------------------------------------
    def profile_enable(self, on):
        """False / True, or 2: also run the candidate halves one after the other (each bracket holds one launch alone)."""
        check(self.lib.m3pc_profile_enable(self._h, int(on)))

    def profile_read(self, precision: int = -1, reset: bool = True):
        n, ms, fl = C.c_longlong(), C.c_double(), C.c_double()
        check(self.lib.m3pc_profile_read(self._h, precision, C.byref(n), C.byref(ms), C.byref(fl), int(reset)))
        return n.value, ms.value, fl.value
