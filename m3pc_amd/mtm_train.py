"""Training the masked-trajectory model on the device (m3pc_mtm_opt_*, m3pc_mtm_train*): ``Learner.mtm_update``
(finetune_omtm/learner.py:506-538) as one library call -- the gradient of m3pc_mtm_grad under the device's own temperature, AdamW in
the two groups of ``omtm.configure_optimizers``, the LambdaLR schedule and the float64 temperature step -- applied to the PLANNER'S
OWN weights, with every derived weight form refreshed behind it.  Nothing crosses the host; the next plan step runs on the trained
weights.  Arithmetic order: m3pc_amd/csrc/mtm_opt.h.

The model trained is the eval-mode one unless the trainer is created with ``dropout=p``: then every step drops with the library's own
keep-mask stream (m3pc_amd/mtm_grad.py), step i of the trainer's life under draw i, and ``get_state`` / ``set_state`` carry (p, seed,
next draw) so that a resumed run continues the stream.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional

import numpy as np
import torch

from . import capi
from .masks import mask_rows
from .mtm import device_batch, form_settings, loss_tuple, named_strict
from .mtm_grad import DeviceMTMGrad

KEYS = capi.KEYS
EXP_AVG, EXP_AVG_SQ = 1, 2


def decays(name: str) -> bool:
    """The weight-decay group of ``omtm.configure_optimizers`` (mtm_model.py:779-841) on this architecture: the weights of Linear and
    MultiheadAttention modules decay; biases, LayerNorm weights (the heads' ``.0.weight`` included), per-dim encodings and mask
    tokens do not.  The Python mirror of m3pc_mtm_opt_decays."""
    return name.endswith("weight") and ".norm" not in name and not name.endswith(".0.weight")


def lr_at(sched_step: int, learning_rate: float, num_train_steps: int, warmup_steps: int = 0) -> float:
    """The Python mirror of m3pc_mtm_lr: learning_rate * lambda(sched_step) (learner.py:50-51; omtm/train.py:889-899)."""
    s = int(sched_step)
    if warmup_steps > 0:
        if s < warmup_steps:
            lam = s / warmup_steps
        else:
            lam = 0.5 * (1.0 + math.cos((s - warmup_steps) / (num_train_steps - warmup_steps) * math.pi))
    else:
        lam = 0.5 * (1.0 + math.cos(s / num_train_steps * math.pi))
    return learning_rate * lam


class DeviceMTMTrainer:
    """One m3pc_mtm_opt object (and the m3pc_mtm_grad object it steps) on a planner's handle.

    opt_args: learning_rate, weight_decay, num_train_steps, target_entropy, init_log_temperature and optionally beta1, beta2, eps,
    warmup_steps, temp_learning_rate, temp_beta1, temp_beta2, temp_eps (``capi.MtmOptArgs.make``).
    dropout, dropout_seed: ``self.grad.set_dropout(dropout, dropout_seed)`` (0: the eval-mode model)."""

    def __init__(self, planner, max_batch: int, dropout: float = 0.0, dropout_seed: int = 0, **opt_args):
        self.planner = planner if hasattr(planner, "handle") else None
        self.handle = getattr(planner, "handle", planner)
        self.lib = self.handle.lib
        self.device = self.handle.device
        self.max_batch = int(max_batch)
        self.args = capi.MtmOptArgs.make(**opt_args)
        self.grad = DeviceMTMGrad(self.handle, self.max_batch)
        self.shapes = self.grad.shapes
        self._o = C.c_void_p()
        try:
            if dropout:
                self.grad.set_dropout(dropout, dropout_seed)
            capi.check(self.lib.m3pc_mtm_opt_create(self.grad._g, C.byref(self.args), C.byref(self._o)))
        except Exception:
            self.grad.close()
            raise

    def close(self):
        if getattr(self, "_o", None) is not None and self._o.value:
            with torch.cuda.device(self.device):
                self.lib.m3pc_mtm_opt_destroy(self._o)
            self._o = C.c_void_p()
        if getattr(self, "grad", None) is not None:
            self.grad.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return capi._stream(self.device)

    def _moved(self):
        if self.planner is not None and hasattr(self.planner, "_reset_calibration"):
            self.planner._reset_calibration()  # (the delta calibration belongs to the weights it was measured on)

    # -- host-only ----------------------------------------------------------------------------------
    def lr(self, sched_step: int) -> float:
        out = C.c_double()
        capi.check(self.lib.m3pc_mtm_lr(C.byref(self.args), int(sched_step), C.byref(out)))
        return out.value

    def decays(self, name: str) -> bool:
        out = C.c_int()
        capi.check(self.lib.m3pc_mtm_opt_decays(self._o, name.encode(), C.byref(out)))
        return bool(out.value)

    def get_state(self) -> Dict[str, float]:
        st = capi.MtmOptState()
        with torch.cuda.device(self.device):
            capi.check(self.lib.m3pc_mtm_opt_get_state(self._o, C.byref(st)))
        out = {n: getattr(st, n) for n, _ in capi.MtmOptState._fields_}
        out["dropout"], out["dropout_seed"], out["dropout_next_draw"] = self.grad.get_dropout()
        return out

    def set_state(self, sched_step: int, temp_step: int, log_temperature: float, temp_exp_avg: float = 0.0, temp_exp_avg_sq: float = 0.0,
                  temperature=None, dropout=None, dropout_seed: int = 0, dropout_next_draw: int = 0):
        """What ``get_state`` returned (``set_state(**get_state())``).  temperature is derived, not set; dropout None leaves the
        keep-mask stream where it stands."""
        st = capi.MtmOptState(int(sched_step), int(temp_step), float(log_temperature), float(temp_exp_avg), float(temp_exp_avg_sq), 0.0)
        with torch.cuda.device(self.device):
            capi.check(self.lib.m3pc_mtm_opt_set_state(self._o, C.byref(st)))
        if dropout is not None:
            self.grad.set_dropout(dropout, dropout_seed, dropout_next_draw)

    # -- the steps ----------------------------------------------------------------------------------
    def opt_step(self):
        """m3pc_mtm_opt_step: applies the gradients and the entropy of ``self.grad``'s last gradient call, once."""
        with torch.cuda.device(self.device):
            capi.check(self.lib.m3pc_mtm_opt_step(self._o, self._stream()))
        self._moved()

    def train_step_record(self, batch, masks, eps=None, form: str = "finetune", flags=None, loss_keys=None):
        """m3pc_mtm_train_step on a raw batch {key: (B,T,D_k)} -> (record: 15 device floats, train_record: 3 device doubles
        {lr used, temperature after, log_temperature after}).  No host wait."""
        B, s, a, r, v, e, f64, f, bits = device_batch(self.handle, batch, eps, form, flags, loss_keys)
        rec = torch.empty(capi.MTM_LOSS_FLOATS, dtype=torch.float32, device=self.device)
        trec = torch.empty(3, dtype=torch.float64, device=self.device)
        mp, keep = self.handle._mask_ptrs(mask_rows(masks))
        with torch.cuda.device(self.device):
            capi.check(self.lib.m3pc_mtm_train_step(self._o, B, capi._ptr(s), capi._ptr(a), capi._ptr(r), capi._ptr(v), f64,
                                                    mp, capi._ptr(e), f, bits, capi._ptr(rec), capi._ptr(trec), self._stream()))
        del keep
        self._moved()
        return rec, trec

    def train_step(self, batch, masks, eps=None, form: str = "finetune") -> Dict[str, float]:
        """One ``Learner.mtm_update``: -> the reference's ``log_dict`` (``train/loss*``, ``train/lr``, ``train/temperature``,
        ``train/entropy``).  Reading the log waits for the device; ``train_step_record`` does not."""
        rec, trec = self.train_step_record(batch, masks, eps, form)
        return self.log_dict(rec, trec, form, list(batch.keys()))

    @staticmethod
    def log_dict(rec, trec, form: str = "finetune", order=KEYS) -> Dict[str, float]:
        loss, losses, masked_losses, masked_c_losses, entropy = loss_tuple(rec, form_settings(form, list(order))[2])
        log = {}
        for k, l in losses.items():
            log[f"train/loss_{k}"] = l
            if k in masked_losses:
                log[f"train/masked_loss_{k}"] = masked_losses[k]
            if k in masked_c_losses:
                log[f"train/masked_c_loss_{k}"] = masked_c_losses[k]
        t = trec.cpu().tolist()
        log["train/loss"] = loss.item()
        log["train/lr"] = t[0]
        log["train/temperature"] = t[1]
        log["train/entropy"] = entropy.item()
        return log

    def train_from(self, replay, n_steps: int, batch: Optional[int] = None, masks=None, form: str = "finetune"):
        """m3pc_mtm_train: ``n_steps`` steps on the segments ``replay`` (a ``DeviceReplayBuffer`` on this handle) draws at (seed, step +
        i), eps library-drawn.  masks: one {key: (T,) row} for every step, or a list of n_steps of them.  -> (records (n_steps, 15)
        float32, train_records (n_steps, 3) float64), on the device; ``replay.step`` advances by n_steps."""
        if replay.handle is not self.handle:
            raise capi.M3pcError("train_from: the replay buffer was created on another handle than this trainer's")
        n_steps = int(n_steps)
        per_step = list(masks) if isinstance(masks, (list, tuple)) else [masks] * n_steps
        if len(per_step) != n_steps:
            raise capi.M3pcError(f"train_from: {len(per_step)} mask sets for {n_steps} steps")
        B = int(replay.traj_batch_size if batch is None else batch)
        rows, keep = [], []
        for m in per_step:
            for row in mask_rows(m):
                r = np.ascontiguousarray(np.asarray(row.cpu() if torch.is_tensor(row) else row).astype(np.uint8).reshape(-1))
                if r.size != self.handle.T:
                    raise capi.M3pcError(f"train_from: a mask row has {r.size} entries, not traj_length = {self.handle.T}")
                keep.append(r)
                rows.append(r.ctypes.data)
        mp = (C.c_void_p * len(rows))(*rows)
        f, bits, _ = form_settings(form, KEYS)
        recs = torch.empty((n_steps, capi.MTM_LOSS_FLOATS), dtype=torch.float32, device=self.device)
        trecs = torch.empty((n_steps, 3), dtype=torch.float64, device=self.device)
        from .replay import _MODES
        with torch.cuda.device(self.device):
            capi.check(self.lib.m3pc_mtm_train(self._o, replay._rb, n_steps, B, _MODES[replay._mode], replay.seed, replay.step, mp, f, bits,
                                               capi._ptr(recs), capi._ptr(trecs), self._stream()))
        replay.step += n_steps
        del keep
        self._moved()
        return recs, trecs

    # -- state in and out ---------------------------------------------------------------------------
    def _new(self, names=None):
        return {k: torch.empty(s, dtype=torch.float32, device=self.device) for k, s in self.shapes.items() if names is None or k in names}

    def export_weights(self, into: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """m3pc_mtm_weights_export: the handle's fp32 weights, each in the torch layout of its parameter."""
        into = self._new() if into is None else into
        arr, keep = named_strict(into, self.device)
        with torch.cuda.device(self.device):
            capi.check(self.lib.m3pc_mtm_weights_export(self.handle._h, arr, len(into), self._stream()))
            if any(not t.is_cuda for t in into.values()):
                torch.cuda.current_stream(self.device).synchronize()
        del keep
        return into

    def export_moments(self, which: int, into: Optional[Dict[str, torch.Tensor]] = None, steps: bool = False):
        """m3pc_mtm_opt_export: exp_avg (which = 1) or exp_avg_sq (2); with ``steps`` -> (tensors, {name: step count}) (waits)."""
        into = self._new() if into is None else into
        arr, keep = named_strict(into, self.device)
        st = (C.c_longlong * max(1, len(into)))() if steps else None
        with torch.cuda.device(self.device):
            capi.check(self.lib.m3pc_mtm_opt_export(self._o, int(which), arr, len(into), st, self._stream()))
            if any(not t.is_cuda for t in into.values()):
                torch.cuda.current_stream(self.device).synchronize()
        del keep
        return (into, {k: int(st[j]) for j, k in enumerate(into)}) if steps else into

    def load_moments(self, which: int, tensors: Dict[str, torch.Tensor], steps: Optional[Dict[str, int]] = None):
        """m3pc_mtm_opt_load; steps: {name: count} for the listed tensors, or None to leave the counts."""
        arr, keep = named_strict(tensors, self.device)
        st = None if steps is None else (C.c_longlong * max(1, len(tensors)))(*[int(steps[k]) for k in tensors])
        with torch.cuda.device(self.device):
            capi.check(self.lib.m3pc_mtm_opt_load(self._o, int(which), arr, len(tensors), st, self._stream()))
        del keep

    # -- a torch learner in and out -----------------------------------------------------------------
    @classmethod
    def from_learner(cls, learner, planner=None, max_batch: Optional[int] = None, num_train_steps: Optional[int] = None,
                     warmup_steps: Optional[int] = None, dropout=None, dropout_seed: int = 0):
        """A trainer that continues where ``learner``'s torch optimizers stand: hyper-parameters from ``learner.cfg`` and the
        optimizers' groups, AdamW state by parameter identity (``learner.mtm.state_dict(keep_vars=True)``), ``mtm_scheduler.last_epoch``,
        the temperature optimizer's state and ``log_temperature``.  The planner (default ``learner._hip_planner``, as ``attach`` leaves
        it) must already hold the model's weights.  num_train_steps / warmup_steps: default ``learner.cfg``'s (the schedule is the library's
        closed form, not the scheduler's lambda).  dropout: None / "eval": the eval-mode model; "device": ``learner.mtm.config.dropout``
        on the library's keep-mask stream of ``dropout_seed``; a number: that probability."""
        planner = getattr(learner, "_hip_planner", None) if planner is None else planner
        if planner is None:
            raise capi.M3pcError("from_learner: no planner (attach(learner) first, or pass planner=)")
        cfg, model = learner.cfg, learner.mtm
        opt, topt = learner.mtm_optimizer, learner.temp_optimizer
        g0, tg = opt.param_groups[0], topt.param_groups[0]
        base_lr = float(g0.get("initial_lr", g0["lr"]))
        wd = max(float(g["weight_decay"]) for g in opt.param_groups)
        log_t = model.log_temperature
        if num_train_steps is None:
            num_train_steps = getattr(cfg, "num_train_steps", None)
            if num_train_steps is None:
                raise capi.M3pcError("from_learner: learner.cfg has no num_train_steps; pass num_train_steps=")
        if warmup_steps is None:
            warmup_steps = getattr(cfg, "warmup_steps", 0) or 0
        if dropout == "device":
            mc = getattr(model, "config", None)
            p_drop = float((mc.get("dropout", 0) if isinstance(mc, dict) else getattr(mc, "dropout", 0)) or 0)
        else:
            p_drop = 0.0 if dropout in (None, "eval") else float(dropout)
        self = cls(planner, int(max_batch if max_batch is not None else getattr(cfg, "traj_batch_size", 1)), dropout=p_drop,
                   dropout_seed=dropout_seed, learning_rate=base_lr, weight_decay=wd,
                   num_train_steps=int(num_train_steps), warmup_steps=int(warmup_steps),
                   beta1=g0["betas"][0], beta2=g0["betas"][1], eps=g0["eps"], temp_learning_rate=tg["lr"], temp_beta1=tg["betas"][0],
                   temp_beta2=tg["betas"][1], temp_eps=tg["eps"], target_entropy=float(model.target_entropy),
                   init_log_temperature=float(log_t.detach().double().cpu()))
        sd = model.state_dict(keep_vars=True)
        m, v, steps = {}, {}, {}
        for name in self.shapes:
            st = opt.state.get(sd[name], None)
            if not st:
                continue
            m[name] = st["exp_avg"].detach().to(self.device, torch.float32).reshape(self.shapes[name]).contiguous()
            v[name] = st["exp_avg_sq"].detach().to(self.device, torch.float32).reshape(self.shapes[name]).contiguous()
            steps[name] = int(st["step"])
        if m:
            self.load_moments(EXP_AVG, m, steps)
            self.load_moments(EXP_AVG_SQ, v)
        ts = topt.state.get(log_t, None) or {}
        self.set_state(int(learner.mtm_scheduler.last_epoch), int(ts.get("step", 0)), float(log_t.detach().double().cpu()),
                       float(ts["exp_avg"].double().cpu()) if ts else 0.0, float(ts["exp_avg_sq"].double().cpu()) if ts else 0.0)
        return self

    def to_learner(self, learner):
        """Writes weights, ``mtm_optimizer.state``, the scheduler's count (and the rate it implies) and ``log_temperature`` with its
        optimizer's state back into ``learner``, so that torch can continue or checkpoint.  A tensor that was never stepped gets no state."""
        model, opt, topt, sched = learner.mtm, learner.mtm_optimizer, learner.temp_optimizer, learner.mtm_scheduler
        sd = model.state_dict(keep_vars=True)
        w = self.export_weights()
        m, steps = self.export_moments(EXP_AVG, steps=True)
        v = self.export_moments(EXP_AVG_SQ)
        torch.cuda.current_stream(self.device).synchronize()
        with torch.no_grad():
            for name in self.shapes:
                p = sd[name]
                p.copy_(w[name].reshape(p.shape).to(p.device, p.dtype))
                if steps[name] == 0:
                    opt.state.pop(p, None)
                    continue
                opt.state[p] = {"step": torch.tensor(float(steps[name])), "exp_avg": m[name].reshape(p.shape).to(p.device, p.dtype).clone(),
                                "exp_avg_sq": v[name].reshape(p.shape).to(p.device, p.dtype).clone()}
            st = self.get_state()
            sched.last_epoch = int(st["sched_step"])
            sched._step_count = int(st["sched_step"]) + 1
            lrs = [base * lmbda(sched.last_epoch) for lmbda, base in zip(sched.lr_lambdas, sched.base_lrs)]
            for g, lr in zip(opt.param_groups, lrs):
                g["lr"] = lr
            sched._last_lr = lrs
            log_t = model.log_temperature
            log_t.fill_(st["log_temperature"])
            if st["temp_step"] > 0:
                topt.state[log_t] = {"step": torch.tensor(float(st["temp_step"])),
                                     "exp_avg": torch.full_like(log_t, st["temp_exp_avg"]), "exp_avg_sq": torch.full_like(log_t, st["temp_exp_avg_sq"])}
        return learner
