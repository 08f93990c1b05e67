"""The IQL trainer on the device (include/m3pc_hip.h: m3pc_iql_*): ``ImplicitQLearning`` of finetune_omtm/model.py over the library's
kernels -- replay batches in, the TwinQ the planner scores with out, without a trip through the host.

    iql = DeviceIQL.from_iql(planner, learner.iql)            # a live ImplicitQLearning, its optimizers included
    for _ in range(cfg.warmup_steps):                          # finetune.py:281-290
        iql.train(buf.trans_sample())                          # {"value_loss", "q_loss", "actor_loss"}: device scalars
    iql.train_from(buf, cfg.v_iter_per_mtm)                    # n steps in one call, batches drawn by the library
    iql.publish(planner)                                       # what planner.set_critic(iql.qf.state_dict()) did, device to device
    torch.save(iql.state_dict(), "iql_%d.pt" % step)           # the reference's layout (model.py:310-320)

Every method enqueues on the current stream of the trainer's device and returns; the step count is a host mirror and the losses stay
on the device (``train(batch, item=True)`` reads them, which waits, as the reference's ``.item()`` per loss does)."""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, Dict, Optional

import numpy as np
import torch

from . import capi

FIELDS = ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias")
QF_NAMES = tuple("%s.%s" % (q, f) for q in ("q1", "q2") for f in FIELDS)
VF_NAMES = tuple("v.%s" % f for f in FIELDS)
ACTOR_NAMES = ("log_std",) + tuple("net.%s" % f for f in FIELDS)  # (the order of GaussianPolicy.parameters(): its own parameter first)
_PARTS = {"qf": (capi.IQL_QF, capi.IQL_QF_ADAM_M, capi.IQL_QF_ADAM_V, QF_NAMES), "vf": (capi.IQL_VF, capi.IQL_VF_ADAM_M, capi.IQL_VF_ADAM_V, VF_NAMES),
          "actor": (capi.IQL_ACTOR, capi.IQL_ACTOR_ADAM_M, capi.IQL_ACTOR_ADAM_V, ACTOR_NAMES)}
_OPT = {"qf": "q_optimizer", "vf": "v_optimizer", "actor": "actor_optimizer"}
_LR = {"qf": "critic_lr", "vf": "v_lr", "actor": "actor_lr"}
LOSSES = ("value_loss", "q_loss", "actor_loss")


class DeviceIQL:
    def __init__(self, planner_or_handle, hidden: int = 256, v_lr: float = 3e-4, critic_lr: float = 3e-4, actor_lr: float = 3e-4,
                 expectile: float = 0.7, beta: float = 3.0, discount: float = 0.99, tau: float = 0.005, max_steps: int = 1000000,
                 max_action: float = 1.0):
        handle = getattr(planner_or_handle, "handle", planner_or_handle)
        self.handle, self.lib, self.device = handle, handle.lib, handle.device
        self.S, self.A, self.hidden = handle.S, handle.A, int(hidden)
        self.v_lr, self.critic_lr, self.actor_lr = float(v_lr), float(critic_lr), float(actor_lr)
        self.expectile, self.beta, self.discount, self.tau = float(expectile), float(beta), float(discount), float(tau)
        self.max_steps, self.max_action = int(max_steps), float(max_action)
        self.obs_mean: Optional[torch.Tensor] = None
        self.obs_std: Optional[torch.Tensor] = None
        self._q = C.c_void_p()
        capi.check(self.lib.m3pc_iql_create(handle._h, self.hidden, C.byref(self._q)))

    def close(self):
        if getattr(self, "_q", None) is not None and self._q.value:
            self.lib.m3pc_iql_destroy(self._q)
            self._q = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------ state
    def _stream(self):
        return capi._stream(self.device)

    def shapes(self, part: str) -> Dict[str, tuple]:
        """name -> shape of the tensors of "qf" / "vf" / "actor" (model.py:146-191, :107-133)."""
        S, A, H = self.S, self.A, self.hidden
        i, o = (S + A, 1) if part == "qf" else ((S, 1) if part == "vf" else (S, A))
        mlp = [(H, i), (H,), (H, H), (H,), (o, H), (o,)]
        if part == "qf":
            return dict(zip(QF_NAMES, mlp + mlp))
        return dict(zip(VF_NAMES, mlp)) if part == "vf" else dict(zip(ACTOR_NAMES, [(A,)] + mlp))

    def load_part(self, code: int, tensors: Dict[str, Any], obs_mean=None, obs_std=None):
        """m3pc_iql_load of one M3PC_IQL_* part: {name: tensor or array} by state_dict names, host or device."""
        sd = {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float32)))) for k, v in tensors.items()}
        arr, keep = capi._named(sd)
        fp = C.POINTER(C.c_float)
        m = s = None
        if obs_mean is not None:
            m = torch.as_tensor(obs_mean, dtype=torch.float32).detach().cpu().reshape(-1).contiguous()
            s = torch.as_tensor(obs_std, dtype=torch.float32).detach().cpu().reshape(-1).contiguous()
            if m.numel() != self.S or s.numel() != self.S:
                raise ValueError(f"obs_mean / obs_std must hold {self.S} values")
            self.obs_mean, self.obs_std = m.clone(), s.clone()
        capi.check(self.lib.m3pc_iql_load(self._q, code, arr, len(sd), None if m is None else C.cast(m.data_ptr(), fp),
                                          None if s is None else C.cast(s.data_ptr(), fp), self._stream()))
        del keep

    def export_part(self, code: int, part: str) -> Dict[str, torch.Tensor]:
        """m3pc_iql_export of one M3PC_IQL_* part of "qf" / "vf" / "actor": {name: device tensor}, in the order of .parameters()."""
        out = {k: torch.empty(shape, dtype=torch.float32, device=self.device) for k, shape in self.shapes(part).items()}
        arr, keep = capi._named(out)
        capi.check(self.lib.m3pc_iql_export(self._q, code, arr, len(out), self._stream()))
        del keep
        return out

    @property
    def total_it(self) -> int:
        v = C.c_longlong()
        capi.check(self.lib.m3pc_iql_get_step(self._q, C.byref(v)))
        return int(v.value)

    @total_it.setter
    def total_it(self, value: int):
        capi.check(self.lib.m3pc_iql_set_step(self._q, int(value)))

    def actor_lr_at(self, k: int) -> float:
        """The actor's rate at 0-based step k: CosineAnnealingLR(max_steps) in closed form (model.py:219)."""
        return self.actor_lr * 0.5 * (1.0 + math.cos(math.pi * k / self.max_steps))

    def _optimizer_state(self, part: str, lr: float, extra: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
        _, cm, cv, names = _PARTS[part]
        m, v = self.export_part(cm, part), self.export_part(cv, part)
        t = self.total_it
        state = {j: {"step": torch.tensor(float(t)), "exp_avg": m[n], "exp_avg_sq": v[n]} for j, n in enumerate(names)} if t > 0 else {}
        group = dict(lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False, foreach=None, capturable=False,
                     differentiable=False, fused=None, params=list(range(len(names))))
        group.update(extra or {})
        return {"state": state, "param_groups": [group]}

    def state_dict(self) -> Dict[str, Any]:
        """ImplicitQLearning.state_dict (model.py:310-320): what ``torch.save`` makes an ``iql_{step}.pt`` of."""
        t = self.total_it
        lr = self.actor_lr_at(t)
        return {
            "qf": self.export_part(capi.IQL_QF, "qf"),
            "q_optimizer": self._optimizer_state("qf", self.critic_lr),
            "vf": self.export_part(capi.IQL_VF, "vf"),
            "v_optimizer": self._optimizer_state("vf", self.v_lr),
            "actor": self.export_part(capi.IQL_ACTOR, "actor"),
            "actor_optimizer": self._optimizer_state("actor", lr, {"initial_lr": self.actor_lr}),
            "actor_lr_schedule": {"T_max": self.max_steps, "eta_min": 0, "base_lrs": [self.actor_lr], "last_epoch": t, "_step_count": t + 1,
                                  "_get_lr_called_within_step": False, "_last_lr": [lr]},
            "total_it": t,
        }

    def load_state_dict(self, sd: Dict[str, Any], obs_mean=None, obs_std=None):
        """ImplicitQLearning.load_state_dict (model.py:322-334), q_target = a copy of qf (:325) included.  obs_mean / obs_std are
        attributes of the reference's networks, not part of its state_dict: pass them with the first load."""
        for part in _PARTS:
            group = sd[_OPT[part]]["param_groups"][0]
            # the device's Adam is torch.optim.Adam at its defaults (iql.h): anything else in a checkpoint would be trained differently
            if (tuple(group.get("betas", (0.9, 0.999))) != (0.9, 0.999) or group.get("eps", 1e-8) != 1e-8 or group.get("weight_decay", 0) != 0
                    or group.get("amsgrad", False) or group.get("maximize", False)):
                raise ValueError(f"{_OPT[part]}: betas / eps / weight_decay / amsgrad / maximize differ from torch.optim.Adam's defaults, "
                                 "which are the only Adam the device trainer runs")
        self.load_part(capi.IQL_QF, sd["qf"], obs_mean, obs_std)
        self.load_part(capi.IQL_Q_TARGET, sd["qf"])
        self.load_part(capi.IQL_VF, sd["vf"])
        self.load_part(capi.IQL_ACTOR, sd["actor"])
        for part, (_, cm, cv, names) in _PARTS.items():
            opt = sd[_OPT[part]]
            st = opt["state"]
            zero = {n: torch.zeros(shape) for n, shape in self.shapes(part).items()}
            self.load_part(cm, {n: (st[j]["exp_avg"] if j in st else zero[n]) for j, n in enumerate(names)})
            self.load_part(cv, {n: (st[j]["exp_avg_sq"] if j in st else zero[n]) for j, n in enumerate(names)})
            group = opt["param_groups"][0]
            setattr(self, _LR[part], float(group.get("initial_lr", group["lr"])))
        sched = sd.get("actor_lr_schedule") or {}
        if "T_max" in sched:
            self.max_steps = int(sched["T_max"])
        self.total_it = int(sd["total_it"])

    @classmethod
    def from_iql(cls, planner_or_handle, iql, hidden: Optional[int] = None) -> "DeviceIQL":
        """A live ``ImplicitQLearning`` (its networks, q_target, the three optimizers, total_it) onto the device."""
        sd = iql.state_dict()
        hidden = int(sd["qf"]["q1.net.0.bias"].numel()) if hidden is None else hidden
        self = cls(planner_or_handle, hidden, expectile=iql.iql_tau, beta=iql.beta, discount=iql.discount, tau=iql.tau,
                   max_steps=iql.actor_lr_schedule.T_max, max_action=getattr(iql, "max_action", 1.0))
        self.load_state_dict(sd, iql.qf.obs_mean, iql.qf.obs_std)
        self.load_part(capi.IQL_Q_TARGET, iql.q_target.state_dict())  # (a live target has moved away from qf)
        return self

    # ------------------------------------------------------------------------------------------ training
    def _args(self, **over) -> capi.IqlArgs:
        a = dict(v_lr=self.v_lr, q_lr=self.critic_lr, actor_lr=self.actor_lr, expectile=self.expectile, beta=self.beta, discount=self.discount,
                 tau=self.tau, actor_t_max=self.max_steps, flags=0)
        a.update(over)
        return capi.IqlArgs(**a)

    def _f32(self, x, shape) -> torch.Tensor:
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
        return t.to(device=self.device, dtype=torch.float32).reshape(shape).contiguous()

    def train(self, batch, item: bool = False, **over) -> Dict[str, Any]:
        """ImplicitQLearning.train (model.py:286-308) on (observations, actions, rewards, next_observations, dones), the tuple
        ``trans_sample`` returns.  -> the three losses as device scalars (``item=True``: Python floats, which waits for the device).
        Keyword arguments override the hyper-parameters of this step (v_lr, q_lr, actor_lr, tau, ...)."""
        s, a, r, s2, d = batch
        B = int(s.shape[0])
        ts = [self._f32(s, (B, self.S)), self._f32(a, (B, self.A)), self._f32(r, (B, 1)), self._f32(s2, (B, self.S)), self._f32(d, (B, 1))]
        losses = torch.empty(3, dtype=torch.float32, device=self.device)
        args = self._args(**over)
        capi.check(self.lib.m3pc_iql_train_step(self._q, C.byref(args), B, *[capi._ptr(t) for t in ts], capi._ptr(losses), self._stream()))
        return {k: (float(losses[j]) if item else losses[j]) for j, k in enumerate(LOSSES)}

    def train_from(self, buffer, n_steps: int, batch_size: Optional[int] = None) -> torch.Tensor:
        """n_steps steps on the batches ``buffer`` (a DeviceReplayBuffer) draws for (seed, step), ..., (seed, step + n_steps - 1), in
        one call; the buffer's step advances as n_steps ``trans_sample()`` calls would.  -> losses (n_steps, 3), a device tensor."""
        n_on, n_off = buffer.split(batch_size)
        losses = torch.empty(int(n_steps), 3, dtype=torch.float32, device=self.device)
        args = self._args()
        capi.check(self.lib.m3pc_iql_train(self._q, C.byref(args), buffer._rb, int(n_steps), n_on + n_off, n_on, buffer.seed, buffer.step,
                                           capi._ptr(losses), self._stream()))
        buffer.step += int(n_steps)
        return losses

    def publish(self, planner_or_handle=None):
        """The TwinQ into the planner's critic, device to device: what ``set_critic(qf.state_dict(), obs_mean, obs_std)`` did."""
        handle = getattr(planner_or_handle, "handle", planner_or_handle) if planner_or_handle is not None else self.handle
        capi.check(self.lib.m3pc_iql_publish_critic(self._q, handle._h, self._stream()))

    def evaluate(self, which: int, states, actions=None) -> torch.Tensor:
        """m3pc_iql_evaluate: capi.IQL_Q_MIN / IQL_Q_TARGET_MIN (rows,), IQL_V (rows,), IQL_ACTOR_MEAN (rows, A)."""
        n = int(states.shape[0])
        s = self._f32(states, (n, self.S))
        a = None if actions is None else self._f32(actions, (n, self.A))
        out = torch.empty((n, self.A) if which == capi.IQL_ACTOR_MEAN else (n,), dtype=torch.float32, device=self.device)
        capi.check(self.lib.m3pc_iql_evaluate(self._q, which, capi._ptr(s), capi._ptr(a), n, capi._ptr(out), self._stream()))
        return out

    def act(self, state) -> np.ndarray:
        """GaussianPolicy.act in evaluation (model.py:135-143): the mean action of one state, scaled and clipped to max_action."""
        mean = self.evaluate(capi.IQL_ACTOR_MEAN, torch.as_tensor(np.asarray(state), dtype=torch.float32).reshape(1, -1))
        return torch.clamp(self.max_action * mean, -self.max_action, self.max_action).cpu().numpy().flatten()
