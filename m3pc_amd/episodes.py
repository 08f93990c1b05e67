"""The episode store (include/m3pc_hip.h: m3pc_episodes_*): the rollout histories of ``n_envs`` environments kept on the device,
and their windows assembled there.

    store = EpisodeStore(planner, n_envs=E)            # or a capi.Handle
    store.reset()                                       # replay_buffer.py:189-203 for every environment
    store.observe(observations)                         # (E, S) numpy / torch, float32 or float64
    s, a, r, h = store.windows(horizon=cfg.horizon)     # (E,T,S) (E,T,A) (E,T,1) on the device, h: numpy (E,) effective horizons
    ...                                                 # any batched entry point of the handle on s, a, r
    store.record(actions, rewards)                      # clip, write, path_length += 1

What the reference keeps per environment as ``current_trajectory`` (finetune_omtm/replay_buffer.py:189-243, learner.py:660-700;
the way-point buffer of zeroshot_omtm/learner.py:515-603) and re-slices on the host at every step.  ``path_length`` is the host
mirror of the device's path lengths: the host makes every call that changes one, so nothing is ever read back.  Every method
enqueues on the current stream of the store's device and returns; tensors come back as device tensors."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import capi

_MODES = {"plan": capi.WINDOW_PLAN, "goal": capi.WINDOW_GOAL}


class EpisodeStore:
    def __init__(self, planner_or_handle, n_envs: int, max_steps: int = 1000):
        handle = getattr(planner_or_handle, "handle", planner_or_handle)
        self.handle, self.lib, self.device = handle, handle.lib, handle.device
        self.T, self.S, self.A = handle.T, handle.S, handle.A
        self.n_envs, self.max_steps = int(n_envs), int(max_steps)
        self._ep = C.c_void_p()
        capi.check(self.lib.m3pc_episodes_create(handle._h, self.n_envs, self.max_steps, C.byref(self._ep)))
        self.path_length = np.zeros((self.n_envs,), dtype=np.int32)

    def close(self):
        if getattr(self, "_ep", None) is not None and self._ep.value:
            self.lib.m3pc_episodes_destroy(self._ep)
            self._ep = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------ arguments
    def _ids(self, env_ids):
        """(ctypes pointer or None, n, index for the mirror)."""
        if env_ids is None:
            return None, self.n_envs, slice(None)
        ids = np.ascontiguousarray(np.asarray(env_ids, dtype=np.int32).reshape(-1))
        return ids.ctypes.data_as(C.POINTER(C.c_int)), int(ids.shape[0]), ids

    def _rows(self, x, shape, f64_ok: bool):
        """A (n, ...) input as (keep-alive, pointer, is_f64, on_device): a tensor of the store's device is read in place, anything
        else goes through NumPy (float64 is kept where the entry point rounds it itself, else rounded here: the same rounding)."""
        if isinstance(x, torch.Tensor) and x.is_cuda:
            if x.device != self.device:
                raise ValueError(f"a device input must live on {self.device}, got {x.device}")
            if x.dtype != torch.float32 and not (f64_ok and x.dtype == torch.float64):
                x = x.to(torch.float32)
            x = x.reshape(shape).contiguous()
            return x, C.c_void_p(x.data_ptr()), int(x.dtype == torch.float64), 1
        a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        if a.dtype != np.float32 and not (f64_ok and a.dtype == np.float64):
            a = a.astype(np.float32)
        a = np.ascontiguousarray(a.reshape(shape))
        return a, C.c_void_p(a.ctypes.data), int(a.dtype == np.float64), 0

    def _stream(self):
        return capi._stream(self.device)

    def _f32(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------------------------------ calls
    def reset(self, env_ids=None, observations=None):
        """Zero the blocks and the path length of the listed environments (None: all).  observations: (n, max_steps, S) (or
        (max_steps, S) for one environment), float32 / float64: the observation block starts out as this table (way-points)."""
        ids, n, idx = self._ids(env_ids)
        keep, ptr, f64, dev = (None, None, 0, 0) if observations is None else self._rows(observations, (n, self.max_steps, self.S), True)
        capi.check(self.lib.m3pc_episodes_reset(self._ep, ids, n, ptr, f64, dev, self._stream()))
        self.path_length[idx] = 0
        del keep

    def observe(self, observations, env_ids=None):
        """obs[e, path_length[e]] = observations[i]; (n, S), float32 or float64."""
        ids, n, _ = self._ids(env_ids)
        keep, ptr, f64, dev = self._rows(observations, (n, self.S), True)
        capi.check(self.lib.m3pc_episodes_observe(self._ep, ids, n, ptr, f64, dev, self._stream()))
        del keep

    def record(self, actions, rewards, env_ids=None, clip_min: float = -1.0, clip_max: float = 1.0):
        """act[e, path_length[e]] = np.clip(actions[i], clip_min, clip_max), rew[e, path_length[e]] = rewards[i], path_length[e] += 1."""
        ids, n, idx = self._ids(env_ids)
        on_dev = isinstance(actions, torch.Tensor) and actions.is_cuda
        if on_dev != (isinstance(rewards, torch.Tensor) and rewards.is_cuda):  # (one flag for both: bring the other side over)
            if on_dev:
                rewards = torch.as_tensor(np.asarray(rewards, dtype=np.float32)).to(self.device)
            else:
                rewards = rewards.cpu()
        ka, pa, _, dev = self._rows(actions, (n, self.A), False)
        kr, pr, _, _ = self._rows(rewards, (n,), False)
        capi.check(self.lib.m3pc_episodes_record(self._ep, ids, n, pa, pr, float(clip_min), float(clip_max), dev, self._stream()))
        self.path_length[idx] += 1
        del ka, kr

    def windows(self, env_ids=None, horizon: int = 4, mode: str = "plan"):
        """(states (n,T,S), actions (n,T,A), rewards (n,T,1)) on the device and the effective horizons, numpy int32 (n,).
        mode "plan": action_sample's window; "goal": action_piid_sample's."""
        ids, n, _ = self._ids(env_ids)
        s, a, r = self._f32(n, self.T, self.S), self._f32(n, self.T, self.A), self._f32(n, self.T, 1)
        h = np.empty((max(n, 1),), dtype=np.int32)
        capi.check(self.lib.m3pc_episodes_windows(self._ep, ids, n, _MODES[mode], int(horizon), capi._ptr(s), capi._ptr(a), capi._ptr(r),
                                                  h.ctypes.data_as(C.POINTER(C.c_int)), self._stream()))
        return s, a, r, h[:n]

    def values(self, discount: float, use_avg: bool = False, env_ids=None) -> torch.Tensor:
        """(n, max_steps): replay_buffer.py:234-243 on the stored rewards."""
        ids, n, _ = self._ids(env_ids)
        v = self._f32(n, self.max_steps)
        capi.check(self.lib.m3pc_episodes_values(self._ep, ids, n, float(discount), int(bool(use_avg)), capi._ptr(v), self._stream()))
        return v

    def export(self, env: int):
        """One environment's blocks as device tensors: {"observations" (max_steps,S), "actions" (max_steps,A), "rewards" (max_steps,1),
        "path_length"}."""
        o, a, r = self._f32(self.max_steps, self.S), self._f32(self.max_steps, self.A), self._f32(self.max_steps, 1)
        pl = C.c_int(0)
        capi.check(self.lib.m3pc_episodes_export(self._ep, int(env), capi._ptr(o), capi._ptr(a), capi._ptr(r), C.byref(pl), 1, self._stream()))
        return {"observations": o, "actions": a, "rewards": r, "path_length": int(pl.value)}

    def trajectory(self, env: int, values: Optional[torch.Tensor] = None):
        """``export`` as the host dict of ``rollout.new_trajectory`` (numpy arrays; one read-back).  values: that environment's
        (max_steps,) row of ``values()``, else zeros."""
        t = self.export(env)
        rew = t["rewards"].cpu().numpy()
        val = np.zeros((self.max_steps, 1), dtype=np.float32) if values is None else values.reshape(self.max_steps, 1).cpu().numpy()
        return {"observations": t["observations"].cpu().numpy(), "actions": t["actions"].cpu().numpy(), "rewards": rew, "values": val,
                "total_return": rew.sum(), "path_length": t["path_length"]}
