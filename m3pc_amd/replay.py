"""The replay buffer on the device (include/m3pc_hip.h: m3pc_replay_*): ``ReplayBuffer`` of finetune_omtm/replay_buffer.py over the
library's trajectory ring and its two transition rings -- episodes in, training batches out, without a trip through the host.

    buf = DeviceReplayBuffer.from_arrays(planner, cfg, observations, actions, rewards, dones, terminals, next_observations,
                                         discount=cfg.discount)                      # replay_buffer.py:42-165, once, on the host
    out = rollout.evaluate_plan(planner, envs, buf.values_up_bound, eval=False, lockstep="native", store=store)
    buf.update_from_store(store, range(E), final_observations)                       # :223-251, device to device
    for batch in buf:                                                                # cfg.mtm_iter_per_rollout x traj_sample()
        ...                                                                          # {"states", "actions", "rewards", "returns"}
        s, a, r, s2, d = buf.trans_sample()                                          # :368-420

Batches are device tensors with the reference's keys and dtypes (``returns`` is float64, as values_segmented is).  Indices are the
caller's (``indices=``: the reference's exact batches) or drawn by the library from ``(seed, step)`` with its counter-based
generator; ``step`` advances by one per drawn batch.  Every method enqueues on the current stream of the buffer's device and returns;
counts and path lengths are host mirrors, nothing is read back (``values_up_bound`` reads max_steps doubles once per update)."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import capi

_MODES = {"uniform": capi.REPLAY_UNIFORM, "prob": capi.REPLAY_LENGTH}


def segment(x: np.ndarray, dones: np.ndarray, max_path_length: int):
    """omtm/datasets/sequence_dataset.py:102-134: split at every done, pad to max_path_length.  -> (padded (N, M, D), early
    termination flags (N, M) bool, path lengths)."""
    assert len(x) == len(dones)
    cuts = [i + 1 for i, t in enumerate(np.asarray(dones).reshape(len(dones), -1)[:, 0]) if t]
    bounds = [0] + cuts + ([len(x)] if (not cuts or cuts[-1] != len(x)) else [])
    lengths = [b - a for a, b in zip(bounds[:-1], bounds[1:])]
    pad = np.zeros((len(lengths), max_path_length, x.shape[1]), dtype=x.dtype)
    early = np.zeros((len(lengths), max_path_length), dtype=bool)
    for i, (a, n) in enumerate(zip(bounds[:-1], lengths)):
        pad[i, :n] = x[a:a + n]
        early[i, n:] = 1
    return pad, early, lengths


def host_buffer(cfg, observations, actions, rewards, dones, terminals, next_observations, discount: float = 0.99,
                max_path_length: int = 1000, shuffle: bool = True) -> SimpleNamespace:
    """``ReplayBuffer.__init__`` (replay_buffer.py:42-165) in NumPy, with the same ``np.random.shuffle`` calls in the same order: under
    the same ``np.random.seed`` this is the reference's buffer, bit for bit.  Returns the arrays it is left with: observations /
    actions / rewards (float32) and values (FLOAT64) (N, M, .), path_lengths, p, values_up_bound, trajectory_returns, the offline
    transitions ``trans`` (state, action, reward, next_state, done), discount and use_avg."""
    observations, actions = np.asarray(observations), np.asarray(actions)
    rewards_raw = np.asarray(rewards).reshape(-1, 1)
    terminals, next_observations = np.asarray(terminals), np.asarray(next_observations)
    M = int(max_path_length)
    act_seg, termination_flags, path_lengths = segment(actions, dones, M)
    obs_seg, *_ = segment(observations, dones, M)
    rew_seg, *_ = segment(rewards_raw, dones, M)
    use_avg = discount > 1.0
    discount = 1.0 if use_avg else discount
    discounts = (discount ** np.arange(M))[:, None]                                   # :70
    val_seg = np.zeros(rew_seg.shape)                                                 # :73: float64
    for t in range(M):
        val_seg[:, t] = (rew_seg[:, t + 1:] * discounts[: -t - 1]).sum(axis=1)        # :75-80: fp64 sums of fp32 rewards
    if use_avg:
        val_seg = val_seg / np.arange(1, M + 1)[::-1][None, :, None]                  # :83-85
    # the offline transitions: the best-rewarded buffer_init_size, shuffled (:108-125)
    init = int(cfg.buffer_init_ratio * cfg.trans_buffer_size)
    sorted_idx = np.argsort(rewards_raw[:, 0], axis=0)[::-1][:init]
    np.random.shuffle(sorted_idx)
    trans = (observations[sorted_idx], actions[sorted_idx], rewards_raw[sorted_idx], next_observations[sorted_idx],
             terminals[sorted_idx] * 0)
    trans = tuple(t[-cfg.trans_buffer_size:] for t in trans)                          # (deque(maxlen): the last ones stay)
    # the trajectories: by return, those of at least traj_length steps, up to traj_buffer_size (:129-163)
    returns = rew_seg.sum(axis=(1, 2), keepdims=False)
    order = np.argsort(returns, axis=0)[::-1]
    path_lengths = np.array(path_lengths)[order]
    keep: List[int] = []
    for idx, pl in enumerate(path_lengths):
        if len(keep) == cfg.traj_buffer_size:
            break
        if pl >= cfg.traj_length:
            keep.append(idx)
    if shuffle:
        shuffle_indices = np.arange(len(keep))
        np.random.shuffle(shuffle_indices)
        keep = [keep[i] for i in shuffle_indices]
    sel = order[keep]
    path_lengths = path_lengths[keep]
    values = val_seg[sel]
    return SimpleNamespace(observations=obs_seg[sel], actions=act_seg[sel], rewards=rew_seg[sel], values=values, path_lengths=path_lengths,
                           p=path_lengths / path_lengths.sum(axis=0), values_up_bound=values.max(axis=0),
                           trajectory_returns=returns[order][keep], trans=trans, discount=discount, use_avg=use_avg)


class _LastObservation:
    """An environment that remembers the observation it returned last (the next state of an episode's last transition)."""

    def __init__(self, env):
        self.env, self.last = env, None

    def reset(self):
        self.last = self.env.reset()
        return self.last

    def step(self, action):
        out = self.env.step(action)
        self.last = out[0]
        return out


class DeviceReplayBuffer:
    def __init__(self, planner_or_handle, cfg, traj_capacity: Optional[int] = None, max_path_length: int = 1000, discount: float = 0.99,
                 seed: int = 0, offline_capacity: Optional[int] = None, online_capacity: Optional[int] = None):
        handle = getattr(planner_or_handle, "handle", planner_or_handle)
        self.handle, self.lib, self.device = handle, handle.lib, handle.device
        self.S, self.A = handle.S, handle.A
        self.cfg = cfg
        self.max_path_length, self.sequence_length = int(max_path_length), int(cfg.traj_length)
        self.traj_batch_size, self.trans_batch_size = int(cfg.traj_batch_size), int(cfg.trans_batch_size)
        self.traj_capacity = int(cfg.traj_buffer_size if traj_capacity is None else traj_capacity)
        self.trans_buffer_size = int(cfg.trans_buffer_size)
        self.offline_capacity = self.trans_buffer_size if offline_capacity is None else int(offline_capacity)
        self.online_capacity = self.trans_buffer_size if online_capacity is None else int(online_capacity)
        self.mtm_iter = int(getattr(cfg, "mtm_iter_per_rollout", 1))
        self._mode = cfg.select_mode
        if self._mode not in _MODES:
            raise ValueError(f"Invalid sampling mode: {self._mode}")
        self.use_avg = discount > 1.0                                                  # replay_buffer.py:63-68
        self.discount = 1.0 if self.use_avg else float(discount)
        self.seed, self.step, self.total_step = int(seed), 0, 0
        self._ub: Optional[np.ndarray] = None
        self._rb = C.c_void_p()
        capi.check(self.lib.m3pc_replay_create(handle._h, self.traj_capacity, self.max_path_length, self.sequence_length,
                                               self.offline_capacity, self.online_capacity, C.byref(self._rb)))

    @classmethod
    def from_arrays(cls, planner_or_handle, cfg, observations, actions, rewards, dones, terminals, next_observations, discount: float = 0.99,
                    max_path_length: int = 1000, shuffle: bool = True, seed: int = 0) -> "DeviceReplayBuffer":
        """The reference's constructor (``host_buffer``), then one upload.  The trajectory capacity is the kept count, so that an
        update replaces the oldest, as in the reference."""
        hb = host_buffer(cfg, observations, actions, rewards, dones, terminals, next_observations, discount, max_path_length, shuffle)
        self = cls(planner_or_handle, cfg, len(hb.path_lengths), max_path_length, discount, seed)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(self.device)  # (one plain upload each: nothing is staged)
        self.append(up(hb.observations), up(hb.actions), up(hb.rewards), up(hb.values), hb.path_lengths)
        if len(hb.trans[0]):
            self.append_transitions(*[up(x) for x in hb.trans], online=False)
        return self

    def close(self):
        if getattr(self, "_rb", None) is not None and self._rb.value:
            self.lib.m3pc_replay_destroy(self._rb)
            self._rb = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------ arguments
    def _stream(self):
        return capi._stream(self.device)

    def _dev(self, x, shape, dtype=torch.float32) -> torch.Tensor:
        """An input as a contiguous tensor of the buffer's device."""
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
        return t.to(device=self.device, dtype=dtype).reshape(shape).contiguous()

    def _arrays(self, xs, shapes, dtypes):
        """The arrays of one call as (keep-alive, pointers, on_device): read in place on the device when any of them lives there,
        else handed over as host arrays (the library stages them before it returns)."""
        if any(isinstance(x, torch.Tensor) and x.is_cuda for x in xs):
            keep = [self._dev(x, sh, torch.float64 if dt is np.float64 else torch.float32) for x, sh, dt in zip(xs, shapes, dtypes)]
            return keep, [capi._ptr(t) for t in keep], 1
        keep = [np.ascontiguousarray(np.asarray(x.numpy() if isinstance(x, torch.Tensor) else x, dtype=dt).reshape(sh))
                for x, sh, dt in zip(xs, shapes, dtypes)]
        return keep, [C.c_void_p(a.ctypes.data) for a in keep], 0

    def _new(self, *shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _index(self, x, n):
        """Caller indices as (keep-alive, pointer, on_device): a device tensor is read in place (and clamped by the kernel), a host
        array is checked by the library."""
        if isinstance(x, torch.Tensor) and x.is_cuda:
            x = x.to(device=self.device, dtype=torch.int32).reshape(n).contiguous()
            return x, C.c_void_p(x.data_ptr()), 1
        a = np.ascontiguousarray(np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x).reshape(n).astype(np.int32))
        return a, C.c_void_p(a.ctypes.data), 0

    # ------------------------------------------------------------------------------------------ filling
    def append(self, observations, actions, rewards, values, path_lengths):
        """n trajectories at the tail, the oldest leaving a full ring: (n, M, S), (n, M, A), (n, M[, 1]) float32, values float64."""
        lens = np.ascontiguousarray(np.asarray(path_lengths, dtype=np.int32).reshape(-1))
        n, M = int(lens.shape[0]), self.max_path_length
        keep, ptrs, dev = self._arrays((observations, actions, rewards, values), ((n, M, self.S), (n, M, self.A), (n, M), (n, M)),
                                       (np.float32, np.float32, np.float32, np.float64))
        capi.check(self.lib.m3pc_replay_append(self._rb, n, *ptrs, lens.ctypes.data_as(C.POINTER(C.c_int)), dev, self._stream()))
        del keep
        self._ub = None

    def append_transitions(self, state, action, reward, next_state, done, online: bool = True):
        n = int(np.shape(state)[0])
        keep, ptrs, dev = self._arrays((state, action, reward, next_state, done), ((n, self.S), (n, self.A), (n,), (n, self.S), (n,)),
                                       (np.float32,) * 5)
        capi.check(self.lib.m3pc_replay_append_transitions(self._rb, capi.REPLAY_ONLINE if online else capi.REPLAY_OFFLINE, n, *ptrs, dev,
                                                           self._stream()))
        del keep

    def update_buffer(self, new_trajectories: Sequence[Dict[str, Any]]):
        """replay_buffer.py:272-310 on host dicts (``rollout.new_trajectory``'s keys; "values" of either float width)."""
        tr = list(new_trajectories)
        self.append(np.stack([t["observations"] for t in tr]), np.stack([t["actions"] for t in tr]), np.stack([t["rewards"] for t in tr]),
                    np.stack([np.asarray(t["values"], dtype=np.float64) for t in tr]), [t["path_length"] for t in tr])
        self.total_step += int(sum(t["path_length"] for t in tr))

    def update_from_store(self, store, env_ids=None, final_observations=None) -> int:
        """The listed episodes of an ``EpisodeStore`` (None: all), device to device: trajectories of at least traj_length steps into
        the ring with their values, every episode's transitions into the online ring.  final_observations (n, S): the next state of
        each episode's last transition (without it that transition is left out).  Returns how many trajectories were taken."""
        ids, n, idx = store._ids(env_ids)
        keep, ptr, dev = None, None, 0
        if final_observations is not None:
            if isinstance(final_observations, torch.Tensor) and final_observations.is_cuda:
                keep, dev = self._dev(final_observations, (n, self.S)), 1
                ptr = capi._ptr(keep)
            else:
                keep = np.ascontiguousarray(np.asarray(final_observations, dtype=np.float32).reshape(n, self.S))
                ptr = C.c_void_p(keep.ctypes.data)
        taken = C.c_int(0)
        capi.check(self.lib.m3pc_replay_push_episodes(self._rb, store._ep, ids, n, self.discount, int(self.use_avg), ptr, dev,
                                                      C.byref(taken), self._stream()))
        self.total_step += int(np.sum(store.path_length[idx]))
        self._ub = None
        del keep
        return int(taken.value)

    def online_rollout(self, planner, envs, store=None, lockstep="native", max_steps: Optional[int] = None, **kw) -> Dict[str, Any]:
        """``ReplayBuffer.online_rollout`` (replay_buffer.py:167-270) for len(envs) environments at once: one exploring episode each
        through ``rollout.evaluate_plan(..., eval=False, store=...)``, then ``update_from_store``.  Returns evaluate_plan's dict with
        "taken" added."""
        from . import rollout
        from .episodes import EpisodeStore
        M = self.max_path_length if max_steps is None else int(max_steps)
        own = store is None
        st = EpisodeStore(planner, len(envs), M) if own else store
        wrapped = [_LastObservation(e) for e in envs]
        out = rollout.evaluate_plan(planner, wrapped, self.values_up_bound, max_steps=M, eval=False, lockstep=lockstep, store=st,
                                    discount=self.discount, use_avg=self.use_avg, **kw)
        out["taken"] = self.update_from_store(st, list(range(len(envs))), np.stack([np.asarray(w.last, dtype=np.float32) for w in wrapped]))
        if own:
            torch.cuda.current_stream(self.device).synchronize()  # (the push reads the store that is closed here)
            st.close()
        return out

    # ------------------------------------------------------------------------------------------ the mirrors
    def counts(self):
        c = [C.c_int(0) for _ in range(3)]
        capi.check(self.lib.m3pc_replay_counts(self._rb, *[C.byref(x) for x in c]))
        return tuple(int(x.value) for x in c)

    def __len__(self):
        return self.counts()[0]

    @property
    def path_lengths(self) -> np.ndarray:
        out = np.zeros((max(self.traj_capacity, 1),), dtype=np.int32)
        capi.check(self.lib.m3pc_replay_path_lengths(self._rb, out.ctypes.data_as(C.POINTER(C.c_int)), int(out.shape[0])))
        return out[: len(self)].astype(np.int64)

    @property
    def p(self) -> np.ndarray:
        pl = self.path_lengths
        return pl / pl.sum(axis=0)

    def values_up_bound_device(self) -> torch.Tensor:
        out = self._new(self.max_path_length, 1, dtype=torch.float64)
        capi.check(self.lib.m3pc_replay_values_up_bound(self._rb, capi._ptr(out), self._stream()))
        return out

    @property
    def values_up_bound(self) -> np.ndarray:
        """(max_path_length, 1) float64: what evaluate_plan takes as episode_rtg_ref (finetune.py:373-377)."""
        if self._ub is None:
            self._ub = self.values_up_bound_device().cpu().numpy()
        return self._ub

    # ------------------------------------------------------------------------------------------ sampling
    def _segment_indices(self, indices, batch_size):
        """(indices, batch_size) of the segment calls -> (B, traj_index pointer, start_index pointer, index_on_device, keep-alives);
        indices None: the pointers are None and the library draws."""
        if indices is None:
            return int(self.traj_batch_size if batch_size is None else batch_size), None, None, 0, None
        B = int(np.prod(np.shape(indices[0])))
        ti, pt, dev = self._index(indices[0], B)
        si, ps, dev2 = self._index(indices[1], B)
        if dev != dev2:
            raise ValueError("trajectory indices and starts must both be on the host or both on the device")
        return B, pt, ps, dev, (ti, si)

    def traj_sample(self, indices=None, batch_size: Optional[int] = None, returns_f32: bool = False, return_indices: bool = False):
        """replay_buffer.py:312-366.  indices: (trajectory indices, starts), each (B,), host or device; None: drawn by the library."""
        B, pt, ps, dev, keep_i = self._segment_indices(indices, batch_size)
        L = self.sequence_length
        s, a, r = self._new(B, L, self.S), self._new(B, L, self.A), self._new(B, L, 1)
        v = self._new(B, L, 1, dtype=torch.float32 if returns_f32 else torch.float64)
        oi = (self._new(B, dtype=torch.int32), self._new(B, dtype=torch.int32)) if return_indices else (None, None)
        capi.check(self.lib.m3pc_replay_sample_segments(self._rb, B, _MODES[self._mode], pt, ps, dev, self.seed, self.step, capi._ptr(s),
                                                        capi._ptr(a), capi._ptr(r), capi._ptr(v), int(returns_f32), capi._ptr(oi[0]),
                                                        capi._ptr(oi[1]), self._stream()))
        if indices is None:
            self.step += 1
        del keep_i
        batch = {"states": s, "actions": a, "rewards": r, "returns": v}
        return (batch, oi) if return_indices else batch

    def mtm_loss(self, masks, entropy_reg: float, form: str = "finetune", indices=None, batch_size: Optional[int] = None, eps=None,
                 precision: int = capi.PREC_FP32, return_indices: bool = False):
        """The masked-trajectory loss (m3pc_mtm_loss_replay) of the batch ``traj_sample`` would return for the same arguments, without
        the batch leaving the library: gather, tokenise, forward under ``masks``, loss.  eps: (B,L,A) standard normals, or None: drawn
        by the library at the same (seed, step).  Returns the reference's 5-tuple of ``form`` (m3pc_amd/mtm.py) as 0-d device tensors;
        ``step`` advances as in ``traj_sample``."""
        from .masks import mask_rows
        from .mtm import form_settings, loss_tuple
        B, pt, ps, dev, keep_i = self._segment_indices(indices, batch_size)
        flags, bits, keys = form_settings(form, capi.KEYS)
        e = None if eps is None else self._dev(eps, (B, self.sequence_length, self.A))
        rec = self._new(capi.MTM_LOSS_FLOATS)
        oi = (self._new(B, dtype=torch.int32), self._new(B, dtype=torch.int32)) if return_indices else (None, None)
        mp, keep = self.handle._mask_ptrs(mask_rows(masks))
        capi.check(self.lib.m3pc_mtm_loss_replay(self.handle._h, self._rb, B, _MODES[self._mode], pt, ps, dev, self.seed, self.step, mp,
                                                 capi._ptr(e), float(entropy_reg), flags, bits, int(precision), capi._ptr(rec),
                                                 capi._ptr(oi[0]), capi._ptr(oi[1]), self._stream()))
        if indices is None:
            self.step += 1
        del keep_i, keep
        out = loss_tuple(rec, keys)
        return (out, oi) if return_indices else out

    def mtm_grad(self, grad, masks, entropy_reg: float, form: str = "finetune", indices=None, batch_size: Optional[int] = None, eps=None,
                 return_indices: bool = False):
        """The gradient of that loss (m3pc_mtm_grad_replay) into ``grad``, a ``DeviceMTMGrad`` on this buffer's handle, for the batch
        ``traj_sample`` would return for the same arguments: per call the bits of ``traj_sample`` followed by ``grad.grad_record``.
        Returns the device record (15 floats; ``grad.export()`` hands out the gradients); ``step`` advances as in ``traj_sample``.
        Dropout is ``grad``'s: after ``grad.set_dropout(p, seed)`` the call drops under ``grad``'s current draw and advances it."""
        from .masks import mask_rows
        from .mtm import form_settings
        if grad.handle is not self.handle:  # (the library compares sizes and device only: another handle's weights would be differentiated)
            raise capi.M3pcError("mtm_grad: the DeviceMTMGrad object was created on another handle than this buffer's")
        B, pt, ps, dev, keep_i = self._segment_indices(indices, batch_size)
        flags, bits, _ = form_settings(form, capi.KEYS)
        e = None if eps is None else self._dev(eps, (B, self.sequence_length, self.A))
        rec = self._new(capi.MTM_LOSS_FLOATS)
        oi = (self._new(B, dtype=torch.int32), self._new(B, dtype=torch.int32)) if return_indices else (None, None)
        mp, keep = self.handle._mask_ptrs(mask_rows(masks))
        capi.check(self.lib.m3pc_mtm_grad_replay(grad._g, self._rb, B, _MODES[self._mode], pt, ps, dev, self.seed, self.step, mp,
                                                 capi._ptr(e), float(entropy_reg), flags, bits, capi._ptr(rec), capi._ptr(oi[0]),
                                                 capi._ptr(oi[1]), self._stream()))
        if indices is None:
            self.step += 1
        del keep_i, keep
        return (rec, oi) if return_indices else rec

    def mtm_train(self, trainer, n_steps: int, masks, batch_size: Optional[int] = None, form: str = "finetune"):
        """``n_steps`` whole training steps of the model (m3pc_mtm_train) on the batches ``traj_sample`` would draw at this ``step``,
        ``step + 1``, ...: ``trainer`` is a ``DeviceMTMTrainer`` on this buffer's handle (``trainer.train_from``).  Returns (records
        (n_steps, 15), train_records (n_steps, 3)) on the device; ``step`` advances by n_steps.  Dropout is ``trainer``'s
        (``DeviceMTMTrainer(dropout=, dropout_seed=)``): step i of the call drops under the trainer's draw + i."""
        return trainer.train_from(self, n_steps, batch_size, masks, form)

    def split(self, batch_size: Optional[int] = None):
        """(rows of the online ring, rows of the offline ring) of a transition batch: replay_buffer.py:370-381."""
        B = int(self.trans_batch_size if batch_size is None else batch_size)
        n_on = 0 if self.counts()[2] < self.cfg.using_online_threshold else B // 2
        return n_on, B - n_on

    def trans_sample(self, indices=None, batch_size: Optional[int] = None, return_indices: bool = False):
        """replay_buffer.py:368-420: (states, actions, rewards, next_states, dones), float32; online rows first.  indices: (B,) logical
        indices, the first ``split()[0]`` into the online ring, the rest into the offline ring; None: drawn, distinct within a ring."""
        n_on, n_off = self.split(batch_size)
        B = n_on + n_off
        keep, ptr, dev = (None, None, 0) if indices is None else self._index(indices, B)
        out = [self._new(B, self.S), self._new(B, self.A), self._new(B, 1), self._new(B, self.S), self._new(B, 1)]
        oi = self._new(B, dtype=torch.int32) if return_indices else None
        capi.check(self.lib.m3pc_replay_sample_transitions(self._rb, B, n_on, ptr, dev, self.seed, self.step, *[capi._ptr(x) for x in out],
                                                           capi._ptr(oi), self._stream()))
        if indices is None:
            self.step += 1
        del keep
        return (tuple(out), oi) if return_indices else tuple(out)

    def __iter__(self):
        self.current_index = 0
        return self

    def __next__(self):
        if self.current_index >= self.mtm_iter:
            raise StopIteration
        self.current_index += 1
        return self.traj_sample()
