"""Rollout-level caller of the pipelined planner: the counterpart of ``Learner.evaluate_plan``
(research/finetune_omtm/learner.py:645-741: ``num_episodes`` independent evaluation episodes, one after the other, one
``action_sample`` per environment step with the action read back each time) and of ``ReplayBuffer.online_rollout``'s env
loop (replay_buffer.py:204-232) for SEVERAL environments at once.

The reference's loops are strictly sequential because one environment's next window needs its last action.  Across
environments nothing couples the plan steps, so ``evaluate_plan`` here steps E environments round-robin and keeps their
plan steps in flight on the device (``HipPlanner.plan_async``): while environment i's candidate pass runs, environment
i+1's policy pass and environment i-1's re-score + select run on the planner's other streams, and the host steps the
simulator of the environment whose action has just arrived.  Per environment, the sequence of windows, draws and actions
is what the reference's loop produces for that environment with the same generator order (tests/test_rollout_gpu.py).

The simulator is the caller's: any object with ``reset() -> obs`` and ``step(action) -> (obs, reward, done, info)``
(gym's API, which is what jaxrl's env wrappers hand to the reference; gym / d4rl / mujoco are not needed here).
"""
from __future__ import annotations

from collections import defaultdict
from typing import Any, Callable, Dict, List, Optional, Sequence

import numpy as np


def new_trajectory(state_dim: int, action_dim: int, max_steps: int = 1000) -> Dict[str, Any]:
    """The episode buffer of learner.py:660-674 / replay_buffer.py:189-203."""
    return {"observations": np.zeros((max_steps, state_dim), dtype=np.float32),
            "actions": np.zeros((max_steps, action_dim), dtype=np.float32),
            "rewards": np.zeros((max_steps, 1), dtype=np.float32), "values": np.zeros((max_steps, 1), dtype=np.float32),
            "total_return": 0, "path_length": 0}


def _rtg_at(episode_rtg_ref, t: int, ratio: float) -> float:
    """episode_rtg_ref[t] * ratio as a float: the reference is (max_steps,) or, as ReplayBuffer.values_up_bound is, (max_steps, 1)."""
    return float(np.asarray(episode_rtg_ref[t]).reshape(-1)[0] * ratio)


class _Episode:
    def __init__(self, env, index, traj):
        self.env, self.index, self.traj = env, index, traj
        self.observation = None
        self.timestep = 0
        self.done = False
        self.info: Dict[str, Any] = {}
        self.ticket = None


def evaluate_plan(planner, envs: Sequence, episode_rtg_ref: np.ndarray, ratio: float = 1.0, max_steps: int = 1000,
                  in_flight: Optional[int] = None, on_step: Optional[Callable] = None, eval: bool = True,
                  percentage: float = 1.0, lockstep=False, store=False, discount: Optional[float] = None,
                  use_avg: bool = False) -> Dict[str, Any]:
    """One evaluation episode in each of ``envs`` (learner.py:645-741 with num_episodes = len(envs)), planned through the
    pipelined planner.  ``episode_rtg_ref[t] * ratio`` is the return-to-go handed to the planner at timestep t (learner.py:
    688); with ``eval=False`` the planner explores as ``online_rollout`` does (sampled action, return-to-go from the
    ``percentage`` of the returns range, replay_buffer.py:206-212).
    in_flight: how many environments have a plan step on the device at the same time (default: planner.pipeline_depth + 1,
    at most the number of slots - 1).
    lockstep: the environments step TOGETHER instead -- per round one ``action_sample_batch(lockstep=True)`` over the windows
    of all live environments (one policy pass at batch E, the candidate passes back to back, one batched fp32 re-score: the
    short launches of the fp32 chains are paid once per round, not once per environment; needs a planner built with
    ``max_batch >= len(envs)``; per environment the actions agree with the pipelined loop to fp32 rounding of the policy
    head, not bit for bit, and the draws are taken per round); ``lockstep="native"``: the same rounds as one library call each
    (``action_sample_batch(lockstep="native")``), the lock-step form a planner with ``eval_tol`` takes.  Returns {"return_mean", "return_std", "length_mean", "length_std", "returns",
    "lengths", "trajectories", "plan_steps"} -- the statistics evaluate_plan logs (learner.py:715-731); with a planner built with
    ``eval_tol`` also "eval_bound_max" (the largest per-step bound on |eval_action - the fp32 step's|) and "eval_steps_everything"
    (the steps that scored every candidate in fp32).
    store: True (or an ``episodes.EpisodeStore`` of at least len(envs) environments and ``max_steps`` steps) keeps the episodes on
    the device (lock-step forms only): per round ONE observe, one planning call fed by the store's windows, one record (which
    clips as the host loop does); per environment the actions, rewards and lengths are those of the same call without the store,
    bit for bit.  ``trajectories[i]`` is exported from the store at the end, with ``values`` filled as ReplayBuffer.online_rollout
    fills them (replay_buffer.py:234-243) for ``discount`` (default: the planner's cfg.discount) and ``use_avg``; without a store
    ``values`` stays zero, as before."""
    from . import capi

    if store and not lockstep:
        raise ValueError("store=: the episode store feeds the lock-step forms (lockstep=True / 'native')")

    E = len(envs)
    S, A = planner.S, planner.A
    cap = max(1, min(in_flight if in_flight is not None else planner.pipeline_depth + 1, capi.SLOTS - 1, E))
    eps_ = [_Episode(env, i, new_trajectory(S, A, max_steps)) for i, env in enumerate(envs)]
    for ep in eps_:
        ep.observation = ep.env.reset()
    waiting: List[_Episode] = list(eps_)   # environments that need a plan step issued, in round-robin order
    flying: List[_Episode] = []            # environments whose plan step is on the device, oldest first
    steps = 0
    with_eval = getattr(planner, "_eval_tol", None) is not None
    bound_max, n_everything = 0.0, 0

    def note(info):
        nonlocal bound_max, n_everything
        if with_eval and info is not None and "eval_bound" in info:
            bound_max = max(bound_max, float(info["eval_bound"]))
            n_everything += int(bool(info.get("everything", False)))

    def issue(ep: _Episode):
        ep.traj["observations"][ep.timestep] = ep.observation
        rtg = _rtg_at(episode_rtg_ref, ep.timestep, ratio) if eval else None
        ep.ticket = planner.plan_async(ep.traj, percentage=percentage, eval=eval, rtg=rtg)
        flying.append(ep)

    def land(ep: _Episode, action=None):
        nonlocal steps
        if action is None:
            action = ep.ticket.result().cpu().numpy()
            note(ep.ticket.info)
            ep.ticket = None
        action = np.clip(action, -1, 1)  # learner.py:690 / replay_buffer.py:213-215
        obs, reward, done, info = ep.env.step(action)
        ep.traj["actions"][ep.timestep] = action
        ep.traj["rewards"][ep.timestep] = reward
        ep.traj["total_return"] += reward
        ep.observation = obs
        ep.timestep += 1
        ep.traj["path_length"] += 1
        ep.done, ep.info = bool(done), info
        steps += 1
        if on_step is not None:
            on_step(ep.index, ep.timestep, action, reward, done)
        if not ep.done and ep.timestep < max_steps:
            waiting.append(ep)

    st = None
    if store:
        from .episodes import EpisodeStore
        st = EpisodeStore(planner, E, max_steps) if store is True else store
        if st.n_envs < E or st.max_steps != max_steps:
            raise ValueError(f"store: {st.n_envs} environments x {st.max_steps} steps, the rollout needs >= {E} x {max_steps}")
        st.reset(list(range(E)))
    while st is not None and waiting:
        live, waiting = waiting, []
        ids = [ep.index for ep in live]
        st.observe(np.stack([np.asarray(ep.observation) for ep in live]), ids)
        rtgs = [_rtg_at(episode_rtg_ref, ep.timestep, ratio) for ep in live] if eval else None
        named = dict(keys=ids) if getattr(planner, "_refine", None) is not None else {}
        acts = planner.action_sample_batch(None, percentage=percentage, eval=eval, rtg=rtgs,
                                           lockstep="native" if lockstep == "native" else True, store=st, env_ids=ids, **named)
        for info in planner.last["windows"] if with_eval else ():
            note(info)
        acts = acts.cpu().numpy()  # one read-back per round
        rewards = np.empty((len(live),), dtype=np.float32)
        for j, ep in enumerate(live):
            obs, reward, done, info = ep.env.step(np.clip(acts[j], -1, 1))  # learner.py:690 / replay_buffer.py:213-215
            rewards[j] = reward
            ep.traj["total_return"] += reward
            ep.observation = obs
            ep.timestep += 1
            ep.done, ep.info = bool(done), info
            steps += 1
            if on_step is not None:
                on_step(ep.index, ep.timestep, np.clip(acts[j], -1, 1), reward, done)
            if not ep.done and ep.timestep < max_steps:
                waiting.append(ep)
        st.record(acts, rewards, ids, clip_min=-1.0, clip_max=1.0)
    if st is not None:
        gamma = float(planner.cfg.discount) if discount is None else float(discount)
        vals = st.values(gamma, use_avg, list(range(E)))
        for ep in eps_:
            total = ep.traj["total_return"]
            ep.traj = st.trajectory(ep.index, vals[ep.index])
            ep.traj["total_return"] = total
        if store is True:
            st.close()
    while lockstep and waiting:
        live, waiting = waiting, []
        for ep in live:
            ep.traj["observations"][ep.timestep] = ep.observation
        rtgs = [_rtg_at(episode_rtg_ref, ep.timestep, ratio) for ep in live] if eval else None
        # (a planner that plans by refinement keeps a warm start per environment: `live` shrinks as episodes end, so the
        # environments are named by their index, not by their position in this round)
        named = dict(keys=[ep.index for ep in live]) if getattr(planner, "_refine", None) is not None else {}
        acts = planner.action_sample_batch([ep.traj for ep in live], percentage=percentage, eval=eval, rtg=rtgs,
                                           lockstep="native" if lockstep == "native" else True, **named)
        for info in planner.last["windows"] if with_eval else ():
            note(info)
        for ep, action in zip(live, acts.cpu().numpy()):  # one read-back per round
            land(ep, action)
    while waiting or flying:
        while waiting and len(flying) < cap:
            issue(waiting.pop(0))
        land(flying.pop(0))
    stats: Dict[str, List[float]] = defaultdict(list)
    for ep in eps_:
        if isinstance(ep.info, dict) and "episode" in ep.info:       # jaxrl's EpisodeMonitor (learner.py:703-708)
            for k, v in ep.info["episode"].items():
                stats[k].append(float(v))
        else:
            stats["return"].append(float(ep.traj["rewards"].sum()))
            stats["length"].append(float(ep.traj["path_length"]))
    out: Dict[str, Any] = {}
    for k, v in stats.items():
        out[k + "_mean"] = float(np.mean(v))
        out[k + "_std"] = float(np.std(v))
    out["returns"], out["lengths"] = stats.get("return", []), stats.get("length", [])
    out["trajectories"] = [ep.traj for ep in eps_]
    out["plan_steps"] = steps
    if with_eval:
        out["eval_bound_max"], out["eval_steps_everything"] = bound_max, n_everything
    return out
