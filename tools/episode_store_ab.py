#!/usr/bin/env python3
"""A/B of the episode store (m3pc_episodes_*, m3pc_amd/episodes.py) against host trajectories, in ONE process on one box: what a
rollout round costs from an idle device to the actions on the host when the windows are built by the host per environment
(leg "host": the code before the store) and when the episodes live on the device (leg "store").

Config-5 shape (zero-shot goal reaching, T = 8, H = 4, E = 8192 windows, bf16):
  host    action_piid_sample_batch on E host trajectories (a Python loop of _goal_window_host over the windows, one pageable
          H2D copy, m3pc_goal_step_batch) and the read-back of the actions
  store   observe (E observations from host memory) + windows + goal_actions + the read-back + record (E actions and rewards
          from host memory) -- a whole round, the two store updates included
  bare    m3pc_goal_step_batch alone on resident windows, no read-back: what the kernels of either leg take
Planning shapes at E = 8, lockstep="native" (the shipped N = 625 / H = 4 / T = 8 and the headline N = 1024 / H = 16 / T = 32):
  host    action_sample_batch(lockstep="native") on host trajectories + the read-back
  store   observe + action_sample_batch(lockstep="native", store=...) + the read-back + record
The legs alternate call by call (clock drift and neighbours on the box hit them alike); a call is timed by the host clock from an
idle device until its last result is on the host.  The host trajectories advance beside the store outside the timed regions (the
round's observation in front of the legs, the store leg's actions and rewards behind them): at every round both legs plan the same
windows, from the first step of the episodes on.  Required at the config-5 shape: median(store) <= median(host) (with --out the
run exits non-zero otherwise); the planning shapes are recorded without a bar -- a planning step does not wait for host gaps
(DESIGN.md section 4).  `--out FILE` also writes the lines to a file (profiles/episode_store_ab.txt)."""
import argparse
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from m3pc_amd import capi, synth  # noqa: E402
from m3pc_amd.episodes import EpisodeStore  # noqa: E402
from m3pc_amd.planner import HipPlanner  # noqa: E402

S, A = 11, 3
q = lambda v, f: sorted(v)[min(len(v) - 1, int(f * len(v)))]


def _cfg(T, N, H):
    return types.SimpleNamespace(traj_length=T, action_samples=N, horizon=H, discount=0.99, temperature=0.01, lmbda=0.6,
                                 plan_guidance="rtg_guiding", index_jump=4)


class _Hosts:
    """E host trajectories -- the episode buffers a rollout keeps, rollout.new_trajectory's layout -- that advance beside the store
    (outside the timed regions), so that at every round both legs plan the SAME windows."""

    def __init__(self, E):
        self.obs, self.act = np.zeros((E, 1000, S), dtype=np.float32), np.zeros((E, 1000, A), dtype=np.float32)
        self.rew, self.t = np.zeros((E, 1000, 1), dtype=np.float32), 0
        self.trajs = [{"observations": self.obs[e], "actions": self.act[e], "rewards": self.rew[e],
                       "values": np.zeros((1000, 1), dtype=np.float32), "total_return": 0, "path_length": 0} for e in range(E)]

    def observe(self, obs):
        self.obs[:, self.t] = obs

    def record(self, acts, rews):
        self.act[:, self.t] = np.clip(acts, -1, 1)
        self.rew[:, self.t, 0] = rews
        self.t += 1
        for tr in self.trajs:
            tr["path_length"] = self.t


def _time(legs, warmup, calls, before, after):
    """before(i): untimed, in front of round i's legs; after(i): untimed, behind them."""
    per = {k: [] for k in legs}
    for i in range(warmup + calls):
        before(i)
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                per[k].append(1e3 * (time.perf_counter() - t0))
        after(i)
    return per


def _rows(name, per, lines):
    for k, v in per.items():
        lines.append(f"{name:34s} {k:6s} {q(v, 0.5):9.4f} {q(v, 0.1):9.4f} {q(v, 0.9):9.4f}")


def goal_shape(E, warmup, calls, lines):
    T, H = 8, 4
    dims = synth.Dims(S, A, T)
    p = HipPlanner(_cfg(T, 1, H), synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), None, precision="bf16",
                   goal_batch=E)
    rng = np.random.RandomState(5)
    hosts = _Hosts(E)
    store = EpisodeStore(p, E, 1000)
    store.reset()
    bank = rng.normal(size=(16, E, S)).astype(np.float32)
    rews = rng.normal(size=(E,)).astype(np.float32)
    g = torch.Generator().manual_seed(5)
    st, ac = torch.randn((E, T, S), generator=g).cuda(), (torch.rand((E, T, A), generator=g) * 2 - 1).cuda()
    buf = (torch.empty((E, A), device="cuda"), torch.empty((E, A), device="cuda"))
    cur = {}

    def host():
        return p.action_piid_sample_batch(hosts.trajs, eval=True, rtg=2.5).cpu()

    def stored():
        store.observe(cur["obs"])
        acts = p.action_piid_sample_batch(None, eval=True, rtg=2.5, store=store).cpu()
        store.record(acts.numpy(), rews)
        cur["acts"] = acts.numpy()

    def bare():
        p.handle.goal_step_batch(st, ac, T - H, capi.GOAL_PIID, capi.PREC_BF16, out=buf)

    def before(i):
        cur["obs"] = bank[i % 16]
        hosts.observe(cur["obs"])

    per = _time({"host": host, "store": stored, "bare": bare}, warmup, calls, before, lambda i: hosts.record(cur["acts"], rews))
    name = f"config 5: zero-shot T 8 H 4 E {E}"
    _rows(name, per, lines)
    mh, ms, mb = (q(per[k], 0.5) for k in ("host", "store", "bare"))
    lines.append(f"{'':34s} store / host = {ms / mh:.4f} ({100.0 * (ms / mh - 1.0):+.2f} %); store - bare = {ms - mb:.4f} ms "
                 f"(store / bare = {ms / mb:.3f}); host - bare = {mh - mb:.4f} ms; {E / ms * 1e3 / 1e6:.3f} M windows/s through the store, "
                 f"{E / mh * 1e3 / 1e6:.3f} M windows/s from host trajectories")
    store.close()
    p.handle.close()
    return ms / mh


def plan_shape(name, N, H, T, E, warmup, calls, lines):
    dims = synth.Dims(S, A, T)
    p = HipPlanner(_cfg(T, N, H), synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), None, precision="bf16",
                   max_batch=E, max_windows=E, generator=torch.Generator(device="cuda").manual_seed(3))
    rng = np.random.RandomState(8)
    hosts = _Hosts(E)
    store = EpisodeStore(p, E, 1000)
    store.reset()
    bank = rng.normal(size=(16, E, S)).astype(np.float32)
    rews = rng.normal(size=(E,)).astype(np.float32)
    rtgs = [3.0 + 0.1 * w for w in range(E)]
    cur = {}

    def host():
        return p.action_sample_batch(hosts.trajs, eval=True, rtg=rtgs, lockstep="native").cpu()

    def stored():
        store.observe(cur["obs"])
        acts = p.action_sample_batch(None, eval=True, rtg=rtgs, lockstep="native", store=store).cpu()
        store.record(acts.numpy(), rews)
        cur["acts"] = acts.numpy()

    def before(i):
        cur["obs"] = bank[i % 16]
        hosts.observe(cur["obs"])

    per = _time({"host": host, "store": stored}, warmup, calls, before, lambda i: hosts.record(cur["acts"], rews))
    _rows(name, per, lines)
    mh, ms = q(per["host"], 0.5), q(per["store"], 0.5)
    lines.append(f"{'':34s} store / host = {ms / mh:.4f} ({100.0 * (ms / mh - 1.0):+.2f} %): recorded, no bar")
    store.close()
    p.handle.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300, help="timed calls per leg (after warm-up)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--windows", type=int, default=8192, help="E of the config-5 shape")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"Episode store A/B: a rollout round from an idle device to the actions on the host, windows from host trajectories "
             f"[host] against the episode store [store]; {a.calls} interleaved calls per leg after {a.warmup} warm-up calls; ms per "
             f"round; bf16; {torch.cuda.get_device_name(0)}",
             f"{'shape':34s} {'leg':6s} {'median':>9s} {'p10':>9s} {'p90':>9s}"]
    ratio = goal_shape(a.windows, a.warmup, a.calls, lines)
    print("\n".join(lines[-5:]), flush=True)
    plan_shape("shipped hopper N 625 H 4 T 8 E 8", 625, 4, 8, 8, a.warmup, a.calls, lines)
    print("\n".join(lines[-3:]), flush=True)
    plan_shape("headline hopper N 1024 H 16 T 32 E 8", 1024, 16, 32, 8, a.warmup, a.calls, lines)
    lines.append("config 5: median(store) <= median(host) (the required bar)" if ratio <= 1.0
                 else f"config 5: median(store) ABOVE median(host) ({ratio:.3f}): the required bar is NOT met")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        if ratio > 1.0:
            sys.exit("episode_store_ab: the store round is slower than the host round at the config-5 shape")


if __name__ == "__main__":
    main()
