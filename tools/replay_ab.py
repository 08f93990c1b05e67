#!/usr/bin/env python3
"""A/B of the replay buffer (m3pc_replay_*, m3pc_amd/replay.py) against a host buffer, in ONE process on one box: what one training
batch costs from an idle device until it is resident there, at the shipped config's shape on hopper dimensions (S = 11, A = 3):
1000 trajectories x 1000 steps, segments of L = 8, B = 512, trajectories in proportion to path length ("prob"); 256 transitions, half
from a 10^6-entry offline ring and half from an online ring of 50 000.

  host    the reference's sampling rules on host NumPy arrays (replay_buffer.py:312-366: np.random.choice with p, a Python loop of
          512 np.random.randint + four slices, np.stack, one pageable .to(device) per key; :368-420: random.sample on each ring, five
          fancy-index gathers, one .to(device) per key).  The transitions are ARRAY rings here, not the reference's deque of
          namedtuples with its per-item np.stack: that is kinder to the host than the reference is.
  device  DeviceReplayBuffer.traj_sample() / trans_sample(): indices drawn by the library, one or two launches, nothing copied.

The legs alternate call by call (clock drift and neighbours on the box hit them alike); a call is timed by the host clock from an
idle device until the device is idle again.  Required: median(device) <= median(host) for the segment batch (with --out the run
exits non-zero otherwise); the transition batch, and the per-rollout supply (200 segment batches + 10 transition batches per model
step as the shipped config has them) derived from the medians, are recorded without a bar.  `--out FILE` also writes the lines to a
file (profiles/replay_ab.txt)."""
import argparse
import os
import random
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from m3pc_amd import capi  # noqa: E402
from m3pc_amd.replay import DeviceReplayBuffer  # noqa: E402

S, A, M, L = 11, 3, 1000, 8
q = lambda v, f: sorted(v)[min(len(v) - 1, int(f * len(v)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300, help="timed calls per leg (after warm-up)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--trajectories", type=int, default=1000)
    ap.add_argument("--offline", type=int, default=1000000)
    ap.add_argument("--online", type=int, default=50000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, B, TB = a.trajectories, 512, 256
    dev = torch.device("cuda", 0)
    cfg = types.SimpleNamespace(traj_length=L, traj_batch_size=B, traj_buffer_size=N, trans_batch_size=TB, trans_buffer_size=a.offline,
                                select_mode="prob", mtm_iter_per_rollout=200, using_online_threshold=10000)
    hd = capi.Handle(S, A, L, n_embd=64, n_head=2, max_candidates=64)
    buf = DeviceReplayBuffer(hd, cfg, N, M, seed=1)
    g = torch.Generator(device=dev).manual_seed(1)
    rng = np.random.RandomState(1)
    lens = rng.randint(200, M + 1, size=N)
    obs, act = torch.randn((N, M, S), generator=g, device=dev), torch.rand((N, M, A), generator=g, device=dev) * 2 - 1
    rew, val = torch.randn((N, M), generator=g, device=dev), torch.randn((N, M), generator=g, device=dev, dtype=torch.float64)
    buf.append(obs, act, rew, val, lens)
    rings = {}
    for online, n in ((False, a.offline), (True, a.online)):
        t = [torch.randn((n, S), generator=g, device=dev), torch.rand((n, A), generator=g, device=dev), torch.randn((n,), generator=g, device=dev),
             torch.randn((n, S), generator=g, device=dev), torch.zeros((n,), device=dev)]
        buf.append_transitions(*t, online=online)
        rings[online] = [x.cpu().numpy().reshape(n, -1) for x in t]
    # the host buffer: the same contents as NumPy arrays (values float64, as values_segmented is)
    h_obs, h_act, h_rew, h_val = obs.cpu().numpy(), act.cpu().numpy(), rew.cpu().numpy()[..., None], val.cpu().numpy()[..., None]
    p = lens / lens.sum(axis=0)
    del obs, act, rew, val
    assert buf.counts() == (N, a.offline, a.online) and buf.split() == (TB // 2, TB - TB // 2)

    def host_segments():
        idx = np.random.choice(np.arange(len(p)), size=B, p=p)
        so, sa, sr, sv = [], [], [], []
        for i in idx:
            k = np.random.randint(0, lens[i] - L + 1)
            so.append(h_obs[i, k:k + L])
            sa.append(h_act[i, k:k + L])
            sr.append(h_rew[i, k:k + L])
            sv.append(h_val[i, k:k + L])
        batch = {"states": np.stack(so), "actions": np.stack(sa), "rewards": np.stack(sr), "returns": np.stack(sv)}
        return {k: torch.from_numpy(v).to(dev) for k, v in batch.items()}

    def host_transitions():
        on = random.sample(range(a.online), TB // 2)
        off = random.sample(range(a.offline), TB - TB // 2)
        return tuple(torch.from_numpy(np.concatenate([rings[True][k][on], rings[False][k][off]])).float().to(dev) for k in range(5))

    legs = {"segments B 512 L 8 prob": {"host": host_segments, "device": buf.traj_sample},
            "transitions B 256 (128 + 128)": {"host": host_transitions, "device": buf.trans_sample}}
    lines = [f"Replay buffer A/B: one training batch from an idle device until it is resident there, the reference's sampling on host "
             f"arrays [host] against the device buffer [device]; {N} trajectories x {M} steps, offline ring {a.offline}, online ring "
             f"{a.online}; {a.calls} interleaved calls per leg after {a.warmup} warm-up calls; ms per batch; {torch.cuda.get_device_name(0)}",
             f"{'batch':34s} {'leg':6s} {'median':>9s} {'p10':>9s} {'p90':>9s}"]
    med = {}
    for name, pair in legs.items():
        per = {k: [] for k in pair}
        for i in range(a.warmup + a.calls):
            for k, fn in pair.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    per[k].append(1e3 * (time.perf_counter() - t0))
                del out
        for k, v in per.items():
            lines.append(f"{name:34s} {k:6s} {q(v, 0.5):9.4f} {q(v, 0.1):9.4f} {q(v, 0.9):9.4f}")
        med[name] = (q(per["host"], 0.5), q(per["device"], 0.5))
        lines.append(f"{'':34s} device / host = {med[name][1] / med[name][0]:.4f}")
    (sh, sd), (th, td) = med.values()
    lines.append(f"per rollout (200 segment batches, 10 transition batches per model step; from the medians): host "
                 f"{200 * sh + 2000 * th:.1f} ms, device {200 * sd + 2000 * td:.1f} ms: recorded, no bar")
    ok = sd <= sh
    lines.append("segments: median(device) <= median(host) (the required bar)" if ok
                 else f"segments: median(device) ABOVE median(host) ({sd / sh:.3f}): the required bar is NOT met")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        if not ok:
            sys.exit("replay_ab: the device segment batch is slower than the host's")
    torch.cuda.synchronize()
    buf.close()
    hd.close()


if __name__ == "__main__":
    main()
