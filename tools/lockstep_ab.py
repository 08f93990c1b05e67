#!/usr/bin/env python3
"""A/B of the lock-step batch of certified bf16 plan steps, in ONE run on one box: ``action_sample_batch(lockstep=True)`` (the Python
protocol of m3pc_amd/lockstep.py: torch gathers, E list launches, E merges, E selects, a .cpu() read) against
``lockstep="native"`` (one m3pc_plan_steps_certified call per group), on two shapes:

  batched.E8  bench.py's `batched.E8_lockstep` leg: BASELINE config 2 (hopper, T = 32, N = 1024, H = 16, rtg_guiding), E = 8
  shipped     the reference's shipped planning config (N = 625, T = 8, H = 4), E = 8

One planner per shape serves both legs (same weights, same workspaces, same calibrated bound); the legs alternate in rounds so
that clock drift and the box's other tenants hit both alike; every timed window ends in a device synchronise.  The yardstick is
``lockstep=True`` in the same run.  A report, not a gate: `--out FILE` also writes the lines to a file
(profiles/ab_lockstep_native.txt)."""
import argparse
import os
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from m3pc_amd import synth  # noqa: E402
from m3pc_amd.planner import HipPlanner  # noqa: E402

SHAPES = {"batched.E8": (32, 1024, 16), "shipped": (8, 625, 4)}  # T, N, H (hopper, rtg_guiding)
LEGS = (("lockstep=True", True), ('lockstep="native"', "native"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8, help="E: windows per call")
    ap.add_argument("--calls", type=int, default=60, help="calls per leg and round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    E = a.envs
    med = lambda v: sorted(v)[len(v) // 2]
    lines = [f"action_sample_batch of E = {E} windows, certified bf16, lockstep=True against lockstep=\"native\": {a.rounds} rounds x "
             f"{a.calls} calls per leg, interleaved, one planner per shape, {torch.cuda.get_device_name(0)}",
             f"{'shape':12s} {'leg':18s} {'median ms/call':>14s} {'plan-steps/s':>12s}  rounds (ms/call)"]
    for name, (T, N, H) in SHAPES.items():
        dims = synth.Dims(11, 3, T)
        cfg = types.SimpleNamespace(traj_length=T, action_samples=N, horizon=H, discount=0.99, temperature=0.01, lmbda=0.6,
                                    plan_guidance="rtg_guiding")
        p = HipPlanner(cfg, synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), None, precision="bf16",
                       generator=torch.Generator(device="cuda").manual_seed(1), max_batch=E, max_windows=E)
        hs = [dict(synth.make_history(dims, i), path_length=500) for i in range(E)]
        call = lambda mode: p.action_sample_batch(hs, eval=True, rtg=3.0, lockstep=mode)
        for _ in range(max(4, -(-p._cal_windows // E) + 2)):  # the weight load's calibration windows (lockstep=True calibrates), untimed
            call(True)
        assert p._cal_left == 0
        for _, mode in LEGS:  # warm-up of both legs
            for _ in range(10):
                call(mode)
        torch.cuda.synchronize()
        per = {k: [] for k, _ in LEGS}
        for _ in range(a.rounds):
            for k, mode in LEGS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    call(mode)
                torch.cuda.synchronize()
                per[k].append(1e3 * (time.perf_counter() - t0) / a.calls)
        for k, _ in LEGS:
            m = med(per[k])
            lines.append(f"{name:12s} {k:18s} {m:14.4f} {1e3 * E / m:12.1f}  {' '.join(f'{v:.4f}' for v in per[k])}")
        py, nat = med(per[LEGS[0][0]]), med(per[LEGS[1][0]])
        w = p.last["windows"]
        lines.append(f"{name:12s} native / python = {nat / py:.4f} ({100.0 * (nat / py - 1.0):+.2f} % time per call); last call: n_rescored "
                     f"{[x['n_rescored'] for x in w]} n_race {[x['n_race'] for x in w]} delta {p.last['delta']:.4g} delta_grown {p.delta_grown}")
        p.handle.close()
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
