#!/usr/bin/env python3
"""A/B of the serial certified bf16 plan step at BASELINE config 2 (hopper, T = 32, N = 1024, H = 16, rtg_guiding), in ONE run on
one box: the Python protocol (m3pc_amd/certificate.py driving seven entry points) against HipPlanner(native_step=True) (one
m3pc_plan_step_certified call per step), plus the host cost of a step from an idle device by the method of tools/host_calls.py.

Both planners see the same weights, the same windows and equally seeded generators; the legs alternate in rounds so that clock
drift hits both alike.  A report, not a gate: `--out FILE` also writes the lines to a file (profiles/native_step_ab.txt)."""
import argparse
import os
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from m3pc_amd import capi, synth  # noqa: E402
from m3pc_amd.planner import HipPlanner  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="serial steps per leg and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dims = synth.Dims(11, 3, 32)
    cfg = types.SimpleNamespace(traj_length=32, action_samples=1024, horizon=16, discount=0.99, temperature=0.01, lmbda=0.6,
                                plan_guidance="rtg_guiding")
    mk = lambda native: HipPlanner(cfg, synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), None, precision="bf16",
                                   native_step=native, generator=torch.Generator(device="cuda").manual_seed(5))
    legs = {"python protocol": mk(False), "native_step=True": mk(True)}
    hist = synth.make_history(dims, 0)
    hist["path_length"] = 500
    wins = {k: p.assemble_window(hist, rtg=3.0) for k, p in legs.items()}

    def step(k):
        s, a_, r, h, rtg = wins[k]
        return legs[k]._guide(capi.MODE_RTG, s, a_, r, rtg, h, 0.6)

    for k in legs:  # calibration passes (16 full fp32 passes) and warm-up
        for _ in range(40):
            step(k)
    torch.cuda.synchronize()
    per = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(k)
            torch.cuda.synchronize()
            per[k].append(1e3 * (time.perf_counter() - t0) / a.steps)
    host = {k: [] for k in legs}
    for k in legs:  # tools/host_calls.py: the device idle before the call, the wall time of the call itself / until complete
        for _ in range(50):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(k)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            host[k].append((1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t0)))
    med = lambda v: sorted(v)[len(v) // 2]
    lines = [f"serial certified bf16 plan step, BASELINE config 2 (N 1024, T 32, H 16), {a.rounds} rounds x {a.steps} steps per leg, "
             f"{torch.cuda.get_device_name(0)}"]
    for k in legs:
        last = legs[k].last
        lines.append(f"{k:18s} {med(per[k]):.4f} ms/step back to back (rounds: {' '.join(f'{v:.4f}' for v in per[k])}); from an idle device: "
                     f"call returns after {med([h[0] for h in host[k]]):.4f} ms, complete after {med([h[1] for h in host[k]]):.4f} ms; "
                     f"n_rescored {last['n_rescored']} n_race {last['n_race']} delta {last['delta']:.4g}")
    py, nat = med(per["python protocol"]), med(per["native_step=True"])
    lines.append(f"native / python = {nat / py:.4f} ({100.0 * (nat / py - 1.0):+.2f} %)")
    same = all(torch.equal(legs["python protocol"].last[n], legs["native_step=True"].last[n]) for n in ("argmax", "sample_idx", "sample_action"))
    lines.append(f"last step of both legs: same argmax / sample_idx / sample_action: {same}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
