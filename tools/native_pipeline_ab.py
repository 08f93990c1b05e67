#!/usr/bin/env python3
"""A/B of the pipelined certified bf16 plan step at BASELINE config 2 (hopper, T = 32, N = 1024, H = 16, rtg_guiding), in ONE run
on one box, three legs:
  plan_async              the Python protocol at depth 3 (planner.py:_issue / _enqueue_tail / _finish + certificate.py:resolve)
  native plan_async       HipPlanner(native_step=True) at depth 3: m3pc_plan_step_certified_begin / _end per step
  serial one-call step    HipPlanner(native_step=True)._guide: m3pc_plan_step_certified, one step at a time
All planners see the same weights, the same windows and equally seeded generators; the legs alternate in rounds so that clock
drift hits them alike.  A report, not a gate: `--out FILE` also writes the lines to a file (profiles/native_pipeline_ab.txt)."""
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
    ap.add_argument("--steps", type=int, default=300, help="plan steps per leg and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dims = synth.Dims(11, 3, 32)
    cfg = types.SimpleNamespace(traj_length=32, action_samples=1024, horizon=16, discount=0.99, temperature=0.01, lmbda=0.6,
                                plan_guidance="rtg_guiding")
    mk = lambda native: HipPlanner(cfg, synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), None, precision="bf16",
                                   native_step=native, generator=torch.Generator(device="cuda").manual_seed(5))
    planners = {"plan_async": mk(False), "native plan_async": mk(True), "serial one-call step": mk(True)}
    hists = []
    for t in range(8):
        hist = synth.make_history(dims, t)
        hist["path_length"] = [500, 37, 321, 998, 640, 77, 250, 123][t]
        hists.append(hist)

    def run(k, n):
        p = planners[k]
        if k.startswith("serial"):
            for t in range(n):
                p.action_sample(hists[t % 8], plan=True, eval=False, rtg=3.0)
            return
        tickets = []
        for t in range(n):
            tickets.append(p.plan_async(hists[t % 8], eval=False, rtg=3.0))
            if len(tickets) == a.depth:
                tickets.pop(0).result()
        for tk in tickets:
            tk.result()

    for k in planners:  # calibration passes (16 full fp32 passes) and warm-up
        run(k, 48)
    torch.cuda.synchronize()
    per = {k: [] for k in planners}
    for _ in range(a.rounds):
        for k in planners:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(k, a.steps)
            torch.cuda.synchronize()
            per[k].append(a.steps / (time.perf_counter() - t0))
    med = lambda v: sorted(v)[len(v) // 2]
    lines = [f"certified bf16 plan step, BASELINE config 2 (N 1024, T 32, H 16), depth {a.depth}, {a.rounds} rounds x {a.steps} steps per leg, "
             f"{torch.cuda.get_device_name(0)}"]
    for k, p in planners.items():
        last = p.last
        lines.append(f"{k:22s} {med(per[k]):8.1f} plan-steps/s ({1e3 / med(per[k]):.4f} ms/step; rounds: {' '.join(f'{v:.1f}' for v in per[k])}); "
                     f"n_rescored {last['n_rescored']} n_race {last['n_race']} delta {last['delta']:.4g}")
    py, nat, ser = (med(per[k]) for k in planners)
    lines.append(f"native / python plan_async = {nat / py:.4f} ({100.0 * (nat / py - 1.0):+.2f} %); native pipelined / serial one-call = {nat / ser:.3f}")
    same = all(torch.equal(planners["plan_async"].last[n], planners["native plan_async"].last[n]) for n in ("argmax", "sample_idx", "sample_action"))
    lines.append(f"last step of both pipelined legs: same argmax / sample_idx / sample_action: {same}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
