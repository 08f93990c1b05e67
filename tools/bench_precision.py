"""ms per plan step of the fp32 / bf16 / bf16x3 planners, one process, same windows and candidates.

For each configuration (C2: hopper rtg_guiding N = 1024, T = 32, H = 16; C3: walker2d critic_lambda_guiding N = 4096) and weight
set (the init recipe, and synth.trained_like with every Linear x 2) every precision plans `warmup` steps (the certified re-score's
calibration passes run there) and then `steps` timed steps, serial (HipPlanner._guide: one step enqueued and resolved at a time,
auto_fp32 off).  Reported per row: ms/step, the mean number of candidates the certificate re-scored in fp32 (score + race entries),
the calibrated delta, and from one profiled step (m3pc_profile_read, events around every MFMA launch) the candidate-pass GEMM time
of the precision's own arithmetic next to the time of all bracketed launches.

    python tools/bench_precision.py [--steps K] [--warmup W] [--configs C2,C3] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from m3pc_amd import capi, synth  # noqa: E402
from m3pc_amd.planner import HipPlanner  # noqa: E402

CONFIGS = {"C2": ("hopper", "rtg_guiding", 0.01, 1024, 32, 16), "C3": ("walker2d", "critic_lambda_guiding", 1.0, 4096, 32, 16)}


def _window(dims, i):
    h = synth.make_history(dims, i % 11)
    h["path_length"] = 33 + (i * 37) % 960
    return h


def run(config, weights, precision, steps, warmup):
    env, guidance, tau, N, T, H = CONFIGS[config]
    S, A = synth.ENV_DIMS[env]
    dims = synth.Dims(S, A, T)
    sd, st = synth.make_state_dict(dims, 1), synth.make_tokenizer_stats(dims, 1)
    if weights == "trained_x2":
        sd, st = synth.trained_like(sd, st, seed=1, linear_scale=2.0, returns_std_scale=0.1)
    mode = capi.MODE_RTG if guidance == "rtg_guiding" else capi.MODE_CRITIC
    qsd, om, os_ = synth.make_critic(dims, 1) if mode == capi.MODE_CRITIC else (None, None, None)
    cfg = types.SimpleNamespace(traj_length=T, action_samples=N, horizon=H, discount=0.99, temperature=tau, lmbda=0.6,
                                plan_guidance=guidance, device="cuda")
    p = HipPlanner(cfg, sd, st, qsd, om, os_, precision=precision, auto_fp32=False,
                   generator=torch.Generator(device="cuda").manual_seed(1))
    eps = [synth.make_eps(N, dims, 100 + t).cuda() for t in range(4)]
    wins = [p.assemble_window(_window(dims, t), rtg=3.0) for t in range(8)]

    def step(t):
        s, a, r, h, g = wins[t % len(wins)]
        p._guide(mode, s, a, r, g, h, 0.6, eps=eps[t % len(eps)])

    for t in range(warmup):
        step(t)
    torch.cuda.synchronize()
    resc = []
    t0 = time.perf_counter()
    for t in range(steps):
        step(warmup + t)
        if p.rescore != "none":
            resc.append(int(p.last["n_rescored"]) + int(p.last.get("n_race", 0)))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    # one profiled step: GEMM time of the pass's arithmetic and of every bracketed launch
    p.handle.profile_read(-1)
    p.handle.profile_enable(True)
    step(0)
    torch.cuda.synchronize()
    own = p.handle.profile_read(p.precision, reset=False)
    allb = p.handle.profile_read(-1)
    p.handle.profile_enable(False)
    out = dict(config=config, weights=weights, precision=precision, N=N, ms_per_step=round(ms, 3),
               n_rescored=round(sum(resc) / len(resc), 1) if resc else None,
               delta=None if p._delta is None else round(float(p._delta), 5),
               gemm_launches=own[0], gemm_ms=round(own[1], 3), all_bracketed_launches=allb[0], all_bracketed_ms=round(allb[1], 3))
    p.handle.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--weights", default="recipe,trained_x2")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    print("| config | weights | precision | ms/step | n_rescored | delta | own-arithmetic GEMM ms (launches) | all bracketed ms |")
    print("|---|---|---|---|---|---|---|---|")
    for c in a.configs.split(","):
        for w in a.weights.split(","):
            for prec in ("fp32", "bf16", "bf16x3"):
                r = run(c, w, prec, a.steps, a.warmup)
                rows.append(r)
                print(f"| {c} | {w} | {prec} | {r['ms_per_step']} | {r['n_rescored']} | {r['delta']} | {r['gemm_ms']} ({r['gemm_launches']}) "
                      f"| {r['all_bracketed_ms']} |", flush=True)
    for c in a.configs.split(","):
        for w in a.weights.split(","):
            by = {r["precision"]: r for r in rows if r["config"] == c and r["weights"] == w}
            print(f"# {c} {w}: x3 / fp32 step = {by['bf16x3']['ms_per_step'] / by['fp32']['ms_per_step']:.3f}, "
                  f"x3 / fp32 GEMM time = {by['bf16x3']['gemm_ms'] / max(by['fp32']['gemm_ms'], 1e-9):.3f}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
