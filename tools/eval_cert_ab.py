#!/usr/bin/env python3
"""A/B of the eval_action certificate, in ONE process on one box: m3pc_plan_step_certified (the baseline) against
m3pc_plan_step_certified_eval at eval_tol = inf (report only: one more launch and one more host read), 1e-3 and 1e-4, for bf16,
bf16x3 and fp32, on the headline shape (BASELINE config 2: hopper, rtg_guiding, N = 1024, T = 32, H = 16, temperature 0.01) and on
the critic shape (config 3: walker2d, critic_lambda_guiding, N = 4096, T = 32, H = 16, temperature 1).

Every leg sees the same weights, the same window and the same cycle of pre-drawn variates; delta is calibrated once per precision
(factor 1.6) on the first of them and grows as the steps ask (grow_delta).  The legs alternate in rounds, so that clock drift and
neighbours hit all of them alike; a leg's time is the median over its rounds of (host clock around `steps` serial calls, ending in a
device synchronisation) / steps.  Reported per leg: ms per step, the fp32 rows re-scored per step (score + race entries; N after
`everything`), eval_bound (median and maximum over the timed steps) and how many steps took the every-candidate path.
A report, not a gate: `--out FILE` also writes the lines (and `FILE.json` the numbers)."""
import argparse
import json
import os
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from m3pc_amd import capi, synth  # noqa: E402
from m3pc_amd.planner import HipPlanner  # noqa: E402

SHAPES = {"headline": ("hopper", "rtg_guiding", 0.01, 1024, 32, 16), "critic": ("walker2d", "critic_lambda_guiding", 1.0, 4096, 32, 16)}
TOLS = (None, float("inf"), 1e-3, 1e-4)  # None: m3pc_plan_step_certified
med = lambda v: sorted(v)[len(v) // 2]


def name(tol):
    return "certified (baseline)" if tol is None else f"eval_tol {tol:g}"


def run_shape(tag, shape, a, lines, out):
    env, guidance, tau, N, T, H = shape
    S, A = synth.ENV_DIMS[env]
    dims = synth.Dims(S, A, T)
    cfg = types.SimpleNamespace(traj_length=T, action_samples=N, horizon=H, discount=0.99, temperature=tau, lmbda=0.6, plan_guidance=guidance)
    critic = guidance != "rtg_guiding"
    qsd, om, os_ = synth.make_critic(dims, 0) if critic else (None, None, None)
    p = HipPlanner(cfg, synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), qsd, om, os_, precision="bf16")
    hd = p.handle
    mode = capi.MODE_CRITIC if critic else capi.MODE_RTG
    hist = synth.make_history(dims, 0)
    hist["path_length"] = 500
    s, ac, r, h, rtg = p.assemble_window(hist, rtg=3.0)
    g = torch.Generator(device="cuda").manual_seed(11)
    draws = [(torch.randn((N, T, A), device="cuda", generator=g), torch.empty(N, device="cuda").exponential_(1, generator=g).clamp_min_(2.0 ** -25))
             for _ in range(a.draws)]
    kmax, R = max(min(128, N - 1), 1), min(32, N)
    lines.append(f"== {tag}: {env} {guidance} N {N} T {T} H {h} temperature {tau}, kmin 8 kmax {kmax} rfirst 2 rmax {R}, {a.rounds} rounds x "
                 f"{a.steps} steps per leg, {torch.cuda.get_device_name(0)}")
    for prec in ("bf16", "bf16x3", "fp32"):
        code = capi.PRECISIONS[prec]
        delta = 0.0
        if code != capi.PREC_FP32:
            hd.policy_pass(mode, s, ac, r, h, rtg, slot=0)
            low = hd.candidate_pass(mode, s, ac, r, draws[0][0], h, 0.6, 0.99, N, precision=code, slot=0)["expect_return"]
            delta = hd.calibrate_delta(mode, s, ac, r, draws[0][0], low, h, 0.6, 0.99, N, factor=1.6, slot=0)
        state = {tol: dict(delta=delta, i=0, ms=[], rows=[], bound=[], everything=0, n_eval=[]) for tol in TOLS}

        def step(tol, record):
            st = state[tol]
            eps, q = draws[st["i"] % len(draws)]
            st["i"] += 1
            o = hd.plan_step_certified(mode, s, ac, r, eps, q, h, rtg, 0.6, 0.99, N, tau, delta=st["delta"], grow_delta=True, kmin=8,
                                       kmax=kmax, rfirst=2, rmax=R, precision=code, slot=0, eval_tol=tol)
            rec = o[1]
            if code != capi.PREC_FP32:
                st["delta"] = max(st["delta"], float(rec.delta))
            if record:
                st["rows"].append(N if rec.everything else rec.n_rescored + rec.n_race)
                st["everything"] += int(bool(rec.everything)) if code != capi.PREC_FP32 else 0
                if tol is not None:
                    st["bound"].append(float(o[2].eval_bound))
                    st["n_eval"].append(int(o[2].n_eval))

        for tol in TOLS:  # warm-up of every leg: every path it takes, every draw once
            for _ in range(max(a.draws, 8)):
                step(tol, False)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for tol in TOLS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step(tol, True)
                torch.cuda.synchronize()
                state[tol]["ms"].append(1e3 * (time.perf_counter() - t0) / a.steps)
        base = med(state[None]["ms"])
        lines.append(f"-- {prec}: delta {delta:.4g}")
        for tol in TOLS:
            st = state[tol]
            m = med(st["ms"])
            row = dict(shape=tag, precision=prec, leg=name(tol), ms_per_step=m, rounds_ms=st["ms"], vs_baseline=m / base,
                       rows_rescored_mean=sum(st["rows"]) / len(st["rows"]), steps_everything=st["everything"], steps=len(st["rows"]))
            txt = (f"{name(tol):22s} {m:8.4f} ms/step ({100.0 * (m / base - 1.0):+6.2f} % vs baseline; rounds {' '.join(f'{v:.4f}' for v in st['ms'])}); "
                   f"fp32 rows re-scored {row['rows_rescored_mean']:.1f}/step")
            if tol is not None:
                row.update(eval_bound_median=med(st["bound"]), eval_bound_max=max(st["bound"]), n_eval_mean=sum(st["n_eval"]) / len(st["n_eval"]))
                txt += (f" (of them for this certificate {row['n_eval_mean']:.1f}); eval_bound median {row['eval_bound_median']:.3e} max "
                        f"{row['eval_bound_max']:.3e}; every candidate in fp32 on {st['everything']} of {len(st['rows'])} steps")
            lines.append(txt)
            out.append(row)
    hd.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="serial steps per leg and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--draws", type=int, default=8, help="pre-drawn (eps, expo) pairs the steps cycle through")
    ap.add_argument("--shapes", default="headline,critic")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_cert_ab.py measures on a GPU: none is visible")
    lines, out = [], []
    for tag in a.shapes.split(","):
        done = len(lines)
        run_shape(tag, SHAPES[tag], a, lines, out)
        print("\n".join(lines[done:]), flush=True)
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
        with open(a.out + ".json", "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
