#!/usr/bin/env python3
"""A/B of the eval_action certificate in the pipelined and the lock-step certified step, in ONE process on one box, on the headline
shape (BASELINE config 2: hopper, rtg_guiding, N = 1024, T = 32, H = 16, temperature 0.01) in bf16 and bf16x3.

pipelined   three planners on the same weights and generator seed, ``plan_async`` with ``pipeline_depth`` tickets in flight:
              (1) eval_tol = inf     m3pc_plan_step_certified_eval_begin / _eval_end: the bound goes out with the step's tail
              (2) no eval_tol        m3pc_plan_step_certified_begin / _end: the yardstick
              (3) eval_tol = inf, one step at a time (m3pc_plan_step_certified_eval): what an eval_tol planner's plan_async ran
                  before the pipelined form existed
            and, for (1), the share of steps whose bound launched in advance was dropped (a further merge was issued first).
lock-step   ``action_sample_batch(lockstep="native")`` at E = 8 with eval_tol = inf (m3pc_plan_steps_certified_eval) against the
            same call without eval_tol (m3pc_plan_steps_certified), tools/lockstep_ab.py's method.

The legs alternate in rounds, so that clock drift and the box's other tenants hit all of them alike; a leg's figure is the median
over its rounds; every timed stretch ends in a device synchronise.  A report, not a gate: `--out FILE` also writes the lines."""
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

T, N, H = 32, 1024, 16
INF = float("inf")
med = lambda v: sorted(v)[len(v) // 2]


def _planner(dims, precision, **kw):
    cfg = types.SimpleNamespace(traj_length=T, action_samples=N, horizon=H, discount=0.99, temperature=0.01, lmbda=0.6,
                                plan_guidance="rtg_guiding")
    return HipPlanner(cfg, synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), None, precision=precision,
                      generator=torch.Generator(device="cuda").manual_seed(1), **kw)


def pipelined(a, lines):
    dims = synth.Dims(11, 3, T)
    hists = [dict(synth.make_history(dims, i), path_length=500 + 7 * i) for i in range(8)]
    lines.append(f"== pipelined: hopper rtg_guiding N {N} T {T} H {H}, {a.rounds} rounds x {a.steps} steps per leg, interleaved, "
                 f"{torch.cuda.get_device_name(0)}")
    for prec in ("bf16", "bf16x3"):
        legs = {"(1) eval_tol=inf pipelined": (_planner(dims, prec, native_step=True, eval_tol=INF), True),
                "(2) no eval_tol pipelined": (_planner(dims, prec, native_step=True), True),
                "(3) eval_tol=inf serial": (_planner(dims, prec, native_step=True, eval_tol=INF), False)}
        stats = {k: dict(ms=[], dropped=0, bounds=0, everything=0) for k in legs}

        def run(k, steps, record):
            p, pipe = legs[k]
            st = stats[k]

            def note(info):
                if record and "eval_rounds" in info and info["eval_rounds"] >= 1:
                    st["bounds"] += 1
                    st["dropped"] += int(info["rounds"] > 1)  # (eval_tol = inf: this certificate asks for no merge of its own)
                if record:
                    st["everything"] += int(bool(info.get("everything", False)))

            if not pipe:
                for i in range(steps):
                    p.action_sample(hists[i % len(hists)], plan=True, eval=True, rtg=3.0)
                    note(p.last)
                return
            flight = []
            for i in range(steps):
                flight.append(p.plan_async(hists[i % len(hists)], eval=True, rtg=3.0))
                if len(flight) > p.pipeline_depth:
                    tk = flight.pop(0)
                    tk.result()
                    note(tk.info)
            for tk in flight:
                tk.result()
                note(tk.info)

        for k in legs:  # the weight load's calibration steps and a warm-up of every leg, untimed
            run(k, legs[k][0]._cal_windows + 24, False)
            assert legs[k][0]._cal_left == 0
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(k, a.steps, True)
                torch.cuda.synchronize()
                stats[k]["ms"].append(1e3 * (time.perf_counter() - t0) / a.steps)
        base = med(stats["(2) no eval_tol pipelined"]["ms"])
        lines.append(f"-- {prec}: pipeline_depth {legs['(1) eval_tol=inf pipelined'][0].pipeline_depth}, delta "
                     f"{[round(float(p._delta), 6) for p, _ in legs.values()]}")
        for k in legs:
            st = stats[k]
            m = med(st["ms"])
            txt = (f"{k:28s} {m:8.4f} ms/step {1e3 / m:8.1f} plan-steps/s ({100.0 * (m / base - 1.0):+6.2f} % time vs (2); rounds "
                   f"{' '.join(f'{v:.4f}' for v in st['ms'])})")
            if st["bounds"] and k.startswith("(1)"):  # (only leg (1) launches a bound in advance)
                txt += f"; bounds read {st['bounds']}, launched in advance and dropped {st['dropped']} ({100.0 * st['dropped'] / st['bounds']:.1f} %)"
            if st["everything"]:
                txt += f"; every candidate in fp32 on {st['everything']} steps"
            lines.append(txt)
        for p, _ in legs.values():
            p.handle.close()


def lockstep(a, lines):
    E = a.envs
    dims = synth.Dims(11, 3, T)
    hs = [dict(synth.make_history(dims, i), path_length=500) for i in range(E)]
    lines.append(f"== lock-step: action_sample_batch(lockstep=\"native\") of E = {E} windows, N {N} T {T} H {H}, {a.rounds} rounds x {a.calls} calls "
                 f"per leg, interleaved")
    for prec in ("bf16", "bf16x3"):
        legs = {"eval_tol=inf": _planner(dims, prec, native_step=True, eval_tol=INF, max_batch=E, max_windows=E),
                "no eval_tol": _planner(dims, prec, max_batch=E, max_windows=E)}
        call = lambda p: p.action_sample_batch(hs, eval=True, rtg=3.0, lockstep="native")
        for p in legs.values():  # calibration (the eval_tol planner calibrates inside its native calls) and warm-up, untimed
            for _ in range(max(4, -(-p._cal_windows // E) + 2) + 10):
                call(p)
            assert p._cal_left == 0
        torch.cuda.synchronize()
        per = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, p in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    call(p)
                torch.cuda.synchronize()
                per[k].append(1e3 * (time.perf_counter() - t0) / a.calls)
        base = med(per["no eval_tol"])
        lines.append(f"-- {prec}: delta {[round(float(p._delta), 6) for p in legs.values()]}")
        for k, p in legs.items():
            m = med(per[k])
            w = p.last["windows"]
            txt = (f"{k:14s} {m:8.4f} ms/call {1e3 * E / m:8.1f} plan-steps/s ({100.0 * (m / base - 1.0):+6.2f} % time vs no eval_tol; rounds "
                   f"{' '.join(f'{v:.4f}' for v in per[k])}); last call n_rescored {[x['n_rescored'] for x in w]}")
            if "eval_bound" in w[0]:
                txt += f" eval_bound max {max(x['eval_bound'] for x in w):.3e} eval_rounds {[x['eval_rounds'] for x in w]}"
            lines.append(txt)
        for p in legs.values():
            p.handle.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300, help="pipelined: plan steps per leg and round")
    ap.add_argument("--calls", type=int, default=40, help="lock-step: calls per leg and round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--envs", type=int, default=8, help="lock-step: E, windows per call")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_async_ab.py measures on a GPU: none is visible")
    lines = []
    for part in (pipelined, lockstep):
        done = len(lines)
        part(a, lines)
        print("\n".join(lines[done:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
