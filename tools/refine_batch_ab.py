#!/usr/bin/env python3
"""A/B of the refinement of a lock-step batch of plans, in ONE process on one box: E calls of m3pc_refine_plan back to back (one
per window: what a caller had before m3pc_refine_plans) against ONE m3pc_refine_plans call over the E windows.

Two shapes, bf16 and fp32 scoring each: the shipped N = 625 / T = 8 / H = 4 shape and the headline shape (hopper, N = 1024,
H = 16, T = 32); E = 8 windows, top_k = 128, 2 iterations.  Both legs see the same handle, the same windows and the same pre-drawn
noise, write into preallocated outputs and alternate call by call, so that clock drift and neighbours on the box hit both alike.
A call is timed by the host clock from an idle device until the device is idle again.  The launches per iteration are counted in
a separate, untimed pass (kernel records of torch.profiler for a call of 3 iterations minus those of a call of 2; for the
sequential leg over all E calls); with --out a run that could not count them exits non-zero.

The batch call shares the policy chain and the short launches of an iteration among the windows, but its one scoring pass over
E x N rows with a window index gives up the first-layer sharing of history rows that a one-window m3pc_score_actions has: at the
shipped shape the batch must not be slower (the run exits non-zero with --out if it is), at the headline shape the number is
recorded whichever way it falls.  `--out FILE` also writes the lines to a file (profiles/refine_batch_ab.txt)."""
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
from tools.refine_ab import _kernel_count  # noqa: E402

SHAPES = [("shipped hopper N 625 H 4 T 8", 625, 4, 8, True), ("headline hopper N 1024 H 16 T 32", 1024, 16, 32, False)]
E, TOP_K, ITERATIONS = 8, 128, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300, help="timed calls per leg (after warm-up)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.calls >= 200, "the report's percentiles want at least 200 calls per leg"
    q = lambda v, f: sorted(v)[min(len(v) - 1, int(f * len(v)))]
    lines = [f"CEM refinement of E = {E} lock-step windows: {E} m3pc_refine_plan calls back to back [sequential] against one "
             f"m3pc_refine_plans call [batch]; top_k {TOP_K}, {ITERATIONS} iterations; {a.calls} interleaved calls per leg after "
             f"{a.warmup} warm-up calls; ms per call (all {E} windows) from an idle device until complete; {torch.cuda.get_device_name(0)}",
             f"{'shape':34s} {'prec':5s} {'leg':10s} {'median':>8s} {'p10':>8s} {'p90':>8s}  launches/iteration"]
    verdict = []
    for name, N, H, T, required in SHAPES:
        dims = synth.Dims(11, 3, T)
        A = dims.action_dim
        cfg = types.SimpleNamespace(traj_length=T, action_samples=N, horizon=H, discount=0.99, temperature=0.01, lmbda=0.6,
                                    plan_guidance="rtg_guiding")
        for prec in ("bf16", "fp32"):
            p = HipPlanner(cfg, synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), None, precision=prec, max_batch=E,
                           max_windows=E)
            hd, pc = p.handle, capi.precision_code(prec)
            parts = []
            for w in range(E):
                hist = synth.make_history(dims, w)
                hist["path_length"] = 500
                s, ac, r, h, _ = p.assemble_window(hist, rtg=3.0)
                parts.append((s.clone(), ac.clone(), r.clone()))
            s, ac, r = (torch.stack([x[i] for x in parts]).contiguous() for i in range(3))
            rtgs = [3.0 + 0.1 * w for w in range(E)]
            noise = torch.randn(ITERATIONS + 2, E, N, h, A, device="cuda", generator=torch.Generator(device="cuda").manual_seed(11))
            per_w = [noise[:, w].contiguous() for w in range(E)]
            f32 = dict(dtype=torch.float32, device="cuda")

            def outputs(shape_of, it):
                return dict(mean=torch.empty(shape_of(it + 1, h, A), **f32), std=torch.empty(shape_of(it + 1, h, A), **f32),
                            candidates=torch.empty(shape_of(None, N, h, A), **f32), scores=torch.empty(shape_of(it, N), **f32),
                            elites=torch.empty(shape_of(it, TOP_K), dtype=torch.int32, device="cuda"))

            one = lambda lead, *rest: tuple(v for v in (lead,) + rest if v is not None)
            many = lambda lead, *rest: ((E,) + rest) if lead is None else ((lead, E) + rest)
            outs = {it: ([dict(outputs(one, it), sample_action=torch.empty((1, A), **f32), eval_action=torch.empty((A,), **f32))
                          for _ in range(E)],
                         dict(outputs(many, it), sample_action=torch.empty((E, A), **f32), eval_action=torch.empty((E, A), **f32)))
                    for it in (ITERATIONS, ITERATIONS + 1)}

            def sequential(it=ITERATIONS):
                for w in range(E):
                    hd.refine_plan(capi.MODE_RTG, s[w], ac[w], r[w], h, rtgs[w], 0.6, 0.99, N, iterations=it, top_k=TOP_K,
                                   noise=per_w[w][: it + 1], precision=pc, out=outs[it][0][w])
                return outs[it][0]

            def batch(it=ITERATIONS):
                hd.refine_plans(capi.MODE_RTG, s, ac, r, h, rtgs, 0.6, 0.99, N, iterations=it, top_k=TOP_K, noise=noise[: it + 1],
                                precision=pc, out=outs[it][1])
                return outs[it][1]

            legs = {"sequential": sequential, "batch": batch}
            for _ in range(a.warmup):
                sequential()
                batch()
            torch.cuda.synchronize()
            per = {k: [] for k in legs}
            for _ in range(a.calls):
                for k, fn in legs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    per[k].append(1e3 * (time.perf_counter() - t0))
            print(f"{name} {prec}: sequential {q(per['sequential'], 0.5):.4f} ms, batch {q(per['batch'], 0.5):.4f} ms (medians)", flush=True)
            # what the two legs computed (same noise): the final means and the elite sets, window by window
            sq, bt = sequential(), batch()
            torch.cuda.synchronize()
            dmean = max(float((sq[w]["mean"] - bt["mean"][:, w]).abs().max()) for w in range(E))
            same_sets = sum(set(sq[w]["elites"][it].cpu().tolist()) == set(bt["elites"][it, w].cpu().tolist())
                            for w in range(E) for it in range(ITERATIONS))
            launches = {}
            for k, fn in legs.items():
                c2, c3 = _kernel_count(lambda: fn(ITERATIONS)), _kernel_count(lambda: fn(ITERATIONS + 1))
                launches[k] = None if c2 is None or c3 is None else c3 - c2
            for k in legs:
                v = per[k]
                lines.append(f"{name:34s} {prec:5s} {k:10s} {q(v, 0.5):8.4f} {q(v, 0.1):8.4f} {q(v, 0.9):8.4f}  "
                             f"{launches[k] if launches[k] is not None else 'not measured'}")
            ratio = q(per["batch"], 0.5) / q(per["sequential"], 0.5)
            lines.append(f"{'':34s} {prec:5s} batch / sequential = {ratio:.4f} ({100.0 * (ratio - 1.0):+.2f} %); max |mean batch - mean "
                         f"sequential| {dmean:.2e}; equal elite sets: {same_sets} of {E * ITERATIONS}")
            verdict.append((name, prec, ratio, required))
            p.handle.close()
    slow = [f"{n} {pr} ({r:.3f})" for n, pr, r, req in verdict if req and r > 1.0]
    lines.append("batch median <= sequential median at the shipped shape (the required bar)" if not slow
                 else "batch median ABOVE sequential median at the shipped shape: " + ", ".join(slow))
    for n, pr, r, req in verdict:
        if not req:
            lines.append(f"{n} {pr}: recorded, no bar: the batch call is {'faster' if r <= 1.0 else 'slower'} ({r:.3f})")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        if any("not measured" in ln for ln in lines):  # the table of record carries every column
            sys.exit("refine_batch_ab: the launches per iteration were not measured; the table written to --out is incomplete")
        if slow:
            sys.exit("refine_batch_ab: the batch call is slower than the sequential calls at the shipped shape")


if __name__ == "__main__":
    main()
