#!/usr/bin/env python3
"""A/B of the CEM refinement of a plan, in ONE process on one box: HipPlanner.cem_guiding(native=False) -- the Python loop
around m3pc_score_actions with torch.topk / gather / mean / std / clamp per iteration -- against native=True, one
m3pc_refine_plan call (refit and resample by the kernels of m3pc_amd/csrc/refine.hip).

Two shapes, bf16 and fp32 scoring each: the headline shape (hopper, N = 1024, H = 16, T = 32) and the shipped N = 625 / T = 8 /
H = 4 shape; top_k = 128, 2 iterations.  Both legs see the same planner, the same window and the same pre-drawn noise, and
alternate call by call so that clock drift and neighbours on the box hit both alike.  A call is timed by the host clock from an
idle device until the device is idle again.  The launches per iteration are counted in a separate, untimed pass (kernel records
of torch.profiler for a call of 3 iterations minus those of a call of 2); with --out a run that could not count them exits non-zero.

A report, not a gate: `--out FILE` also writes the lines to a file (profiles/refine_ab.txt)."""
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

SHAPES = [("headline hopper N 1024 H 16 T 32", 1024, 16, 32), ("shipped hopper N 625 H 4 T 8", 625, 4, 8)]
TOP_K, ITERATIONS = 128, 2


def _kernel_count(fn):
    """Device kernels one call of ``fn`` launches (None where the profiler gives no kernel records)."""
    try:
        from torch.profiler import ProfilerActivity, profile
    except ImportError as e:  # (a torch built without its profiler: the only failure that is not an error of this tool)
        print(f"(launch count not available: {e})")
        return None
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
            and "memset" not in e.name.lower())
    return n or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300, help="timed calls per leg (after warm-up)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.calls >= 200, "the report's percentiles want at least 200 calls per leg"
    dims_of = lambda T: synth.Dims(11, 3, T)
    q = lambda v, f: sorted(v)[min(len(v) - 1, int(f * len(v)))]
    lines = [f"CEM refinement, cem_guiding(native=False) [python loop] against native=True [one m3pc_refine_plan call]; top_k {TOP_K}, "
             f"{ITERATIONS} iterations; {a.calls} interleaved calls per leg after {a.warmup} warm-up calls; ms per call from an idle device "
             f"until complete; {torch.cuda.get_device_name(0)}",
             f"{'shape':34s} {'prec':5s} {'leg':7s} {'median':>8s} {'p10':>8s} {'p90':>8s}  launches/iteration"]
    verdict = []
    for name, N, H, T in SHAPES:
        dims = dims_of(T)
        cfg = types.SimpleNamespace(traj_length=T, action_samples=N, horizon=H, discount=0.99, temperature=0.01, lmbda=0.6,
                                    plan_guidance="rtg_guiding")
        hist = synth.make_history(dims, 0)
        hist["path_length"] = 500
        for prec in ("bf16", "fp32"):
            p = HipPlanner(cfg, synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), None, precision=prec)
            s, ac, r, h, rtg = p.assemble_window(hist, rtg=3.0)
            traj = {"states": s[None].clone(), "actions": ac[None].clone(), "rewards": r[None].clone(), "_rtg": rtg}
            noise = torch.randn(ITERATIONS + 2, N, h, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(11))
            call = lambda native, it=ITERATIONS: p.cem_guiding(traj, h, iterations=it, top_k=TOP_K, noise=noise[: it + 1], native=native)
            for _ in range(a.warmup):
                call(False)
                call(True)
            torch.cuda.synchronize()
            per = {False: [], True: []}
            for _ in range(a.calls):
                for native in (False, True):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call(native)
                    torch.cuda.synchronize()
                    per[native].append(1e3 * (time.perf_counter() - t0))
            print(f"{name} {prec}: python {q(per[False], 0.5):.4f} ms, native {q(per[True], 0.5):.4f} ms (medians)", flush=True)
            # what the two legs computed (same noise): the final mean and the elite sets
            call(False)
            py = [(t["mean"].clone(), set(t["top"].cpu().tolist())) for t in p.last["cem"]]
            call(True)
            nat = [(t["mean"].clone(), set(t["top"].cpu().tolist())) for t in p.last["cem"]]
            dmean = max(float((m0 - m1).abs().max()) for (m0, _), (m1, _) in zip(py, nat))
            same_sets = all(s0 == s1 for (_, s0), (_, s1) in zip(py, nat))
            launches = {}
            for native in (False, True):
                c2, c3 = _kernel_count(lambda: call(native, ITERATIONS)), _kernel_count(lambda: call(native, ITERATIONS + 1))
                launches[native] = None if c2 is None or c3 is None else c3 - c2
            for native in (False, True):
                v = per[native]
                lines.append(f"{name:34s} {prec:5s} {'native' if native else 'python':7s} {q(v, 0.5):8.4f} {q(v, 0.1):8.4f} {q(v, 0.9):8.4f}  "
                             f"{launches[native] if launches[native] is not None else 'not measured'}")
            ratio = q(per[True], 0.5) / q(per[False], 0.5)
            lines.append(f"{'':34s} {prec:5s} native / python = {ratio:.4f} ({100.0 * (ratio - 1.0):+.2f} %); max |mean native - mean python| "
                         f"{dmean:.2e}; same elite sets: {same_sets}")
            verdict.append((name, prec, ratio))
            p.handle.close()
    slow = [f"{n} {pr} ({r:.3f})" for n, pr, r in verdict if r > 1.0]
    lines.append("native median <= python median on every leg" if not slow else "native median ABOVE python median on: " + ", ".join(slow))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        if any("not measured" in ln for ln in lines):  # the table of record carries every column
            sys.exit("refine_ab: the launches per iteration were not measured; the table written to --out is incomplete")


if __name__ == "__main__":
    main()
