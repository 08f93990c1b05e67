#!/usr/bin/env python3
"""A/B of one whole training step of the masked-trajectory model, in ONE process on one box, from an idle device until the device is
idle again, fp32, eval-mode model (no dropout; `--dropout P` below), on the headline dimensions (hopper: S = 11, A = 3; n_embd 512, 4 heads, 2 encoder
layers, 1 decoder layer) at batch 64 / T = 32 and batch 512 / T = 8:

  route A   HipPlanner.mtm_update(sync=False) with torch's AdamW (two groups), LambdaLR and temperature Adam on a torch module that
            mirrors the model, then what attach's _sync does behind it: m3pc_load_weights of every tensor the step moved
  route B   one m3pc_mtm_train_step (DeviceMTMTrainer.train_step_record): gradient under the device temperature, AdamW, schedule,
            temperature, re-derivation -- the planner's own weights move, nothing crosses the host

The routes alternate call by call on two planners that start from the same weights.  Then the split: the gradient call alone
(DeviceMTMGrad.grad_record) and the optimizer half of route B alone (m3pc_mtm_opt_step: the AdamW launch, the temperature kernel and
the re-derivation), each from idle to idle.  The condition recorded: route B is not slower than route A.  `--out FILE` also writes
the lines to a file (profiles/mtm_train_ab.txt).  `--leg one` runs route B alone at one shape (for a kernel trace of its launches).

`--dropout P` measures something else: route B alone, twice -- one trainer without dropout, one with dropout P on the library's own
keep-mask stream (DeviceMTMTrainer(dropout=P)) -- alternating call by call from the same weights; what is recorded is the cost of the
masks, with no bar.  In this mode `--out FILE` APPENDS (profiles/mtm_dropout_ab.txt, shared with tools/mtm_grad_ab.py --dropout)."""
import argparse
import math
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from m3pc_amd import capi, synth  # noqa: E402
from m3pc_amd.mtm_train import DeviceMTMTrainer, decays  # noqa: E402
from m3pc_amd.planner import HipPlanner  # noqa: E402

S, A = 11, 3
SHAPES = ((64, 32), (512, 8))
KEYS = capi.KEYS
q = lambda v, f: sorted(v)[min(len(v) - 1, int(f * len(v)))]
HYPER = dict(learning_rate=1e-4, weight_decay=5e-3, num_train_steps=100000)


class Module(torch.nn.Module):
    """The model as a trainer holds it: Parameters under their state_dict names, pos_embed a buffer, the reference's temperature."""

    def __init__(self, sd, device):
        super().__init__()
        self.names = [k for k in sd if k != "pos_embed"]
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(sd[k].clone().to(device)) for k in self.names])
        self.register_buffer("pos", sd["pos_embed"].clone().to(device))
        self.log_temperature = torch.tensor(math.log(0.1), dtype=torch.float64, requires_grad=True)
        self.target_entropy = -float(A)
        self.config = types.SimpleNamespace(n_embd=512, n_head=4, n_enc_layer=2, n_dec_layer=1, dropout=0.0)

    def temperature(self):
        return self.log_temperature.exp()

    def state_dict(self, *a, keep_vars=False, **k):
        out = {n: (p if keep_vars else p.detach()) for n, p in zip(self.names, self.ps)}
        out["pos_embed"] = self.pos
        return out


def setup(B, T):
    dims = synth.Dims(S, A, T, n_embd=512, n_head=4)
    cfg = types.SimpleNamespace(traj_length=T, action_samples=64, horizon=4, discount=0.99, temperature=0.01, lmbda=0.6, plan_guidance="rtg_guiding",
                                device="cuda", mask_ratio=(0.5,), p_weights=(1.0,), **HYPER)
    sd, stats = synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0)
    mk = lambda: HipPlanner(cfg, sd, stats, None, n_embd=512, n_head=4, precision="fp32", max_batch=1, max_windows=1)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    batch = {"states": torch.randn((B, T, S), generator=g, device=dev), "actions": torch.rand((B, T, A), generator=g, device=dev) * 1.9 - 0.95,
             "rewards": torch.randn((B, T, 1), generator=g, device=dev), "returns": torch.randn((B, T, 1), generator=g, device=dev, dtype=torch.float64) * 3 + 5}
    eps = torch.randn((B, T, A), generator=g, device=dev)
    rng = np.random.RandomState(1)
    masks = {}
    for k in KEYS:
        r = (rng.uniform(size=T) < 0.4).astype(np.float64)
        r[0], r[-1] = 1, 0
        masks[k] = torch.from_numpy(r)
    return dims, sd, mk, batch, eps, masks


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = 1e3 * (time.perf_counter() - t0)
    del out
    return dt


def dropout_ab(a):
    """Route B without dropout against route B with dropout a.dropout: -> the lines."""
    lines = [f"MTM training step, dropout {a.dropout} against none: one m3pc_mtm_train_step from an idle device until it is idle again, two trainers "
             f"from the same weights, alternating call by call; S {S}, A {A}, n_embd 512, 4 heads, 2 + 1 layers, fp32; {a.calls} calls per leg "
             f"after {a.warmup} warm-up calls; ms per call; {torch.cuda.get_device_name(0)}"]
    for si, (B, T) in enumerate(SHAPES):
        if a.shape >= 0 and si != a.shape:
            continue
        dims, sd, mk, batch, eps, masks = setup(B, T)
        legs, per = {}, {}
        for name, p in (("p = 0", 0.0), (f"p = {a.dropout}", a.dropout)):
            pl = mk()
            tr = DeviceMTMTrainer(pl, B, dropout=p, dropout_seed=1, target_entropy=-float(A), init_log_temperature=math.log(0.1), **HYPER)
            legs[name], per[name] = (pl, tr), []
        for i in range(a.warmup + a.calls):
            for name, (pl, tr) in legs.items():
                dt = timed(lambda: tr.train_step_record(batch, masks, eps))
                if i >= a.warmup:
                    per[name].append(dt)
        lines.append(f"B {B:4d}, T {T:3d}  {'leg':26s} {'median':>9s} {'p10':>9s} {'p90':>9s}")
        for name, v in per.items():
            lines.append(f"                 {name:26s} {q(v, 0.5):9.4f} {q(v, 0.1):9.4f} {q(v, 0.9):9.4f}")
        m0, m1 = (q(v, 0.5) for v in per.values())
        lines.append(f"                 dropout costs {m1 - m0:+.4f} ms per step ({100 * (m1 / m0 - 1):+.2f} %; recorded, no bar); draws used: "
                     f"{legs[f'p = {a.dropout}'][1].grad.get_dropout()[2]}")
        torch.cuda.synchronize()
        for pl, tr in legs.values():
            tr.close()
            pl.handle.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30, help="timed calls per route (after warm-up)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default="both", choices=("both", "one"))
    ap.add_argument("--shape", type=int, default=-1, help="index into the two shapes; -1: both")
    ap.add_argument("--dropout", type=float, default=0.0, help="P > 0: route B with dropout P against route B without (module docstring)")
    a = ap.parse_args()
    if a.dropout > 0:
        lines = dropout_ab(a)
        print("\n".join(lines))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    lines = [f"MTM training-step A/B: one whole step from an idle device until it is idle again; route A = HipPlanner.mtm_update (device gradient, "
             f"torch AdamW + LambdaLR + temperature Adam) + the upload of the moved tensors (m3pc_load_weights), route B = one m3pc_mtm_train_step; "
             f"S {S}, A {A}, n_embd 512, 4 heads, 2 + 1 layers, fp32, no dropout; {a.calls} interleaved calls per route after {a.warmup} warm-up calls; "
             f"ms per call; {torch.cuda.get_device_name(0)}"]
    no = {k: False for k in KEYS}
    for si, (B, T) in enumerate(SHAPES):
        if a.shape >= 0 and si != a.shape:
            continue
        dims, sd, mk, batch, eps, masks = setup(B, T)
        pb = mk()
        tr = DeviceMTMTrainer(pb, B, target_entropy=-float(A), init_log_temperature=math.log(0.1), **HYPER)
        n_par = sum(int(np.prod(s)) for s in tr.shapes.values())
        n_gemm = sum(int(np.prod(s)) for n, s in tr.shapes.items() if len(s) == 2 and not n.startswith("encoder_embed_dict"))
        route_b = lambda: tr.train_step_record(batch, masks, eps)
        routes = {"route B": route_b}
        pa = None
        if a.leg == "both":
            pa = mk()
            model = Module(sd, pa.handle.device)
            named = dict(zip(model.names, model.ps))
            opt = torch.optim.AdamW([{"params": [p for n, p in named.items() if decays(n)], "weight_decay": HYPER["weight_decay"]},
                                     {"params": [p for n, p in named.items() if not decays(n)], "weight_decay": 0.0}],
                                    lr=HYPER["learning_rate"], betas=(0.9, 0.999))
            sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 0.5 * (1 + np.cos(s / HYPER["num_train_steps"] * np.pi)))
            topt = torch.optim.Adam([model.log_temperature], lr=1e-4, betas=[0.9, 0.999])
            moved = [n for n in model.names if not (n.startswith("output_head_dict.rewards.") or n.startswith("output_head_dict.returns."))]

            def route_a():
                log = pa.mtm_update(batch, None, no, model, opt, sched, topt, masks=masks, eps=eps, sync=False)
                pa.load_state_dict({n: named[n].detach() for n in moved})
                return log

            routes = {"route A": route_a, **routes}
        per = {k: [] for k in routes}
        for i in range(a.warmup + a.calls):
            for k, fn in routes.items():
                dt = timed(fn)
                if i >= a.warmup:
                    per[k].append(dt)
        lines.append(f"B {B:4d}, T {T:3d}  {'route':26s} {'median':>9s} {'p10':>9s} {'p90':>9s}      ({n_par} parameters, {n_gemm} of them in GEMM weights)")
        for k, v in per.items():
            lines.append(f"                 {k:26s} {q(v, 0.5):9.4f} {q(v, 0.1):9.4f} {q(v, 0.9):9.4f}")
        if a.leg == "both":
            ratio = q(per["route B"], 0.5) / q(per["route A"], 0.5)
            lines.append(f"                 route B / route A = {ratio:.4f}  ({'route B is not slower' if ratio <= 1.0 else 'ROUTE B IS SLOWER'})")
            # the split: the gradient call alone, and the optimizer half of route B alone
            grad, step = [], []
            for i in range(a.warmup + a.calls):
                dg = timed(lambda: tr.grad.grad_record(batch, masks, 0.1, "finetune", eps))
                ds = timed(tr.opt_step)
                if i >= a.warmup:
                    grad.append(dg)
                    step.append(ds)
            lines.append(f"                 {'m3pc_mtm_grad alone':26s} {q(grad, 0.5):9.4f} {q(grad, 0.1):9.4f} {q(grad, 0.9):9.4f}")
            lines.append(f"                 {'m3pc_mtm_opt_step alone':26s} {q(step, 0.5):9.4f} {q(step, 0.1):9.4f} {q(step, 0.9):9.4f}")
            lines.append(f"                 optimizer share: route A {q(per['route A'], 0.5) - q(grad, 0.5):.4f} ms (torch optimizers + upload), "
                         f"route B {q(per['route B'], 0.5) - q(grad, 0.5):.4f} ms")
        torch.cuda.synchronize()
        tr.close()
        pb.handle.close()
        if pa is not None:
            if getattr(pa, "_mtm_grad", None) is not None:
                pa._mtm_grad.close()
            pa.handle.close()
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
