#!/usr/bin/env python3
"""A/B of the device gradient of the masked-trajectory loss (m3pc_mtm_grad) against what a user of the library does without it, in ONE
process on one box: forward + ``loss.backward()`` of one traj_sample batch (finetune_omtm/learner.py:506-538 without the optimizer
steps) from an idle device until the device is idle again, fp32, eval-mode model (no dropout on either side; `--dropout P` below), on the headline
dimensions (hopper: S = 11, A = 3; n_embd 512, 4 heads, 2 encoder layers, 1 decoder layer) at two shapes: batch 64 / T = 32 and
batch 512 / T = 8 (the shipped traj_batch_size).

  torch     torch-eager autograd through the restatement of the model and the loss (tests/mtm_grad_ref.py over oracle/mtm_oracle.py)
            on device tensors: tokenise, forward, loss, ``torch.autograd.grad`` for every parameter
  one call  DeviceMTMGrad.grad_record: tokenise, forward, loss record, backward -- the gradients stay in the object's buffers

Both legs read the same raw batch, masks and eps, and are checked against each other before anything is timed.  The legs alternate
call by call; a call is timed by the host clock from an idle device until the device is idle again.  There is no bar: the table is
recorded, whichever side wins.  `--out FILE` also writes the lines to a file (profiles/mtm_grad_ab.txt).  `--leg one` runs the library
leg alone at one shape (for a kernel trace of its launches).

`--dropout P` measures something else: the library leg alone, twice -- one object without dropout, one after set_dropout(P, seed) (the
library's own keep-mask stream) -- alternating call by call; what is recorded is the cost of the masks, with no bar.  In this mode
`--out FILE` APPENDS (profiles/mtm_dropout_ab.txt, shared with tools/mtm_train_ab.py --dropout)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mtm_grad_ref as GR  # noqa: E402
from m3pc_amd import capi, synth  # noqa: E402
from m3pc_amd.mtm_grad import DeviceMTMGrad  # noqa: E402
from oracle import mtm_oracle as O  # noqa: E402

S, A = 11, 3
SHAPES = ((64, 32), (512, 8))
q = lambda v, f: sorted(v)[min(len(v) - 1, int(f * len(v)))]


def setup(B, T):
    dims = synth.Dims(S, A, T, n_embd=512, n_head=4)
    hd = capi.Handle(S, A, T, n_embd=512, n_head=4, n_enc_layer=2, n_dec_layer=1, max_candidates=64, max_batch=1)
    sd = synth.make_state_dict(dims, 0)
    hd.load_weights(sd)
    stats = synth.make_tokenizer_stats(dims, 0)
    for k, (name, st) in enumerate(stats.items()):
        hd.set_tokenizer(k, st["mean"], st["std"], name != "actions")
    ostats = O.make_stats(stats)
    for st in ostats.values():
        st.mean, st.std = st.mean.to(hd.device), st.std.to(hd.device)
    g = torch.Generator(device=hd.device).manual_seed(1)
    batch = {"states": torch.randn((B, T, S), generator=g, device=hd.device), "actions": torch.rand((B, T, A), generator=g, device=hd.device) * 1.9 - 0.95,
             "rewards": torch.randn((B, T, 1), generator=g, device=hd.device),
             "returns": torch.randn((B, T, 1), generator=g, device=hd.device, dtype=torch.float64) * 3 + 5}
    eps = torch.randn((B, T, A), generator=g, device=hd.device)
    rng = np.random.RandomState(1)
    masks = {}
    for k in GR.KEYS:
        r = (rng.uniform(size=T) < 0.4).astype(np.float64)
        r[0], r[-1] = 1, 0
        masks[k] = r
    params = {k: v.to(hd.device).requires_grad_(k != "pos_embed") for k, v in sd.items()}
    return dims, hd, ostats, batch, eps, masks, params


def torch_leg(dims, ostats, batch, eps, masks, params, reg):
    names = GR.param_names(params)
    tokens = O.encode_all(batch, ostats)
    out = O.mtm_forward(params, tokens, masks, dims.n_head)
    total, _ = GR.loss_total(out, tokens, masks, eps, reg, *GR.FINETUNE, torch.float32, True)
    return total.detach(), dict(zip(names, torch.autograd.grad(total, [params[k] for k in names], allow_unused=True)))


def dropout_ab(a):
    lines = [f"MTM gradient, dropout {a.dropout} against none: one m3pc_mtm_grad from an idle device until it is idle again, two objects on one "
             f"handle, alternating call by call; S {S}, A {A}, n_embd 512, 4 heads, 2 + 1 layers, fp32; {a.calls} calls per leg after "
             f"{a.warmup} warm-up calls; ms per call; {torch.cuda.get_device_name(0)}"]
    for si, (B, T) in enumerate(SHAPES):
        if a.shape >= 0 and si != a.shape:
            continue
        dims, hd, ostats, batch, eps, masks, params = setup(B, T)
        objs = {"p = 0": DeviceMTMGrad(hd, B), f"p = {a.dropout}": DeviceMTMGrad(hd, B)}
        objs[f"p = {a.dropout}"].set_dropout(a.dropout, 1)
        per = {k: [] for k in objs}
        for i in range(a.warmup + a.calls):
            for k, obj in objs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = obj.grad_record(batch, masks, 0.1, "finetune", eps)
                torch.cuda.synchronize()
                if i >= a.warmup:
                    per[k].append(1e3 * (time.perf_counter() - t0))
                del out
        lines.append(f"B {B:4d}, T {T:3d}  {'leg':10s} {'median':>9s} {'p10':>9s} {'p90':>9s}")
        for k, v in per.items():
            lines.append(f"                 {k:10s} {q(v, 0.5):9.4f} {q(v, 0.1):9.4f} {q(v, 0.9):9.4f}")
        m0, m1 = (q(v, 0.5) for v in per.values())
        lines.append(f"                 dropout costs {m1 - m0:+.4f} ms per call ({100 * (m1 / m0 - 1):+.2f} %; recorded, no bar)")
        torch.cuda.synchronize()
        for obj in objs.values():
            obj.close()
        hd.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40, help="timed calls per leg (after warm-up)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default="both", choices=("both", "one"))
    ap.add_argument("--shape", type=int, default=-1, help="index into the two shapes; -1: both")
    ap.add_argument("--dropout", type=float, default=0.0, help="P > 0: the library leg with dropout P against without (module docstring)")
    a = ap.parse_args()
    if a.dropout > 0:
        lines = dropout_ab(a)
        print("\n".join(lines))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    reg = 0.1
    lines = [f"MTM gradient A/B: forward + backward of one batch from an idle device until it is idle again, torch-eager autograd through the "
             f"restatement [torch] against m3pc_mtm_grad [one call]; S {S}, A {A}, n_embd 512, 4 heads, 2 + 1 layers, fp32, no dropout; "
             f"{a.calls} interleaved calls per leg after {a.warmup} warm-up calls; ms per call; {torch.cuda.get_device_name(0)}"]
    for si, (B, T) in enumerate(SHAPES):
        if a.shape >= 0 and si != a.shape:
            continue
        dims, hd, ostats, batch, eps, masks, params = setup(B, T)
        obj = DeviceMTMGrad(hd, B)
        legs = {"one call": lambda: obj.grad_record(batch, masks, reg, "finetune", eps)}
        if a.leg == "both":
            legs = {"torch": lambda: torch_leg(dims, ostats, batch, eps, masks, params, reg), **legs}
            total, ref = legs["torch"]()
            rec = legs["one call"]()
            got = obj.export()
            torch.cuda.synchronize()
            worst = 0.0
            for n, g in ref.items():
                if g is None:
                    assert not got[n].any(), n
                    continue
                worst = max(worst, float((got[n].reshape(-1) - g.reshape(-1)).abs().max() / g.abs().max()))
            assert worst < 1e-3 and abs(float(rec[capi.MTM_TOTAL]) - float(total)) < 1e-3 * max(1.0, abs(float(total))), (worst, rec, total)
            lines.append(f"B {B}, T {T}: the two legs agree to {worst:.1e} (max over tensors of max |d| / max |g|)")
        per = {k: [] for k in legs}
        for i in range(a.warmup + a.calls):
            for k, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    per[k].append(1e3 * (time.perf_counter() - t0))
                del out
        lines.append(f"B {B:4d}, T {T:3d}  {'leg':10s} {'median':>9s} {'p10':>9s} {'p90':>9s}")
        for k, v in per.items():
            lines.append(f"                 {k:10s} {q(v, 0.5):9.4f} {q(v, 0.1):9.4f} {q(v, 0.9):9.4f}")
        if a.leg == "both":
            lines.append(f"                 one call / torch = {q(per['one call'], 0.5) / q(per['torch'], 0.5):.4f} (recorded, no bar)")
        torch.cuda.synchronize()
        obj.close()
        hd.close()
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
