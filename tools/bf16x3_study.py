"""CPU emulation of the split-bf16 ("bf16x3", M3PC_PREC_BF16X3) candidate pass against fp32 and bf16.

The oracle's candidate pass (oracle/mtm_oracle.py) with every Linear of K % 32 == 0 computed as the x3 kernel does
(csrc/gemm_x3.hip): both operands split into x = hi + lo, hi = bf16(x), lo = bf16(x - hi) (round to nearest even), the product
taken as hi.hi + hi.lo + lo.hi, fp32 accumulation.  Everything else stays fp32: attention, LayerNorm, GELU, the K = 11 / 3 / 1
embeddings -- as in the HIP x3 pass, which keeps the fp32 pass structure.  The "bf16" mode is oracle/lowprec_study.py's (every
such Linear with bf16 operands): the reference point of the certified re-score.

Per mode: d_j = score_j - fp32 score_j over all N candidates, the common shift c = median(d), dev = |d - c| (rms, max), and
need = #{j : b_j > f* + c - 1.5 max dev} -- the candidates an arg-max certificate with that bound re-scores in fp32.
oracle/ is imported, not changed: the split linear is patched into O.F the way lowprec_study.scores patches its own.

    python tools/bf16x3_study.py [N] [seeds]      -> a markdown table on stdout (recipe weights, three seeds, and the
                                                     trained-like families of tests/test_certificate_gpu.py)
"""
from __future__ import annotations

import os
import sys
import types

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from m3pc_amd import synth  # noqa: E402
from oracle import lowprec_study as L  # noqa: E402
from oracle import mtm_oracle as O  # noqa: E402

# (linear_scale, returns_std_scale) of tests/test_certificate_gpu.py's trained-like families
TRAINED = [(1.0, 10.0), (1.5, 1.0), (2.0, 0.1), (2.0, 10.0), (4.0, 0.1), (4.0, 10.0)]


def split_bf16(x: torch.Tensor):
    hi = x.to(torch.bfloat16).to(torch.float32)
    lo = (x - hi).to(torch.bfloat16).to(torch.float32)
    return hi, lo


def make_x3_linear():
    """An F.linear stand-in with the x3 kernel's arithmetic (weights split once per tensor)."""
    cache = {}

    def linear(x, W, b=None):
        if W.shape[-1] % 32 != 0:  # (the tiny-K encoder embeddings: fp32 in the HIP x3 pass too)
            return F.linear(x, W, b)
        if id(W) not in cache:
            cache[id(W)] = (W, split_bf16(W))
        w_hi, w_lo = cache[id(W)][1]
        x_hi, x_lo = split_bf16(x)
        return F.linear(x_hi, w_hi) + F.linear(x_hi, w_lo) + F.linear(x_lo, w_hi) + (0.0 if b is None else b)

    return linear


def scores(sd, stats, cfg, win, h, acts, mode):
    if mode != "bf16x3":
        return L.scores(sd, stats, cfg, win, h, acts, mode)
    keep = O.F
    O.F = types.SimpleNamespace(linear=make_x3_linear(), layer_norm=F.layer_norm, gelu=F.gelu)
    try:
        return torch.cat([O.plan_candidates(sd, stats, cfg, win, h, acts[c0 : c0 + 256], "rtg", 0.6)
                          for c0 in range(0, acts.shape[0], 256)])
    finally:
        O.F = keep


def study(N: int, weight_seed: int, linear_scale: float = 0.0, returns_std_scale: float = 1.0, modes=("bf16", "bf16x3"),
          T: int = 32, H: int = 16):
    """Rows of (mode, shift, dev_rms, dev_max, need, argmax_match) for one weight set: the recipe of `weight_seed`, or, with
    linear_scale > 0, synth.trained_like of it."""
    dims = synth.Dims(11, 3, T)
    sd, st = synth.make_state_dict(dims, weight_seed), synth.make_tokenizer_stats(dims, weight_seed)
    if linear_scale > 0:
        sd, st = synth.trained_like(sd, st, seed=weight_seed, linear_scale=linear_scale, returns_std_scale=returns_std_scale)
    stats = O.make_stats(st)
    cfg = O.PlanCfg(T, H, N, 0.99, 0.01, 0.6)
    win, h = O.assemble_window(cfg, synth.make_history(dims, 0), 500, 3.0)
    eps = synth.make_eps(N, dims, 1)
    loc, std = O.policy_pass(sd, stats, cfg, win, h)
    acts = O.sample_candidates(loc, std, eps, T, h) if hasattr(O, "sample_candidates") else torch.tanh(loc + std * eps)[:, 0, T - h :, 0, :]
    with torch.no_grad():
        f = scores(sd, stats, cfg, win, h, acts, "fp32")
        fbest = float(f.max())
        rows = []
        for mode in modes:
            b = scores(sd, stats, cfg, win, h, acts, mode)
            d = b - f
            c = float(d.median())
            dev = (d - c).abs()
            delta = 1.5 * float(dev.max())
            rows.append(dict(mode=mode, shift=float(c), dev_rms=float(dev.pow(2).mean().sqrt()), dev_max=float(dev.max()),
                             need=int((b > fbest + c - delta).sum()), argmax_match=int(torch.argmax(b)) == int(torch.argmax(f)),
                             score_scale=float(f.abs().max())))
    return rows


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    seeds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    sets = [(f"recipe seed {s}", s, 0.0, 1.0) for s in range(seeds)]
    sets += [(f"trained-like x{ls:g} retstd x{rs:g} (seed {vi})", vi, ls, rs) for vi, (ls, rs) in enumerate(TRAINED)]
    print(f"| weights | mode | shift c | dev rms | dev max | need (of {N}) | arg-max = fp32 | max abs score |")
    print("|---|---|---|---|---|---|---|---|")
    for name, s, ls, rs in sets:
        for r in study(N, s, ls, rs):
            print(f"| {name} | {r['mode']} | {r['shift']:.3g} | {r['dev_rms']:.3g} | {r['dev_max']:.3g} | {r['need']} | "
                  f"{'yes' if r['argmax_match'] else 'NO'} | {r['score_scale']:.4g} |", flush=True)


if __name__ == "__main__":
    main()
