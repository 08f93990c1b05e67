#!/usr/bin/env python3
"""A/B of the masked-trajectory loss (m3pc_mtm_loss) against what a user of the library did before it existed, in ONE process on one
box: the validation loss of one traj_sample batch (finetune_omtm/learner.py:419-504) from an idle device until the device is idle
again, at the fine-tuning loop's shape -- batch 64, T = 32 -- on the headline dimensions (hopper: S = 11, A = 3; n_embd 512, 4 heads,
2 encoder layers, 1 decoder layer), fp32.

  torch     Handle.tokenize x 4, Handle.forward under the masks, then the reference's loss restated in torch ops on the device tensors
            (MSE terms with the three reductions for `states`, the clip, atanh, Normal.log_prob, the tanh Jacobian, the sampled
            entropy, the total)
  one call  Handle.mtm_loss: tokenise, forward, two loss launches, one 15-float record

Both legs read the same raw batch, masks and eps, and are checked against each other before anything is timed.  The legs alternate
call by call (clock drift and neighbours on the box hit them alike); a call is timed by the host clock from an idle device until the
device is idle again.  Nobody has measured either side before, so there is no bar: the table is recorded.  `--out FILE` also writes
the lines to a file (profiles/mtm_loss_ab.txt)."""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from m3pc_amd import capi, synth  # noqa: E402

S, A, T, B = 11, 3, 32, 64
q = lambda v, f: sorted(v)[min(len(v) - 1, int(f * len(v)))]


def torch_loss(hd, batch, masks, eps, reg):
    """The fine-tuning form in torch ops: (total, loss_states, masked_loss_states, masked_c_loss_states, entropy, nll)."""
    tok = [hd.tokenize(k, batch[k]) for k in range(4)]
    out = hd.forward(tok, masks)
    m = [torch.tensor(r, dtype=torch.float32, device=hd.device) for r in masks]
    raw = (out["states"] - tok[0]) ** 2
    ms = m[0][None, :, None]
    loss_s = raw.mean()
    masked_c = ((raw * ms).sum(dim=(1, 2)) / m[0].sum()).mean()
    masked = ((raw * (1 - ms)).sum(dim=(1, 2)) / (1 - m[0]).sum()).mean()
    mu, sd = out["actions"]
    a = tok[1].clip(-1 + 1e-6, 1 - 1e-6)
    z = 0.5 * (a.log1p() - (-a).log1p())

    def log_prob(x):
        normal = -((x - mu) ** 2) / (2 * sd ** 2) - sd.log() - math.log(math.sqrt(2 * math.pi))
        return normal - 2.0 * (math.log(2.0) - x - torch.nn.functional.softplus(-2.0 * x))

    hidden = m[1] == 0
    ll = log_prob(z)[:, hidden, :].mean()
    ent = -log_prob(mu + eps * sd)[:, hidden, :].mean()
    return torch.stack([loss_s - (ll + reg * ent), loss_s, masked, masked_c, ent, -ll])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300, help="timed calls per leg (after warm-up)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dims = synth.Dims(S, A, T, n_embd=512, n_head=4)
    hd = capi.Handle(S, A, T, n_embd=512, n_head=4, n_enc_layer=2, n_dec_layer=1, max_candidates=64, max_batch=B)
    hd.load_weights(synth.make_state_dict(dims, 0))
    for k, (name, st) in enumerate(synth.make_tokenizer_stats(dims, 0).items()):
        hd.set_tokenizer(k, st["mean"], st["std"], name != "actions")
    g = torch.Generator(device=hd.device).manual_seed(1)
    batch = [torch.randn((B, T, S), generator=g, device=hd.device), torch.rand((B, T, A), generator=g, device=hd.device) * 1.9 - 0.95,
             torch.randn((B, T, 1), generator=g, device=hd.device), torch.randn((B, T, 1), generator=g, device=hd.device, dtype=torch.float64) * 3 + 5]
    eps = torch.randn((B, T, A), generator=g, device=hd.device)
    rng = np.random.RandomState(1)
    masks = []
    for _ in range(4):
        r = (rng.uniform(size=T) < 0.4).astype(np.uint8)
        r[0], r[-1] = 1, 0
        masks.append(r.tolist())
    reg = 0.1
    legs = {"torch": lambda: torch_loss(hd, batch, masks, eps, reg),
            "one call": lambda: hd.mtm_loss(*batch, masks, eps, reg, capi.MTM_CLIP_ACTIONS, 1)}
    ref, rec = legs["torch"]().cpu().numpy(), legs["one call"]().cpu().numpy()
    got = rec[[capi.MTM_TOTAL, 0, 1, 2, capi.MTM_ENTROPY, capi.MTM_NLL]]
    dev = np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)
    assert dev.max() < 1e-3, (got, ref)
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
    lines = [f"MTM loss A/B: the validation loss of one batch from an idle device until it is idle again, Handle.tokenize + Handle.forward + "
             f"the loss in torch ops [torch] against m3pc_mtm_loss [one call]; B {B}, T {T}, S {S}, A {A}, n_embd 512, fp32; {a.calls} "
             f"interleaved calls per leg after {a.warmup} warm-up calls; ms per call; {torch.cuda.get_device_name(0)}",
             f"the two legs agree to {dev.max():.1e} (relative, on total / loss_states / masked / masked_c / entropy / nll)",
             f"{'leg':10s} {'median':>9s} {'p10':>9s} {'p90':>9s}"]
    for k, v in per.items():
        lines.append(f"{k:10s} {q(v, 0.5):9.4f} {q(v, 0.1):9.4f} {q(v, 0.9):9.4f}")
    lines.append(f"one call / torch = {q(per['one call'], 0.5) / q(per['torch'], 0.5):.4f} (recorded, no bar)")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    torch.cuda.synchronize()
    hd.close()


if __name__ == "__main__":
    main()
