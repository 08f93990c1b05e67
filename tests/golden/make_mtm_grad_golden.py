#!/usr/bin/env python3
"""Generate tests/golden/g9_mtm_grad.npz, g9_mtm_grad_finetune.npz and g9_mtm_grad_pretrain.npz by running the REAL reference on the CPU: ``loss.backward()``
behind ``Learner.compute_mtm_loss`` (finetune_omtm/learner.py:419-504, what mtm_update trains on, :506-538) and behind
``omtm.forward_loss(norm="l2")`` (omtm/models/mtm_model.py:440-532), on the g1_tiny model, batch, eps and mask cases c0, c1, c2 of
g8_mtm_loss.npz, with the ``Eps`` and ``FixedMasks`` devices of make_mtm_loss_golden.py (imported from it, so the usage is the same).
The model is in ``.eval()`` (no dropout), grad is enabled, and both forms run in float32 and in float64.

The g8 batch carries exact +1.0 / -1.0 target actions at timesteps 1, 2, 5 and 6.  Without the clip (the pretraining form) such an
action gives z = +-inf: at a hidden timestep the loss itself is NaN (c0, c1), at a visible one the loss is finite but autograd's
0 * inf makes every tensor upstream of mu NaN (c2: 71 of the 90 tensors).  So of the pretraining form the cases c0, c1, c2 pin only
the NaN structure and, for c2, the 19 tensors that are not upstream of mu.  Case c3 is what pins the pretraining backward: the masks
and eps of c2 on the same batch with those four actions moved to +-0.9 (``c3/actions``), finite in every tensor (the pretraining form alone).

Per case and form (prefix ``{case}/{form}/``): ``total32`` / ``total64``; ``ref32_grad_dev`` (per tensor, max |g32 - g64| / max |g64|:
the reference arithmetic's own float32 deviation; 0 where both are zero; NaN where the float64 gradient is not finite); ``none`` (per
tensor: .grad is None); ``sums`` ((n, 2): the float64 sum and sum of squares of each whole tensor).  For the fine-tuning form of c0, c1,
c2 also ``ref32_grad_dev_f32clip``: the same deviation from a pair of runs on the batch with its actions clipped beforehand to the
float32-rounded bounds (float)(-1 + 1e-6), (float)(1 - 1e-6).  The reference's float64 run clips at the float64 bounds and its float32
run at the rounded ones, so with an exact +-1 action at a hidden timestep (c1) ``ref32_grad_dev`` measures that difference of
definition, 1.6e-3, not float32 rounding; on the pre-clipped batch both runs clip at the same place.
The float64 run's gradients, rounded to float32: every tensor whole (``full/{name}``) for c2 of both forms and for c3 of the
pretraining form -- g9_mtm_grad.npz holds c2 / pretrain, g9_mtm_grad_finetune.npz c2 / finetune, g9_mtm_grad_pretrain.npz everything
of c3 (two whole gradients do not fit into one file under 1 MiB); for the other cases the leading 4096 entries of each flattened
tensor (``head/{name}``).  ``grad_names``: the tensors, in order.  The files hold data only.

Usage:  python tests/golden/make_mtm_grad_golden.py /path/to/reference
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_mtm_loss_golden as G  # noqa: E402  (parses the reference path and imports the reference)

from research.omtm.models.mtm_model import omtm  # noqa: E402

CASES = ("c0", "c1", "c2")
FULL_CASE = "c2"
HEAD = 4096


def c3_actions(g8):
    """The g8 actions with the four exact +-1 entries moved to +-0.9."""
    a = g8["batch/actions"].copy()
    a[np.abs(a) == 1.0] *= np.float32(0.9)
    assert np.abs(a).max() < 1.0 and (a != g8["batch/actions"]).sum() == 4
    return a


def run(g8, case, form, dtype, actions=None):
    """-> (total, {name: .grad as float64 ndarray or None}) of one backward pass of the reference.  case c3: the masks and eps of c2."""
    L = G.build(dtype)
    model = L.mtm
    assert not model.training
    batch = {k: torch.from_numpy(g8["batch/" + k]) for k in G.R.KEYS}
    if actions is not None:
        batch["actions"] = torch.from_numpy(actions)
    T = G.DIMS.traj_length
    mcase = "c2" if case == "c3" else case
    masks = {k: torch.from_numpy(g8[f"{mcase}/mask/{k}"].astype(np.float64)).reshape(T, 1) for k in G.R.KEYS}
    eps = torch.from_numpy(g8[f"{mcase}/eps"])[None, :, :, None, :]
    model.zero_grad(set_to_none=True)
    with torch.enable_grad():
        if form == "finetune":
            with G.Eps(eps), G.FixedMasks(masks):
                loss = L.compute_mtm_loss(batch, G.DIMS.data_shapes, G.DISCRETE, G.ENTROPY_REG)[0]
        else:
            enc = L.tokenizer_manager.encode(batch)
            preds = model(enc, masks)
            with G.Eps(eps):
                loss = omtm.forward_loss(enc, preds, masks, G.ENTROPY_REG, G.DISCRETE, norm="l2", reduce_use_sum=False, loss_keys=None)[0]
        loss.backward()
    grads = {n: (None if p.grad is None else p.grad.detach().to(torch.float64).numpy().copy()) for n, p in model.named_parameters()}
    return float(loss), grads


def deviations(names, g32, g64):
    dev = np.zeros(len(names))
    for i, n in enumerate(names):
        a, b = g32[n], g64[n]
        if b is None:
            continue
        top = np.abs(b).max()
        dev[i] = 0.0 if top == 0 and np.abs(a).max() == 0 else np.abs(a - b).max() / top
    return dev


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    g8 = np.load(os.path.join(HERE, "g8_mtm_loss.npz"))
    names = [k for k in G.synth.make_state_dict(G.DIMS, 0) if k != "pos_embed"]
    out = {"grad_names": np.array(names), "torch_version": np.array(torch.__version__), "head": np.int64(HEAD)}
    out2 = {"grad_names": np.array(names)}
    out3 = {"grad_names": np.array(names), "c3/actions": c3_actions(g8)}
    lo, hi = np.float32(-1 + 1e-6), np.float32(1 - 1e-6)
    for case in CASES + ("c3",):
        for form in (("pretrain",) if case == "c3" else ("finetune", "pretrain")):
            acts = out3["c3/actions"] if case == "c3" else None
            dst = out3 if case == "c3" else out
            t32, g32 = run(g8, case, form, torch.float32, acts)
            t64, g64 = run(g8, case, form, torch.float64, acts)
            extra = sorted(set(g64) - set(names))
            assert all(g64[n] is None for n in extra), extra  # (log_temperature: entropy_reg comes in detached)
            assert set(names) <= set(g64), sorted(set(names) - set(g64))
            pre = f"{case}/{form}/"
            dst[pre + "total32"], dst[pre + "total64"] = np.float64(t32), np.float64(t64)
            none = np.array([g64[n] is None for n in names])
            assert none.tolist() == [g32[n] is None for n in names]
            dev = deviations(names, g32, g64)
            sums = np.zeros((len(names), 2))
            for i, n in enumerate(names):
                if none[i]:
                    continue
                b = g64[n]
                sums[i] = b.sum(), (b * b).sum()
                if case == FULL_CASE:
                    (out if form == "pretrain" else out2)[pre + "full/" + n] = b.astype(np.float32)
                elif case == "c3" and form == "pretrain":
                    out3[pre + "full/" + n] = b.astype(np.float32)
                else:
                    dst[pre + "head/" + n] = b.reshape(-1)[:HEAD].astype(np.float32)
            dst[pre + "none"], dst[pre + "ref32_grad_dev"], dst[pre + "sums"] = none, dev, sums
            if form == "finetune" and case != "c3":  # both runs clip at the same, float32-rounded, bounds
                pre_clipped = np.clip(g8["batch/actions"], lo, hi)
                _, c32 = run(g8, case, form, torch.float32, pre_clipped)
                _, c64 = run(g8, case, form, torch.float64, pre_clipped)
                dst[pre + "ref32_grad_dev_f32clip"] = deviations(names, c32, c64)
                print(case, form, "ref32_grad_dev_f32clip: median %.2e max %.2e" % (np.median(dst[pre + "ref32_grad_dev_f32clip"][~none]),
                                                                                   dst[pre + "ref32_grad_dev_f32clip"][~none].max()))
            ok = np.isfinite(dev) & ~none
            print(case, form, "total64 %.6f  dev32: median %.2e max %.2e  none: %d  finite: %s" % (
                t64, np.median(dev[ok]) if ok.any() else np.nan, dev[ok].max() if ok.any() else np.nan, none.sum(), np.isfinite(t64)))
    for name, o in (("g9_mtm_grad.npz", out), ("g9_mtm_grad_finetune.npz", out2), ("g9_mtm_grad_pretrain.npz", out3)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **o)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
