#!/usr/bin/env python3
"""Generate tests/golden/g11_mtm_dropout.npz by running the REAL reference on the CPU in TRAINING mode: ``loss.backward()`` behind
``Learner.compute_mtm_loss`` (the fine-tuning form) and behind ``omtm.forward_loss(norm="l2")`` (the pretraining form) on the g1_tiny
model, the batch, eps and masks of g8_mtm_loss.npz, with ``model.train()`` and ``dropout = p`` in both ``nn.TransformerEncoder`` stacks
-- under the keep masks of the library's own stream (tests/mtm_dropout_ref.keep), not torch's generator.

How the masks get in, without touching reference code or torch's layers:
  * ``torch.nn.functional.dropout`` is replaced for the duration of a run by a function that multiplies by ``keep(seed, draw, site,
    shape, p) * (float)(1 / (1 - p))``.  Which site a call is comes from forward pre-hooks on the modules of the real
    ``nn.TransformerEncoderLayer``: ``self_attn`` (s 0), ``dropout1`` (s 1), ``dropout`` (s 2), ``dropout2`` (s 3) of layer ``li``,
    layers counted encoder first.  So the real layer code decides which dropout runs where and in which order; the order is recorded
    (``{tag}/order``: the site ids in call order) and the CPU test asserts it is 0, 1, 2, 3 per layer.
  * the attention probabilities: with ``need_weights=False`` ``F.multi_head_attention_forward`` hands dropout_p to
    ``scaled_dot_product_attention``, whose kernel draws inside.  That name is looked up in ``torch.nn.functional``'s globals at call
    time, so it is replaced too, by softmax(q k^T / sqrt(hd)) -> the replaced ``F.dropout`` -> @ v.  This one site is therefore a
    restatement of the kernel's mathematics (torch documents exactly this formula for it); the call, its arguments (dropout_p = p, no
    mask, not causal) and its place in the layer are the real module's, and the script asserts that the replacement was reached.

Cases (the g8 batch; seed and draw below): ``ft_c0_p10`` the fine-tuning form on c0 at p = 0.1; ``ft_c0_p50`` the same at p = 0.5;
``pt_c3_p10`` the pretraining form on c3 (c2's masks and eps, the four +-1 actions at +-0.9: g9_mtm_grad_pretrain.npz) at p = 0.1.
Per case: ``p``, ``total32`` / ``total64``, ``order``, ``none``, ``ref32_grad_dev`` (per tensor: max |g32 - g64| / max |g64|),
``sums`` (float64 sum and sum of squares of each whole tensor), ``head/{name}`` (the leading 2048 entries of the float64 gradient,
rounded to float32); for the fine-tuning cases also ``ref32_grad_dev_f32clip`` (both runs on actions clipped beforehand to the
float32-rounded bounds: make_mtm_grad_golden.py explains why).  The file holds data only.

Usage:  python tests/golden/make_mtm_dropout_golden.py /path/to/reference
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_mtm_loss_golden as G  # noqa: E402  (parses the reference path and imports the reference)
import make_mtm_grad_golden as GG  # noqa: E402

import torch.nn.functional as F  # noqa: E402
from research.omtm.models.mtm_model import omtm  # noqa: E402

import mtm_dropout_ref as DR  # noqa: E402

SEED, DRAW = 20261021, 3
HEAD = 2048
CASES = (("ft_c0_p10", "c0", "finetune", 0.1), ("ft_c0_p50", "c0", "finetune", 0.5), ("pt_c3_p10", "c3", "pretrain", 0.1))


class LibraryMasks:
    """F.dropout and F.scaled_dot_product_attention replaced as the module docstring says, for one model."""

    def __init__(self, model, p):
        self.model, self.p, self.order, self.cur, self.sdpa_calls = model, p, [], None, 0

    def __enter__(self):
        me = self
        self.orig = (F.dropout, F.scaled_dot_product_attention)
        self.hooks = []
        layers = list(self.model.encoder.layers) + list(self.model.decoder.layers)
        for li, layer in enumerate(layers):
            for s, mod in enumerate((layer.self_attn, layer.dropout1, layer.dropout, layer.dropout2)):
                self.hooks.append(mod.register_forward_pre_hook(lambda m, a, site=4 * li + s: setattr(me, "cur", site)))

        def dropout(x, p=0.5, training=True, inplace=False):
            assert training and p == me.p and not inplace and me.cur is not None, (training, p, me.cur)
            site, me.cur = me.cur, None
            me.order.append(site)
            shape = tuple(x.shape) if site % 4 == 0 else (x.shape[0] * x.shape[1], x.shape[2])
            k = DR.keep(SEED, DRAW, site, shape, p).astype(np.float64) * DR.scale(p)
            return x * torch.from_numpy(k).to(x.dtype).reshape(x.shape)

        def sdpa(q, k, v, attn_mask=None, dropout_p=0.0, is_causal=False, **kw):
            assert attn_mask is None and not is_causal and dropout_p == me.p and not kw and q.dim() == 4 and me.cur % 4 == 0
            me.sdpa_calls += 1
            pr = torch.softmax((q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(q.shape[-1])), dim=-1)
            return F.dropout(pr, dropout_p, True) @ v

        F.dropout, F.scaled_dot_product_attention = dropout, sdpa
        return self

    def __exit__(self, *a):
        F.dropout, F.scaled_dot_product_attention = self.orig
        for h in self.hooks:
            h.remove()


def run(g8, mcase, form, p, dtype, actions=None):
    L = G.build(dtype)
    model = L.mtm.train()
    for layer in list(model.encoder.layers) + list(model.decoder.layers):
        for mod in (layer.dropout1, layer.dropout, layer.dropout2):
            mod.p = p
        layer.self_attn.dropout = p
    batch = {k: torch.from_numpy(g8["batch/" + k]) for k in G.R.KEYS}
    if actions is not None:
        batch["actions"] = torch.from_numpy(actions)
    T = G.DIMS.traj_length
    masks = {k: torch.from_numpy(g8[f"{mcase}/mask/{k}"].astype(np.float64)).reshape(T, 1) for k in G.R.KEYS}
    eps = torch.from_numpy(g8[f"{mcase}/eps"])[None, :, :, None, :]
    model.zero_grad(set_to_none=True)
    with torch.enable_grad(), LibraryMasks(model, p) as lm:
        if form == "finetune":
            with G.Eps(eps), G.FixedMasks(masks):
                loss = L.compute_mtm_loss(batch, G.DIMS.data_shapes, G.DISCRETE, G.ENTROPY_REG)[0]
        else:
            enc = L.tokenizer_manager.encode(batch)
            preds = model(enc, masks)
            with G.Eps(eps):
                loss = omtm.forward_loss(enc, preds, masks, G.ENTROPY_REG, G.DISCRETE, norm="l2", reduce_use_sum=False, loss_keys=None)[0]
        loss.backward()
    n_layers = G.DIMS.n_enc_layer + G.DIMS.n_dec_layer
    assert lm.sdpa_calls == n_layers and len(lm.order) == 4 * n_layers, (lm.sdpa_calls, lm.order)
    grads = {n: (None if q.grad is None else q.grad.detach().to(torch.float64).numpy().copy()) for n, q in model.named_parameters()}
    return float(loss), grads, np.array(lm.order)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    g8 = np.load(os.path.join(HERE, "g8_mtm_loss.npz"))
    names = [k for k in G.synth.make_state_dict(G.DIMS, 0) if k != "pos_embed"]
    out = {"grad_names": np.array(names), "torch_version": np.array(torch.__version__), "head": np.int64(HEAD), "seed": np.int64(SEED),
           "draw": np.int64(DRAW)}
    lo, hi = np.float32(-1 + 1e-6), np.float32(1 - 1e-6)
    for tag, case, form, p in CASES:
        mcase = "c2" if case == "c3" else case
        acts = GG.c3_actions(g8) if case == "c3" else None
        t32, g32, o32 = run(g8, mcase, form, p, torch.float32, acts)
        t64, g64, o64 = run(g8, mcase, form, p, torch.float64, acts)
        assert o32.tolist() == o64.tolist()
        pre = tag + "/"
        none = np.array([g64[n] is None for n in names])
        assert none.tolist() == [g32[n] is None for n in names]
        out[pre + "p"], out[pre + "total32"], out[pre + "total64"], out[pre + "order"] = np.float64(p), np.float64(t32), np.float64(t64), o64
        out[pre + "none"], out[pre + "ref32_grad_dev"] = none, GG.deviations(names, g32, g64)
        sums = np.zeros((len(names), 2))
        for i, n in enumerate(names):
            if none[i]:
                continue
            b = g64[n]
            sums[i] = b.sum(), (b * b).sum()
            out[pre + "head/" + n] = b.reshape(-1)[:HEAD].astype(np.float32)
        out[pre + "sums"] = sums
        if form == "finetune":
            pre_clipped = np.clip(g8["batch/actions"], lo, hi)
            _, c32, _ = run(g8, mcase, form, p, torch.float32, pre_clipped)
            _, c64, _ = run(g8, mcase, form, p, torch.float64, pre_clipped)
            out[pre + "ref32_grad_dev_f32clip"] = GG.deviations(names, c32, c64)
        dev = out[pre + "ref32_grad_dev"][~none]
        print(tag, "total64 %.6f  dev32: median %.2e max %.2e  none: %d  order: %s" % (t64, np.median(dev), dev.max(), none.sum(), o64.tolist()))
    path = os.path.join(HERE, "g11_mtm_dropout.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
