"""The gradient of the masked-trajectory loss on the device (m3pc_mtm_grad*): the forward of ``Learner.compute_mtm_loss`` /
``omtm.forward_loss`` and ``loss.backward()`` through the whole model in one library call -- a raw batch in, one gradient tensor per
parameter out, under the reference's ``state_dict`` names.  The optimizers stay torch's.

The model differentiated is the eval-mode one until ``set_dropout(p, seed)`` switches on the four dropout sites of every transformer
layer of the training-mode model (the shipped configs train with ``dropout: 0.1``).  The keep-masks are the library's own
counter-based stream -- a pure function of (seed, draw, site, element), NOT torch's generator: a step is reproducible from
(seed, draw), not comparable mask for mask with ``model.train()`` under ``torch.manual_seed``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import capi
from .masks import mask_rows
from .mtm import device_batch, form_settings, loss_tuple, named_strict

KEYS = capi.KEYS


def param_shapes(S: int, A: int, d: int, n_enc_layer: int, n_dec_layer: int) -> Dict[str, tuple]:
    """name -> torch shape of every parameter the library differentiates (the model's state_dict without the buffer pos_embed)."""
    feat = dict(states=S, actions=A, rewards=1, returns=1)
    ff = 4 * d
    out = {}
    for k in KEYS:
        out[f"encoder_embed_dict.{k}.weight"] = (d, feat[k])
        out[f"encoder_embed_dict.{k}.bias"] = (d,)
        out[f"decoder_embed_dict.{k}.weight"] = (d, d)
        out[f"decoder_embed_dict.{k}.bias"] = (d,)
        out[f"mask_token_dict.{k}"] = (1, 1, d)
        out[f"encoder_per_dim_encoding.{k}"] = (1, 1, 1, d)
        out[f"decoder_per_dim_encoding.{k}"] = (1, 1, 1, d)
        if k == "actions":
            for part in ("mu", "log_std"):
                out[f"output_head_dict.actions.{part}.weight"] = (A, d)
                out[f"output_head_dict.actions.{part}.bias"] = (A,)
        else:
            out[f"output_head_dict.{k}.0.weight"] = (d,)
            out[f"output_head_dict.{k}.0.bias"] = (d,)
            out[f"output_head_dict.{k}.1.weight"] = (d, d)
            out[f"output_head_dict.{k}.1.bias"] = (d,)
            out[f"output_head_dict.{k}.3.weight"] = (feat[k], d)
            out[f"output_head_dict.{k}.3.bias"] = (feat[k],)
    for stack, n in (("encoder", n_enc_layer), ("decoder", n_dec_layer)):
        for i in range(n):
            p = f"{stack}.layers.{i}"
            out[p + ".self_attn.in_proj_weight"] = (3 * d, d)
            out[p + ".self_attn.in_proj_bias"] = (3 * d,)
            out[p + ".self_attn.out_proj.weight"] = (d, d)
            out[p + ".self_attn.out_proj.bias"] = (d,)
            out[p + ".linear1.weight"] = (ff, d)
            out[p + ".linear1.bias"] = (ff,)
            out[p + ".linear2.weight"] = (d, ff)
            out[p + ".linear2.bias"] = (d,)
            for nm in ("norm1", "norm2"):
                out[p + f".{nm}.weight"] = (d,)
                out[p + f".{nm}.bias"] = (d,)
        out[f"{stack}.norm.weight"] = (d,)
        out[f"{stack}.norm.bias"] = (d,)
    return out


class DeviceMTMGrad:
    """One m3pc_mtm_grad object on a planner's (or a bare ``capi.Handle``'s) device.  It reads the handle's fp32 weights and tokenizers
    at the time of each call and owns its workspace; the handle must outlive it.  Eval-mode model unless ``set_dropout`` says
    otherwise (module docstring)."""

    def __init__(self, planner_or_handle, max_batch: int):
        self.handle = getattr(planner_or_handle, "handle", planner_or_handle)
        self.lib = self.handle.lib
        self.device = self.handle.device
        self.max_batch = int(max_batch)
        dm = self.handle.dims
        self.shapes = param_shapes(dm.state_dim, dm.action_dim, dm.n_embd, dm.n_enc_layer, dm.n_dec_layer)
        self._g = C.c_void_p()
        capi.check(self.lib.m3pc_mtm_grad_create(self.handle._h, self.max_batch, C.byref(self._g)))

    def close(self):
        if getattr(self, "_g", None) is not None and self._g.value:
            with torch.cuda.device(self.device):
                self.lib.m3pc_mtm_grad_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return capi._stream(self.device)

    # -- dropout (host state: no device call) ---------------------------------------------------------
    def set_dropout(self, p: float, seed: int, draw: int = 0):
        """m3pc_mtm_grad_set_dropout: every later gradient call (this object's, and a trainer's on it) drops with probability ``p``
        under the keep-masks of (seed, draw) and advances ``draw`` by one.  p = 0 switches dropout off."""
        capi.check(self.lib.m3pc_mtm_grad_set_dropout(self._g, float(p), int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1)))

    def get_dropout(self):
        """-> (p, seed, next_draw): what the next gradient call will use."""
        p, seed, draw = C.c_double(), C.c_ulonglong(), C.c_ulonglong()
        capi.check(self.lib.m3pc_mtm_grad_get_dropout(self._g, C.byref(p), C.byref(seed), C.byref(draw)))
        return p.value, seed.value, draw.value

    # -- the calls ---------------------------------------------------------------------------------
    def grad_record(self, batch, masks, entropy_reg: float, form: str = "finetune", eps=None, flags=None, loss_keys=None) -> torch.Tensor:
        """m3pc_mtm_grad on a raw batch {key: (B,T,D_k)} (returns float32 or float64) under ``masks``; the gradients stay in the
        object (``export``).  flags / loss_keys override those of ``form``.  Returns the device record (15 floats)."""
        B, s, a, r, v, e, f64, f, bits = device_batch(self.handle, batch, eps, form, flags, loss_keys)
        rec = torch.empty(capi.MTM_LOSS_FLOATS, dtype=torch.float32, device=self.device)
        mp, keep = self.handle._mask_ptrs(mask_rows(masks))
        with torch.cuda.device(self.device):
            capi.check(self.lib.m3pc_mtm_grad(self._g, B, capi._ptr(s), capi._ptr(a), capi._ptr(r), capi._ptr(v), f64,
                                              mp, capi._ptr(e), float(entropy_reg), f, bits, capi._ptr(rec), self._stream()))
        del keep
        return rec

    def export(self, into: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """The gradients of the last call, each in the torch layout of its parameter.  into: {name: fp32 contiguous tensor, host or
        on the library's GPU} to write to (any subset of the parameters); None: new device tensors for every parameter."""
        if into is None:
            into = {k: torch.empty(s, dtype=torch.float32, device=self.device) for k, s in self.shapes.items()}
        arr, keep = named_strict(into, self.device, "export target ")
        with torch.cuda.device(self.device):
            capi.check(self.lib.m3pc_mtm_grad_export(self._g, arr, len(into), self._stream()))
            if any(not t.is_cuda for t in into.values()):
                torch.cuda.current_stream(self.device).synchronize()
        del keep
        return into

    def grad(self, batch, masks, entropy_reg: float, form: str = "finetune", eps=None):
        """-> (record, {name: device tensor}): the 15 floats of m3pc_mtm_loss and the gradient of its ``total`` with respect to every
        parameter ("finetune": Learner.compute_mtm_loss, "pretrain": omtm.forward_loss(norm="l2")).  With ``set_dropout``: of the
        dropped forward under the current draw."""
        rec = self.grad_record(batch, masks, entropy_reg, form, eps)
        return rec, self.export()

    def backward_into(self, module, batch, masks, entropy_reg: float, form: str = "finetune", eps=None, unused: str = "zero") -> torch.Tensor:
        """``loss.backward()`` for ``module``: sets ``.grad`` on the parameters ``module.state_dict(keep_vars=True)`` hands out under
        the names the library differentiates, and on nothing else (device to device when they live on the library's GPU).  Returns
        the device record.  The module's weights must be the handle's (``attach``'s ``_sync`` / ``load_weights``).
        unused: what the heads of the keys outside the form's loss_keys get -- "zero": the library's exact zeros; "none": ``.grad =
        None``, as the reference's backward leaves them (an optimizer with weight decay then skips them, as it does there)."""
        if unused not in ("zero", "none"):
            raise ValueError('unused must be "zero" or "none"')
        rec = self.grad_record(batch, masks, entropy_reg, form, eps)
        sd = module.state_dict(keep_vars=True)
        bits = form_settings(form, list(batch.keys()))[1]
        outside = tuple(f"output_head_dict.{k}." for j, k in enumerate(KEYS) if k != "actions" and not (bits >> j) & 1)
        targets, staged = {}, {}
        for name, shape in self.shapes.items():
            p = sd.get(name)
            if p is None or not getattr(p, "requires_grad", False):
                continue
            if unused == "none" and name.startswith(outside):
                p.grad = None
                continue
            if p.dtype == torch.float32 and (not p.is_cuda or p.device == self.device):
                g = torch.empty(p.shape, dtype=torch.float32, device=p.device)
                targets[name] = g
                p.grad = g
            else:  # another dtype or another GPU: through a device tensor of ours
                staged[name] = (p, torch.empty(shape, dtype=torch.float32, device=self.device))
                targets[name] = staged[name][1]
        self.export(targets)
        for name, (p, g) in staged.items():
            p.grad = g.reshape(p.shape).to(device=p.device, dtype=p.dtype)
        return rec


def loss_outputs(record: torch.Tensor, form: str, order=KEYS):
    """The reference's 5-tuple of ``form`` out of a record (m3pc_amd/mtm.py: loss_tuple)."""
    return loss_tuple(record, form_settings(form, list(order))[2])
