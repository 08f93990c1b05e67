"""Host-side mirror of the reference model interface (research/omtm/models/mtm_model.py:200-221,
324-437, 440-532, 593-607): ``omtmConfig.create(data_shapes, traj_length, discrete_map) -> omtm``,
``omtm.forward(trajectories, masks)`` and ``omtm.forward_loss(targets, preds, masks, ...)``.  The transformer
and the loss live in libm3pc_hip.so; the backward pass is m3pc_amd/mtm_grad.py (``DeviceMTMGrad``), the optimizers stay torch's.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Tuple

import torch

from . import capi
from .masks import mask_rows
from .tokenizers import SquashedNormal

KEYS = capi.KEYS
FORMS = ("finetune", "pretrain")


def early_return_keys(order) -> List[str]:
    """The keys Learner.compute_mtm_loss (finetune_omtm/learner.py:443-504) has in its dicts when it returns: its last lines sit
    inside the key loop, so it stops behind the first key that is not "actions" (which ``continue``s)."""
    out = []
    for k in order:
        out.append(k)
        if k != "actions":
            break
    return out


def key_bits(keys) -> int:
    """The 4-bit ``loss_keys`` mask of m3pc_mtm_loss*."""
    return sum(1 << KEYS.index(k) for k in set(keys))


def loss_tuple(record: torch.Tensor, dict_keys):
    """The reference's 5-tuple (loss, losses, masked_losses, masked_c_losses, entropy) out of a device record, as 0-d views of it:
    ``losses`` holds dict_keys in their order, then "entropy" and "nll"; the masked dicts hold dict_keys without "actions"."""
    losses, masked, masked_c = {}, {}, {}
    for k in dict_keys:
        i = 3 * KEYS.index(k)
        losses[k] = record[i]
        if k != "actions":
            masked[k] = record[i + 1]
            masked_c[k] = record[i + 2]
    losses["entropy"] = record[capi.MTM_ENTROPY]
    losses["nll"] = record[capi.MTM_NLL]
    return record[capi.MTM_TOTAL], losses, masked, masked_c, record[capi.MTM_ENTROPY]


def form_settings(form: str, order):
    """(flags, loss_keys bits, the keys of the returned dicts) of a reference form for a batch in key order ``order``: "finetune" is
    Learner.compute_mtm_loss (clip, no norm, the early return), "pretrain" omtm.forward_loss(norm="l2", loss_keys=None)."""
    if form == "finetune":
        keys = early_return_keys(order)
        return capi.MTM_CLIP_ACTIONS, key_bits(keys), keys
    if form == "pretrain":
        return capi.MTM_NORM_L2, key_bits(order), list(order)
    raise ValueError(f"form must be one of {FORMS}, got {form!r}")


def device_batch(handle, batch, eps=None, form: str = "finetune", flags=None, loss_keys=None):
    """A raw batch {key: (B,T,D_k)} as m3pc_mtm_grad / m3pc_mtm_train_step take it: -> (B, states, actions, rewards, returns, eps,
    returns_f64, flags, loss_keys): the tensors contiguous on the handle's device, float32 except returns that came as float64.  eps:
    (B,T,A) standard normals; None: torch.randn on the handle's device.  flags / loss_keys override those of ``form``."""
    order = list(batch.keys())
    if sorted(order) != sorted(KEYS):
        raise capi.M3pcError(f"the batch must hold exactly the keys {KEYS}")
    f, bits, _ = form_settings(form, order)
    f = f if flags is None else int(flags)
    bits = bits if loss_keys is None else int(loss_keys)
    h, dev = handle, handle.device
    B = int(batch["states"].shape[0])
    s, a, r = (h._f32(batch[k].to(dev)).reshape(B, h.T, -1) for k in ("states", "actions", "rewards"))
    v = batch["returns"].to(dev)
    v = v.contiguous() if v.dtype == torch.float64 else h._f32(v)
    if eps is None:
        eps = torch.randn((B, h.T, h.A), dtype=torch.float32, device=dev)
    e = h._f32(eps.to(dev)).reshape(B, h.T, h.A)
    return B, s, a, r, v, e, int(v.dtype == torch.float64), f, bits


def named_strict(tensors: Dict[str, torch.Tensor], device, what: str = ""):
    """{name: tensor} -> (NamedTensor array, keep-alives) for the calls that write to or read the caller's own storage: every tensor
    must be contiguous float32, on the host or on ``device`` (``capi._named`` converts instead).  what: prefix of the messages."""
    arr = (capi.NamedTensor * len(tensors))()
    keep = []
    for j, (k, t) in enumerate(tensors.items()):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise capi.M3pcError(f"{what}'{k}' must be a contiguous float32 tensor")
        if t.is_cuda and t.device != device:
            raise capi.M3pcError(f"{what}'{k}' lives on {t.device}, not on {device} or the host")
        nb = k.encode()
        keep.append(nb)
        arr[j] = capi.NamedTensor(nb, t.data_ptr(), t.numel(), 1 if t.is_cuda else 0)
    return arr, keep


def raw_batch_loss(handle, batch, masks, entropy_reg, form="finetune", eps=None, precision=capi.PREC_FP32, want_heads=False):
    """m3pc_mtm_loss on a raw batch dict {key: (B,T,D)} (``traj_sample``'s) under ``masks`` -> the reference's 5-tuple of ``form``
    (and the five head outputs with want_heads).  eps: (B,T,A) standard normals; None: torch.randn on the handle's device."""
    order = list(batch.keys())
    if sorted(order) != sorted(KEYS):
        raise capi.M3pcError(f"the batch must hold exactly the keys {KEYS}")
    flags, bits, keys = form_settings(form, order)
    B = batch["states"].shape[0]
    if eps is None:
        eps = torch.randn((B, handle.T, handle.A), dtype=torch.float32, device=handle.device)
    dev = [batch[k].to(handle.device) for k in KEYS]
    out = handle.mtm_loss(*[t.reshape(B, handle.T, -1) for t in dev], mask_rows(masks), eps.reshape(B, handle.T, handle.A),
                          float(entropy_reg), flags, bits, precision=precision, want_heads=want_heads)
    if want_heads:
        return loss_tuple(out[0], keys), out[1]
    return loss_tuple(out, keys)


@dataclasses.dataclass
class omtmConfig:
    """Field-for-field the reference dataclass (mtm_model.py:200-221); only the architecture fields
    matter at test time."""

    n_embd: int = 128
    n_head: int = 2
    n_enc_layer: int = 1
    n_dec_layer: int = 1
    dropout: float = 0
    embd_pdrop: float = 0
    resid_pdrop: float = 0
    attn_pdrop: float = 0
    norm: str = "l2"
    loss: str = "total"
    reduce_use_sum: bool = False
    loss_keys: Optional[List[str]] = None
    latent_dim: Optional[int] = None
    use_masked_loss: bool = False
    init_temperature: float = 0.1
    target_entropy: float = -3
    use_entropy: bool = True

    def create(self, data_shape, traj_length, discrete_map, **handle_kw):
        return omtm(data_shape, traj_length, discrete_map, self, **handle_kw)


class omtm:
    """Masked trajectory model on one MI355X: the forward pass and the training loss (no backward pass).

    ``data_shapes`` = {key: (tokens_per_timestep == 1, feature_dim)} (mtm_model.py:327-331).
    ``handle_kw`` sizes the device workspace: max_candidates, max_batch, critic_hidden, device.
    """

    def __init__(self, data_shapes: Dict[str, Tuple[int, ...]], traj_length: int, discrete_map: Dict[str, bool],
                 config: omtmConfig, max_candidates: int = 1024, max_batch: int = 1, critic_hidden: int = 256,
                 device: int = 0, precision: int = capi.PREC_FP32):
        if config.latent_dim is not None:
            raise capi.M3pcError("latent_dim is not used by any m3pc config and is not supported")
        if any(discrete_map.get(k, False) for k in KEYS):
            raise capi.M3pcError("discrete heads are not used by any m3pc config and are not supported")
        for k in KEYS:
            if k not in data_shapes or data_shapes[k][0] != 1:
                raise capi.M3pcError(f"data_shapes[{k!r}] must be (1, feature_dim)")
        if data_shapes["rewards"][1] != 1 or data_shapes["returns"][1] != 1:
            raise capi.M3pcError("rewards / returns are scalar per timestep")
        self.data_shapes = dict(data_shapes)
        self.config = config
        self.n_embd = config.n_embd
        self.max_len = traj_length
        self.precision = precision
        self.handle = capi.Handle(data_shapes["states"][1], data_shapes["actions"][1], traj_length, config.n_embd,
                                  config.n_head, config.n_enc_layer, config.n_dec_layer, max_candidates=max_candidates,
                                  max_batch=max_batch, critic_hidden=critic_hidden, device=device)
        self._sd: Dict[str, torch.Tensor] = {}

    # nn.Module-shaped conveniences used by the reference's callers (learner.py:32-36, finetune.py:298)
    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        self.handle.load_weights(state_dict)
        self._sd = {k: v.detach().clone() for k, v in state_dict.items()}
        return self

    def state_dict(self):
        return dict(self._sd)

    def eval(self):
        return self

    def to(self, device):
        return self

    @torch.no_grad()
    def forward(self, trajectories: Dict[str, torch.Tensor], masks) -> Dict[str, object]:
        """mtm_model.py:593-607.  trajectories[k]: (B,T,1,D_k) tokenised; masks[k]: (T,) or (T,1).
        Returns {k: (B,T,1,D_k)} in the input key order, ``SquashedNormal`` for "actions"."""
        keys = list(trajectories.keys())
        toks = []
        for k in KEYS:
            t = trajectories.get(k)
            if t is not None:
                assert t.dim() == 4 and t.shape[2] == 1, f"{k}: expected (B,T,1,D)"
                t = t[:, :, 0]
            toks.append(t)
        out = self.handle.forward(toks, mask_rows(masks), want=keys, precision=self.precision)
        res = {}
        for k in keys:
            if k == "actions":
                mu, sd = out[k]
                res[k] = SquashedNormal(mu.unsqueeze(2), sd.unsqueeze(2))
            else:
                res[k] = out[k].unsqueeze(2)
        return res

    __call__ = forward

    @torch.no_grad()
    def forward_loss(self, targets: Dict[str, torch.Tensor], preds: Dict[str, object], masks, entropy_reg: float,
                     discrete_map: Dict[str, bool], norm="l2", reduce_use_sum=False, loss_keys: Optional[List[str]] = None,
                     eps: Optional[torch.Tensor] = None):
        """mtm_model.py:440-532 on the device (m3pc_mtm_loss_terms): targets[k] (B,T,1,D_k) tokenised, preds as ``forward`` returns
        them.  Returns the reference's (loss, losses, masked_losses, masked_c_losses, entropy), 0-d device tensors.  ``eps``: the
        (B,T,A) standard normals of the sampled entropy (None: torch.randn).  norm: "l2", or anything else for none ("mae" changes
        nothing in the reference either: its normalised target is never used)."""
        if reduce_use_sum:
            raise capi.M3pcError("reduce_use_sum is not used by any m3pc config and is not supported")
        if any(discrete_map.get(k, False) for k in targets):
            raise capi.M3pcError("discrete heads are not used by any m3pc config and are not supported")
        order = list(targets.keys())
        if sorted(order) != sorted(KEYS):
            raise capi.M3pcError(f"targets must hold exactly the keys {KEYS}")
        h = self.handle
        B = targets["states"].shape[0]
        tg = [targets[k].reshape(B, h.T, -1) for k in KEYS]
        dist = preds["actions"]
        pr = [preds["states"], preds["rewards"], preds["returns"], dist.loc, dist.std]
        if eps is None:
            eps = torch.randn((B, h.T, h.A), dtype=torch.float32, device=h.device)
        rec = h.mtm_loss_terms([t.reshape(B, h.T, -1) for t in pr], tg, mask_rows(masks), eps.reshape(B, h.T, h.A), float(entropy_reg),
                               capi.MTM_NORM_L2 if norm == "l2" else 0, key_bits(order if loss_keys is None else loss_keys))
        return loss_tuple(rec, order)

    @torch.no_grad()
    def compute_loss(self, batch: Dict[str, torch.Tensor], masks, entropy_reg: float, form: str = "finetune",
                     eps: Optional[torch.Tensor] = None):
        """One call (m3pc_mtm_loss) on a RAW batch {key: (B,T,D_k)}: tokenise, ``forward`` under the masks, the loss of ``form`` --
        "finetune": Learner.compute_mtm_loss (finetune_omtm/learner.py:419-504), "pretrain": ``forward_loss(norm="l2")``.  Needs the
        handle's tokenizers (``handle.set_tokenizer``)."""
        return raw_batch_loss(self.handle, batch, masks, entropy_reg, form, eps, self.precision)
