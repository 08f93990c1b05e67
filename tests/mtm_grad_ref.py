"""Torch restatement of the gradient of the masked-trajectory loss (include/m3pc_hip.h: m3pc_mtm_grad*): autograd through
``oracle.mtm_oracle.mtm_forward`` and the loss of the header written in torch ops, in float64 or float32.

``mtm_forward`` casts the tokens to float32 in front of the encoder embedding, so in the float64 run the four
``encoder_embed_dict.*`` Linears stay float32 (the reference's float64 run in tests/golden/make_mtm_grad_golden.py does the same) and
their gradients come out in float32.

Held constant, as the header says: the tokenised targets (the l2-normalised ones too), the clipped action and its z, entropy_reg,
the masks.  u = mu + std eps is differentiated through mu and std.
"""
import math

import numpy as np
import torch

from oracle import mtm_oracle as O

KEYS = ("states", "actions", "rewards", "returns")
NORM_L2, CLIP_ACTIONS = 1, 2
FINETUNE = (CLIP_ACTIONS, 1)
PRETRAIN = (NORM_L2, 15)
FORMS = {"finetune": FINETUNE, "pretrain": PRETRAIN}
LOG_SQRT_2PI = math.log(math.sqrt(2 * math.pi))
LOG2 = math.log(2.0)


def param_names(sd):
    return [k for k in sd if k != "pos_embed"]


def cast_state_dict(sd, dtype):
    """Leaf tensors of ``dtype`` (the encoder embedding stays float32); everything but pos_embed requires grad."""
    out = {}
    for k, v in sd.items():
        dt = torch.float32 if k.startswith("encoder_embed_dict.") else dtype
        out[k] = torch.as_tensor(np.asarray(v)).detach().clone().to(dt).requires_grad_(k != "pos_embed")
    return out


def _log_prob(x, mu, sd):
    return -((x - mu) ** 2) / (2.0 * sd * sd) - torch.log(sd) - LOG_SQRT_2PI


def _ladj(x):
    return 2.0 * (LOG2 - x - torch.nn.functional.softplus(-2.0 * x))


def loss_total(out, tokens, masks, eps, entropy_reg, flags, loss_keys, dtype, f32_clip=True):
    """``total`` of the header from mtm_forward's outputs.  tokens[k] (B,T,1,D) float32; masks[k] (T,) 0/1; eps (B,T,A)."""
    total = 0.0
    parts = {}
    for j, k in enumerate(KEYS):
        if k == "actions":
            continue
        t = tokens[k].to(dtype)
        if flags & NORM_L2:
            t = t / torch.sqrt((t * t).sum(dim=-1, keepdim=True))
        parts[k] = ((out[k] - t.detach()) ** 2).mean()
    mu, sd = out["actions"]
    a = tokens["actions"].to(dtype)
    ma = torch.as_tensor(np.asarray(masks["actions"], np.float64)).to(dtype).reshape(1, -1, 1, 1).to(mu.device)
    parts["actions"] = ((torch.tanh(mu) - a) ** 2 * ma).mean()
    ac = a
    if flags & CLIP_ACTIONS:
        lo, hi = (float(np.float32(-1 + 1e-6)), float(np.float32(1 - 1e-6))) if f32_clip else (-1 + 1e-6, 1 - 1e-6)
        ac = torch.clip(a, lo, hi)
    z = (0.5 * (torch.log1p(ac) - torch.log1p(-ac))).detach()
    lp = _log_prob(z, mu, sd) - _ladj(z)
    u = mu + sd * eps.to(dtype).reshape(mu.shape)
    lq = _log_prob(u, mu, sd) - _ladj(u)
    hidden = torch.as_tensor(np.asarray(masks["actions"]).reshape(-1) == 0)
    ll = lp[:, hidden].mean()
    ent = -lq[:, hidden].mean()
    for j, k in enumerate(KEYS):
        if (loss_keys >> j) & 1:
            total = total + parts[k]
    total = total - (ll + float(entropy_reg) * ent)
    return total, dict(parts, entropy=ent, nll=-ll)


def tokens_of(batch, stats):
    """The tokenised batch: {k: (B,T,1,D) float32} (returns normalised in float64 first, as the reference does)."""
    return O.encode_all({k: torch.as_tensor(np.asarray(batch[k])) for k in KEYS}, stats)


def grads(sd, stats, batch, masks, eps, entropy_reg, flags, loss_keys, n_head, dtype=torch.float64, f32_clip=True):
    """-> (total as a float, {name: float64 ndarray in the parameter's shape, or None where autograd reaches nothing})."""
    p = cast_state_dict(sd, dtype)
    tokens = tokens_of(batch, stats)
    m = {k: np.asarray(masks[k], np.float64).reshape(-1) for k in KEYS}
    out = O.mtm_forward(p, tokens, m, n_head)
    total, _ = loss_total(out, tokens, m, torch.as_tensor(np.asarray(eps)), entropy_reg, flags, loss_keys, dtype, f32_clip)
    names = param_names(p)
    gs = torch.autograd.grad(total, [p[k] for k in names], allow_unused=True)
    return float(total.detach()), {k: None if g is None else g.detach().to(torch.float64).numpy() for k, g in zip(names, gs)}


def deviation(g, g64):
    """max |g - g64| / max |g64| of one tensor (None counts as zeros); 0 / 0 is 0."""
    a = np.zeros_like(g64) if g is None else np.asarray(g, np.float64).reshape(g64.shape)
    top = np.abs(g64).max() if g64.size else 0.0
    diff = np.abs(a - g64).max() if g64.size else 0.0
    if top == 0.0:
        return 0.0 if diff == 0.0 else np.inf
    return float(diff / top)


def zeros_where_none(gd, shapes=None):
    return {k: (np.zeros(shapes[k]) if v is None else v) for k, v in gd.items()}
