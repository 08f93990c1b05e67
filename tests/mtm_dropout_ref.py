"""Host mirror of the dropout keep masks of m3pc_mtm_grad* (m3pc_amd/csrc/mtm_grad.h, DROPOUT) on tests/variates_ref.philox4x32_10,
and the restatement of the gradient with them: tests/mtm_grad_ref.grads with ``oracle.mtm_oracle._block`` replaced, for the duration
of a call, by the training-mode block of nn.TransformerEncoderLayer(norm_first=True) under those masks.

Sites: 4 * layer + s, layers counted encoder first; s 0 the attention probabilities (B, nh, L, L), s 1 dropout1 on the out-proj output
(B L, d), s 2 the feed-forward's dropout on gelu(linear1) (B L, ff), s 3 dropout2 on the linear2 output (B L, d).
"""
import math
from unittest import mock

import numpy as np
import torch
import torch.nn.functional as F

import mtm_grad_ref as GR
import variates_ref as V
from oracle import mtm_oracle as O

ARRAY_MATRIX, ARRAY_ATTN = 5, 6
M64 = (1 << 64) - 1


def threshold(p):
    """thr = (uint32) floor(p 2^32), computed in double."""
    return int(math.floor(float(p) * 4294967296.0))


def scale(p):
    """(float)(1.0 / (1.0 - p)) as a Python float."""
    return float(np.float32(1.0 / (1.0 - float(p))))


def words(seed, draw, site, array, quad):
    """The four Philox words of every quad index in ``quad`` (uint64 array) -> (4, ...) uint32."""
    seed, draw = int(seed) & M64, int(draw) & M64
    key = (seed & V.MASK, (seed >> 32) & V.MASK)
    c3 = array | (int(site) << 8)
    w = V.philox4x32_10((quad, draw & V.MASK, (draw >> 32) & V.MASK, c3), key)
    return np.stack(w)


def keep(seed, draw, site, shape, p):
    """The keep mask of one site as a bool array of ``shape``: (R, C) a matrix site, (B, nh, L, L) the attention probabilities."""
    thr = threshold(p)
    if len(shape) == 2:
        R, C = shape
        r, c = np.meshgrid(np.arange(R, dtype=np.uint64), np.arange(C, dtype=np.uint64), indexing="ij")
        quad, word, array = (r >> np.uint64(2)) * np.uint64(C) + c, (r & np.uint64(3)).astype(np.int64), ARRAY_MATRIX
    else:
        B, nh, L, L2 = shape
        assert L == L2
        nq = (L + 3) // 4
        row = np.arange(B * nh * L, dtype=np.uint64).reshape(B, nh, L, 1)
        j = np.arange(L, dtype=np.uint64).reshape(1, 1, 1, L)
        quad, word, array = row * np.uint64(nq) + (j >> np.uint64(2)), (j & np.uint64(3)).astype(np.int64), ARRAY_ATTN
        quad, word = np.broadcast_arrays(quad, word)
    assert int(quad.max()) < (1 << 32)
    w = words(seed, draw, site, array, quad)
    sel = np.take_along_axis(w, word[None].astype(np.int64), axis=0)[0]
    return sel.astype(np.uint64) >= np.uint64(thr)


def dropped_block(p, seed, draw, n_enc, order=None):
    """A replacement for oracle.mtm_oracle._block: the same layer in training mode under keep(seed, draw, 4 layer + s, ...)."""
    sc = scale(p)

    def k(x, li, s, shape):
        if order is not None:
            order.append((li, s))
        m = keep(seed, draw, 4 * li + s, shape, p)
        return torch.as_tensor(m.astype(np.float64) * sc).to(x.dtype).reshape(x.shape)

    def block(x, sd, prefix, n_head):
        stack, _, idx = prefix.split(".")
        li = int(idx) + (n_enc if stack == "decoder" else 0)
        B, L, d = x.shape
        hd = d // n_head
        h = O._ln(x, sd, prefix + ".norm1")
        qkv = F.linear(h, sd[prefix + ".self_attn.in_proj_weight"], sd[prefix + ".self_attn.in_proj_bias"])
        q, kk, v = qkv.split(d, dim=-1)
        q = q.reshape(B, L, n_head, hd).transpose(1, 2) * (1.0 / math.sqrt(hd))
        kk = kk.reshape(B, L, n_head, hd).transpose(1, 2)
        v = v.reshape(B, L, n_head, hd).transpose(1, 2)
        pr = torch.softmax(q @ kk.transpose(-1, -2), dim=-1)
        pr = pr * k(pr, li, 0, (B, n_head, L, L))
        o = (pr @ v).transpose(1, 2).reshape(B, L, d)
        y = F.linear(o, sd[prefix + ".self_attn.out_proj.weight"], sd[prefix + ".self_attn.out_proj.bias"])
        x = x + y * k(y, li, 1, (B * L, d))
        h = O._ln(x, sd, prefix + ".norm2")
        h = F.gelu(F.linear(h, sd[prefix + ".linear1.weight"], sd[prefix + ".linear1.bias"]))
        h = h * k(h, li, 2, (B * L, h.shape[-1]))
        y = F.linear(h, sd[prefix + ".linear2.weight"], sd[prefix + ".linear2.bias"])
        return x + y * k(y, li, 3, (B * L, d))

    return block


def grads_dropout(sd, stats, batch, masks, eps, entropy_reg, flags, loss_keys, n_head, p, seed, draw, dtype=torch.float64, f32_clip=True,
                  order=None):
    """mtm_grad_ref.grads of the training-mode model under the keep masks of (p, seed, draw).  order: optional list that receives the
    (layer, s) of every mask in the order the forward applies them."""
    n_enc = O._n_layers(sd, "encoder")
    with mock.patch.object(O, "_block", dropped_block(p, seed, draw, n_enc, order)):
        return GR.grads(sd, stats, batch, masks, eps, entropy_reg, flags, loss_keys, n_head, dtype, f32_clip)


# The attention edge case of tests/test_mtm_dropout_kernel_edges_gpu.py: under this (seed, draw, site), at p = 0.5 and (B, nh, L) =
# (2, 2, 5), one attention row has every key dropped and one has every key kept (tests/test_mtm_dropout_cpu.py asserts it).
ATT_EDGE = dict(seed=7004, draw=2, site=8, B=2, nh=2, L=5, p=0.5)
