#!/usr/bin/env python3
"""Generate tests/golden/g8_mtm_loss.npz by running the REAL reference on the CPU: ``Learner.compute_mtm_loss``
(finetune_omtm/learner.py:419-504) and ``omtm.forward_loss(norm="l2")`` (omtm/models/mtm_model.py:440-532) on the g1_tiny model
(m3pc_amd.synth, dims 11 / 3 / 8 / 64 / 2, seed 0), once in float32 and once in float64.

Runs only where the reference checkout exists (pass its path, or set M3PC_REFERENCE); the .npz written here is data only.  The
reference is imported unmodified with empty stub modules for ``wandb`` and ``gym``; the Learner is built with ``object.__new__``, as
tests/golden/make_golden.py does.

How things are made explicit, without touching reference code:
  * eps: ``SquashedNormal.entropy`` draws through ``Normal.rsample``, which calls ``torch.distributions.normal._standard_normal``;
    that name is wrapped for the duration of a call to RECORD what it returns (the float32 run of the fine-tuning form) or to hand
    the recorded array back (every other run of the same mask case), and ``Normal.rsample`` is wrapped to assert that what it
    returns is loc + eps * scale on the recorded eps, bit for bit;
  * masks: the two drawn cases run under ``np.random.seed(seed)`` (the seeds are stored; each was searched for visible and hidden
    tokens in every key); the hand-made case replaces the name ``create_random_autoregressize_mask`` in the learner module;
  * float64: ``model.double()``, with the tokenised batch (which ``ContinuousTokenizer.encode`` always casts to float32) widened in
    front of it -- the float64 run therefore sees the float32 run's targets, in float64 arithmetic from there on.  One module stays
    float32, the input embedding, whose input ``trajectory_encoding`` casts to float32 (mtm_model.py:550); its sum with the float64
    encodings is float64.  That moves the float64 run's head outputs, which are stored, and nothing of the loss arithmetic.

Contents: the raw batch (B = 3; returns float64; target actions with an exact +1.0 and an exact -1.0), entropy_reg, and per mask case
c0, c1 (drawn), c2 (hand-made, rewards fully visible): the four masks, eps, the tokenised targets, the five head outputs of both runs,
and the records of both forms in both runs (tests/mtm_loss_ref.py: RECORD_NAMES; a slot the reference does not compute is NaN in
"have").  Then eight (seed -> four masks) pairs for the mask mirror.

Usage:  python tests/golden/make_mtm_loss_golden.py /path/to/reference
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("M3PC_REFERENCE")
if not REFERENCE or not os.path.isdir(os.path.join(REFERENCE, "research")):
    sys.exit("usage: make_mtm_loss_golden.py /path/to/reference  (the checkout that holds research/finetune_omtm/learner.py)")
for _name in ("wandb", "gym"):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules["gym"].Env = object
sys.path.insert(0, REFERENCE)

import torch.distributions.normal as tdn  # noqa: E402
from research.finetune_omtm import learner as learner_mod  # noqa: E402
from research.finetune_omtm import masks as ft_masks  # noqa: E402
from research.finetune_omtm.learner import Learner  # noqa: E402
from research.omtm.datasets.base import DataStatistics  # noqa: E402
from research.omtm.models.mtm_model import omtm, omtmConfig  # noqa: E402
from research.omtm.tokenizers.base import TokenizerManager  # noqa: E402
from research.omtm.tokenizers.continuous import ContinuousTokenizer  # noqa: E402

import mtm_loss_ref as R  # noqa: E402
from m3pc_amd import synth  # noqa: E402

DIMS = synth.Dims(11, 3, 8, n_embd=64, n_head=2)
B = 3
MASK_RATIO = (0.5, 0.6, 0.7, 0.8)
P_WEIGHTS = (0.2, 0.1, 0.6, 0.1)
ENTROPY_REG = 0.1
DISCRETE = {k: False for k in synth.KEYS}


class Eps:
    """Record (eps is None) or replay the standard normals of Normal.rsample, and check rsample against them."""

    def __init__(self, eps=None):
        self.eps, self.calls = eps, 0

    def __enter__(self):
        self.orig_sn, self.orig_rs = tdn._standard_normal, tdn.Normal.rsample
        me = self

        def standard_normal(shape, dtype, device):
            me.calls += 1
            if me.eps is None:
                me.eps = me.orig_sn(shape, dtype=dtype, device=device)
            assert tuple(shape) == tuple(me.eps.shape), (shape, me.eps.shape)
            me.last = me.eps.to(dtype)
            return me.last

        def rsample(dist, sample_shape=torch.Size()):
            out = me.orig_rs(dist, sample_shape)
            assert torch.equal(out, dist.loc + me.last * dist.scale), "rsample is not loc + eps * scale on this build"
            return out

        tdn._standard_normal, tdn.Normal.rsample = standard_normal, rsample
        return self

    def __exit__(self, *a):
        tdn._standard_normal, tdn.Normal.rsample = self.orig_sn, self.orig_rs
        assert self.calls == 1, self.calls


class FixedMasks:
    """The learner module's mask drawer returns the given masks."""

    def __init__(self, masks):
        self.masks = masks

    def __enter__(self):
        self.orig = learner_mod.create_random_autoregressize_mask
        learner_mod.create_random_autoregressize_mask = lambda *a, **k: {n: m.clone() for n, m in self.masks.items()}

    def __exit__(self, *a):
        learner_mod.create_random_autoregressize_mask = self.orig


class Widen:
    """tokenizer_manager whose encode widens what the real one returns (float32, always) to ``dtype``."""

    def __init__(self, tm, dtype):
        self.tm, self.dtype = tm, dtype

    def encode(self, batch):
        return {k: v.to(self.dtype) for k, v in self.tm.encode(batch).items()}


def build(dtype):
    sd = synth.make_state_dict(DIMS, 0)
    mc = omtmConfig(norm="none", n_embd=DIMS.n_embd, n_enc_layer=DIMS.n_enc_layer, n_dec_layer=DIMS.n_dec_layer, n_head=DIMS.n_head,
                    dropout=0.1)
    model = mc.create(DIMS.data_shapes, DIMS.traj_length, DISCRETE).eval()
    model.load_state_dict(sd, strict=True)
    model = model.to(dtype)
    if dtype == torch.float64:  # trajectory_encoding casts its input to float32 (mtm_model.py:550): the embedding stays float32
        model.encoder_embed_dict.float()
    stats = synth.make_tokenizer_stats(DIMS, 0)
    toks = {k: ContinuousTokenizer(s["mean"], s["std"], DataStatistics(s["mean"], s["std"], s["min"], s["max"]), normalize=(k != "actions"))
            for k, s in stats.items()}
    L = object.__new__(Learner)
    L.cfg = types.SimpleNamespace(traj_length=DIMS.traj_length, device="cpu", mask_ratio=MASK_RATIO, p_weights=P_WEIGHTS)
    L.tokenizer_manager = Widen(TokenizerManager(toks), dtype)
    L.mtm = model
    return L


def make_batch():
    g = torch.Generator().manual_seed(20260821)
    T, S, A = DIMS.traj_length, DIMS.state_dim, DIMS.action_dim
    stats = synth.make_tokenizer_stats(DIMS, 0)
    states = torch.randn(B, T, S, generator=g) * torch.tensor(stats["states"]["std"]) + torch.tensor(stats["states"]["mean"])
    actions = torch.rand(B, T, A, generator=g) * 1.9 - 0.95
    actions[0, 2, 0], actions[1, 5, 1], actions[2, 6, 2], actions[2, 1, 0] = 1.0, -1.0, 1.0, -1.0
    rewards = torch.randn(B, T, 1, generator=g)
    returns = torch.randn(B, T, 1, generator=g, dtype=torch.float64) * 3.0 + 5.0
    return {"states": states, "actions": actions, "rewards": rewards, "returns": returns}


def rows(masks):
    return {k: np.asarray(m.detach().cpu().numpy(), np.float64).reshape(-1) for k, m in masks.items()}


def mixed(masks):
    return all(0 < r.sum() < len(r) for r in rows(masks).values())


def record(tup):
    """The reference's 5-tuple -> (values in the record's layout, which slots it holds)."""
    loss, losses, masked, masked_c, entropy = tup
    val, have = np.full(15, np.nan), np.zeros(15, bool)
    for j, k in enumerate(R.KEYS):
        for o, d in ((0, losses), (1, masked), (2, masked_c)):
            if k in d:
                val[3 * j + o], have[3 * j + o] = float(d[k]), True
    val[R.ENTROPY], val[R.NLL], val[R.TOTAL] = float(losses["entropy"]), float(losses["nll"]), float(loss)
    have[[R.ENTROPY, R.NLL, R.TOTAL]] = True
    assert float(entropy) == float(losses["entropy"]) or np.isnan(float(entropy))
    return val, have


def run_case(out, tag, batch, masks, seed):
    """Both forms in both precisions under `masks` (seed: the np.random.seed that draws them inside the reference, or None)."""
    eps = None
    for dtype, sfx in ((torch.float32, "32"), (torch.float64, "64")):
        L = build(dtype)
        with torch.no_grad():
            with Eps(eps) as e:
                if seed is None:
                    with FixedMasks(masks):
                        ft = L.compute_mtm_loss(batch, DIMS.data_shapes, DISCRETE, ENTROPY_REG)
                else:
                    np.random.seed(seed)
                    ft = L.compute_mtm_loss(batch, DIMS.data_shapes, DISCRETE, ENTROPY_REG)
            eps = e.eps
            enc = L.tokenizer_manager.encode(batch)
            preds = L.mtm(enc, masks)
            with Eps(eps):
                pt = omtm.forward_loss(enc, preds, masks, ENTROPY_REG, DISCRETE, norm="l2", reduce_use_sum=False, loss_keys=None)
        heads = [preds["states"][:, :, 0], preds["rewards"][:, :, 0], preds["returns"][:, :, 0], preds["actions"].loc[:, :, 0],
                 preds["actions"].std[:, :, 0]]
        for name, hd in zip(("states", "rewards", "returns", "mu", "std"), heads):
            out[f"{tag}/head{sfx}/{name}"] = hd.numpy().copy()
        for form, tup in (("finetune", ft), ("pretrain", pt)):
            val, have = record(tup)
            out[f"{tag}/{form}{sfx}"], out[f"{tag}/{form}_have"] = val, have
        if sfx == "32":
            for k in R.KEYS:
                out[f"{tag}/target/{k}"] = enc[k][:, :, 0].numpy().copy()
            out[f"{tag}/eps"] = eps[0, :, :, 0].numpy().copy()  # rsample((1,)) over loc (B,T,1,A) -> (1,B,T,1,A)
        # the restatement on this run's own head outputs
        mr = [rows(masks)[k] for k in R.KEYS]
        tg = [out[f"{tag}/target/{k}"] for k in R.KEYS]
        for form, (flags, bits) in (("finetune", R.FINETUNE), ("pretrain", R.PRETRAIN)):
            got, scale = R.loss_terms(*[h.numpy() for h in heads], tg, mr, out[f"{tag}/eps"], ENTROPY_REG, flags, bits, f32_clip=(sfx == "32"))
            ref, have = out[f"{tag}/{form}{sfx}"], out[f"{tag}/{form}_have"]
            ok = np.isfinite(ref) & have
            dev = np.abs(got - ref)[ok] / scale[ok]
            print(tag, form, sfx, "restatement vs reference: max |d| / scale = %.2e" % (dev.max() if dev.size else 0.0),
                  "specials equal:", R.same_specials(got[have], ref[have]))
    for k in R.KEYS:
        out[f"{tag}/mask/{k}"] = rows(masks)[k].astype(np.uint8)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    batch = make_batch()
    out = {"dims": np.array([DIMS.state_dim, DIMS.action_dim, DIMS.traj_length, DIMS.n_embd, DIMS.n_head]), "entropy_reg": np.float64(ENTROPY_REG),
           "mask_ratio": np.array(MASK_RATIO), "p_weights": np.array(P_WEIGHTS), "torch_version": np.array(torch.__version__)}
    for k, v in batch.items():
        out["batch/" + k] = v.numpy().copy()
    draw = lambda: ft_masks.create_random_autoregressize_mask(DIMS.data_shapes, MASK_RATIO, DIMS.traj_length, "cpu", P_WEIGHTS)
    seeds, seed = [], 0
    while len(seeds) < 2:
        np.random.seed(seed)
        if mixed(draw()):
            seeds.append(seed)
        seed += 1
    out["case_seeds"] = np.array(seeds)
    for c, s in enumerate(seeds):
        np.random.seed(s)
        run_case(out, f"c{c}", batch, draw(), s)
    T = DIMS.traj_length
    hand = {"states": torch.tensor([1, 1, 0, 1, 0, 0, 0, 0.0]).reshape(T, 1).double(), "actions": torch.tensor([0, 1, 1, 0, 0, 1, 1, 0.0]).reshape(T, 1).double(),
            "rewards": torch.ones(T, 1).double(), "returns": torch.tensor([1, 1, 1, 0, 0, 0, 0, 0.0]).reshape(T, 1).double()}
    run_case(out, "c2", batch, hand, None)
    # the mask mirror: eight seeds, mask_ratio as a sequence and as a scalar
    out["mirror_seeds"] = np.arange(100, 108)
    for s in out["mirror_seeds"]:
        np.random.seed(int(s))
        ratios = MASK_RATIO if s % 2 == 0 else 0.75
        m = rows(ft_masks.create_random_autoregressize_mask(DIMS.data_shapes, ratios, T, "cpu", P_WEIGHTS))
        out[f"mirror/{s}"] = np.stack([m[k] for k in R.KEYS]).astype(np.uint8)
    path = os.path.join(HERE, "g8_mtm_loss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
