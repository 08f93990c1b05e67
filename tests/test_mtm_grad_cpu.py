"""The torch restatement of the MTM gradient (tests/mtm_grad_ref.py) against the golden captured from the real reference's
loss.backward() (tests/golden/g9_mtm_grad*.npz), and the names of the new C entries across the header, exports.map and capi.

What each golden case pins (the g8 batch has exact +-1 actions at timesteps 1, 2, 5, 6): the fine-tuning form, which clips, is compared
in every tensor for c0, c1, c2.  Of the pretraining form c0 and c1 pin only that total is NaN (a +-1 action at a hidden timestep), c2
the 19 tensors that are not upstream of mu (a +-1 action at a visible timestep: autograd's 0 * inf makes the other 71 NaN in the
reference and in the restatement alike).  c3 -- c2's masks and eps with those four actions at +-0.9 -- pins every tensor of the
pretraining form: l2-normalised targets, loss_keys = 15, all heads feeding the trunk, the masked action MSE."""
import fnmatch
import os
import re

import numpy as np
import pytest
import torch

import mtm_grad_ref as GR
from m3pc_amd import capi, synth
from oracle import mtm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = synth.Dims(11, 3, 8, n_embd=64, n_head=2)
CASES = ("c0", "c1", "c2")
PAIRS = [(c, f) for c in CASES for f in ("finetune", "pretrain")] + [("c3", "pretrain")]
NEW = ("m3pc_mtm_grad_create", "m3pc_mtm_grad_destroy", "m3pc_mtm_grad", "m3pc_mtm_grad_replay", "m3pc_mtm_grad_export")
# the bound is the golden's ref32_grad_dev per tensor plus 2^-24: the stored gradients are the float64 run's rounded to float32, half an
# ulp of the largest element relative to it (ref32_grad_dev itself drops to 1e-8 for single tensors, below that rounding)
STORE = 2.0 ** -24


@pytest.fixture(scope="module")
def goldens(golden_dir):
    return (np.load(golden_dir + "/g8_mtm_loss.npz"), np.load(golden_dir + "/g9_mtm_grad.npz"), np.load(golden_dir + "/g9_mtm_grad_finetune.npz"),
            np.load(golden_dir + "/g9_mtm_grad_pretrain.npz"))


def _restate(g8, case, form, dtype, f32_clip, actions=None):
    flags, bits = GR.FORMS[form]
    sd = synth.make_state_dict(DIMS, 0)
    stats = O.make_stats(synth.make_tokenizer_stats(DIMS, 0))
    batch = {k: g8["batch/" + k] for k in GR.KEYS}
    if actions is not None:
        batch["actions"] = actions
    mcase = "c2" if case == "c3" else case  # (c3: the masks and eps of c2)
    masks = {k: g8[f"{mcase}/mask/{k}"] for k in GR.KEYS}
    return GR.grads(sd, stats, batch, masks, g8[f"{mcase}/eps"], float(g8["entropy_reg"]), flags, bits, DIMS.n_head, dtype, f32_clip)


@pytest.mark.parametrize("case,form", PAIRS)
def test_the_float64_restatement_is_the_reference(goldens, case, form):
    g8, g9, g9f, g9p = goldens
    names = [str(n) for n in g9["grad_names"]]
    pre = f"{case}/{form}/"
    src = g9p if case == "c3" else g9
    # (the reference's float64 run clips at the float64 bounds)
    total, gd = _restate(g8, case, form, torch.float64, f32_clip=False, actions=g9p["c3/actions"] if case == "c3" else None)
    assert list(gd) == names
    none, dev32, sums = src[pre + "none"], src[pre + "ref32_grad_dev"], src[pre + "sums"]
    assert [gd[n] is None for n in names] == none.tolist(), "the same tensors are out of autograd's reach"
    t64 = float(src[pre + "total64"])
    if not np.isfinite(t64):  # an exact +-1 action at a hidden timestep without the clip: the gradients are unspecified
        assert not np.isfinite(total)
        return
    assert abs(total - t64) <= 1e-9 * abs(t64)
    worst = 0.0
    for i, n in enumerate(names):
        if none[i]:
            continue
        g = gd[n].reshape(-1)
        if not np.isfinite(dev32[i]):  # an exact +-1 action at a VISIBLE timestep without the clip: z = inf, and autograd's 0 * inf
            assert not np.isfinite(g).all(), n  # is NaN in the reference and here alike (the device selects, and stays finite)
            continue
        bound = dev32[i] + STORE
        if case == "c3":
            assert np.isfinite(dev32[i]) and np.isfinite(g).all(), n  # the case that pins every tensor of the pretraining form
        if case in ("c2", "c3"):
            gold = (g9p if case == "c3" else g9 if form == "pretrain" else g9f)[pre + "full/" + n].astype(np.float64).reshape(-1)
            assert gold.size == g.size
        else:
            gold = g9[pre + "head/" + n].astype(np.float64)
            g_all, g = g, g[: gold.size]
            top_all = np.abs(g_all).max()
            assert abs(g_all.sum() - sums[i, 0]) <= bound * top_all * g_all.size + 1e-300, n
            assert abs((g_all * g_all).sum() - sums[i, 1]) <= 2 * bound * top_all * top_all * g_all.size + 1e-300, n
        top = np.abs(gd[n]).max()
        if top == 0.0:
            assert not gold.any(), n
            continue
        d = np.abs(g - gold).max() / top
        worst = max(worst, d / bound)
        assert d <= bound, (n, d, bound)
        if not gold.any():
            assert not g.any(), n
    print(case, form, "largest deviation / bound over the tensors: %.3f" % worst)


def test_structural_zeros_of_the_restatement(goldens):
    """What the header promises as exact zeros is zero (or None) in the reference arithmetic: c2 keeps every reward token visible."""
    g8 = goldens[0]
    _, gd = _restate(g8, "c2", "pretrain", torch.float64, True)
    assert not gd["mask_token_dict.rewards"].any()
    _, gd = _restate(g8, "c2", "finetune", torch.float64, True)
    for n, g in gd.items():
        if n.startswith("output_head_dict.rewards") or n.startswith("output_head_dict.returns"):
            assert g is None, n


def test_float32_restatement_deviates_like_the_reference(goldens):
    g8, g9, _, g9p = goldens
    _, g64 = _restate(g8, "c3", "pretrain", torch.float64, True, g9p["c3/actions"])
    _, g32 = _restate(g8, "c3", "pretrain", torch.float32, True, g9p["c3/actions"])
    dev = np.array([GR.deviation(g32[n], g64[n]) for n in g64 if np.isfinite(g64[n]).all()])
    ref = g9p["c3/pretrain/ref32_grad_dev"]
    assert np.isfinite(ref).all() and dev.size == 90
    print("restatement dev32: median %.2e max %.2e; the reference's: median %.2e max %.2e" % (
        np.median(dev), dev.max(), np.median(ref), ref.max()))
    assert dev.size == ref.size and dev.max() <= 16 * max(ref.max(), 2.0 ** -23)


def test_new_entries_agree_across_header_map_and_capi():
    header = open(os.path.join(ROOT, "include", "m3pc_hip.h")).read()
    declared = set(re.findall(r"^int (m3pc_\w+)\(", header, re.M))
    patterns = re.findall(r"global:\s*([^;]+);", open(os.path.join(ROOT, "m3pc_amd", "csrc", "exports.map")).read())
    for name in NEW:
        assert name in declared, name
        assert name in capi.EXPORTS, name
        assert any(fnmatch.fnmatch(name, p.strip()) for p in patterns), name
    assert "struct m3pc_mtm_grad;" in header
    assert re.search(r"#define M3PC_ABI_VERSION 7\b", header)
    # the shapes the Python side hands out are the model's
    from m3pc_amd.mtm_grad import param_shapes
    sd = synth.make_state_dict(DIMS, 0)
    shapes = param_shapes(DIMS.state_dim, DIMS.action_dim, DIMS.n_embd, DIMS.n_enc_layer, DIMS.n_dec_layer)
    assert {k: tuple(v.shape) for k, v in sd.items() if k != "pos_embed"} == shapes
