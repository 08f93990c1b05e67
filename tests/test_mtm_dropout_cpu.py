"""Dropout of m3pc_mtm_grad* without a GPU: the restatement with the library's keep masks (tests/mtm_dropout_ref.py) against the golden
captured from the REAL reference in training mode under the same masks (tests/golden/g11_mtm_dropout.npz), the properties of the
mask stream, the fixture conditions the GPU kernel tests rely on, and the refusals of m3pc_mtm_grad_set_dropout through the C ABI.

The restatement is held to the golden as tests/test_mtm_grad_cpu.py holds the eval-mode one to g9: per tensor within the golden's
ref32_grad_dev + 2^-24 (the stored gradients are the float64 run's rounded to float32)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import mtm_dropout_ref as DR
import mtm_grad_ref as GR
from m3pc_amd import build, capi, synth
from oracle import mtm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = synth.Dims(11, 3, 8, n_embd=64, n_head=2)
STORE = 2.0 ** -24
CASES = (("ft_c0_p10", "c0", "finetune"), ("ft_c0_p50", "c0", "finetune"), ("pt_c3_p10", "c3", "pretrain"))


@pytest.fixture(scope="module")
def goldens(golden_dir):
    return np.load(golden_dir + "/g8_mtm_loss.npz"), np.load(golden_dir + "/g9_mtm_grad_pretrain.npz"), np.load(golden_dir + "/g11_mtm_dropout.npz")


@pytest.fixture(scope="module")
def lib():
    return capi.load_library(build.build_library())


def golden_inputs(g8, g9p, case):
    batch = {k: g8["batch/" + k] for k in GR.KEYS}
    if case == "c3":
        batch["actions"] = g9p["c3/actions"]
    mcase = "c2" if case == "c3" else case
    return batch, {k: g8[f"{mcase}/mask/{k}"] for k in GR.KEYS}, g8[f"{mcase}/eps"]


@pytest.mark.parametrize("tag,case,form", CASES)
def test_the_float64_restatement_is_the_training_mode_reference(goldens, tag, case, form):
    g8, g9p, g11 = goldens
    names = [str(n) for n in g11["grad_names"]]
    p, seed, draw = float(g11[tag + "/p"]), int(g11["seed"]), int(g11["draw"])
    flags, bits = GR.FORMS[form]
    sd, stats = synth.make_state_dict(DIMS, 0), O.make_stats(synth.make_tokenizer_stats(DIMS, 0))
    batch, masks, eps = golden_inputs(g8, g9p, case)
    order = []
    # (the reference's float64 run clips at the float64 bounds)
    total, gd = DR.grads_dropout(sd, stats, batch, masks, eps, float(g8["entropy_reg"]), flags, bits, DIMS.n_head, p, seed, draw, torch.float64,
                                 f32_clip=False, order=order)
    assert list(gd) == names
    # the real nn.TransformerEncoderLayer applied the sites 0, 1, 2, 3 of each layer in this order, encoder layers first
    n_layers = DIMS.n_enc_layer + DIMS.n_dec_layer
    assert g11[tag + "/order"].tolist() == list(range(4 * n_layers)) == [4 * li + s for li, s in order]
    none, dev32, sums, head = g11[tag + "/none"], g11[tag + "/ref32_grad_dev"], g11[tag + "/sums"], int(g11["head"])
    assert [gd[n] is None for n in names] == none.tolist()
    t64 = float(g11[tag + "/total64"])
    assert np.isfinite(t64) and abs(total - t64) <= 1e-9 * abs(t64)
    worst = 0.0
    for i, n in enumerate(names):
        if none[i]:
            continue
        assert np.isfinite(dev32[i]), n
        g_all = gd[n].reshape(-1)
        gold = g11[f"{tag}/head/{n}"].astype(np.float64)
        g = g_all[:head]
        assert gold.size == g.size
        bound, top = dev32[i] + STORE, np.abs(g_all).max()
        assert abs(g_all.sum() - sums[i, 0]) <= bound * top * g_all.size + 1e-300, n
        assert abs((g_all * g_all).sum() - sums[i, 1]) <= 2 * bound * top * top * g_all.size + 1e-300, n
        if top == 0.0:
            assert not gold.any(), n
            continue
        d = np.abs(g - gold).max() / top
        worst = max(worst, d / bound)
        assert d <= bound, (n, d, bound)
    print(tag, "largest deviation / bound over the tensors: %.3f" % worst)
    # dropout is in the numbers: the eval-mode restatement is far outside the same bound
    _, g0 = GR.grads(sd, stats, batch, masks, eps, float(g8["entropy_reg"]), flags, bits, DIMS.n_head, torch.float64, False)
    n = "decoder.layers.0.linear1.weight"
    assert GR.deviation(g0[n], gd[n]) > 1e-2


def test_p_zero_is_the_eval_mode_restatement(goldens):
    g8, g9p, _ = goldens
    sd, stats = synth.make_state_dict(DIMS, 0), O.make_stats(synth.make_tokenizer_stats(DIMS, 0))
    batch, masks, eps = golden_inputs(g8, g9p, "c3")
    flags, bits = GR.FORMS["pretrain"]
    t0, g0 = GR.grads(sd, stats, batch, masks, eps, 0.1, flags, bits, DIMS.n_head)
    t1, g1 = DR.grads_dropout(sd, stats, batch, masks, eps, 0.1, flags, bits, DIMS.n_head, 0.0, 5, 6)
    assert t0 == t1 and all(np.array_equal(g0[n], g1[n]) for n in g0)


# ------------------------------------------------------------------------------------------------ the mask stream
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("shape", [(1024, 1024), (4, 16, 128, 128)])
def test_keep_fraction(p, shape):
    k = DR.keep(99, 1, 5, shape, p)
    n = k.size
    assert n == 2 ** 20 and k.shape == shape
    q = 1.0 - DR.threshold(p) / 2.0 ** 32
    sigma = math.sqrt(n * q * (1 - q))
    assert abs(int(k.sum()) - n * q) <= 6 * sigma, (int(k.sum()), n * q, sigma)


def test_threshold_and_scale():
    assert DR.threshold(0.0) == 0 and DR.threshold(0.5) == 2 ** 31 and DR.threshold(0.1) == int(0.1 * 2 ** 32)
    assert DR.threshold(1.0 - 2.0 ** -40) == 2 ** 32 - 1
    assert DR.scale(0.5) == 2.0 and DR.scale(0.0) == 1.0 and DR.scale(0.1) == float(np.float32(1.0 / 0.9))


def test_p_zero_keeps_everything():
    assert DR.keep(3, 4, 5, (33, 96), 0.0).all() and DR.keep(3, 4, 4, (2, 2, 9, 9), 0.0).all()


def test_sites_draws_seeds_and_arrays_differ():
    base = DR.keep(7, 0, 1, (64, 64), 0.5)
    assert np.array_equal(base, DR.keep(7, 0, 1, (64, 64), 0.5))
    for other in (DR.keep(7, 0, 2, (64, 64), 0.5), DR.keep(7, 1, 1, (64, 64), 0.5), DR.keep(8, 0, 1, (64, 64), 0.5),
                  DR.keep(7 + 2 ** 32, 0, 1, (64, 64), 0.5), DR.keep(7, 2 ** 32, 1, (64, 64), 0.5)):
        frac = float((base != other).mean())
        assert 0.4 < frac < 0.6, frac
    att = DR.keep(7, 0, 1, (1, 1, 64, 64), 0.5).reshape(64, 64)
    assert 0.4 < float((base != att).mean()) < 0.6


def test_the_mask_of_the_leading_rows_does_not_depend_on_the_extent():
    """A larger batch appends rows: the rows of the smaller one keep their bits (matrix sites: rows = batch x L; attention: b major)."""
    small = DR.keep(11, 3, 6, (40, 64), 0.1)
    big = DR.keep(11, 3, 6, (141, 64), 0.1)
    assert np.array_equal(small, big[:40])
    a_small, a_big = DR.keep(11, 3, 4, (2, 2, 9, 9), 0.1), DR.keep(11, 3, 4, (5, 2, 9, 9), 0.1)
    assert np.array_equal(a_small, a_big[:2])


def test_the_attention_edge_fixture_has_an_all_dropped_and_an_all_kept_row():
    e = DR.ATT_EDGE
    k = DR.keep(e["seed"], e["draw"], e["site"], (e["B"], e["nh"], e["L"], e["L"]), e["p"]).reshape(-1, e["L"])
    assert (k.sum(1) == 0).any() and (k.sum(1) == e["L"]).any()


# ------------------------------------------------------------------------------------------------ the C ABI, without a GPU
def test_set_dropout_refusals(lib):
    err = lib.m3pc_last_error
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        assert lib.m3pc_mtm_grad_set_dropout(None, bad, 1, 0) == -1 and b"set_dropout: p" in err(), bad
    assert lib.m3pc_mtm_grad_set_dropout(None, 0.1, 1, 0) == -1 and b"set_dropout: null g" in err()
    assert lib.m3pc_mtm_grad_get_dropout(None, None, None, None) == -1 and b"get_dropout: null g" in err()


def test_new_entries_agree_across_header_and_capi():
    header = open(os.path.join(ROOT, "include", "m3pc_hip.h")).read()
    declared = set(re.findall(r"^int (m3pc_\w+)\(", header, re.M))
    for name in ("m3pc_mtm_grad_set_dropout", "m3pc_mtm_grad_get_dropout"):
        assert name in declared and name in capi.EXPORTS, name
    dbg = open(os.path.join(ROOT, "include", "m3pc_hip_debug.h")).read()
    block = dbg[dbg.index("MTM-dropout kernel ids"):dbg.index("(end of the MTM-dropout kernel ids)")]
    ids = {int(n): k for n, k in re.findall(r"(\d+) (mg_[a-z0-9_]+_kernel)", block)}
    src = open(os.path.join(ROOT, "m3pc_amd", "csrc", "mtm_dropout.hip")).read()
    kernels = set(re.findall(r"__global__ __launch_bounds__\(256\) void (mg_[a-z0-9_]+_kernel)", src))
    assert sorted(ids) == list(range(16, 22)) and set(ids.values()) == kernels
    assert sorted(int(n) for n in re.findall(r"M3PC_MG_PICK\((\d+)\)", src)) == sorted(ids)
    lab = capi.load_library(build.build_library(lab=True))
    for name in ("m3pc_debug_mg_gemm_drop", "m3pc_debug_mg_attention_drop", "m3pc_debug_mg_drop_rows", "m3pc_debug_mtm_keep"):
        assert hasattr(lab, name), name
    assert lab.m3pc_debug_mtm_keep(None, 0, C.c_longlong(1), 1, None, None, None) == -1


def test_the_quad_limit_of_a_site_is_refused_before_any_device_call():
    """A site numbers its groups of four elements in 32 bits.  No gradient call can reach the limit with the sizes m3pc_mtm_grad_create
    accepts; the mask hook can, and refuses on the host (keep is never dereferenced)."""
    lab = capi.load_library(build.build_library(lab=True))
    fn = lab.m3pc_debug_mtm_keep

    class Drop(C.Structure):
        _fields_ = [("p", C.c_double), ("seed", C.c_ulonglong), ("draw", C.c_ulonglong), ("site", C.c_int)]

    fn.restype, fn.argtypes = C.c_int, [C.POINTER(Drop), C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    d, dummy, err = Drop(0.1, 1, 0, 3), C.create_string_buffer(16), lab.m3pc_last_error
    picked = (C.c_int * 2)(7, 7)
    for attention, R, Cc in ((0, 2 ** 34 + 4, 4), (1, 2 ** 33, 5), (0, 2 ** 32 + 1, 8)):
        assert fn(C.byref(d), attention, R, Cc, dummy, None, picked) == -1 and b"2^32 quads" in err() and picked[0] == 0, (attention, R, Cc)
    # exactly 2^32 quads is inside the stream's range (the largest index is 2^32 - 1); the hook then refuses the byte count
    assert fn(C.byref(d), 0, 2 ** 32, 4, dummy, None, picked) == -1 and b"beyond int" in err()
    assert fn(C.byref(d), 1, 2 ** 31, 5, dummy, None, picked) == -1 and b"beyond int" in err()
