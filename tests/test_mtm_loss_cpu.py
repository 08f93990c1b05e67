"""The masked-trajectory loss without a GPU: m3pc_mtm_loss_terms / m3pc_mtm_loss / m3pc_mtm_loss_replay are declared in
include/m3pc_hip.h, exported by the library and bound by m3pc_amd/capi.py; every refusal that needs no device comes before any HIP
call; the float64 NumPy restatement the GPU tests compare against (tests/mtm_loss_ref.py) reproduces tests/golden/g8_mtm_loss.npz --
captured from the real reference Learner.compute_mtm_loss and omtm.forward_loss -- to 1e-12 of its float64 run and to the project's
fp32 tolerance (1e-4 of scale) of its float32 run, with NaN / inf at the same places; the Python mirrors reproduce the reference's
early return and its dict contents; and the mask mirror draws the reference's masks bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mtm_loss_ref as R
from m3pc_amd import build, capi, masks, mtm
from m3pc_amd.capi import MTM_CLIP_ACTIONS, MTM_LOSS_FLOATS, MTM_NORM_L2  # (the constants the restatement's layout is checked against)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m3pc_mtm_loss_terms", "m3pc_mtm_loss", "m3pc_mtm_loss_replay")
S, A, T = 11, 3, 8
CASES = ("c0", "c1", "c2")
FORMS = {"finetune": R.FINETUNE, "pretrain": R.PRETRAIN}
HEADS = ("states", "rewards", "returns", "mu", "std")


@pytest.fixture(scope="module")
def lib():
    return capi.load_library(build.build_library())


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "g8_mtm_loss.npz"))


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_every_entry_point_is_declared_exported_and_bound(lib):
    header = _read("include", "m3pc_hip.h")
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/m3pc_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in capi.EXPORTS
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    for macro, value in (("M3PC_MTM_LOSS_FLOATS", capi.MTM_LOSS_FLOATS), ("M3PC_MTM_NORM_L2", capi.MTM_NORM_L2),
                         ("M3PC_MTM_CLIP_ACTIONS", capi.MTM_CLIP_ACTIONS)):
        assert int(re.search(r"#define %s (\d+)" % macro, code).group(1)) == value
    assert (R.NORM_L2, R.CLIP_ACTIONS, len(R.RECORD_NAMES)) == (MTM_NORM_L2, MTM_CLIP_ACTIONS, MTM_LOSS_FLOATS)
    assert (R.ENTROPY, R.NLL, R.TOTAL) == (capi.MTM_ENTROPY, capi.MTM_NLL, capi.MTM_TOTAL)
    assert R.KEYS == capi.KEYS
    assert "m3pc_mtm_loss_terms" in re.search(r"/\* ABI history\..*?\*/", header, flags=re.S).group(0)
    assert "m3pc_mtm_loss" in header[: header.index("#ifndef M3PC_HIP_H")], "the workspace paragraph does not name the call"
    assert "mtm_loss.hip" in build.SOURCES
    # the kernel file takes its reductions from the shared header and defines none of its own
    src = _read("m3pc_amd", "csrc", "mtm_loss.hip")
    assert '#include "device_util.h"' in src and "wave_sum_f64(" in src and "block_sum_f64(" in src
    assert not re.search(r"__shfl|atomicAdd|atomic_add", src)


# ------------------------------------------------------------------------------------------ the restatement is the reference
def _inputs(golden, case, sfx):
    heads = [golden[f"{case}/head{sfx}/{n}"] for n in HEADS]
    tg = [golden[f"{case}/target/{k}"] for k in R.KEYS]
    mk = [golden[f"{case}/mask/{k}"] for k in R.KEYS]
    return heads, tg, mk, golden[f"{case}/eps"], float(golden["entropy_reg"])


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_the_restatement_is_the_reference(golden, case, form):
    flags, bits = FORMS[form]
    have = golden[f"{case}/{form}_have"]
    for sfx, tol in (("64", 1e-12), ("32", 1e-4)):
        heads, tg, mk, eps, reg = _inputs(golden, case, sfx)
        got, scale = R.loss_terms(*heads, tg, mk, eps, reg, flags, bits, f32_clip=(sfx == "32"))
        ref = golden[f"{case}/{form}{sfx}"]
        assert R.same_specials(got[have], ref[have]), (case, form, sfx, got, ref)
        ok = have & np.isfinite(ref)
        assert ok.sum() >= 4
        denom = np.abs(ref[ok]) if sfx == "64" else scale[ok]
        dev = np.abs(got[ok] - ref[ok]) / denom
        print(case, form, sfx, "max deviation", dev.max())
        assert dev.max() <= tol, (case, form, sfx, dev)
        # a scale bounds its scalar, and the slots that do not exist are zero
        assert (np.abs(got[ok]) <= scale[ok] * (1 + 1e-12)).all()
        assert got[4] == 0 and got[5] == 0


def test_the_golden_covers_what_it_should(golden):
    acts = golden["batch/actions"]
    assert (acts == 1.0).any() and (acts == -1.0).any() and golden["batch/returns"].dtype == np.float64 and acts.shape == (3, T, A)
    for case in CASES[:2]:  # drawn: visible and hidden tokens in every key
        for k in R.KEYS:
            m = golden[f"{case}/mask/{k}"]
            assert 0 < m.sum() < T, (case, k)
    # the clip is hit: a target action of +-1 at a hidden timestep, so that the unclipped form is NaN and the clipped one finite
    hidden = golden["c0/mask/actions"] == 0
    assert (np.abs(acts[:, hidden]) == 1.0).any()
    assert np.isnan(golden["c0/pretrain32"][R.NLL]) and np.isfinite(golden["c0/finetune32"][R.NLL])
    # x / 0: every rewards token visible -> masked_loss_rewards is 0 / 0
    assert golden["c2/mask/rewards"].all() and np.isnan(golden["c2/pretrain32"][3 * 2 + 1]) and np.isfinite(golden["c2/pretrain32"][3 * 2 + 2])
    assert np.isfinite(golden["c2/pretrain32"][R.TOTAL])
    # the reference's fine-tuning form holds `states` only (its early return)
    for case in CASES:
        have = golden[f"{case}/finetune_have"]
        assert have.tolist() == [True] * 3 + [False] * 9 + [True] * 3
        assert golden[f"{case}/pretrain_have"].tolist() == [True] * 4 + [False] * 2 + [True] * 9


# ------------------------------------------------------------------------------------------ the Python mirrors
def test_the_early_return_key_set():
    for order, keys, bits in ((("states", "actions", "rewards", "returns"), ["states"], 1),
                              (("actions", "states", "rewards", "returns"), ["actions", "states"], 3),
                              (("actions", "rewards", "states", "returns"), ["actions", "rewards"], 6)):
        assert mtm.early_return_keys(order) == keys == R.early_return_keys(order)
        assert mtm.form_settings("finetune", order) == (capi.MTM_CLIP_ACTIONS, bits, keys)
        assert mtm.form_settings("pretrain", order) == (capi.MTM_NORM_L2, 15, list(order))
    with pytest.raises(ValueError):
        mtm.form_settings("other", R.KEYS)


def test_the_tuple_has_the_reference_dict_contents(golden):
    rec = torch.arange(15, dtype=torch.float32)
    loss, losses, masked, masked_c, entropy = mtm.loss_tuple(rec, ["states"])
    assert list(losses) == ["states", "entropy", "nll"] and list(masked) == ["states"] and list(masked_c) == ["states"]
    assert (float(loss), float(entropy), float(losses["nll"]), float(masked["states"]), float(masked_c["states"])) == (14, 12, 13, 1, 2)
    loss, losses, masked, masked_c, entropy = mtm.loss_tuple(rec, ["actions", "states"])
    assert list(losses) == ["actions", "states", "entropy", "nll"] and list(masked) == ["states"] and float(losses["actions"]) == 3
    loss, losses, masked, masked_c, entropy = mtm.loss_tuple(rec, list(R.KEYS))
    assert list(losses) == list(R.KEYS) + ["entropy", "nll"] and list(masked) == ["states", "rewards", "returns"] == list(masked_c)


def test_unsupported_options_raise():
    m = object.__new__(mtm.omtm)
    t = {k: torch.zeros(1, T, 1, 1) for k in R.KEYS}
    no = {k: False for k in R.KEYS}
    with pytest.raises(capi.M3pcError, match="reduce_use_sum"):
        m.forward_loss(t, t, t, 0.1, no, reduce_use_sum=True)
    with pytest.raises(capi.M3pcError, match="discrete"):
        m.forward_loss(t, t, t, 0.1, dict(no, rewards=True))


def _mask_rows(m):
    return np.stack([np.asarray(m[k].numpy()).reshape(-1) for k in R.KEYS]).astype(np.uint8)


def test_the_mask_mirror_is_the_reference(golden):
    shapes = {"states": (1, S), "actions": (1, A), "rewards": (1, 1), "returns": (1, 1)}
    ratios, pw = tuple(golden["mask_ratio"].tolist()), tuple(golden["p_weights"].tolist())
    for s in golden["mirror_seeds"]:
        np.random.seed(int(s))
        m = masks.create_random_autoregressive_mask(shapes, ratios if s % 2 == 0 else 0.75, T, pw)
        assert list(m) == list(shapes) and all(v.dtype == torch.float64 and v.shape == (T, 1) for v in m.values())
        assert np.array_equal(_mask_rows(m), golden[f"mirror/{s}"]), s
        # the same draws from a RandomState of its own
        m2 = masks.create_random_autoregressive_mask(shapes, ratios if s % 2 == 0 else 0.75, T, pw, rnd=np.random.RandomState(int(s)))
        assert np.array_equal(_mask_rows(m2), golden[f"mirror/{s}"]), s
    for c, s in enumerate(golden["case_seeds"]):
        np.random.seed(int(s))
        m = masks.create_random_autoregressive_mask(shapes, ratios, T, pw)
        assert np.array_equal(_mask_rows(m), np.stack([golden[f"c{c}/mask/{k}"] for k in R.KEYS])), s
    assert len({golden[f"mirror/{s}"].tobytes() for s in golden["mirror_seeds"]}) >= 6  # (the eight are not one mask)


# ------------------------------------------------------------------------------------------ refusals
def _fake_handle(max_batch=4, traj_length=T):
    """Stands in for a handle: the refusals read the m3pc_dims a handle starts with, and its device index behind them."""
    buf = C.create_string_buffer(1 << 16)
    C.memmove(buf, C.byref(capi.Dims(S, A, traj_length, 64, 2, 2, 1, 64, max_batch, 0, 64, 0)), C.sizeof(capi.Dims))
    return buf, C.c_void_p(C.addressof(buf))


def _masks(*rows):
    bufs = [C.create_string_buffer(bytes(r), len(r)) for r in rows]
    return (C.c_void_p * 4)(*[C.addressof(b) for b in bufs]), bufs


def test_every_bad_argument_is_refused_without_a_gpu(lib):
    keep, h = _fake_handle()
    err = lib.m3pc_last_error
    buf = C.create_string_buffer(4096)
    p = C.c_void_p(C.addressof(buf))
    four = (C.c_void_p * 4)(p, p, p, p)
    good, keep_m = _masks(*[[1, 0] * (T // 2)] * 4)
    bad, keep_b = _masks([1, 0] * (T // 2), [1, 0, 2, 0, 0, 0, 0, 0], [0] * T, [1] * T)

    def terms(hh=h, b=2, ps=p, pr=p, pv=p, mu=p, sd=p, tg=four, mk=good, eps=p, flags=0, keys=15, rec=p):
        return lib.m3pc_mtm_loss_terms(hh, b, ps, pr, pv, mu, sd, tg, mk, eps, 0.1, flags, keys, rec, None)

    def loss(hh=h, b=2, s=p, a=p, r=p, v=p, mk=good, eps=p, flags=0, keys=15, prec=0, rec=p):
        return lib.m3pc_mtm_loss(hh, b, s, a, r, v, 1, mk, eps, 0.1, flags, keys, prec, rec, None, None, None, None, None, None)

    for call, nullable in ((terms, ("hh", "ps", "pr", "pv", "mu", "sd", "tg", "mk", "eps", "rec")), (loss, ("hh", "s", "a", "r", "v", "mk", "eps", "rec"))):
        for k in nullable:
            assert call(**{k: None}) == -1 and b"null" in err(), (call.__name__, k)
        for b in (0, -1, 5):
            assert call(b=b) == -1 and b"outside [1, max_batch=4]" in err(), b
        assert call(mk=bad) == -1 and b"mask byte 2 of 'actions' is 2" in err()
        for flags in (4, 8, -1):
            assert call(flags=flags) == -1 and b"flag" in err(), flags
        for keys in (-1, 16):
            assert call(keys=keys) == -1 and b"loss_keys" in err(), keys
    assert terms(tg=(C.c_void_p * 4)(p, None, p, p)) == -1 and b"targets of 'actions'" in err()
    assert terms(mk=(C.c_void_p * 4)(p, p, None, p)) == -1 and b"null mask of 'rewards'" in err()
    assert loss(prec=3) == -1 and b"precision" in err()

    # the replay form: a buffer is created without a HIP call, so its refusals can be met here too
    rb, other, short = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert lib.m3pc_replay_create(h, 5, 40, T, 0, 0, C.byref(rb)) == 0
    assert lib.m3pc_replay_create(h, 5, 40, T - 1, 0, 0, C.byref(short)) == 0
    keep2, h2 = _fake_handle()
    C.memmove(keep2, C.byref(capi.Dims(S + 1, A, T, 64, 2, 2, 1, 64, 4, 0, 64, 0)), C.sizeof(capi.Dims))
    assert lib.m3pc_replay_create(h2, 5, 40, T, 0, 0, C.byref(other)) == 0

    def replay(hh=h, r=rb, b=2, mode=capi.REPLAY_UNIFORM, ti=None, si=None, mk=good, flags=0, keys=1, prec=0, rec=p):
        return lib.m3pc_mtm_loss_replay(hh, r, b, mode, ti, si, 0, 1, 2, mk, None, 0.1, flags, keys, prec, rec, None, None, None)

    for k in ("hh", "r", "mk", "rec"):
        assert replay(**{k: None}) == -1 and b"null" in err(), k
    for b in (0, 5):
        assert replay(b=b) == -1 and b"max_batch" in err(), b
    assert replay(mk=bad) == -1 and b"mask byte" in err()
    assert replay(flags=4) == -1 and b"flag" in err()
    assert replay(keys=16) == -1 and b"loss_keys" in err()
    assert replay(prec=7) == -1 and b"precision" in err()
    assert replay(r=short) == -1 and b"does not fit" in err()
    assert replay(r=other) == -1 and b"does not fit" in err()
    assert replay(mode=2) == -1 and b"mode" in err()
    assert replay(ti=p) == -1 and b"come together" in err()
    assert replay() == -2 and b"holds no trajectory" in err()  # (M3PC_ESTATE: nothing stored, still no HIP call)
    # what the raw and the replay entry refuse alike: the same code and, behind the entry's name, the same text
    null_row = (C.c_void_p * 4)(p, p, None, p)
    for kw in (dict(b=0), dict(b=5), dict(mk=bad), dict(mk=null_row), dict(flags=4), dict(flags=-1), dict(keys=16)):
        rc_l, text_l = loss(**kw), err()
        rc_r, text_r = replay(**kw), err()
        assert rc_l == rc_r == -1, kw
        assert text_l.startswith(b"m3pc_mtm_loss: ") and text_r.startswith(b"m3pc_mtm_loss_replay: "), (kw, text_l, text_r)
        assert text_l[len(b"m3pc_mtm_loss: "):] == text_r[len(b"m3pc_mtm_loss_replay: "):] != b"", (kw, text_l, text_r)
    for r in (rb, other, short):
        assert lib.m3pc_replay_destroy(r) == 0


def test_the_example_compiles(lib, tmp_path):
    """examples/mtm_loss.c against the header and the built library, gcc -Wall -Werror: it calls what it says it calls."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    libpath = build.build_library()
    so = tmp_path / "libmtm_loss_example.so"
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(rocm, "include"), os.path.join(ROOT, "examples", "mtm_loss.c"), "-o", str(so),
                           "-L", os.path.dirname(libpath), "-l:" + os.path.basename(libpath), "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-lm"])
    out = subprocess.check_output(["nm", "-u", str(so)], text=True)
    for name in ("m3pc_mtm_loss_replay", "m3pc_replay_create", "m3pc_replay_append", "m3pc_load_weights", "m3pc_set_tokenizer"):
        assert name in out, name
