"""The eval_action certificate without a GPU: the fp64 reference of the bound (tests/eval_bound_ref.py) is sound and not vacuous on
six seeded regimes; m3pc_eval_bound / m3pc_plan_step_certified_eval are declared, exported and bound, m3pc_eval_record has the
header's layout, the ABI version did not move; null and bad arguments are refused before any HIP call; examples/certified_eval.c
compiles and links against the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import eval_bound_ref as R
from m3pc_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m3pc_eval_bound", "m3pc_plan_step_certified_eval")
EINVAL = -1

# (temperature, spread of the scores, delta, N, A): rtg guidance at bf16's and bf16x3's delta (a nearly flat softmax), critic
# guidance (a peaked one) at two deltas, a wide rtg vector with more candidates and actions, a small critic vector with many actions
REGIMES = [(0.01, 15.0, 4.87, 1024, 3), (0.01, 15.0, 0.012, 1024, 3), (1.0, 3.0, 0.05, 1024, 3), (1.0, 3.0, 0.012, 1024, 3),
           (0.01, 100.0, 4.87, 4096, 6), (1.0, 3.0, 0.05, 256, 17)]


def _regime(i):
    """fp32 scores f, a merged vector m = f + (an error within +-delta) off the re-scored set, and the lists of a step: 2 race
    entries, 128 score entries of which 8 are re-scored."""
    tau, spread, delta, N, A = REGIMES[i]
    g = np.random.default_rng(100 + i)
    f = g.normal(size=N) * spread + 50.0
    a0 = np.tanh(g.normal(size=(N, A)))
    m = f + g.uniform(-delta, delta, size=N)
    q = g.exponential(size=N)
    race = np.argsort(-(tau * m - np.log(q)), kind="stable")[:2]
    lst = np.concatenate([race, np.argsort(-m, kind="stable")[:128]])
    in_L = np.zeros(N, dtype=bool)
    in_L[lst[: 2 + 8]] = True
    m[in_L] = f[in_L]
    return tau, delta, f, m, a0, lst, in_L, g


@pytest.mark.parametrize("i", range(len(REGIMES)))
def test_reference_bound_is_sound_and_not_vacuous(i):
    """|e_k - e32_k| <= B_k for 20 random error vectors within +-delta and for the adversarial one, delta sign(a0_j0 - e_0), which
    reaches at least half of B_0; bound(n') does not increase with n'; the cumulative-sum form of the reference agrees."""
    tau, delta, _, m, a0, lst, in_L, g = _regime(i)
    ref = R.eval_bound(m, a0, lst, 2, 8, 128, tau, delta)
    p, e = ref["p"], ref["e"]
    B, _ = R.bound_given(p, e, a0, ~in_L, ref["eps"])
    assert ref["eval_bound"] == B.max() and ref["n_U"] == int((~in_L).sum())
    assert np.all(np.diff(ref["bounds"]) <= 0.0)
    fast = R.eval_bound_fast(m, a0, lst, 2, 8, 128, tau, delta)
    np.testing.assert_allclose(fast["bounds"], ref["bounds"], rtol=1e-10, atol=0)
    assert abs(fast["P_U"] - ref["P_U"]) <= 1e-12 and fast["k"] == ref["k"] and fast["n_U"] == ref["n_U"]
    worst = 0.0
    for _ in range(20):
        f = m.copy()
        f[~in_L] -= g.uniform(-delta, delta, size=int((~in_L).sum()))
        _, e32 = R.softmax_mean(f, a0, tau)
        assert np.all(np.abs(e - e32) <= B), (np.abs(e - e32), B)
        worst = max(worst, float((np.abs(e - e32) / B).max()))
    f = m.copy()
    f[~in_L] += (delta * np.sign(a0[:, 0] - e[0]))[~in_L]
    _, e32 = R.softmax_mean(f, a0, tau)
    reach = abs(e32[0] - e[0]) / B[0]
    print(f"regime {i}: bound {ref['eval_bound']:.4g} bound(128) {ref['bound_listed']:.4g} random errors reach {worst:.3f}, "
          f"adversarial {reach:.3f}")
    assert np.all(np.abs(e - e32) <= B)
    assert reach >= 0.5


def test_reference_need_eval():
    """need_eval is the smallest n' whose bound is within the tolerance, n for +inf, N when the list cannot reach it."""
    tau, delta, _, m, a0, lst, _, _ = _regime(2)
    ref = R.eval_bound(m, a0, lst, 2, 8, 128, tau, delta)
    b = ref["bounds"]
    assert R.eval_bound(m, a0, lst, 2, 8, 128, tau, delta, np.inf)["need_eval"] == 8
    assert R.eval_bound(m, a0, lst, 2, 8, 128, tau, delta, 0.5 * b[-1])["need_eval"] == m.size
    t = 40
    assert b[t] < b[t - 1]
    assert R.eval_bound(m, a0, lst, 2, 8, 128, tau, delta, 0.5 * (b[t] + b[t - 1]))["need_eval"] == 8 + t
    assert R.eval_bound_fast(m, a0, lst, 2, 8, 128, tau, delta, 0.5 * (b[t] + b[t - 1]))["need_eval"] == 8 + t


# ------------------------------------------------------------------------------------------------------------------ the ABI
@pytest.fixture(scope="module")
def lib():
    return capi.load_library(build.build_library())


def _header():
    return open(os.path.join(ROOT, "include", "m3pc_hip.h")).read()


def test_both_symbols_are_declared_exported_and_bound(lib):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/m3pc_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in capi.EXPORTS
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    assert hasattr(capi.Handle, "eval_bound") and hasattr(capi.Handle, "plan_step_certified_eval")


def test_abi_version_did_not_move(lib):
    assert lib.m3pc_abi_version() == 7 == capi.ABI_VERSION
    assert int(re.search(r"#define M3PC_ABI_VERSION (\d+)", _header()).group(1)) == 7


def test_eval_record_layout_matches_the_header():
    assert C.sizeof(capi.EvalRecord) == 20
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct m3pc_eval_record \{(.*?)\} m3pc_eval_record;", code, flags=re.S).group(1)
    fields = [tuple(d.split()) for d in body.split(";") if d.strip()]
    assert fields == [("float", "eval_bound"), ("int", "need_eval_first"), ("int", "n_eval"), ("int", "eval_rounds"), ("int", "eval_certified")]
    ctypes_of = {"int": C.c_int, "float": C.c_float}
    for i, ((ctype, n), (name, ct)) in enumerate(zip(fields, capi.EvalRecord._fields_)):
        assert n == name and ct is ctypes_of[ctype]
        assert getattr(capi.EvalRecord, n).offset == 4 * i, n


def test_eval_bound_refuses_bad_arguments_without_a_gpu(lib):
    fake = C.create_string_buffer(64)  # stands in for a handle and for every buffer: the checks come before anything is touched
    p = C.c_void_p(C.addressof(fake))
    ok = dict(h=p, merged=p, n_total=64, lst=p, r=2, n=8, n_listed=32, a0=p, a0_stride=3, A=3, tau=0.01, delta=1.0, tol=1e-3, stats=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.m3pc_eval_bound(a["h"], a["merged"], a["n_total"], a["lst"], a["r"], a["n"], a["n_listed"], a["a0"], a["a0_stride"],
                                   a["A"], a["tau"], a["delta"], a["tol"], a["stats"], None, 0.0, None)

    for name in ("h", "merged", "lst", "a0", "stats"):
        assert call(**{name: None}) == EINVAL and b"null" in lib.m3pc_last_error(), name
    for bad, word in ((dict(tol=0.0), b"eval_tol"), (dict(tol=-1.0), b"eval_tol"), (dict(tol=float("nan")), b"eval_tol"),
                      (dict(delta=-1.0), b"delta"), (dict(delta=float("nan")), b"delta"),
                      (dict(n_total=0), b"n_total"), (dict(n_total=16385), b"n_total"), (dict(A=0), b"A "), (dict(A=1025), b"A "),
                      (dict(r=64, n_listed=961), b"n_listed"), (dict(r=-1), b"n_listed"), (dict(n=-1), b"n "), (dict(n=33), b"n "),
                      (dict(n_listed=-1, n=0), b"n_listed")):
        assert call(**bad) == EINVAL, bad
        assert word in lib.m3pc_last_error(), (bad, lib.m3pc_last_error())


def test_certified_eval_refuses_bad_arguments_without_a_gpu(lib):
    fake = C.create_string_buffer(64)
    h = p = C.c_void_p(C.addressof(fake))
    args = capi.PlanArgs(capi.MODE_RTG, capi.PREC_BF16, 4, 64, 0, 64, 0.6, 0.99, 3.0, 0, 0, None, 0, 0)
    cert = capi.CertArgs(0.01, 1.0, 0, 8, 32, 2, 32)
    rec, erec = capi.CertRecord(), capi.EvalRecord()

    def call(h=h, a=C.byref(args), c=C.byref(cert), rec=C.byref(rec), tol=1e-3, erec=C.byref(erec), req=p):
        return lib.m3pc_plan_step_certified_eval(h, a, c, req, req, req, req, req, None, None, req, req, req, None, None, None, None, None,
                                                 None, rec, tol, erec, None)

    for kw in (dict(h=None), dict(a=None), dict(c=None), dict(rec=None), dict(erec=None), dict(req=None)):
        assert call(**kw) == EINVAL and b"null" in lib.m3pc_last_error(), kw
    for tol in (0.0, -1.0, float("nan")):
        assert call(tol=tol) == EINVAL and b"eval_tol" in lib.m3pc_last_error(), tol
    # the refusals of m3pc_plan_step_certified come first
    a2 = capi.PlanArgs.from_buffer_copy(args)
    a2.n_count = 32
    assert call(a=C.byref(a2)) == EINVAL and b"one rank" in lib.m3pc_last_error()
    c2 = capi.CertArgs.from_buffer_copy(cert)
    c2.kmin = 0
    assert call(c=C.byref(c2)) == EINVAL and b"kmin" in lib.m3pc_last_error()
    c2 = capi.CertArgs.from_buffer_copy(cert)
    c2.delta = -1.0
    assert call(c=C.byref(c2), tol=0.0) == EINVAL and b"delta" in lib.m3pc_last_error()


def test_planner_refuses_eval_tol_without_the_native_step():
    """The constructor's checks come before anything touches a device."""
    from m3pc_amd.planner import HipPlanner
    for kw in (dict(), dict(native_step=True, rescore="topk")):
        with pytest.raises(ValueError, match="eval_tol"):
            HipPlanner(None, {}, None, eval_tol=1e-3, **kw)
    with pytest.raises(ValueError, match="eval_tol"):
        HipPlanner(None, {}, None, eval_tol=0.0, native_step=True)


def test_example_compiles_and_links(tmp_path):
    so = tmp_path / "libcertified_eval.so"
    libpath = build.build_library()
    libdir = os.path.dirname(libpath)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "certified_eval.c"), "-o", str(so), "-L", libdir,
                           "-l:" + os.path.basename(libpath), "-Wl,-rpath," + libdir])
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(so)], text=True)
    assert " certified_eval" in out
