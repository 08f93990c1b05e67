"""The lock-step batch of certified plan steps as one C call, without a GPU: m3pc_plan_steps_certified is declared in
include/m3pc_hip.h, exported by the library and bound by m3pc_amd/capi.py; the addition did not move the ABI version; every refusal
that does not need the handle comes before the handle is touched (a fake handle and dummy pointers stand in); the lab hook of the
one new kernel is in the lab build only; examples/lockstep_steps.c is plain C against the header."""
import ctypes as C
import os
import re
import subprocess

import pytest

from m3pc_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "m3pc_plan_steps_certified"
HOOK = "m3pc_debug_select_batch"
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    return capi.load_library(build.build_library())


def _header(name="m3pc_hip.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def test_symbol_is_declared_exported_and_bound(lib):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % NAME, code, flags=re.S)
    assert decl, f"{NAME} is not declared in include/m3pc_hip.h"
    params = [p.strip() for p in decl.group(1).split(",")]
    assert len(params) == 23 and params[3] == "int n_windows" and params[7] == "const double* rtg"
    assert params[-2] == "m3pc_cert_record* records" and params[-1] == "void* stream"
    assert hasattr(lib, NAME), f"{NAME} is not exported"
    assert NAME in capi.EXPORTS
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int and len(fn.argtypes) == 23
    assert hasattr(capi.Handle, "plan_steps_certified")


def test_abi_version_did_not_move(lib):
    assert lib.m3pc_abi_version() == 7 == capi.ABI_VERSION
    assert int(re.search(r"#define M3PC_ABI_VERSION (\d+)", _header()).group(1)) == 7


# positions of the call's pointer arguments (after h, args, cert, n_windows)
PTRS = ("states", "actions", "rewards", "rtg", "eps", "expo", "loc", "std", "sample_actions", "scores_low", "merged", "list", "p",
        "eval_action", "argmax", "sample_idx", "sample_action", "records")
REQUIRED = ("states", "actions", "rewards", "rtg", "eps", "expo", "sample_actions", "scores_low", "merged", "records")


def _call(lib, h, a, c, n_windows=2, **null):
    """The call with dummy non-null pointers for the required arguments (nothing is dereferenced before the checks pass)."""
    buf = C.create_string_buffer(256)
    p = C.addressof(buf)
    vals = {k: (p if k in REQUIRED else None) for k in PTRS}
    for k in null:
        vals[k] = None
    rtg = C.cast(vals["rtg"], C.POINTER(C.c_double)) if vals["rtg"] else None
    rec = C.cast(vals["records"], C.POINTER(capi.CertRecord)) if vals["records"] else None
    mid = [vals[k] for k in PTRS[4:-1]]
    return lib.m3pc_plan_steps_certified(h, a, c, n_windows, vals["states"], vals["actions"], vals["rewards"], rtg, *mid, rec, None)


def test_handle_free_refusals_come_before_the_handle_is_touched(lib):
    fake = C.create_string_buffer(64)  # stands in for a handle: these checks come before the handle is read
    h = C.c_void_p(C.addressof(fake))
    args = capi.PlanArgs(capi.MODE_RTG, capi.PREC_BF16, 4, 64, 0, 64, 0.6, 0.99, 0.0, 0, 0, None, 0, 0)
    cert = capi.CertArgs(0.01, 1.0, 0, 6, 32, 2, 32)
    a, c = C.byref(args), C.byref(cert)
    assert _call(lib, None, a, c) == EINVAL and b"null" in lib.m3pc_last_error()
    assert _call(lib, h, None, c) == EINVAL and b"null" in lib.m3pc_last_error()
    assert _call(lib, h, a, None) == EINVAL and b"null" in lib.m3pc_last_error()
    for name in REQUIRED:
        assert _call(lib, h, a, c, **{name: True}) == EINVAL and b"null" in lib.m3pc_last_error(), name
    for e in (0, -3):
        assert _call(lib, h, a, c, n_windows=e) == EINVAL and b"n_windows" in lib.m3pc_last_error(), e
    # the batched policy pass takes rtg only: a returns row is refused
    a2 = capi.PlanArgs.from_buffer_copy(args)
    a2.returns = C.addressof(fake)
    assert _call(lib, h, C.byref(a2), c) == EINVAL and b"returns" in lib.m3pc_last_error()

    def bad(what, **kw):
        a2 = capi.PlanArgs.from_buffer_copy(args)
        c2 = capi.CertArgs.from_buffer_copy(cert)
        for k, v in kw.items():
            setattr(a2 if hasattr(a2, k) else c2, k, v)
        assert _call(lib, h, C.byref(a2), C.byref(c2)) == EINVAL, kw
        msg = lib.m3pc_last_error()
        assert what in msg, (kw, msg)

    # every check of the single-window certified step (tests/test_certified_step_cpu.py)
    bad(b"one rank", n_count=32)
    bad(b"one rank", n_begin=1, n_count=63)
    bad(b"n_total", n_total=20000, n_count=20000)
    bad(b"precision", precision=5)
    bad(b"slot", slot=4)
    bad(b"kmax", kmax=1000, rmax=32)
    bad(b"kmin", kmin=0)
    bad(b"kmin", kmin=33)
    bad(b"kmin", kmax=1024)
    bad(b"rmax", rmax=65)
    bad(b"rmax", n_total=16, n_count=16, kmin=6, rmax=17)
    bad(b"rfirst", rfirst=0)
    bad(b"rfirst", rfirst=33)
    bad(b"rfirst", rmax=0, rfirst=2)
    bad(b"delta", delta=-1.0)
    bad(b"delta", delta=float("nan"))
    bad(b"temperature", temperature=float("nan"))
    bad(b"mode", mode=3)


def test_select_batch_hook_is_in_the_lab_build_only():
    hdr = _header("m3pc_hip_debug.h")
    lab = C.CDLL(build.build_library(lab=True))
    prod = C.CDLL(build.build_library())
    assert re.search(r"\bint %s\(" % HOOK, hdr)
    assert HOOK not in _header()
    assert hasattr(lab, HOOK) and not hasattr(prod, HOOK)
    assert hasattr(lab, NAME) and prod.m3pc_abi_version() == lab.m3pc_abi_version() == 7
    # its refusals come before any launch
    vp, ci, cf, ll = C.c_void_p, C.c_int, C.c_float, C.c_longlong
    fn = lab.m3pc_debug_select_batch
    fn.restype = ci
    fn.argtypes = [vp, vp, ll, ll, ci, ci, ci, cf, vp, vp, vp, vp, vp, vp, vp]
    fake = 0x1000
    ok = dict(scores=fake, a0=fake, ws=64 * 6, st=6, E=2, n=64, A=3, expo=fake, ev=fake, si=fake)

    def call(**kw):
        f = dict(ok, **kw)
        return fn(f["scores"], f["a0"], f["ws"], f["st"], f["E"], f["n"], f["A"], 0.05, f["expo"], None, f["ev"], None, f["si"], None, None)

    for kw in (dict(scores=None), dict(n=0), dict(n=16385), dict(E=0), dict(a0=None), dict(A=0), dict(expo=None)):
        assert call(**kw) == EINVAL, kw


def test_example_is_plain_c_against_the_header(tmp_path):
    src = os.path.join(ROOT, "examples", "lockstep_steps.c")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "ls.o")])
    text = open(src).read()
    assert NAME in text and "m3pc_draw_variates" in text and "m3pc_calibrate_delta" in text
