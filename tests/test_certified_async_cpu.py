"""The pipelined certified step and the library's variates, without a GPU: the four new entry points are declared in
include/m3pc_hip.h, covered by csrc/exports.map, exported by the library and bound by m3pc_amd/capi.py with the header's
parameter lists; the ABI version did not move; null and bad arguments are refused before any HIP call is made."""
import ctypes as C
import fnmatch
import os
import re

import pytest

from m3pc_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m3pc_set_step_streams", "m3pc_plan_step_certified_begin", "m3pc_plan_step_certified_end", "m3pc_draw_variates")


@pytest.fixture(scope="module")
def lib():
    return capi.load_library(build.build_library())


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "m3pc_hip.h")).read(), flags=re.S)


def _params(name):
    """The parameter declarations of `int name(...)` in the header."""
    body = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _code(), flags=re.S).group(1)
    return [" ".join(p.split()) for p in body.split(",")]


def test_new_symbols_are_declared_exported_and_bound(lib):
    exported = re.findall(r"global:\s*([^;]+);", open(os.path.join(build.CSRC, "exports.map")).read())
    patterns = [p for e in exported for p in e.split()]
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, _code()), f"{name} is not declared in include/m3pc_hip.h"
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), f"{name} is not covered by csrc/exports.map"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in capi.EXPORTS
        assert getattr(lib, name).restype is C.c_int
    for meth in ("set_step_streams", "plan_step_certified_begin", "plan_step_certified_end", "draw_variates"):
        assert hasattr(capi.Handle, meth)
    assert lib.m3pc_abi_version() == 7 == capi.ABI_VERSION


def _ctype(decl):
    if "*" in decl:
        return {"const m3pc_plan_args*": C.POINTER(capi.PlanArgs), "const m3pc_cert_args*": C.POINTER(capi.CertArgs),
                "m3pc_cert_record*": C.POINTER(capi.CertRecord)}.get(decl.rsplit(" ", 1)[0], C.c_void_p)
    return {"int": C.c_int, "unsigned long long": C.c_ulonglong}[decl.rsplit(" ", 1)[0]]


@pytest.mark.parametrize("name", NEW)
def test_prototypes_agree_with_the_header(lib, name):
    want = [_ctype(p) for p in _params(name)]
    assert list(getattr(lib, name).argtypes) == want, (name, _params(name))


def test_begin_takes_the_serial_calls_arguments_without_the_record():
    serial, begin = _params("m3pc_plan_step_certified"), _params("m3pc_plan_step_certified_begin")
    assert [p for p in serial if "m3pc_cert_record" not in p] == begin
    assert int(re.search(r"#define M3PC_PLAN_INPUTS_READY (\d+)", _code()).group(1)) == capi.PLAN_INPUTS_READY == 4


def test_null_and_bad_arguments_are_refused_without_a_gpu(lib):
    fake = C.create_string_buffer(64)  # stands in for a handle: the argument checks come before the handle is touched
    h = C.c_void_p(C.addressof(fake))
    buf = C.create_string_buffer(64)
    p = C.c_void_p(C.addressof(buf))
    args = capi.PlanArgs(capi.MODE_RTG, capi.PREC_BF16, 4, 64, 0, 64, 0.6, 0.99, 3.0, 0, 0, None, 0, 0)
    cert = capi.CertArgs(0.01, 1.0, 0, 8, 32, 2, 32)

    def begin(h_=h, a=args, c=cert, ins=(p,) * 5, outs=(p,) * 3):
        return lib.m3pc_plan_step_certified_begin(h_, C.byref(a) if a is not None else None, C.byref(c) if c is not None else None, *ins,
                                                  None, None, *outs, None, None, None, None, None, None, None)

    assert begin(h_=None) == -1 and b"null" in lib.m3pc_last_error()
    assert begin(a=None) == -1 and begin(c=None) == -1
    for i in range(5):
        assert begin(ins=tuple(None if j == i else p for j in range(5))) == -1 and b"null" in lib.m3pc_last_error()
    for i in range(3):
        assert begin(outs=tuple(None if j == i else p for j in range(3))) == -1

    def bad(what, **kw):
        a2, c2 = capi.PlanArgs.from_buffer_copy(args), capi.CertArgs.from_buffer_copy(cert)
        for k, v in kw.items():
            setattr(a2 if hasattr(a2, k) else c2, k, v)
        assert begin(a=a2, c=c2) == -1, kw
        assert what in lib.m3pc_last_error(), (kw, lib.m3pc_last_error())

    bad(b"one rank", n_count=32)
    bad(b"n_total", n_total=20000, n_count=20000)
    bad(b"precision", precision=5)
    bad(b"slot", slot=4)
    bad(b"kmax", kmax=1000, rmax=32)
    bad(b"kmin", kmin=0)
    bad(b"kmin", kmin=33)
    bad(b"rmax", rmax=65)
    bad(b"rfirst", rfirst=0)
    bad(b"rfirst", rmax=0, rfirst=2)
    bad(b"delta", delta=-1.0)
    bad(b"delta", delta=float("nan"))
    rec = capi.CertRecord()
    assert lib.m3pc_plan_step_certified_end(None, 0, C.byref(rec), None) == -1 and b"null" in lib.m3pc_last_error()
    assert lib.m3pc_plan_step_certified_end(h, 0, None, None) == -1
    assert lib.m3pc_plan_step_certified_end(h, -1, C.byref(rec), None) == -1 and b"slot" in lib.m3pc_last_error()
    assert lib.m3pc_plan_step_certified_end(h, capi.SLOTS, C.byref(rec), None) == -1
    assert lib.m3pc_set_step_streams(None, None, None) == -1
    assert lib.m3pc_set_step_streams(h, p, None) == -1 and lib.m3pc_set_step_streams(h, p, p) == -1
    assert lib.m3pc_draw_variates(None, 1, 1, 0, 4, 3, None, None, None) == -1
    for b_, c_, r_ in ((-1, 4, 3), (0, 0, 3), (0, 4, 0), (2 ** 31 - 4, 8, 1), (0, 2 ** 20, 2 ** 14)):
        assert lib.m3pc_draw_variates(h, 1, 1, b_, c_, r_, None, None, None) == -1, (b_, c_, r_)
        assert b"m3pc_draw_variates" in lib.m3pc_last_error()
