"""The certified plan step as one C call, without a GPU: m3pc_plan_step_certified / m3pc_calibrate_delta are declared in
include/m3pc_hip.h, exported by the library and bound by m3pc_amd/capi.py; the two new structures have the header's layout; the
additions did not move the ABI version; null and bad arguments are refused before any HIP call is made."""
import ctypes as C
import os
import re

import pytest

from m3pc_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m3pc_plan_step_certified", "m3pc_calibrate_delta")


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
    assert hasattr(capi.Handle, "plan_step_certified") and hasattr(capi.Handle, "calibrate_delta")


def test_abi_version_did_not_move(lib):
    assert lib.m3pc_abi_version() == 7 == capi.ABI_VERSION
    assert int(re.search(r"#define M3PC_ABI_VERSION (\d+)", _header()).group(1)) == 7


def _struct_fields(name):
    """Field names of `typedef struct name { ... } name;` in the header, in declaration order (comments stripped)."""
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), code, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            out += [(ctype, n.strip()) for n in names.split(",")]
    return out


@pytest.mark.parametrize("cname,struct,size", [("m3pc_cert_args", capi.CertArgs, 28), ("m3pc_cert_record", capi.CertRecord, 48)])
def test_struct_layouts_match_the_header(cname, struct, size):
    assert C.sizeof(struct) == size
    fields = _struct_fields(cname)
    assert [n for _, n in fields] == [n for n, _ in struct._fields_]
    ctypes_of = {"int": C.c_int, "float": C.c_float}
    for i, ((ctype, n), (_, ct)) in enumerate(zip(fields, struct._fields_)):
        assert ct is ctypes_of[ctype], n
        assert getattr(struct, n).offset == 4 * i, n  # (4-byte fields only: the header's order IS the layout)


def _call(lib, h, a, c, rec, n_null=0):
    """m3pc_plan_step_certified with dummy non-null pointers everywhere (nothing is dereferenced before the checks pass)."""
    buf = C.create_string_buffer(64)
    p = C.c_void_p(C.addressof(buf))
    req = [p] * 5  # states, actions, rewards, eps, expo
    return lib.m3pc_plan_step_certified(h, a, c, *req, None, None, p, p, p, None, None, None, None, None, None, rec, None)


def test_null_and_bad_arguments_are_refused_without_a_gpu(lib):
    fake = C.create_string_buffer(64)  # stands in for a handle: the argument checks come before the handle is touched
    h = C.c_void_p(C.addressof(fake))
    args = capi.PlanArgs(capi.MODE_RTG, capi.PREC_BF16, 4, 64, 0, 64, 0.6, 0.99, 3.0, 0, 0, None, 0, 0)
    cert = capi.CertArgs(0.01, 1.0, 0, 8, 32, 2, 32)
    rec = capi.CertRecord()
    a, c, r = C.byref(args), C.byref(cert), C.byref(rec)
    assert _call(lib, None, a, c, r) == -1 and b"null" in lib.m3pc_last_error()
    assert _call(lib, h, None, c, r) == -1 and b"null" in lib.m3pc_last_error()
    assert _call(lib, h, a, None, r) == -1 and b"null" in lib.m3pc_last_error()
    assert _call(lib, h, a, c, None) == -1 and b"null" in lib.m3pc_last_error()

    def bad(what, **kw):
        a2 = capi.PlanArgs.from_buffer_copy(args)
        c2 = capi.CertArgs.from_buffer_copy(cert)
        for k, v in kw.items():
            setattr(a2 if hasattr(a2, k) else c2, k, v)
        assert _call(lib, h, C.byref(a2), C.byref(c2), r) == -1, kw
        msg = lib.m3pc_last_error()
        assert what in msg, (kw, msg)

    bad(b"one rank", n_count=32)
    bad(b"one rank", n_begin=1, n_count=63)
    bad(b"n_total", n_total=20000, n_count=20000)
    bad(b"precision", precision=5)
    bad(b"kmax", kmax=1000, rmax=32)          # kmax + rmax > 1023
    bad(b"kmin", kmin=0)
    bad(b"kmin", kmin=33)                     # kmin > kmax
    bad(b"kmin", kmax=1024)
    bad(b"rmax", rmax=65)                     # > 64
    bad(b"rmax", n_total=16, n_count=16, kmin=8, rmax=17)  # > n_total
    bad(b"rfirst", rfirst=0)
    bad(b"rfirst", rfirst=33)
    bad(b"rfirst", rmax=0, rfirst=2)
    bad(b"delta", delta=-1.0)
    bad(b"delta", delta=float("nan"))
    # m3pc_calibrate_delta
    buf = C.create_string_buffer(64)
    p = C.c_void_p(C.addressof(buf))
    out = C.c_float()
    assert lib.m3pc_calibrate_delta(None, a, p, p, p, p, p, 1.6, C.byref(out), None) == -1 and b"null" in lib.m3pc_last_error()
    assert lib.m3pc_calibrate_delta(h, a, p, p, p, p, None, 1.6, C.byref(out), None) == -1 and b"null" in lib.m3pc_last_error()
    assert lib.m3pc_calibrate_delta(h, a, p, p, p, p, p, 1.6, None, None) == -1 and b"null" in lib.m3pc_last_error()
    a2 = capi.PlanArgs.from_buffer_copy(args)
    a2.n_count = 10
    assert lib.m3pc_calibrate_delta(h, C.byref(a2), p, p, p, p, p, 1.6, C.byref(out), None) == -1 and b"one rank" in lib.m3pc_last_error()
    assert lib.m3pc_calibrate_delta(h, a, p, p, p, p, p, 0.0, C.byref(out), None) == -1 and b"factor" in lib.m3pc_last_error()
