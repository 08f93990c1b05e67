"""The eval_action certificate in the pipelined and the lock-step certified step, without a GPU: m3pc_plan_step_certified_eval_begin /
_eval_end and m3pc_plan_steps_certified_eval are declared, exported and bound, refuse bad arguments before any HIP call, the ABI
version did not move, and the header states their contracts instead of calling them out of scope."""
import ctypes as C
import os
import re

import pytest

from m3pc_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
NEW = ("m3pc_plan_step_certified_eval_begin", "m3pc_plan_step_certified_eval_end", "m3pc_plan_steps_certified_eval")


@pytest.fixture(scope="module")
def lib():
    return capi.load_library(build.build_library())


def _header():
    return open(os.path.join(ROOT, "include", "m3pc_hip.h")).read()


def test_the_three_symbols_are_declared_exported_and_bound(lib):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/m3pc_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in capi.EXPORTS
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    # the ctypes signatures follow the declarations: as many arguments, floats where the header has eval_tol
    for name in NEW:
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        params = [p.strip() for p in decl.split(",")]
        argtypes = getattr(lib, name).argtypes
        assert len(params) == len(argtypes), name
        for p, t in zip(params, argtypes):
            if p.startswith("float eval_tol"):
                assert t is C.c_float, (name, p)
            elif p.startswith("int "):
                assert t is C.c_int, (name, p)
            else:
                assert "*" in p and t not in (C.c_float, C.c_int), (name, p)


def test_abi_version_did_not_move(lib):
    assert lib.m3pc_abi_version() == 7 == capi.ABI_VERSION
    assert int(re.search(r"#define M3PC_ABI_VERSION (\d+)", _header()).group(1)) == 7


def test_header_states_the_contracts():
    h = _header()
    assert "Out of scope" not in h
    for phrase in ("m3pc_plan_step_certified_eval_begin", "returns M3PC_ESTATE and leaves the step", "m3pc_plan_steps_certified_eval"):
        assert phrase in h, phrase


def _step_args():
    fake = C.create_string_buffer(64)  # stands in for a handle and for every buffer: the checks come before anything is touched
    p = C.c_void_p(C.addressof(fake))
    args = capi.PlanArgs(capi.MODE_RTG, capi.PREC_BF16, 4, 64, 0, 64, 0.6, 0.99, 3.0, 0, 0, None, 0, 0)
    cert = capi.CertArgs(0.01, 1.0, 0, 8, 32, 2, 32)
    return fake, p, args, cert


def test_eval_begin_refuses_bad_arguments_without_a_gpu(lib):
    fake, p, args, cert = _step_args()

    def call(h=p, a=C.byref(args), c=C.byref(cert), tol=1e-3, req=p):
        return lib.m3pc_plan_step_certified_eval_begin(h, a, c, req, req, req, req, req, None, None, req, req, req, None, None, None, None,
                                                       None, None, tol, None)

    for kw in (dict(h=None), dict(a=None), dict(c=None), dict(req=None)):
        assert call(**kw) == EINVAL and b"null" in lib.m3pc_last_error(), kw
    for tol in (0.0, -1.0, float("nan")):
        assert call(tol=tol) == EINVAL and b"eval_tol" in lib.m3pc_last_error(), tol
    # the refusals of m3pc_plan_step_certified_begin come first
    a2 = capi.PlanArgs.from_buffer_copy(args)
    a2.n_count = 32
    assert call(a=C.byref(a2)) == EINVAL and b"one rank" in lib.m3pc_last_error()
    c2 = capi.CertArgs.from_buffer_copy(cert)
    c2.kmin = 0
    assert call(c=C.byref(c2), tol=0.0) == EINVAL and b"kmin" in lib.m3pc_last_error()
    a2 = capi.PlanArgs.from_buffer_copy(args)
    a2.slot = capi.SLOTS
    assert call(a=C.byref(a2)) == EINVAL and b"slot" in lib.m3pc_last_error()


def test_eval_end_refuses_bad_arguments_without_a_gpu(lib):
    fake, p, _, _ = _step_args()
    rec, erec = capi.CertRecord(), capi.EvalRecord()
    for h, r, e in ((None, C.byref(rec), C.byref(erec)), (p, None, C.byref(erec)), (p, C.byref(rec), None)):
        assert lib.m3pc_plan_step_certified_eval_end(h, 0, r, e, None) == EINVAL and b"null" in lib.m3pc_last_error()
    for slot in (-1, capi.SLOTS):
        assert lib.m3pc_plan_step_certified_eval_end(p, slot, C.byref(rec), C.byref(erec), None) == EINVAL and b"slot" in lib.m3pc_last_error()


def test_lockstep_eval_refuses_bad_arguments_without_a_gpu(lib):
    fake, p, args, cert = _step_args()
    E = 2
    recs, erecs = (capi.CertRecord * E)(), (capi.EvalRecord * E)()
    rtg = (C.c_double * E)(3.0, 3.0)

    def call(h=p, a=C.byref(args), c=C.byref(cert), n=E, rtg=rtg, recs=recs, tol=1e-3, erecs=erecs, req=p):
        return lib.m3pc_plan_steps_certified_eval(h, a, c, n, req, req, req, rtg, req, req, None, None, req, req, req, None, None, None, None,
                                                  None, None, recs, tol, erecs, None)

    for kw in (dict(h=None), dict(a=None), dict(c=None), dict(rtg=None), dict(recs=None), dict(erecs=None), dict(req=None)):
        assert call(**kw) == EINVAL and b"null" in lib.m3pc_last_error(), kw
    for tol in (0.0, -1.0, float("nan")):
        assert call(tol=tol) == EINVAL and b"eval_tol" in lib.m3pc_last_error(), tol
    # the refusals of m3pc_plan_steps_certified that need no handle
    assert call(n=0) == EINVAL and b"n_windows" in lib.m3pc_last_error()
    c2 = capi.CertArgs.from_buffer_copy(cert)
    c2.rfirst = 0
    assert call(c=C.byref(c2)) == EINVAL and b"rfirst" in lib.m3pc_last_error()
    a2 = capi.PlanArgs.from_buffer_copy(args)
    a2.mode = 7
    assert call(a=C.byref(a2)) == EINVAL and b"mode" in lib.m3pc_last_error()


def test_binding_has_the_new_keywords():
    import inspect
    assert "eval_tol" in inspect.signature(capi.Handle.plan_step_certified_begin).parameters
    assert "eval" in inspect.signature(capi.Handle.plan_step_certified_end).parameters
    assert "eval_tol" in inspect.signature(capi.Handle.plan_steps_certified).parameters
