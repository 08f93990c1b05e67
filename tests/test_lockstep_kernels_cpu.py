"""The lab hooks of the lock-step batch's tail kernels (include/m3pc_hip_debug.h) without a GPU: they are declared, the lab library
exports them and the product library does not, the ctypes mirror of m3pc_debug_tail_args in tests/test_lockstep_kernels_gpu.py has
the header's fields in the header's order, and every refusal comes before any HIP call (this machine has no device to call)."""
import ctypes as C
import os
import re

from m3pc_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("m3pc_debug_topk_race_batch", "m3pc_debug_gather_listed", "m3pc_debug_merge_select_batch")
EINVAL = -1
vp, ci, cf = C.c_void_p, C.c_int, C.c_float


def _lab():
    from test_lockstep_kernels_gpu import TailArgs
    lib = capi.load_library(build.build_library(lab=True))
    lib.m3pc_debug_topk_race_batch.restype = ci
    lib.m3pc_debug_topk_race_batch.argtypes = [vp, vp, cf, ci, ci, ci, ci, ci, vp, vp, vp]
    lib.m3pc_debug_gather_listed.restype = ci
    lib.m3pc_debug_gather_listed.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp]
    lib.m3pc_debug_merge_select_batch.restype = ci
    lib.m3pc_debug_merge_select_batch.argtypes = [C.POINTER(TailArgs)]
    return lib, TailArgs


def test_hooks_are_declared_and_exported_by_the_lab_build_only():
    hdr = open(os.path.join(ROOT, "include", "m3pc_hip_debug.h")).read()
    pub = open(os.path.join(ROOT, "include", "m3pc_hip.h")).read()
    lab = C.CDLL(build.build_library(lab=True))
    prod = C.CDLL(build.build_library())
    for name in HOOKS:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name not in pub
        assert hasattr(lab, name), name
        assert not hasattr(prod, name), name
    assert prod.m3pc_abi_version() == lab.m3pc_abi_version() == capi.ABI_VERSION == 7


def test_tail_args_mirror_follows_the_header():
    from test_lockstep_kernels_gpu import TailArgs
    hdr = open(os.path.join(ROOT, "include", "m3pc_hip_debug.h")).read()
    body = re.search(r"typedef struct m3pc_debug_tail_args \{(.*?)\} m3pc_debug_tail_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    ctype = {"int": ci, "float": cf, "long long": C.c_longlong}
    want = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const )?(void|float|int|long long)\s*(\*?)\s*(.*)", decl)
        base, ptr, names = m.group(2), m.group(3), m.group(4)
        for nm in names.split(","):
            nm = nm.strip()
            want.append((nm, "ptr" if ptr else ctype[base]))
    got = [(n, "ptr" if t in (vp, C.POINTER(ci), C.POINTER(cf)) else t) for n, t in TailArgs._fields_]
    assert got == want


def test_refusals_come_before_any_launch():
    lib, TailArgs = _lab()
    fake = 0x1000  # never dereferenced: every call below is refused on its arguments
    ok = dict(scores=fake, expo=fake, tau=0.05, E=2, n=64, kmax=16, kmin=1, rmax=4, lst=fake, ls=fake)

    def lists(**kw):
        a = dict(ok, **kw)
        return lib.m3pc_debug_topk_race_batch(a["scores"], a["expo"], a["tau"], a["E"], a["n"], a["kmax"], a["kmin"], a["rmax"], a["lst"],
                                              a["ls"], None)

    for bad in (dict(scores=None), dict(lst=None), dict(expo=None), dict(E=0), dict(n=0), dict(n=16385), dict(kmax=0), dict(kmax=1024),
                dict(kmin=0), dict(kmin=17), dict(rmax=-1), dict(rmax=65), dict(rmax=4, n=3)):
        assert lists(**bad) == EINVAL and lib.m3pc_last_error(), bad

    def gather(sa=fake, lst=fake, E=2, n=64, row=6, stride=21, lo=0, hi=4, cand=fake):
        return lib.m3pc_debug_gather_listed(sa, lst, E, n, row, stride, lo, hi, cand, None, None)

    for bad in (dict(sa=None), dict(lst=None), dict(cand=None), dict(E=0), dict(n=0), dict(row=0), dict(lo=-1), dict(lo=5, hi=4),
                dict(hi=22)):
        assert gather(**bad) == EINVAL, bad

    r, n, d = (ci * 2)(4, 2), (ci * 2)(8, 3), (cf * 2)(0.5, 0.25)

    def merge(**kw):
        f = dict(scores=fake, expo=fake, race=1, select=1, temperature=0.05, n_windows=2, n_total=64, list=fake, list_scores=fake,
                 list_rescored=fake, rmax=4, list_stride=21, f_stride=21, f_lo=0, r=r, n=n, delta=d, merged=fake, stats=fake, a0=fake,
                 a0_window_stride=64 * 6, a0_stride=6, A=3, eval_action=fake)
        f.update(kw)
        return lib.m3pc_debug_merge_select_batch(C.byref(TailArgs(**f)))

    assert lib.m3pc_debug_merge_select_batch(None) == EINVAL
    for bad in (dict(scores=None), dict(list=None), dict(list_scores=None), dict(list_rescored=None), dict(merged=None), dict(stats=None),
                dict(expo=None), dict(n_windows=0), dict(n_total=0), dict(n_total=16385), dict(rmax=65), dict(list_stride=4),
                dict(f_stride=0), dict(f_lo=-1), dict(a0=None), dict(r=(ci * 2)(5, 2)), dict(r=(ci * 2)(-1, 2)), dict(n=(ci * 2)(0, 3)),
                dict(n=(ci * 2)(8, 18)), dict(n=(ci * 2)(8, 65)), dict(delta=(cf * 2)(0.5, -0.25)), dict(delta=(cf * 2)(float("nan"), 0.0)),
                dict(race=0), dict(f_lo=1), dict(f_stride=11), dict(n_total=3)):
        assert merge(**bad) == EINVAL and lib.m3pc_last_error(), bad
