"""The certified plan step in two halves (m3pc_plan_step_certified_begin / _end) against the one call it splits
(m3pc_plan_step_certified): the same bits at any depth and in any order of the _ends, in every regime of the certificate, with
neighbours in flight; the state machine of the slots; the planner's opt-in and the C example."""
import ctypes as C
import os
import subprocess
import types
import warnings

import numpy as np
import pytest
import torch

from m3pc_amd import capi, synth
from m3pc_amd.planner import HipPlanner

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = lambda x: float(np.float32(x))
ESTATE, EINVAL = -2, -1
SHAPES = [("hopper", "rtg_guiding", 0.01, 625, 8, 4), ("walker2d", "critic_lambda_guiding", 1.0, 512, 16, 8)]
IDS = [f"{s[0]}-N{s[3]}" for s in SHAPES]
# multiples of the calibrated deviation (the grid of tests/test_certified_step_gpu.py) and 1e6, ordered so that neighbours in
# flight differ: small bounds (first pass enough / lists extended) beside large ones (window set / every candidate)
GRID = (0.0, 1e6, 0.5, 32.0, 1.0, 24.0, 2.0, 16.0, 4.0, 12.0, 8.0)
PATHS = [500, 37, 321, 998, 640, 77, 250, 123, 411]
CERT = dict(kmin=8, kmax=128, rfirst=2, rmax=32)
TENSORS = ("loc", "std", "sample_actions", "expect_return_low", "expect_return")


def _cfg(T, N, H, tau=0.01, guidance="rtg_guiding"):
    return types.SimpleNamespace(traj_length=T, action_samples=N, horizon=H, discount=0.99, temperature=tau, lmbda=0.6,
                                 plan_guidance=guidance, device="cuda")


def _planner(env, guidance, tau, N, T, H, precision="bf16", **kw):
    S, A = synth.ENV_DIMS[env]
    dims = synth.Dims(S, A, T)
    qsd, om, os_ = synth.make_critic(dims, 0) if guidance != "rtg_guiding" else (None, None, None)
    p = HipPlanner(_cfg(T, N, H, tau, guidance), synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), qsd, om, os_,
                   precision=precision, **kw)
    return p, dims


def _step_inputs(p, dims, N, seed=1, path_length=500, expo_seed=77, hist_seed=0):
    eps = synth.make_eps(N, dims, seed).cuda().reshape(N, -1).contiguous()
    q = torch.empty(N, dtype=torch.float32).exponential_(1, generator=torch.Generator().manual_seed(expo_seed)).cuda()
    hist = synth.make_history(dims, hist_seed)
    hist["path_length"] = path_length
    s, a, r, h, rtg = p.assemble_window(hist, rtg=3.0)
    return eps, q, (s.clone(), a.clone(), r.clone(), h, rtg)


class Bench:
    """One shape: a handle, `n` steps' inputs and the deviation a calibration on the first of them returns."""

    def __init__(self, shape, n_steps, same_window=False):
        env, guidance, self.tau, self.N, T, H = shape
        self.mode = capi.MODE_RTG if guidance == "rtg_guiding" else capi.MODE_CRITIC
        self.p, self.dims = _planner(env, guidance, self.tau, self.N, T, H, rescore_delta=1.0)
        self.hd = self.p.handle
        self.steps = [_step_inputs(self.p, self.dims, self.N) if same_window else
                      _step_inputs(self.p, self.dims, self.N, seed=1 + t, path_length=PATHS[t % len(PATHS)], expo_seed=77 + t, hist_seed=t)
                      for t in range(n_steps)]
        eps, q, (s, a, r, h, rtg) = self.steps[0]
        self.hd.policy_pass(self.mode, s, a, r, h, rtg, slot=0)
        self.dev = {}
        for prec in (capi.PREC_BF16, capi.PREC_BF16X3):
            low = self.hd.candidate_pass(self.mode, s, a, r, eps, h, 0.6, 0.99, self.N, precision=prec, slot=0)["expect_return"]
            self.dev[prec] = self.hd.calibrate_delta(self.mode, s, a, r, eps, low, h, 0.6, 0.99, self.N, factor=1.0, slot=0)
        self.dev[capi.PREC_FP32] = 0.0
        torch.cuda.synchronize()

    def args(self, t, delta, grow, prec, slot, **cert):
        eps, q, (s, a, r, h, rtg) = self.steps[t]
        kw = dict(CERT, delta=delta, grow_delta=grow, precision=prec, slot=slot)
        kw.update(cert)
        return (self.mode, s, a, r, eps, q, h, rtg, 0.6, 0.99, self.N, self.tau), kw

    def serial(self, t, delta, grow, prec, slot=0, **cert):
        a, kw = self.args(t, delta, grow, prec, slot, **cert)
        res, rec = self.hd.plan_step_certified(*a, **kw)
        torch.cuda.synchronize()
        return res, rec

    def begin(self, t, delta, grow, prec, slot, **cert):
        a, kw = self.args(t, delta, grow, prec, slot, **cert)
        return self.hd.plan_step_certified_begin(*a, **kw)

    def close(self):
        self.hd.close()


def _fields(rec):
    return {n: getattr(rec, n) for n, _ in capi.CertRecord._fields_}


def _same(got, rec, want, wrec, what, rmax=CERT["rmax"]):
    """Every output tensor torch.equal and every record field equal.  (list: the entries the step re-scored, as documented --
    the buffer beyond them is not written.)"""
    assert bytes(rec) == bytes(wrec), (what, _fields(rec), _fields(wrec))
    for k in TENSORS:
        assert torch.equal(got[k], want[k]), (what, k)
    for i, name in enumerate(("p", "eval_action", "argmax", "sample_idx", "sample_action")):
        assert torch.equal(got["sel"][i], want["sel"][i]), (what, name)
    if not rec.everything:
        lo, hi = rmax - rec.n_race, rmax + rec.n_rescored
        assert torch.equal(got["list"][lo:hi], want["list"][lo:hi]), (what, "list")


def _regime(rec, kmin=CERT["kmin"], rfirst=CERT["rfirst"]):
    if rec.everything:
        return "everything"
    if rec.saturated:
        return "saturated"
    return "extended" if rec.n_rescored > kmin or rec.n_race > rfirst else "first"


def _run_groups(b, deltas, grow, prec, depth, reverse, twins, what):
    """The steps in groups of `depth`: every step of a group begun (slots 0 .. depth - 1), then ended in issue or reversed
    order, each compared with its serial twin."""
    n = len(deltas)
    for g0 in range(0, n, depth):
        group = list(range(g0, min(n, g0 + depth)))
        res = {t: b.begin(t, deltas[t], grow, prec, slot=t - g0) for t in group}
        for t in (reversed(group) if reverse else group):
            rec = b.hd.plan_step_certified_end(t - g0)
            torch.cuda.synchronize()
            _same(res[t], rec, *twins[t], (what, "depth", depth, "reversed", reverse, "step", t))


# ---------------------------------------------------------------------------------------------- 1. bit identity at depth
@pytest.fixture(scope="module")
def benches():
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = Bench(shape, 9)
        return made[shape]

    yield get
    for b in made.values():
        b.close()


@pytest.mark.parametrize("prec", ["bf16", "bf16x3", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_begin_end_equals_the_serial_call_at_every_depth(benches, shape, prec):
    """9 steps with distinct windows and variates under a fixed bound (1.6 x the calibrated deviation of the precision), at
    depths 1 .. 4, the _ends in issue order and reversed within each group: every output tensor and every record field equals
    the serial m3pc_plan_step_certified of the same step (run in another slot: the slot picks workspaces, not arithmetic)."""
    b = benches(shape)
    code = capi.PRECISIONS[prec]
    delta = f32(1.6 * b.dev[code])
    deltas = [delta] * 9
    twins = [b.serial(t, delta, False, code, slot=(t + 1) % capi.SLOTS) for t in range(9)]
    print(f"{shape[0]} {prec}: delta {delta:.4g}; serial n_rescored {[r.n_rescored for _, r in twins]} rounds {[r.rounds for _, r in twins]}")
    for depth in (1, 2, 3, 4):
        for reverse in (False, True):
            _run_groups(b, deltas, False, code, depth, reverse, twins, (shape[0], prec))


# ---------------------------------------------------------------------------------------------- 2. mixed regimes in flight
@pytest.fixture(scope="module")
def mixed():
    """grow_delta = 0 and a bound per step from the grid, on the window and variates of the serial call's own sweep: the serial
    records (the regimes are a condition on these inputs) and, per depth, what differed between a step and its serial twin."""
    out = {}
    for shape in SHAPES:
        b = Bench(shape, len(GRID), same_window=True)
        deltas = [f32(m * b.dev[capi.PREC_BF16]) if m < 1e6 else 1e6 for m in GRID]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            twins = [b.serial(t, deltas[t], False, capi.PREC_BF16, slot=t % capi.SLOTS) for t in range(len(GRID))]
            regimes = [_regime(r) for _, r in twins]
            print(f"{shape[0]}: regimes {list(zip(GRID, regimes))}")
            errs = []
            for depth, reverse in ((4, False), (4, True), (3, False), (2, True)):
                try:
                    _run_groups(b, deltas, False, capi.PREC_BF16, depth, reverse, twins, shape[0])
                except AssertionError as e:
                    errs.append(str(e) or repr(e))
        out[shape] = (regimes, errs)
        b.close()
    return out


def test_the_mixed_steps_visit_every_regime(mixed):
    seen = {r for regimes, _ in mixed.values() for r in regimes}
    assert seen == {"first", "extended", "saturated", "everything"}, {k[0]: v[0] for k, v in mixed.items()}


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_mixed_regimes_in_flight_equal_their_serial_twins(mixed, shape):
    """First-pass, extended, window-set and every-candidate steps in flight side by side: the slow paths of one step run beside
    (and are ordered against) the candidate passes of its neighbours, and every step still equals its serial twin."""
    regimes, errs = mixed[shape]
    assert not errs, (regimes, errs)


# ---------------------------------------------------------------------------------------------- 3. delta growth
def test_growing_delta_from_zero_equals_the_serial_call(benches):
    """grow_delta = 1 and delta = 0 going in: the record's delta (1.5 x the deviation the step saw) and rounds are the serial
    call's, four steps in flight."""
    b = benches(SHAPES[0])
    twins = [b.serial(t, 0.0, True, capi.PREC_BF16, slot=3 - t) for t in range(4)]
    print(f"grown deltas {[r.delta for _, r in twins]} deviations {[r.deviation for _, r in twins]} rounds {[r.rounds for _, r in twins]}")
    for _, rec in twins:
        # a condition on the inputs: every step raised delta (to 1.5 x the largest deviation any of its merges saw -- the last
        # merge's, which the record carries, need not be the largest: the shift moves with the listed set) and merged again
        assert rec.delta >= f32(1.5 * float(rec.deviation)) > 0 and rec.rounds >= 2 and rec.certified == 1, _fields(rec)
    for reverse in (False, True):
        _run_groups(b, [0.0] * 4, True, capi.PREC_BF16, 4, reverse, twins, "growth")


# ---------------------------------------------------------------------------------------------- 4. state and arguments
def test_state_errors_and_bad_arguments_leave_the_handle_usable(benches):
    b = benches(SHAPES[0])
    hd, lib = b.hd, b.hd.lib
    delta = f32(1.6 * b.dev[capi.PREC_BF16])
    twin = b.serial(0, delta, False, capi.PREC_BF16)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def good(what):
        res = b.begin(0, delta, False, capi.PREC_BF16, slot=1)
        rec = hd.plan_step_certified_end(1)
        torch.cuda.synchronize()
        _same(res, rec, *twin, what)

    def code(fn, *a, **kw):
        try:
            fn(*a, **kw)
        except capi.M3pcError as e:
            return int(str(e).split()[2].rstrip(":"))
        return 0

    rec = capi.CertRecord()
    # idle slot
    assert lib.m3pc_plan_step_certified_end(hd._h, 2, C.byref(rec), st) == ESTATE
    assert lib.m3pc_plan_step_certified_end(hd._h, capi.SLOTS, C.byref(rec), st) == EINVAL
    assert lib.m3pc_plan_step_certified_end(hd._h, 0, None, st) == EINVAL
    good("after idle-slot errors")
    # busy slot, and the serial calls with a step begun
    res = b.begin(0, delta, False, capi.PREC_BF16, slot=1)
    assert code(b.begin, 1, delta, False, capi.PREC_BF16, slot=1) == ESTATE
    assert code(b.serial, 1, delta, False, capi.PREC_BF16, slot=0) == ESTATE
    eps, q, (s, a, r, h, rtg) = b.steps[0]
    assert code(hd.calibrate_delta, b.mode, s, a, r, eps, res["expect_return_low"], h, 0.6, 0.99, b.N, slot=0) == ESTATE
    assert code(hd.set_step_streams, None, None) == ESTATE
    rec1 = hd.plan_step_certified_end(1)
    torch.cuda.synchronize()
    _same(res, rec1, *twin, "the step the refused calls found in flight")
    # bad arguments: refused, nothing begun
    for kw in (dict(kmin=0), dict(kmin=200), dict(kmax=1024), dict(rmax=65), dict(rfirst=0), dict(kmax=1000), dict(delta=-1.0)):
        kw2 = dict(delta=delta)
        kw2.update(kw)
        d = kw2.pop("delta")
        assert code(b.begin, 0, d, False, capi.PREC_BF16, slot=1, **kw2) == EINVAL, kw
    args = hd._args(b.mode, capi.PREC_BF16, h, b.N, 0, b.N, 0.6, 0.99, rtg, 1)
    cert = capi.CertArgs(b.tau, delta, 0, 8, 128, 2, 32)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    out = [torch.empty(b.N * h * b.dims.action_dim, device="cuda"), torch.empty(b.N, device="cuda"), torch.empty(b.N, device="cuda")]
    ins = [ptr(s), ptr(a), ptr(r), ptr(eps), ptr(q)]
    for null in range(5):
        bad = list(ins)
        bad[null] = None
        assert lib.m3pc_plan_step_certified_begin(hd._h, C.byref(args), C.byref(cert), *bad, None, None, ptr(out[0]), ptr(out[1]), ptr(out[2]),
                                                  None, None, None, None, None, None, st) == EINVAL
    assert lib.m3pc_plan_step_certified_begin(hd._h, C.byref(args), C.byref(cert), *ins, None, None, ptr(out[0]), None, ptr(out[2]),
                                              None, None, None, None, None, None, st) == EINVAL
    assert lib.m3pc_plan_step_certified_end(hd._h, 1, C.byref(rec), st) == ESTATE  # (none of them began a step)
    good("after bad arguments")


def test_destroy_with_a_step_begun_returns():
    b = Bench(SHAPES[0], 2)
    delta = f32(1.6 * b.dev[capi.PREC_BF16])
    keep = [b.begin(0, delta, False, capi.PREC_BF16, slot=0), b.begin(1, delta, False, capi.PREC_BF16, slot=1)]
    b.close()  # (m3pc_destroy drains: the steps' kernels are through before the handle's buffers go)
    torch.cuda.synchronize()
    assert all(0 <= int(res["expect_return_low"].argmax()) < b.N for res in keep)


# ---------------------------------------------------------------------------------------------- 5. the planner's opt-in
def _lab_planner(*a, **kw):
    """A planner whose handle lives in libm3pc_hip_lab.so (the same sources with -DM3PC_LAB: the product ABI plus the hooks of
    include/m3pc_hip_debug.h), for the lab-only counter of the streams a handle created for its pipelined steps."""
    from hip_util import lab_library
    lab = lab_library()
    lab.m3pc_debug_step_streams_created.restype = C.c_int
    lab.m3pc_debug_step_streams_created.argtypes = [C.c_void_p]
    prod, capi._lib = capi._lib, lab
    try:
        p, dims = _planner(*a, **kw)
    finally:
        capi._lib = prod
    assert p.handle.lib is lab
    return p, dims, lab


def test_native_pipelined_planner_equals_the_default_planner():
    """HipPlanner(native_step=True) against the default: plan_async at depth 3 over 8 windows from the same generator seed, with
    calibration on (calibration_factor 1.625 is a float: tests/test_certified_step_gpu.py).  The library was given the planner's
    chain-stream pair and created no stream of its own."""
    env, guidance, tau, N, T, H = SHAPES[0]
    kw = dict(calibration_windows=4, calibration_factor=1.625)
    pn, dims, lab = _lab_planner(env, guidance, tau, N, T, H, native_step=True, generator=torch.Generator(device="cuda").manual_seed(5), **kw)
    pd, _ = _planner(env, guidance, tau, N, T, H, native_step=False, generator=torch.Generator(device="cuda").manual_seed(5), **kw)
    runs = []
    for p in (pn, pd):
        tickets, got = [], []
        for t in range(8):
            hist = synth.make_history(dims, t)
            hist["path_length"] = PATHS[t]
            tickets.append(p.plan_async(hist, eval=bool(t & 1), rtg=3.0))
            if len(tickets) == 3:
                tk = tickets.pop(0)
                got.append((tk.result().clone(), dict(tk.info)))
        for tk in tickets:
            got.append((tk.result().clone(), dict(tk.info)))
        torch.cuda.synchronize()
        runs.append(got)
    for t, ((an, ln), (ad, ld)) in enumerate(zip(*runs)):
        assert an.shape == ad.shape and torch.equal(an, ad), t
        assert torch.equal(ln["argmax"], ld["argmax"]) and torch.equal(ln["sample_idx"], ld["sample_idx"]), t
        assert torch.equal(ln["expect_return"], ld["expect_return"]), t
        assert ln["n_rescored"] == ld["n_rescored"] and ln["n_race"] == ld["n_race"], (t, ln["n_rescored"], ld["n_rescored"])
        assert f32(ln["delta"]) == f32(ld["delta"]), (t, ln["delta"], ld["delta"])
    print(f"n_rescored {[l['n_rescored'] for _, l in runs[0]]} delta {[l['delta'] for _, l in runs[0]]}")
    assert f32(pn._delta0) == f32(pd._delta0)
    assert pn.fp32_fallback == pd.fp32_fallback and pn.fallback_precision == pd.fallback_precision  # the fallback decision
    assert pn._cal_left == pd._cal_left == 0
    assert pn._step_streams_set and pn.handle._step_streams == pn._chain_streams()
    assert lab.m3pc_debug_step_streams_created(pn.handle._h) == 0
    pn.handle.close()
    pd.handle.close()


def test_a_handle_without_a_registered_pair_creates_its_two_streams_once():
    env, guidance, tau, N, T, H = SHAPES[0]
    p, dims, lab = _lab_planner(env, guidance, tau, N, T, H, rescore_delta=1.0)
    hd = p.handle
    eps, q, (s, a, r, h, rtg) = _step_inputs(p, dims, N)
    assert lab.m3pc_debug_step_streams_created(hd._h) == 0
    for _ in range(2):
        res = hd.plan_step_certified_begin(capi.MODE_RTG, s, a, r, eps, q, h, rtg, 0.6, 0.99, N, tau, delta=1.0, slot=0, **CERT)
        rec = hd.plan_step_certified_end(0)
        torch.cuda.synchronize()
        assert rec.certified == 1 and 0 <= int(res["sel"][2]) < N
        assert lab.m3pc_debug_step_streams_created(hd._h) == 2
    hd.close()


# ---------------------------------------------------------------------------------------------- 6. the C example
def test_c_example_pipelines_six_windows(tmp_path):
    """examples/pipelined_steps.c compiled with gcc -Wall -Werror against include/m3pc_hip.h, linked to the built library and
    run on 6 windows: every step's arg-max and multinomial index are the serial call's on the variates m3pc_draw_variates gives
    for that step index."""
    so = tmp_path / "libpipelined_steps.so"
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "pipelined_steps.c"), "-o", str(so), "-L", libdir,
                           "-l:" + os.path.basename(capi.LIB_PATH), "-Wl,-rpath," + libdir])
    env, guidance, tau, N, T, H = SHAPES[0]
    K, seed = 6, 2024
    b = Bench(SHAPES[0], K)
    p, dims, hd = b.p, b.dims, b.hd
    A, S = dims.action_dim, dims.state_dim
    h, rtg = b.steps[0][2][3], b.steps[0][2][4]
    assert all(st[2][3] == h for st in b.steps), "the example plans one horizon"
    fp, vp = C.POINTER(C.c_float), C.c_void_p

    class IO(C.Structure):
        _fields_ = [("dims", C.POINTER(capi.Dims)), ("weights", C.POINTER(capi.NamedTensor)), ("n_weights", C.c_int),
                    ("tok_mean", fp * 4), ("tok_std", fp * 4), ("tok_dim", C.c_int * 4), ("tok_normalize", C.c_int * 4),
                    ("n_windows", C.c_int), ("states", vp), ("actions", vp), ("rewards", vp), ("n", C.c_int), ("horizon", C.c_int),
                    ("rtg", C.c_double), ("lmbda", C.c_double), ("discount", C.c_double), ("temperature", C.c_float),
                    ("seed", C.c_ulonglong), ("eps", vp), ("expo", vp),
                    ("sample_actions", vp), ("scores_low", vp), ("merged", vp), ("eval_action", vp), ("argmax", vp),
                    ("sample_idx", vp), ("sample_action", vp), ("records", C.POINTER(capi.CertRecord)), ("delta", C.c_float)]

    sd = synth.make_state_dict(dims, 0)
    arr, keep = capi._named(sd)
    io = IO()
    io.dims, io.weights, io.n_weights = C.pointer(hd.dims), C.cast(arr, C.POINTER(capi.NamedTensor)), len(sd)
    toks = []
    for k, name in enumerate(capi.KEYS):
        t = p.tokenizer_manager.tokenizers[name]
        m, sdv = t._data_mean.float().contiguous().reshape(-1), t._data_std.float().contiguous().reshape(-1)
        toks.append((m, sdv))
        io.tok_mean[k], io.tok_std[k] = C.cast(m.data_ptr(), fp), C.cast(sdv.data_ptr(), fp)
        io.tok_dim[k], io.tok_normalize[k] = m.numel(), int(bool(t.normalize))
    dev = dict(device="cuda")
    wins = dict(states=torch.stack([st[2][0] for st in b.steps]).contiguous(), actions=torch.stack([st[2][1] for st in b.steps]).contiguous(),
                rewards=torch.stack([st[2][2] for st in b.steps]).contiguous())
    bufs = dict(eps=torch.empty((capi.SLOTS, N, T * A), **dev), expo=torch.empty((capi.SLOTS, N), **dev),
                sample_actions=torch.empty((K, N, h, A), **dev), scores_low=torch.empty((K, N), **dev), merged=torch.empty((K, N), **dev),
                eval_action=torch.empty((K, A), **dev), argmax=torch.full((K,), -1, dtype=torch.int32, **dev),
                sample_idx=torch.full((K,), -1, dtype=torch.int32, **dev), sample_action=torch.empty((K, A), **dev))
    for name, t in dict(**wins, **bufs).items():
        setattr(io, name, t.data_ptr())
    records = (capi.CertRecord * K)()
    io.records = C.cast(records, C.POINTER(capi.CertRecord))
    io.n_windows, io.n, io.horizon, io.rtg, io.lmbda, io.discount, io.temperature, io.seed = K, N, h, rtg, 0.6, 0.99, tau, seed
    torch.cuda.synchronize()
    lib = C.CDLL(str(so))
    lib.pipelined_steps.restype = C.c_int
    lib.pipelined_steps.argtypes = [C.POINTER(IO), C.c_int, vp]
    rc = lib.pipelined_steps(C.byref(io), torch.cuda.current_device(), vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, hd.lib.m3pc_last_error()
    torch.cuda.synchronize()
    assert io.delta > 0
    for t in range(K):
        eps, q = hd.draw_variates(seed, t, N, T * A)
        s, a, r = b.steps[t][2][:3]
        res, rec = hd.plan_step_certified(capi.MODE_RTG, s, a, r, eps, q, h, rtg, 0.6, 0.99, N, tau, delta=io.delta, grow_delta=True,
                                          kmin=6, kmax=128, rfirst=2, rmax=32, precision=capi.PREC_BF16, slot=0)
        torch.cuda.synchronize()
        print(f"window {t}: C argmax {int(bufs['argmax'][t])} sample_idx {int(bufs['sample_idx'][t])}, serial {int(res['sel'][2])} "
              f"{int(res['sel'][3])}; n_rescored {records[t].n_rescored} n_race {records[t].n_race}")
        assert records[t].certified == 1
        assert int(bufs["argmax"][t]) == int(res["sel"][2]) and int(bufs["sample_idx"][t]) == int(res["sel"][3]), t
    del keep, toks
    b.close()
