"""The certified plan step as ONE C call (m3pc_plan_step_certified) and the on-device calibration of its bound
(m3pc_calibrate_delta), against the Python protocol they restate (m3pc_amd/certificate.py:resolve, HipPlanner._enqueue_tail /
_rescore_window_set / _calibrate).

delta crosses the C ABI as a float while the Python planner keeps Python floats (doubles); every kernel sees float(delta) either
way (ctypes rounds at the call).  The tests therefore hand both sides float-representable bounds, and where the Python side
forms a bound itself (1.5 x a deviation, factor x a deviation: 25-28 significant bits) they compare it rounded once to float
-- the value the kernels got."""
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
GD = os.path.join(ROOT, "tests", "golden")
f32 = lambda x: float(np.float32(x))


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


# ---------------------------------------------------------------------------------------------- 1. the statistics kernel
@pytest.mark.parametrize("n", [1, 2, 3, 625, 1024, 4096, 16384])
def test_deviation_statistics_against_torch(n):
    """deviation_stats_kernel on synthetic low-precision scores b = f + 3.25 + noise with two exact ties planted in d = b - f:
    the lower median is torch's (sort(d)[(n - 1) // 2], the element torch.median returns), the deviation and the scale are exact
    (max is exact in any order), and the bound is max(factor dev, 1e-6 max|f|, 1e-30) formed in double and rounded once."""
    from hip_util import lab_library
    lib = lab_library()
    fn = lib.m3pc_debug_calibrate_stats
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.POINTER(C.c_float), C.c_void_p]
    g = torch.Generator(device="cuda").manual_seed(100 + n)
    f = (torch.randn(n, device="cuda", generator=g) * 15.0 + 100.0).contiguous()
    d0 = 3.25 + (torch.rand(n, device="cuda", generator=g) - 0.5) * 2.0
    if n >= 8:
        # two exact ties in d (b = f + d0 rounds, so plant them on the values the kernel sees: d = b - f); one of them AT the
        # median, so that the (value, index) order is what decides the rank there
        b = f + d0
        d = b - f
        order = torch.argsort(d)
        mid, far = int(order[(n - 1) // 2]), int(order[n // 4])
        for src, dst in ((mid, int(order[(n - 1) // 2 + 1])), (far, int(order[n // 4 + 1]))):
            f[dst] = f[src]
            b[dst] = b[src]
        b = b.contiguous()
    else:
        b = (f + d0).contiguous()
    d = b - f
    if n >= 8:
        assert int((d == d[mid]).sum()) >= 2 and int((d == d[far]).sum()) >= 2
    stats = torch.full((8,), float("nan"), device="cuda")
    out = C.c_float()
    factor = 1.6
    rc = fn(b.data_ptr(), f.data_ptr(), n, factor, stats.data_ptr(), C.byref(out), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.m3pc_last_error()
    st = stats.cpu().tolist()
    c = torch.sort(d).values[(n - 1) // 2]
    assert st[0] == float(c) == float(d.median())
    dev = float((d - c).abs().max())
    assert st[1] == dev
    assert st[2] == float(f.abs().max())
    want = np.float32(max(float(np.float32(factor)) * dev, 1e-6 * float(f.abs().max()), 1e-30))
    print(f"n {n}: c {st[0]!r} dev {st[1]!r} scale {st[2]!r} delta {out.value!r} want {float(want)!r}")
    assert np.float32(out.value) == want


# ---------------------------------------------------------------------------------------------- helpers of 2-4
def _step_inputs(p, dims, N, seed=1, path_length=500, expo_seed=77):
    eps = synth.make_eps(N, dims, seed).cuda()
    q = torch.empty(N, dtype=torch.float32).exponential_(1, generator=torch.Generator().manual_seed(expo_seed)).cuda()
    hist = synth.make_history(dims, 0)
    hist["path_length"] = path_length
    s, a, r, h, rtg = p.assemble_window(hist, rtg=3.0)
    return eps, q, (s.clone(), a.clone(), r.clone(), h, rtg)


def _kmax(p, N):
    return max(min(p.rescore_max, N - 1 if N > 1 else 1, 1024 - p._R - 1), 1)


def _regime(last, N):
    if last["n_rescored"] >= N:
        return "everything"
    if last["saturated"]:
        return "saturated"
    if last["n_rescored"] > last["n_first"] or last["n_race"] > last["n_race_first"]:
        return "extended"
    return "first"


def _assert_same_step(res, rec, last, what):
    sel = res["sel"]
    assert torch.equal(sel[2], last["argmax"]), what
    assert torch.equal(sel[3], last["sample_idx"]), what
    assert torch.equal(sel[4], last["sample_action"]), what
    assert torch.equal(sel[1], last["eval_action"]), what
    assert torch.equal(res["expect_return"], last["expect_return"]), what
    got = dict(n_rescored=rec.n_rescored, n_race=rec.n_race, need_first=rec.need_first, need_race_first=rec.need_race_first,
               saturated=bool(rec.saturated), certified=bool(rec.certified), delta=rec.delta, shift=rec.shift, deviation=rec.deviation)
    want = dict(n_rescored=last["n_rescored"], n_race=last["n_race"], need_first=last["n_in_window"], need_race_first=last["need_race"],
                saturated=bool(last["saturated"]), certified=bool(last["certified"]), delta=f32(last["delta"]), shift=f32(last["shift"]),
                deviation=f32(last["deviation"]))
    assert got == want, (what, got, want)


SHAPES = [("hopper", "rtg_guiding", 0.01, 625, 8, 4), ("walker2d", "critic_lambda_guiding", 1.0, 512, 16, 8),
          ("hopper", "rtg_guiding", 0.01, 2048, 8, 4)]
# the issue's multiples of the calibrated deviation, and four more: up to 8 x the arg-max certificate of these shapes asks for fewer
# than rescore_max = 128 candidates (scores spread with sigma ~ 5 deviations: 128 of 625 lie within ~ 11 deviations of the best, 128
# of 2048 within ~ 9), so the window set -- more than 128, fewer than all -- needs bounds between those and the everything end
GRID = (0.0, 0.5, 1.0, 2.0, 4.0, 8.0, 12.0, 16.0, 24.0, 32.0)


@pytest.fixture(scope="module")
def sweep():
    """Fixed delta (rescore_delta on the planner, grow_delta = 0 on the call), the same eps / expo / window, every shape and every
    delta of the grid -- multiples of the deviation a calibration on the shape returns, and 1e6 -- once for the tests below:
    {shape: [(delta, the Python planner's regime, None or what differed)]}."""
    rows = {}
    for shape in SHAPES:
        env, guidance, tau, N, T, H = shape
        mode = capi.MODE_RTG if guidance == "rtg_guiding" else capi.MODE_CRITIC
        p, dims = _planner(env, guidance, tau, N, T, H, rescore_delta=1.0)
        hd = p.handle
        eps, q, (s, a, r, h, rtg) = _step_inputs(p, dims, N)
        p._draw_expo = lambda: q
        # the deviation a calibration on this step returns (factor 1: the bound IS the deviation unless the 1e-6 floor rules)
        hd.policy_pass(mode, s, a, r, h, rtg, slot=0)
        low = hd.candidate_pass(mode, s, a, r, eps, h, 0.6, 0.99, N, precision=capi.PREC_BF16, slot=0)["expect_return"]
        dev = hd.calibrate_delta(mode, s, a, r, eps, low, h, 0.6, 0.99, N, factor=1.0, slot=0)
        assert dev > 1e-5 * float(low.abs().max())
        rows[shape] = []
        for delta in [f32(m * dev) for m in GRID] + [1e6]:
            p._delta_fixed = p._delta0 = delta
            p._hist = {}
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")  # (the slow paths warn once)
                p._guide(mode, s, a, r, rtg, h, 0.6, eps=eps)
            last = dict(p.last)
            reg = _regime(last, N)
            res, rec = hd.plan_step_certified(mode, s, a, r, eps, q, h, rtg, 0.6, 0.99, N, tau, delta=delta, grow_delta=False,
                                              kmin=last["n_first"], kmax=_kmax(p, N), rfirst=last["n_race_first"], rmax=p._R,
                                              precision=capi.PREC_BF16, slot=0)
            torch.cuda.synchronize()
            print(f"{env} N {N} delta {delta:.4g} ({reg}): python n_rescored {last['n_rescored']} n_race {last['n_race']} need "
                  f"{last['n_in_window']}/{last['need_race']}; call n_rescored {rec.n_rescored} n_race {rec.n_race} need "
                  f"{rec.need_first}/{rec.need_race_first} saturated {rec.saturated} everything {rec.everything} rounds {rec.rounds}")
            err = None
            try:
                _assert_same_step(res, rec, last, (env, N, delta, reg))
                assert bool(rec.everything) == (reg == "everything"), "everything"
                assert torch.equal(res["expect_return_low"], last["expect_return_bf16"]), "low-precision scores"
                if not rec.everything:  # the final lists: race entries in front of rmax, score entries behind
                    assert set(res["list"][p._R : p._R + rec.n_rescored].tolist()) == set(last["topk"].tolist()), "score list"
                    assert set(res["list"][p._R - rec.n_race : p._R].tolist()) == set(last["race"].tolist()), "race list"
            except AssertionError as e:
                err = str(e) or repr(e)
            rows[shape].append((delta, reg, err))
        p.handle.close()
    return rows


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}-N{s[3]}")
def test_one_call_equals_the_python_protocol(sweep, shape):
    """For every delta of the sweep the one call ends on the Python protocol's tensors (argmax, sample_idx, sample_action,
    eval_action, merged: torch.equal) and on its record (n_rescored, n_race, both first certificates, saturated, certified,
    delta, shift, deviation)."""
    bad = [(d, reg, err) for d, reg, err in sweep[shape] if err is not None]
    assert not bad, bad


def test_the_sweep_visits_every_regime(sweep):
    """A condition on the INPUTS of the test above, read from the Python planner's records: first pass enough, lists extended,
    window set (saturated) and every candidate in fp32 all occur."""
    seen = {reg for rows in sweep.values() for _, reg, _ in rows}
    assert seen == {"first", "extended", "saturated", "everything"}, {k[0] + str(k[3]): [r for _, r, _ in v] for k, v in sweep.items()}


# ---------------------------------------------------------------------------------------------- 3. short first pass, golden step
def _golden_step(prec):
    p, dims = _planner("hopper", "rtg_guiding", 0.01, 1024, 32, 16, precision=prec)
    eps, q, win = _step_inputs(p, dims, 1024)  # (expo: torch.Generator().manual_seed(77), the golden draw's variates)
    return p, dims, eps, q, win


@pytest.mark.parametrize("prec", ["bf16", "bf16x3"])
def test_short_first_pass_ends_on_the_golden_step(prec):
    """BASELINE config 2's golden step (tests/golden/g2_c2.npz) from one candidate by score and one racer: the call extends its
    lists as the certificates ask and ends on the reference's arg-max, multinomial index (8) and sampled action."""
    g = np.load(os.path.join(GD, "g2_c2.npz"))
    p, dims, eps, q, (s, a, r, h, rtg) = _golden_step(prec)
    hd, N, code = p.handle, 1024, capi.PRECISIONS[prec]
    # delta: the bound a calibration of the BF16 pass returns, for both precisions.  It bounds the split-bf16 pass too (whose
    # deviation is ~400 x smaller), and it is what makes a one-entry first pass too short in either precision: under the x3 pass's
    # own bound (~1e-2 against several units between the two best scores) the first certificates would hold at once and no
    # list would be extended -- the path this test is about.
    hd.policy_pass(capi.MODE_RTG, s, a, r, h, rtg, slot=0)
    low = hd.candidate_pass(capi.MODE_RTG, s, a, r, eps, h, 0.6, 0.99, N, precision=capi.PREC_BF16, slot=0)["expect_return"]
    delta = hd.calibrate_delta(capi.MODE_RTG, s, a, r, eps, low, h, 0.6, 0.99, N, factor=1.6, slot=0)
    res, rec = hd.plan_step_certified(capi.MODE_RTG, s, a, r, eps, q, h, rtg, 0.6, 0.99, N, 0.01, delta=delta, grow_delta=True,
                                      kmin=1, kmax=128, rfirst=1, rmax=32, precision=code, slot=0)
    torch.cuda.synchronize()
    p_, ev, am, si, sa = res["sel"]
    print(f"{prec}: delta {delta:.4g} -> {rec.delta:.4g}, n_rescored {rec.n_rescored} n_race {rec.n_race} need {rec.need_first}/"
          f"{rec.need_race_first} rounds {rec.rounds} argmax {int(am)} sample_idx {int(si)}")
    assert rec.n_rescored > 1 or rec.n_race > 1, "the one-entry first pass cannot have certified this step"
    assert rec.rounds > 1 and rec.certified == 1 and not rec.saturated
    assert int(am.item()) == int(g["argmax"])
    assert int(si.item()) == int(g["sample_idx"].reshape(-1)[0]) == 8
    assert np.abs(sa.cpu().numpy().reshape(-1) - g["sample_action"].reshape(-1)).max() < 2e-5
    p.handle.close()


# ---------------------------------------------------------------------------------------------- 4. delta growth
def test_delta_growth_equals_the_planners():
    """grow_delta = 1 from a bound far below the step's deviation: delta comes out as 1.5 x the deviation, certified, and the
    step equals a planner run that starts from the same _delta0."""
    env, guidance, tau, N, T, H = SHAPES[0]
    p, dims = _planner(env, guidance, tau, N, T, H)
    eps, q, (s, a, r, h, rtg) = _step_inputs(p, dims, N)
    p._draw_expo = lambda: q
    d0 = f32(1e-3)
    p._delta = d0  # (an explicit bound: no calibration passes; the per-step check still raises it)
    assert p._delta_fixed is None and p._cal_left == 0
    p._guide(capi.MODE_RTG, s, a, r, rtg, h, 0.6, eps=eps)
    last = dict(p.last)
    assert p.delta_grown >= 1
    res, rec = p.handle.plan_step_certified(capi.MODE_RTG, s, a, r, eps, q, h, rtg, 0.6, 0.99, N, tau, delta=d0, grow_delta=True,
                                            kmin=last["n_first"], kmax=_kmax(p, N), rfirst=last["n_race_first"], rmax=p._R,
                                            precision=capi.PREC_BF16, slot=0)
    torch.cuda.synchronize()
    print(f"delta {d0} -> {rec.delta!r}, deviation {rec.deviation!r}, python {last['delta']!r} / {last['deviation']!r}; n_rescored "
          f"{rec.n_rescored} n_race {rec.n_race} rounds {rec.rounds}")
    assert rec.delta == f32(1.5 * float(rec.deviation)) and rec.delta > d0
    assert rec.certified == 1
    _assert_same_step(res, rec, last, "growth")
    p.handle.close()


# ---------------------------------------------------------------------------------------------- 5. the planner's opt-in
def test_native_planner_equals_the_default_planner():
    """HipPlanner(native_step=True) against the default over 8 serial steps with calibration on: returned actions (eval and
    sampled) bit for bit, the same bound and the same counts.  calibration_factor 1.625 is a float: the factor crosses the C
    ABI as one (the default 1.6 is not: there m3pc_calibrate_delta multiplies by float(1.6), 1.5e-8 off)."""
    env, guidance, tau, N, T, H = SHAPES[0]
    mk = lambda native: _planner(env, guidance, tau, N, T, H, calibration_windows=4, calibration_factor=1.625, native_step=native,
                                 generator=torch.Generator(device="cuda").manual_seed(5))
    (pn, dims), (pd, _) = mk(True), mk(False)
    for t in range(8):
        hist = synth.make_history(dims, t)
        hist["path_length"] = [500, 37, 321, 998, 640, 77, 250, 123][t]
        for ev in (True, False):
            an = pn.action_sample(hist, plan=True, eval=ev, rtg=3.0)
            ad = pd.action_sample(hist, plan=True, eval=ev, rtg=3.0)
            ln, ld = pn.last, pd.last
            assert torch.equal(an, ad), (t, ev)
            assert an.shape == ad.shape
            assert torch.equal(ln["argmax"], ld["argmax"]) and torch.equal(ln["sample_idx"], ld["sample_idx"])
            assert f32(ln["delta"]) == f32(ld["delta"]), (t, ev, ln["delta"], ld["delta"])
            assert (ln["n_rescored"], ln["n_race"]) == (ld["n_rescored"], ld["n_race"]), (t, ev)
            assert set(ln["topk"].tolist()) == set(ld["topk"].tolist()) and set(ln["race"].tolist()) == set(ld["race"].tolist())
            assert set(ld.keys()) <= set(ln.keys())
            assert pn.delta_grown == pd.delta_grown
            assert f32(pn._delta0) == f32(pd._delta0), (t, ev, pn._delta0, pd._delta0)
    assert pn._cal_left == pd._cal_left == 0
    pn.handle.close()
    pd.handle.close()


# ---------------------------------------------------------------------------------------------- 6. the C example
def test_c_example_runs_the_golden_step(tmp_path):
    """examples/certified_step.c compiled with gcc against include/m3pc_hip.h, linked to the built library and run on the
    golden step: the reference's arg-max and multinomial index."""
    so = tmp_path / "libcertified_step.so"
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "certified_step.c"), "-o", str(so), "-L", libdir,
                           "-l:" + os.path.basename(capi.LIB_PATH), "-Wl,-rpath," + libdir])
    g = np.load(os.path.join(GD, "g2_c2.npz"))
    p, dims, eps, q, (s, a, r, h, rtg) = _golden_step("bf16")
    N, A = 1024, dims.action_dim
    fp, vp = C.POINTER(C.c_float), C.c_void_p

    class IO(C.Structure):
        _fields_ = [("dims", C.POINTER(capi.Dims)), ("weights", C.POINTER(capi.NamedTensor)), ("n_weights", C.c_int),
                    ("tok_mean", fp * 4), ("tok_std", fp * 4), ("tok_dim", C.c_int * 4), ("tok_normalize", C.c_int * 4),
                    ("states", vp), ("actions", vp), ("rewards", vp), ("eps", vp), ("expo", vp), ("n", C.c_int), ("horizon", C.c_int),
                    ("rtg", C.c_double), ("lmbda", C.c_double), ("discount", C.c_double), ("temperature", C.c_float),
                    ("sample_actions", vp), ("scores_low", vp), ("merged", vp), ("eval_action", vp), ("argmax", vp),
                    ("sample_idx", vp), ("sample_action", vp), ("record", capi.CertRecord), ("delta", C.c_float)]

    sd = synth.make_state_dict(dims, 0)
    arr, keep = capi._named(sd)
    io = IO()
    io.dims, io.weights, io.n_weights = C.pointer(p.handle.dims), C.cast(arr, C.POINTER(capi.NamedTensor)), len(sd)
    toks = []
    for k, name in enumerate(capi.KEYS):
        t = p.tokenizer_manager.tokenizers[name]
        m, sdv = t._data_mean.float().contiguous().reshape(-1), t._data_std.float().contiguous().reshape(-1)
        toks.append((m, sdv))
        io.tok_mean[k], io.tok_std[k] = C.cast(m.data_ptr(), fp), C.cast(sdv.data_ptr(), fp)
        io.tok_dim[k], io.tok_normalize[k] = m.numel(), int(bool(t.normalize))
    dev = dict(device="cuda")
    outs = dict(sample_actions=torch.empty((N, h, A), **dev), scores_low=torch.empty(N, **dev), merged=torch.empty(N, **dev),
                eval_action=torch.empty(A, **dev), argmax=torch.full((1,), -1, dtype=torch.int32, **dev),
                sample_idx=torch.full((1,), -1, dtype=torch.int32, **dev), sample_action=torch.empty(A, **dev))
    for name, t in dict(states=s, actions=a, rewards=r, eps=eps.contiguous(), expo=q, **outs).items():
        setattr(io, name, t.data_ptr())
    io.n, io.horizon, io.rtg, io.lmbda, io.discount, io.temperature = N, h, rtg, 0.6, 0.99, 0.01
    torch.cuda.synchronize()
    lib = C.CDLL(str(so))
    lib.certified_step.restype = C.c_int
    lib.certified_step.argtypes = [C.POINTER(IO), C.c_int, vp]
    rc = lib.certified_step(C.byref(io), torch.cuda.current_device(), vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, p.handle.lib.m3pc_last_error()
    torch.cuda.synchronize()
    print(f"C example: delta {io.delta:.4g} n_rescored {io.record.n_rescored} n_race {io.record.n_race} argmax "
          f"{int(outs['argmax'])} sample_idx {int(outs['sample_idx'])}")
    assert io.record.certified == 1 and io.delta > 0
    assert int(outs["argmax"].item()) == int(g["argmax"])
    assert int(outs["sample_idx"].item()) == int(g["sample_idx"].reshape(-1)[0]) == 8
    assert np.abs(outs["sample_action"].cpu().numpy().reshape(-1) - g["sample_action"].reshape(-1)).max() < 2e-5
    del keep, toks
    p.handle.close()


# ---------------------------------------------------------------------------------------------- 7. errors
def test_bad_arguments_leave_the_handle_usable():
    env, guidance, tau, N, T, H = SHAPES[0]
    p, dims = _planner(env, guidance, tau, N, T, H)
    hd = p.handle
    eps, q, (s, a, r, h, rtg) = _step_inputs(p, dims, N)
    dev = dict(device="cuda")
    acts, low, merged = torch.empty((N, h, dims.action_dim), **dev), torch.empty(N, **dev), torch.empty(N, **dev)
    rec = capi.CertRecord()

    def call(n_count=N, n_total=N, **cert_kw):
        args = hd._args(capi.MODE_RTG, capi.PREC_BF16, h, n_total, 0, n_count, 0.6, 0.99, rtg, 0)
        kw = dict(temperature=tau, delta=1.0, grow_delta=0, kmin=6, kmax=128, rfirst=2, rmax=32)
        kw.update(cert_kw)
        cert = capi.CertArgs(*[kw[n] for n, _ in capi.CertArgs._fields_])
        ptr = lambda t: C.c_void_p(t.data_ptr())
        return hd.lib.m3pc_plan_step_certified(hd._h, C.byref(args), C.byref(cert), ptr(s), ptr(a), ptr(r), ptr(eps), ptr(q), None, None,
                                               ptr(acts), ptr(low), ptr(merged), None, None, None, None, None, None, C.byref(rec),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream))

    for kw, word in ((dict(n_count=N - 1), b"one rank"), (dict(kmax=1000), b"1023"), (dict(rmax=65), b"rmax"),
                     (dict(n_total=16, n_count=16, rmax=17), b"rmax")):
        assert call(**kw) == -1, kw  # M3PC_EINVAL
        assert word in hd.lib.m3pc_last_error(), (kw, hd.lib.m3pc_last_error())
    res, rec2 = hd.plan_step_certified(capi.MODE_RTG, s, a, r, eps, q, h, rtg, 0.6, 0.99, N, tau, delta=1.0, kmin=6, kmax=128, rfirst=2,
                                       rmax=32)
    torch.cuda.synchronize()
    assert rec2.certified == 1 and 0 <= int(res["sel"][2]) < N
    assert call() == 0
    torch.cuda.synchronize()
    assert rec.certified == 1 and rec.n_rescored == rec2.n_rescored
    p.handle.close()
