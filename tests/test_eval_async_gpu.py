"""The eval_action certificate in the pipelined step (m3pc_plan_step_certified_eval_begin / _eval_end) against the one call it splits
(m3pc_plan_step_certified_eval), on twins of the same inputs: every output tensor, every field of the record and every field of
the eval record bit for bit -- at depths 1 .. 4, the _ends in issue order and reversed, in every regime of the three certificates
(the bound launched in advance taken / dropped for an extension / dropped for a raised delta / behind a window set / every
candidate in fp32 / an extension this certificate asked for), with plain and eval steps mixed in flight; the state machine; fp32;
soundness against the fp32 step; the planner's plan_async with eval_tol; the C example.

Bench, the delta grid and the comparison of test_certified_async_gpu.py are used as they are."""
import ctypes as C
import math
import os
import subprocess
import warnings

import numpy as np
import pytest
import torch

import eval_bound_ref as R
import test_certified_async_gpu as base
from m3pc_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = lambda x: float(np.float32(x))
INF = float("inf")
ESTATE, EINVAL = -2, -1
RTG = ("hopper", "rtg_guiding", 0.01, 625, 8, 4)
CRITIC = ("walker2d", "critic_lambda_guiding", 1.0, 256, 16, 8)
SHAPES = (RTG, CRITIC)
GRID, CERT = base.GRID, base.CERT
EREC_FIELDS = [n for n, _ in capi.EvalRecord._fields_]


def _efields(erec):
    return {n: getattr(erec, n) for n in EREC_FIELDS}


def _cert(rmax):
    return dict(rmax=rmax, rfirst=2 if rmax else 0)


def serial_eval(b, t, delta, grow, prec, tol, slot=0, **cert):
    a, kw = b.args(t, delta, grow, prec, slot, **cert)
    res, rec, erec = b.hd.plan_step_certified(*a, eval_tol=tol, **kw)
    torch.cuda.synchronize()
    return res, rec, erec


def begin_eval(b, t, delta, grow, prec, tol, slot, **cert):
    a, kw = b.args(t, delta, grow, prec, slot, **cert)
    return b.hd.plan_step_certified_begin(*a, eval_tol=tol, **kw)


def same_eval(got, rec, erec, twin, what, rmax):
    want, wrec, werec = twin
    base._same(got, rec, want, wrec, what, rmax=rmax)
    assert bytes(erec) == bytes(werec), (what, _efields(erec), _efields(werec))


def run_groups(b, deltas, grow, prec, tols, depth, reverse, twins, what, **cert):
    """The steps in groups of `depth`: every step of a group begun (slots 0 .. depth - 1), then ended in issue or reversed order,
    each compared with its serial twin."""
    n = len(deltas)
    for g0 in range(0, n, depth):
        group = list(range(g0, min(n, g0 + depth)))
        res = {t: begin_eval(b, t, deltas[t], grow, prec, tols[t], slot=t - g0, **cert) for t in group}
        for t in (reversed(group) if reverse else group):
            rec, erec = b.hd.plan_step_certified_end(t - g0, eval=True)
            torch.cuda.synchronize()
            same_eval(res[t], rec, erec, twins[t], (what, "depth", depth, "reversed", reverse, "step", t), cert["rmax"])


def regimes_of(rec, erec, delta_in, kmin=CERT["kmin"], rfirst=CERT["rfirst"]):
    """What a step's records say about the path it took (a step may be in several)."""
    out = set()
    if rec.everything:
        out.add("everything")
        if erec.eval_rounds >= 1:
            out.add("everything because of the eval certificate")
    elif erec.n_eval > 0:
        out.add("eval extension")
    if rec.saturated and not rec.everything and erec.eval_rounds >= 1:
        out.add("bound behind a window set")
    if rec.delta > f32(delta_in) and erec.eval_rounds >= 1:
        out.add("bound under a raised delta")
    if erec.eval_rounds >= 1 and not rec.saturated and erec.n_eval == 0 and not rec.everything:
        if rec.rounds == 1:
            out.add("bound launched in advance taken")
        elif rec.delta == f32(delta_in):
            out.add("bound launched in advance dropped for an extension")
    return out


# ---------------------------------------------------------------------------------------------- the serial twins, computed once
class Twins:
    """One shape: a Bench on ONE window (the grid's regimes are a condition on these inputs), one on distinct windows, and the
    serial results by (precision, rmax, tolerance kind) -- computed once, shared, left unchanged."""

    def __init__(self, shape):
        self.shape = shape
        self.grid = base.Bench(shape, len(GRID), same_window=True)
        self.many = base.Bench(shape, 4)
        self.cache = {}

    def deltas(self, prec):
        dev = self.grid.dev[prec]
        return [f32(m * dev) if m < 1e6 else 1e6 for m in GRID]

    def ext_tol(self, prec, rmax):
        """As tests/test_eval_bound_gpu.py:test_extension_reaches_the_tolerance: 1.05 x the REFERENCE's bound(n') on the report-only
        run's merged vector at n' = min(kmax, 4 n_rescored), under 2 x the calibrated deviation."""
        b = self.grid
        delta = f32(2.0 * b.dev[prec])
        rep, rec0, _ = serial_eval(b, 0, delta, False, prec, INF, **_cert(rmax))
        kmax = min(CERT["kmax"], b.N)
        npr = min(kmax, 4 * rec0.n_rescored)
        lst = rep["list"][rmax - rec0.n_race : rmax + kmax].cpu().numpy()
        ref = R.eval_bound(rep["expect_return"].cpu().numpy(), rep["sample_actions"][:, 0].cpu().numpy(), lst, rec0.n_race, rec0.n_rescored,
                           kmax, f32(b.tau), rec0.delta)
        return f32(1.05 * float(ref["bounds"][npr - rec0.n_rescored]))

    def get(self, prec, rmax, kind):
        key = (prec, rmax, kind)
        if key not in self.cache:
            tol = {"inf": INF, "tiny": 1e-9}[kind] if kind in ("inf", "tiny") else self.ext_tol(prec, rmax)
            deltas = self.deltas(prec)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                twins = [serial_eval(self.grid, t, deltas[t], False, prec, tol, slot=t % capi.SLOTS, **_cert(rmax)) for t in range(len(GRID))]
            self.cache[key] = (tol, deltas, twins)
        return self.cache[key]

    def close(self):
        self.grid.close()
        self.many.close()


@pytest.fixture(scope="module")
def twins():
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = Twins(shape)
        return made[shape]

    yield get
    for t in made.values():
        t.close()


IDS = lambda s: s[0]


# ---------------------------------------------------------------------------------------------- 1. bit identity in every regime
@pytest.mark.parametrize("kind", ["inf", "ext", "tiny"])
@pytest.mark.parametrize("rmax", [0, 32])
@pytest.mark.parametrize("prec", ["bf16", "bf16x3"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_eval_begin_end_equals_the_serial_eval_call(twins, shape, prec, rmax, kind):
    """A bound per step from the grid (grow_delta = 0) on one window: first-pass, extended, window-set and every-candidate steps
    in flight side by side, at depths 1 .. 4, ends in order and reversed, under a report-only tolerance, one that asks for an
    extension, and 1e-9, which no list reaches."""
    tw = twins(shape)
    code = capi.PRECISIONS[prec]
    tol, deltas, tws = tw.get(code, rmax, kind)
    print(f"{shape[0]} {prec} rmax {rmax} tol {tol:.4g}: " + "; ".join(
        f"{m:g}: n {r.n_rescored} rounds {r.rounds} sat {r.saturated} all {r.everything} bound {e.eval_bound:.3g} need {e.need_eval_first} "
        f"n_eval {e.n_eval} er {e.eval_rounds}" for m, (_, r, e) in zip(GRID, tws)))
    for d, (_, rec, erec) in zip(deltas, tws):
        assert rec.certified == 1 and erec.eval_certified == 1
        assert rec.everything or erec.eval_bound <= tol
        if kind == "inf":
            assert erec.n_eval == 0 and erec.eval_rounds == (0 if rec.everything else 1)
        if kind == "tiny":  # (delta = 0 is eps = 0: the bound is exactly 0 with nothing extra re-scored)
            assert (rec.everything == 1 or d == 0.0) and erec.eval_bound == 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for depth in (1, 2, 3, 4):
            for reverse in (False, True):
                run_groups(tw.grid, deltas, False, code, [tol] * len(GRID), depth, reverse, tws, (shape[0], prec, rmax, kind), **_cert(rmax))


def test_the_steps_visit_every_regime(twins):
    """The regimes are a condition on the inputs: over both shapes, both tiers and the three tolerances the serial twins take
    every path the launch in advance has to be right about."""
    seen = set()
    for shape in SHAPES:
        tw = twins(shape)
        for prec in (capi.PREC_BF16, capi.PREC_BF16X3):
            for kind in ("inf", "ext", "tiny"):
                _, deltas, tws = tw.get(prec, 32, kind)
                for d, (_, rec, erec) in zip(deltas, tws):
                    seen |= regimes_of(rec, erec, d)
    # (a raised delta needs grow_delta: test_growing_delta_equals_the_serial_eval_call)
    want = {"everything", "everything because of the eval certificate", "eval extension", "bound behind a window set",
            "bound launched in advance taken", "bound launched in advance dropped for an extension"}
    assert want <= seen, sorted(want - seen)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_growing_delta_equals_the_serial_eval_call(twins, shape):
    """grow_delta = 1 and delta = 0 going in, four distinct windows in flight: every step raises delta and merges again, so the
    bound launched in advance (under delta = 0: exactly 0) is dropped and the bound is the serial call's under the raised delta."""
    tw = twins(shape)
    b = tw.many
    for kind, tol in (("inf", INF), ("ext", tw.ext_tol(capi.PREC_BF16, 32))):
        tws = [serial_eval(b, t, 0.0, True, capi.PREC_BF16, tol, slot=3 - t, **_cert(32)) for t in range(4)]
        print(f"{shape[0]} tol {tol:.4g}: delta {[r.delta for _, r, _ in tws]} rounds {[r.rounds for _, r, _ in tws]} bound "
              f"{[e.eval_bound for _, _, e in tws]} n_eval {[e.n_eval for _, _, e in tws]}")
        for _, rec, erec in tws:
            assert rec.delta > 0 and rec.rounds >= 2 and rec.certified == 1 and erec.eval_certified == 1
            assert "bound under a raised delta" in regimes_of(rec, erec, 0.0) or rec.everything
            assert rec.everything or erec.eval_bound > 0.0  # (not the block launched under delta = 0)
        for reverse in (False, True):
            run_groups(b, [0.0] * 4, True, capi.PREC_BF16, [tol] * 4, 4, reverse, tws, ("growth", shape[0], kind), **_cert(32))


# ---------------------------------------------------------------------------------------------- 2. plain and eval steps mixed
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_plain_and_eval_steps_mixed_in_flight(twins, shape):
    tw = twins(shape)
    b, prec = tw.many, capi.PREC_BF16
    delta = f32(1.6 * b.dev[prec])
    tol = tw.ext_tol(prec, 32)
    plain = [b.serial(t, delta, False, prec, slot=(t + 1) % capi.SLOTS) for t in range(4)]
    evals = [serial_eval(b, t, delta, False, prec, tol, slot=(t + 2) % capi.SLOTS, **_cert(32)) for t in range(4)]
    for reverse in (False, True):
        res = {}
        for t in range(4):  # even steps plain, odd steps with the eval certificate
            res[t] = begin_eval(b, t, delta, False, prec, tol, slot=t, **_cert(32)) if t & 1 else b.begin(t, delta, False, prec, slot=t)
        for t in (reversed(range(4)) if reverse else range(4)):
            if t & 1:
                rec, erec = b.hd.plan_step_certified_end(t, eval=True)
                torch.cuda.synchronize()
                same_eval(res[t], rec, erec, evals[t], ("mixed eval", reverse, t), 32)
            else:
                rec = b.hd.plan_step_certified_end(t)
                torch.cuda.synchronize()
                base._same(res[t], rec, *plain[t], ("mixed plain", reverse, t))
    # the plain _end on a step begun with a tolerance: the two certificates only -- the plain serial call's bits
    res = begin_eval(b, 2, delta, False, prec, tol, slot=1, **_cert(32))
    rec = b.hd.plan_step_certified_end(1)
    torch.cuda.synchronize()
    base._same(res, rec, *plain[2], "plain end of an eval step")


# ---------------------------------------------------------------------------------------------- 3. state and arguments
def test_state_errors_leave_the_handle_usable(twins):
    tw = twins(RTG)
    b, prec = tw.many, capi.PREC_BF16
    hd, lib = b.hd, b.hd.lib
    delta = f32(1.6 * b.dev[prec])
    twin = serial_eval(b, 0, delta, False, prec, INF, **_cert(32))
    plain = b.serial(0, delta, False, prec)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rec, erec = capi.CertRecord(), capi.EvalRecord()

    def good(what):
        res = begin_eval(b, 0, delta, False, prec, INF, slot=1, **_cert(32))
        r, e = hd.plan_step_certified_end(1, eval=True)
        torch.cuda.synchronize()
        same_eval(res, r, e, twin, what, 32)

    def code(fn, *a, **kw):
        try:
            fn(*a, **kw)
        except capi.M3pcError as e:
            return int(str(e).split()[2].rstrip(":"))
        return 0

    # idle slot; bad slot; null records
    assert lib.m3pc_plan_step_certified_eval_end(hd._h, 2, C.byref(rec), C.byref(erec), st) == ESTATE
    assert lib.m3pc_plan_step_certified_eval_end(hd._h, capi.SLOTS, C.byref(rec), C.byref(erec), st) == EINVAL
    good("after idle-slot errors")
    # _eval_end on a step begun WITHOUT a tolerance: refused, and the step is still begun
    res = b.begin(0, delta, False, prec, slot=1)
    assert lib.m3pc_plan_step_certified_eval_end(hd._h, 1, C.byref(rec), C.byref(erec), st) == ESTATE
    assert b"eval_tol" in lib.m3pc_last_error()
    r1 = hd.plan_step_certified_end(1)
    torch.cuda.synchronize()
    base._same(res, r1, *plain, "the plain step an _eval_end was refused on")
    # a step begun with a tolerance: erec == NULL is refused and leaves it begun; so do the serial calls and a second _begin
    res = begin_eval(b, 0, delta, False, prec, INF, slot=1, **_cert(32))
    assert lib.m3pc_plan_step_certified_eval_end(hd._h, 1, C.byref(rec), None, st) == EINVAL
    assert lib.m3pc_plan_step_certified_eval_end(hd._h, 1, None, C.byref(erec), st) == EINVAL
    assert code(serial_eval, b, 1, delta, False, prec, INF, slot=0, **_cert(32)) == ESTATE
    assert code(b.serial, 1, delta, False, prec, slot=0) == ESTATE
    assert code(begin_eval, b, 1, delta, False, prec, INF, slot=1, **_cert(32)) == ESTATE
    r1, e1 = hd.plan_step_certified_end(1, eval=True)
    torch.cuda.synchronize()
    same_eval(res, r1, e1, twin, "the step the refused calls found in flight", 32)
    # a bad tolerance: refused, nothing begun
    for tol in (0.0, -1.0, float("nan")):
        assert code(begin_eval, b, 0, delta, False, prec, tol, slot=1, **_cert(32)) == EINVAL, tol
    assert code(begin_eval, b, 0, delta, False, prec, INF, slot=1, rmax=32, rfirst=0) == EINVAL
    assert lib.m3pc_plan_step_certified_eval_end(hd._h, 1, C.byref(rec), C.byref(erec), st) == ESTATE  # (none of them began a step)
    good("after bad arguments")


# ---------------------------------------------------------------------------------------------- 4. fp32; soundness
def test_fp32_precision(twins):
    b = twins(RTG).many
    tws = [serial_eval(b, t, 0.0, False, capi.PREC_FP32, 1e-3, slot=3 - t, **_cert(32)) for t in range(4)]
    for _, rec, erec in tws:
        assert (erec.eval_bound, erec.need_eval_first, erec.n_eval, erec.eval_rounds, erec.eval_certified) == (0.0, 0, 0, 0, 1)
        assert rec.everything == 1 and rec.certified == 1 and rec.n_rescored == b.N
    for reverse in (False, True):
        run_groups(b, [0.0] * 4, False, capi.PREC_FP32, [1e-3] * 4, 4, reverse, tws, "fp32", **_cert(32))


@pytest.mark.parametrize("prec", ["bf16", "bf16x3"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bound_of_the_pipelined_step_holds_against_the_fp32_step(twins, shape, prec):
    """max_k |eval_action_k - e32_k| <= eval_bound + slack at 1.6 x the calibrated deviation, four windows in flight; slack =
    expm1(tau 2e-5 max|f|) max_jk |a0_jk - e_k|, 2e-5 being the project's fp32 forward parity between evaluation orders
    (tests/test_eval_bound_gpu.py)."""
    b = twins(shape).many
    code = capi.PRECISIONS[prec]
    delta = f32(1.6 * b.dev[code])
    res = {t: begin_eval(b, t, delta, False, code, INF, slot=t, **_cert(32)) for t in range(4)}
    recs = {t: b.hd.plan_step_certified_end(t, eval=True) for t in range(4)}
    torch.cuda.synchronize()
    for t in range(4):
        f, _ = b.serial(t, 0.0, False, capi.PREC_FP32)
        fv = f["expect_return"].cpu().numpy().astype(np.float64)
        e32 = f["sel"][1].cpu().numpy().astype(np.float64)
        a0 = f["sample_actions"][:, 0].cpu().numpy().astype(np.float64)
        ev = res[t]["sel"][1].cpu().numpy().astype(np.float64)
        slack = math.expm1(b.tau * 2e-5 * np.abs(fv).max()) * np.abs(a0 - ev[None, :]).max()
        err = float(np.abs(ev - e32).max())
        rec, erec = recs[t]
        print(f"{shape[0]} {prec} window {t}: eval_bound {erec.eval_bound:.4g} |eval_action - fp32| {err:.4g} slack {slack:.3g} rounds {rec.rounds}")
        assert (erec.eval_rounds == 1 or rec.everything) and rec.certified == 1
        assert err <= erec.eval_bound + slack


# ---------------------------------------------------------------------------------------------- 5. the planner
def test_planner_keeps_three_eval_tickets_in_flight():
    """HipPlanner(eval_tol=1e-4) in bf16x3: plan_async with three tickets unresolved at once (m3pc_plan_step_certified_eval_begin /
    _eval_end) equals, step for step, a planner with the same seed that runs every step serially (m3pc_plan_step_certified_eval)."""
    mk = lambda: base._planner(*RTG, precision="bf16x3", native_step=True, eval_tol=1e-4, calibration_windows=2, calibration_factor=1.625,
                               generator=torch.Generator(device="cuda").manual_seed(5))
    (pa, dims), (ps, _) = mk(), mk()
    K = 9
    hists = []
    for t in range(K):
        h = synth.make_history(dims, t)
        h["path_length"] = base.PATHS[t]
        hists.append(h)
    tickets, got, most = [], [], 0
    for t in range(K):
        tickets.append(pa.plan_async(hists[t], eval=True, rtg=3.0))
        most = max(most, sum(1 for tk in tickets if tk.out is None and tk.native))
        if len(tickets) == 3:
            tk = tickets.pop(0)
            got.append((tk.result().clone(), dict(tk.info)))
    for tk in tickets:
        got.append((tk.result().clone(), dict(tk.info)))
    torch.cuda.synchronize()
    assert most == 3, most  # (three steps begun in the library and not ended)
    for t in range(K):
        want = ps.action_sample(hists[t], plan=True, eval=True, rtg=3.0).clone()
        ls = dict(ps.last)
        torch.cuda.synchronize()
        act, la = got[t]
        assert torch.equal(act, want), t
        for k in ("eval_bound", "need_eval_first", "n_eval", "eval_rounds", "eval_certified", "n_rescored", "n_race", "rounds"):
            assert la[k] == ls[k], (t, k, la[k], ls[k])
        assert f32(la["delta"]) == f32(ls["delta"]), t
        assert torch.equal(la["argmax"], ls["argmax"]) and torch.equal(la["sample_idx"], ls["sample_idx"]), t
        assert torch.equal(la["expect_return"], ls["expect_return"]), t
        assert la["eval_bound"] <= 1e-4 and la["eval_certified"], (t, la["eval_bound"])
    print(f"eval_bound {[l['eval_bound'] for _, l in got]} rounds {[l['rounds'] for _, l in got]}")
    pa.handle.close()
    ps.handle.close()


# ---------------------------------------------------------------------------------------------- 6. the C example
def test_c_example_pipelines_eval_windows(tmp_path):
    """examples/pipelined_eval.c compiled with gcc -Wall -Werror against include/m3pc_hip.h, linked to the built library and run on
    6 windows in split bf16 with eval_tol = 1e-4: it returns 0, every step certified within the tolerance, and every step's
    eval_action is the serial call's on the variates m3pc_draw_variates gives for that step index."""
    so = tmp_path / "libpipelined_eval.so"
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "pipelined_eval.c"), "-o", str(so), "-L", libdir,
                           "-l:" + os.path.basename(capi.LIB_PATH), "-Wl,-rpath," + libdir])
    env, guidance, tau, N, T, H = RTG
    K, seed, tol = 6, 2024, 1e-4
    b = base.Bench(RTG, K)
    p, dims, hd = b.p, b.dims, b.hd
    A = dims.action_dim
    h, rtg = b.steps[0][2][3], b.steps[0][2][4]
    assert all(st[2][3] == h for st in b.steps), "the example plans one horizon"
    fp, vp = C.POINTER(C.c_float), C.c_void_p

    class IO(C.Structure):
        _fields_ = [("dims", C.POINTER(capi.Dims)), ("weights", C.POINTER(capi.NamedTensor)), ("n_weights", C.c_int),
                    ("tok_mean", fp * 4), ("tok_std", fp * 4), ("tok_dim", C.c_int * 4), ("tok_normalize", C.c_int * 4),
                    ("n_windows", C.c_int), ("states", vp), ("actions", vp), ("rewards", vp), ("n", C.c_int), ("horizon", C.c_int),
                    ("precision", C.c_int), ("rtg", C.c_double), ("lmbda", C.c_double), ("discount", C.c_double),
                    ("temperature", C.c_float), ("eval_tol", C.c_float), ("seed", C.c_ulonglong), ("eps", vp), ("expo", vp),
                    ("sample_actions", vp), ("scores_low", vp), ("merged", vp), ("eval_action", vp), ("argmax", vp),
                    ("sample_idx", vp), ("sample_action", vp), ("records", C.POINTER(capi.CertRecord)),
                    ("eval_records", C.POINTER(capi.EvalRecord)), ("delta", C.c_float)]

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
    records, erecords = (capi.CertRecord * K)(), (capi.EvalRecord * K)()
    io.records, io.eval_records = C.cast(records, C.POINTER(capi.CertRecord)), C.cast(erecords, C.POINTER(capi.EvalRecord))
    io.n_windows, io.n, io.horizon, io.precision, io.rtg, io.lmbda, io.discount = K, N, h, capi.PREC_BF16X3, rtg, 0.6, 0.99
    io.temperature, io.eval_tol, io.seed = tau, tol, seed
    torch.cuda.synchronize()
    lib = C.CDLL(str(so))
    lib.pipelined_eval.restype = C.c_int
    lib.pipelined_eval.argtypes = [C.POINTER(IO), C.c_int, vp]
    rc = lib.pipelined_eval(C.byref(io), torch.cuda.current_device(), vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, hd.lib.m3pc_last_error()
    torch.cuda.synchronize()
    assert io.delta > 0
    for t in range(K):
        eps, q = hd.draw_variates(seed, t, N, T * A)
        s, a, r = b.steps[t][2][:3]
        res, rec, erec = hd.plan_step_certified(capi.MODE_RTG, s, a, r, eps, q, h, rtg, 0.6, 0.99, N, tau, delta=io.delta, grow_delta=True,
                                                kmin=6, kmax=128, rfirst=2, rmax=32, precision=capi.PREC_BF16X3, slot=0, eval_tol=tol)
        torch.cuda.synchronize()
        print(f"window {t}: eval_bound {erecords[t].eval_bound:.4g} rounds {records[t].rounds} eval_rounds {erecords[t].eval_rounds}")
        assert records[t].certified == 1 and erecords[t].eval_certified == 1 and erecords[t].eval_bound <= tol
        assert bytes(erecords[t]) == bytes(erec) and bytes(records[t]) == bytes(rec), t
        assert torch.equal(bufs["eval_action"][t], res["sel"][1]) and int(bufs["argmax"][t]) == int(res["sel"][2]), t
    del keep, toks
    b.close()
