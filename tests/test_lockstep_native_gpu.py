"""m3pc_plan_steps_certified -- a lock-step batch of certified plan steps as one C call -- and ``action_sample_batch(lockstep="native")``
on the GPU.  The yardstick is the Python lock-step path (``lockstep=True``, m3pc_amd/lockstep.py + certificate.py): for the same
weights, generator state and bound, every window of a native call must give its bits.

Shapes: hopper rtg T=8 H=4 N=625 and N=2048 (the two sides of the ranking kernel's 2048 split), walker2d critic tau=1.0 T=16 H=8
N=512; E = 1, 2, 5 windows on planners built for 5 (max_batch = 5), windows that differ in path_length and rtg.

Bounds: multiples of the deviation ONE calibration returns on the shape (the grid idea of tests/test_certified_step_gpu.py) and 1e6,
so that the protocol's regimes -- first pass only, lists extended, window set, every candidate in fp32 -- are exercised: the PYTHON
path's records must show each of them at least once per shape, else the test fails (coverage is never read from the path under test).

Known divergence: the Python window set takes ``torch.topk`` while the library ranks ties to the lower index; the merged vector
depends on the set only.  No case of the grids below has met a tie at the set's boundary."""
import ctypes as C
import os
import subprocess
import types
import warnings

import numpy as np
import pytest
import torch

from m3pc_amd import capi, synth
from m3pc_amd import lockstep as lockstep_mod
from m3pc_amd.planner import HipPlanner

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GD = os.path.join(ROOT, "tests", "golden")
f32 = lambda x: float(np.float32(x))
NAN = float("nan")
ESTATE, EINVAL = -2, -1
SHAPES = {"hopper-N625": ("hopper", "rtg_guiding", 0.01, 625, 8, 4), "hopper-N2048": ("hopper", "rtg_guiding", 0.01, 2048, 8, 4),
          "walker2d-N512": ("walker2d", "critic_lambda_guiding", 1.0, 512, 16, 8)}
MAX_E = 5
PLS = [500, 37, 321, 998, 640]       # path_length per window (all give the configured horizon)
RTGS = [3.0, 2.0, 2.5, 1.0, 3.5]     # return-to-go per window
MULT = (0.0, 0.5, 1.0, 2.0, 4.0, 8.0, 12.0, 16.0, 24.0, 32.0, 64.0)  # x the calibrated deviation; then 1e6
KMIN1, RFIRST1 = 6, 2                # a first pass of the planners below: rescore_min 8 = 2 race + 6 score entries
REGIMES = ("first", "extended", "window-set", "everything")
KEYS = ("expect_return", "argmax", "sample_idx", "eval_action", "sample_action")


def _cfg(T, N, H, tau, guidance):
    return types.SimpleNamespace(traj_length=T, action_samples=N, horizon=H, discount=0.99, temperature=tau, lmbda=0.6,
                                 plan_guidance=guidance, device="cuda")


def _planner(shape, precision="bf16", **kw):
    env, guidance, tau, N, T, H = shape
    S, A = synth.ENV_DIMS[env]
    dims = synth.Dims(S, A, T)
    qsd, om, os_ = synth.make_critic(dims, 0) if guidance != "rtg_guiding" else (None, None, None)
    kw.setdefault("rescore_delta", 1.0)
    p = HipPlanner(_cfg(T, N, H, tau, guidance), synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), qsd, om, os_,
                   precision=precision, max_windows=MAX_E, generator=torch.Generator(device="cuda"), **kw)
    p._warned_saturated = True  # (the slow paths are what the large bounds are for)
    return p, dims


class Pair:
    """Two planners on the same weights -- one for ``lockstep=True``, one for ``lockstep="native"`` -- their E windows and the
    deviation one calibration returns on window 0."""

    def __init__(self, shape, precision="bf16", **kw):
        self.shape = shape
        env, guidance, self.tau, self.N, self.T, self.H = shape
        self.mode = capi.MODE_RTG if guidance == "rtg_guiding" else capi.MODE_CRITIC
        self.py, self.dims = _planner(shape, precision, **kw)
        self.nat, _ = _planner(shape, precision, **kw)
        self.hists = []
        for i in range(MAX_E):
            h = synth.make_history(self.dims, i)
            h["path_length"] = PLS[i]
            self.hists.append(h)
        N = self.N
        wins = [self.py.assemble_window(h, rtg=RTGS[i]) for i, h in enumerate(self.hists)]
        torch.cuda.synchronize()
        assert all(w[3] == self.H for w in wins)
        self.s = torch.stack([w[0] for w in wins]).contiguous()
        self.a = torch.stack([w[1] for w in wins]).contiguous()
        self.r = torch.stack([w[2] for w in wins]).contiguous()
        self.eps1 = synth.make_eps(N, self.dims, 1).cuda().reshape(N, -1).contiguous()
        # The calibration runs on BOTH handles, in the same order: the candidate-independent decoder tables of a handle are built by
        # whichever pass needs them first (m3pc_plans.hip: build_tables), so two handles give the same bits when they share a history.
        self.dev = {}
        for hd in (self.py.handle, self.nat.handle):
            for prec in sorted({capi.PREC_BF16, self.py.precision} - {capi.PREC_FP32}):
                hd.policy_pass(self.mode, self.s[0], self.a[0], self.r[0], self.H, RTGS[0], slot=0)
                low = hd.candidate_pass(self.mode, self.s[0], self.a[0], self.r[0], self.eps1, self.H, 0.6, 0.99, N, precision=prec,
                                        slot=0)["expect_return"]
                dev = hd.calibrate_delta(self.mode, self.s[0], self.a[0], self.r[0], self.eps1, low, self.H, 0.6, 0.99, N, factor=1.0,
                                         slot=0)
                assert self.dev.setdefault(prec, dev) == dev, "the two handles calibrate differently"
        torch.cuda.synchronize()

    def run(self, p, lockstep, E, seed, eval, delta=None, grow_from=None):
        if grow_from is None:
            p._delta_fixed = p._delta0 = float(delta)
        else:  # an adaptive bound that starts at grow_from (the setter ends the calibration)
            p._delta_fixed = None
            p._delta = float(grow_from)
        p._cal_left, p._hist, p.delta_grown = 0, {}, 0
        p.generator.manual_seed(seed)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = p.action_sample_batch(self.hists[:E], eval=eval, rtg=RTGS[:E], lockstep=lockstep)
        torch.cuda.synchronize()
        return out.clone(), p.last

    def grid(self, prec=capi.PREC_BF16):
        return [m * self.dev[prec] for m in MULT] + [1e6]

    def close(self):
        self.py.handle.close()
        self.nat.handle.close()


_PAIRS = {}


@pytest.fixture(scope="module")
def pairs():
    def get(name, precision="bf16", **kw):
        key = (name, precision, tuple(sorted(kw.items())))
        if key not in _PAIRS:
            _PAIRS[key] = Pair(SHAPES[name], precision, **kw)
        return _PAIRS[key]

    yield get
    for p in _PAIRS.values():
        p.close()
    _PAIRS.clear()


def _regime(w, N):
    if w["n_rescored"] >= N:
        return "everything"
    if w["saturated"]:
        return "window-set"
    return "extended" if w["n_rescored"] > KMIN1 or w["n_race"] > RFIRST1 else "first"


def _same_delta(a, b):
    return (a is None and b is None) or (a is not None and b is not None and f32(a) == f32(b))  # (None: an fp32 planner has no bound)


def _same(want, got, what):
    """(actions, planner.last) of the Python path and of the native path: tensors torch.equal, counts equal, delta equal after one
    rounding to float (the convention of tests/test_certified_step_gpu.py)."""
    (out_w, last_w), (out_g, last_g) = want, got
    assert out_w.shape == out_g.shape and torch.equal(out_w, out_g), (what, "actions")
    assert len(last_w["windows"]) == len(last_g["windows"])
    assert set(last_w) == set(last_g)
    for w, (a, b) in enumerate(zip(last_w["windows"], last_g["windows"])):
        assert set(a) == set(b), (what, w)
        for k in KEYS:
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (what, "window", w, k)
        for k in ("n_rescored", "n_race", "saturated", "horizon"):
            assert a[k] == b[k], (what, "window", w, k, a[k], b[k])
        ma, mb = a["min_margin_outside"], b["min_margin_outside"]
        assert ma == mb or (ma != ma and mb != mb), (what, "window", w, "margin", ma, mb)
        assert _same_delta(a["delta"], b["delta"]), (what, "window", w, "delta")
    assert _same_delta(last_w["delta"], last_g["delta"]), (what, "delta")


# ---------------------------------------------------------------------------------------------- 1. bit equality with lockstep=True
@pytest.mark.parametrize("name", list(SHAPES))
def test_native_equals_the_python_lockstep_path_in_every_regime(pairs, name):
    b = pairs(name)
    seen = {}
    for E in (1, 2, MAX_E):
        for i, delta in enumerate(b.grid()):
            for ev in ((True, False) if i in (2, len(MULT)) else (bool(i & 1),)):
                seed = 1000 + 31 * E + i
                want = b.run(b.py, True, E, seed, ev, delta=delta)
                regs = [_regime(w, b.N) for w in want[1]["windows"]]  # (coverage is read from the Python path alone)
                for r in regs:
                    seen[r] = seen.get(r, 0) + 1
                got = b.run(b.nat, "native", E, seed, ev, delta=delta)
                _same(want, got, (name, "E", E, "delta", delta, "eval", ev, regs))
    print(f"{name}: deviation {b.dev[capi.PREC_BF16]:.4g}, regimes of the Python path {seen}")
    for r in REGIMES:
        assert seen.get(r, 0) >= 1, (name, "the grid never reached regime", r, seen)


def test_native_without_race_entries_is_the_argmax_certificate_alone(pairs):
    """certify_sample=False: rmax == 0 in the call -- m3pc_topk_window's lists, m3pc_rescore_merge + m3pc_select per window."""
    b = pairs("hopper-N625", certify_sample=False)
    seen = set()
    for E in (2, MAX_E):
        for i, delta in enumerate([m * b.dev[capi.PREC_BF16] for m in (0.0, 1.0, 8.0, 24.0)] + [1e6]):
            want = b.run(b.py, True, E, 2000 + 7 * E + i, bool(i & 1), delta=delta)
            got = b.run(b.nat, "native", E, 2000 + 7 * E + i, bool(i & 1), delta=delta)
            _same(want, got, ("rmax 0", "E", E, "delta", delta))
            assert all(w["n_race"] == 0 for w in got[1]["windows"])
            seen |= {_regime(w, b.N) for w in want[1]["windows"]}
    assert "everything" in seen and len(seen) >= 2, seen


# ---------------------------------------------------------------------------------------------- 2. the delta rule across windows
@pytest.mark.parametrize("name", list(SHAPES))
def test_a_raised_bound_reaches_every_later_window(pairs, name, monkeypatch):
    b = pairs(name)
    start = f32(0.25 * b.dev[capi.PREC_BF16])
    trace = []
    inner = lockstep_mod._resolve_certificate

    def recording(planner, N, kmax, rmax, n_done, r_done, delta, ops):
        rec = inner(planner, N, kmax, rmax, n_done, r_done, delta, ops)
        trace.append((delta, rec["delta"]))
        return rec

    monkeypatch.setattr(lockstep_mod, "_resolve_certificate", recording)
    want = b.run(b.py, True, MAX_E, 3000, False, grow_from=start)
    monkeypatch.setattr(lockstep_mod, "_resolve_certificate", inner)
    grown_py, final_py = b.py.delta_grown, b.py._delta
    print(f"{name}: bound in / out per window of the Python path {trace}, delta_grown {grown_py}")
    assert len(trace) == MAX_E and grown_py >= 1
    # some window w > 0 went in under a bound an earlier window had raised: it was merged again before its certificate was read
    assert any(trace[w][0] > trace[0][0] for w in range(1, MAX_E)), trace
    got = b.run(b.nat, "native", MAX_E, 3000, False, grow_from=start)
    _same(want, got, (name, "grow"))
    assert f32(b.nat._delta) == f32(final_py) and f32(final_py) > start
    assert b.nat.delta_grown >= 1
    # the records of the call itself: window w's delta is the bound coming out of window w
    eps, expo = _variates(b, MAX_E, 3000)
    res, recs = b.nat.handle.plan_steps_certified(b.mode, b.s, b.a, b.r, RTGS, eps, expo, b.H, 0.6, 0.99, b.N, b.tau, delta=start,
                                                  grow_delta=True, kmin=KMIN1, kmax=128, rfirst=RFIRST1, rmax=32)
    torch.cuda.synchronize()
    assert [f32(t[1]) for t in trace] == [r.delta for r in recs], (trace, [r.delta for r in recs])
    assert recs[-1].delta == f32(final_py)
    assert all(r.rounds >= 1 and r.certified == 1 for r in recs)
    assert any(recs[w].rounds >= 2 for w in range(1, MAX_E))  # (the merge under the raised bound counts)
    for w in range(MAX_E):
        assert torch.equal(res["expect_return"][w], want[1]["windows"][w]["expect_return"]), w


def _variates(b, E, seed):
    """eps and expo as the planners draw them for a group of E windows from generator state `seed`."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    eps = torch.randn((E, b.N, b.T, b.dims.action_dim), device="cuda", dtype=torch.float32, generator=g)
    expo = torch.stack([torch.empty((b.N,), dtype=torch.float32, device="cuda").exponential_(1, generator=g) for _ in range(E)])
    return eps, expo


# ---------------------------------------------------------------------------------------------- 3. the C call directly
def _padded(shape, dtype):
    """A buffer of `shape` with 64 NaN-filled (as float32 bit patterns) elements behind it: (whole flat buffer, the view)."""
    n = int(np.prod(shape))
    flat = torch.full((n + 64,), NAN, dtype=torch.float32, device="cuda")
    view = (flat if dtype == torch.float32 else flat.view(torch.int32))[:n].view(shape)
    return flat, view


def _outputs(b, E, rmax, skip=()):
    N, T, A, H = b.N, b.T, b.dims.action_dim, b.H
    shapes = dict(loc=(E, T, A), std=(E, T, A), sample_actions=(E, N, H, A), expect_return_low=(E, N), expect_return=(E, N),
                  list=(E, rmax + 1024), p=(E, N), eval_action=(E, A), argmax=(E,), sample_idx=(E,), sample_action=(E, A))
    flats, out = {}, {}
    for k, shape in shapes.items():
        if k not in skip:
            flats[k], out[k] = _padded(shape, torch.int32 if k in ("list", "argmax", "sample_idx") else torch.float32)
    return flats, out


def _flat(res):
    d = {k: v for k, v in res.items() if k != "sel"}
    d.update(zip(("p", "eval_action", "argmax", "sample_idx", "sample_action"), res["sel"]))
    return d


@pytest.mark.parametrize("name,rmax", [("hopper-N625", 32), ("hopper-N2048", 32), ("walker2d-N512", 32), ("hopper-N625", 0)])
def test_the_c_call_writes_what_it_documents_and_nothing_else(pairs, name, rmax):
    b = pairs(name)
    hd, N, E = b.nat.handle, b.N, MAX_E
    eps, expo = _variates(b, E, 4000)
    smode = capi.MODE_RTG if b.mode == capi.MODE_RTG else capi.MODE_CRITIC
    for mult in (1.0, 16.0):
        kw = dict(delta=mult * b.dev[capi.PREC_BF16], grow_delta=False, kmin=KMIN1, kmax=128, rfirst=RFIRST1 if rmax else 0, rmax=rmax)
        args = (b.mode, b.s, b.a, b.r, RTGS, eps, expo, b.H, 0.6, 0.99, N, b.tau)
        flats, out = _outputs(b, E, rmax)
        res, recs = hd.plan_steps_certified(*args, out=out, **kw)
        torch.cuda.synchronize()
        full = _flat(res)
        for k, fl in flats.items():
            assert bool(fl[-64:].isnan().all()), (name, k, "wrote behind its end")
        # loc / std / p / list omitted: every other output identical, the same records
        optional = ("loc", "std", "p", "list")
        flats2, out2 = _outputs(b, E, rmax, skip=optional)
        res2, recs2 = hd.plan_steps_certified(*args, out=out2, want_policy=False, want_list=False, want_p=False, **kw)
        torch.cuda.synchronize()
        less = _flat(res2)
        for k in optional:
            assert less[k] is None
        for k, fl in flats2.items():
            assert bool(fl[-64:].isnan().all()), (name, k, "wrote behind its end")
            assert torch.equal(full[k], less[k]), (name, mult, k)
        assert [bytes(r) for r in recs] == [bytes(r) for r in recs2]
        low, merged, lst = full["expect_return_low"], full["expect_return"], full["list"]
        assert not bool(merged.isnan().any()) and not bool(full["loc"].isnan().any()) and not bool(full["p"].isnan().any())
        for w, rec in enumerate(recs):
            assert rec.certified == 1 and rec.rounds >= 1
            if rmax == 0:
                assert rec.n_race == 0 and rec.need_race_first == 0
            if rec.everything:
                continue
            # per window: the re-scored race entries in front of list[rmax], the re-scored score entries from it on
            sc = lst[w, rmax : rmax + rec.n_rescored].long()
            assert sc.unique().numel() == rec.n_rescored and int(sc.min()) >= 0 and int(sc.max()) < N
            vals = low[w][sc]
            assert bool((vals[:-1] >= vals[1:]).all()), (name, w, "score entries are not in descending order")
            rest = torch.ones(N, dtype=torch.bool, device="cuda")
            rest[sc] = False
            assert not bool(rest.any()) or float(low[w][rest].max()) <= float(vals[-1]), (name, w, "score entries are not the best")
            ids = sc
            if rec.n_race:
                rc = lst[w, rmax - rec.n_race : rmax].long()
                assert rc.unique().numel() == rec.n_race and int(rc.min()) >= 0 and int(rc.max()) < N
                key = b.tau * low[w].double() - expo[w].double().log()
                rest = torch.ones(N, dtype=torch.bool, device="cuda")
                rest[rc] = False
                tol = 1e-5 * max(1.0, float(key.abs().max()))
                assert float(key[rest].max()) <= float(key[rc].min()) + tol, (name, w, "race entries are not the best racers")
                assert bool((key[rc][1:] >= key[rc][:-1] - tol).all()), (name, w, "race entries: the best racer sits next to rmax")
                ids = torch.cat([rc, sc]).unique()
            # the listed candidates carry fp32 scores in the merged vector (a few-row fp32 pass: equal up to its tiling)
            f = hd.score_actions(smode, b.s[w], b.a[w], b.r[w], full["sample_actions"][w][ids], None, b.H, 0.6, 0.99)
            scale = max(1.0, float(f.abs().max()))
            assert float((merged[w][ids] - f).abs().max()) <= 1e-4 * scale, (name, w, float((merged[w][ids] - f).abs().max()), scale)


# ---------------------------------------------------------------------------------------------- 4. fp32
@pytest.mark.parametrize("name", list(SHAPES))
def test_fp32_windows_are_m3pc_select_on_their_scores(pairs, name):
    b = pairs(name)
    hd, N = b.nat.handle, b.N
    for E in (1, MAX_E):
        eps, expo = _variates(b, E, 5000 + E)
        flats, out = _outputs(b, E, 0)
        res, recs = hd.plan_steps_certified(b.mode, b.s[:E], b.a[:E], b.r[:E], RTGS[:E], eps, expo, b.H, 0.6, 0.99, N, b.tau,
                                            kmin=1, kmax=1, rfirst=0, rmax=0, precision=capi.PREC_FP32, out=out)
        torch.cuda.synchronize()
        for k, fl in flats.items():
            if k != "list":  # (fp32 lists nothing)
                assert bool(fl[-64:].isnan().all()), (name, k)
                assert not bool(fl[:-64].isnan().any()), (name, k)
        assert torch.equal(res["expect_return"], res["expect_return_low"])
        for w, rec in enumerate(recs):
            assert (rec.certified, rec.everything, rec.n_rescored, rec.n_race, rec.saturated) == (1, 1, N, 0, 0)
            want = hd.select(res["expect_return_low"][w], res["sample_actions"][w][:, 0], b.tau, expo[w])
            for i, k in enumerate(("p", "eval_action", "argmax", "sample_idx", "sample_action")):
                assert torch.equal(res["sel"][i][w].reshape(-1), want[i].reshape(-1)), (name, E, w, k)


@pytest.mark.parametrize("n", [1, 625, 2048, 16384])
def test_select_batch_kernel_equals_m3pc_select(pairs, n):
    """select_batch_kernel through its lab hook, E = 1 and 5: per window m3pc_select's results on that row, bit for bit."""
    from hip_util import lab_library
    lab = lab_library()
    vp, ci, cf, ll = C.c_void_p, C.c_int, C.c_float, C.c_longlong
    lab.m3pc_debug_select_batch.restype = ci
    lab.m3pc_debug_select_batch.argtypes = [vp, vp, ll, ll, ci, ci, ci, cf, vp, vp, vp, vp, vp, vp, vp]
    hd = pairs("hopper-N625").py.handle
    A, H, tau = 3, 4, 0.05
    g = torch.Generator(device="cuda")
    g.manual_seed(60 + n)
    for E in (1, MAX_E):
        v = (20.0 * torch.randn((E, n), device="cuda", generator=g)).contiguous()
        if n > 4:
            v[:, n // 2] = v[:, 1]  # a tie: the lower index wins
        q = torch.empty((E, n), device="cuda").exponential_(1, generator=g)
        sa = torch.randn((E, n, H, A), device="cuda", generator=g)
        fp, p = _padded((E, n), torch.float32)
        fe, ev = _padded((E, A), torch.float32)
        fa, am = _padded((E,), torch.int32)
        fi, si = _padded((E,), torch.int32)
        fs, sact = _padded((E, A), torch.float32)
        rc = lab.m3pc_debug_select_batch(v.data_ptr(), sa.data_ptr(), n * H * A, H * A, E, n, A, tau, q.data_ptr(), p.data_ptr(),
                                         ev.data_ptr(), am.data_ptr(), si.data_ptr(), sact.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lab.m3pc_last_error()
        torch.cuda.synchronize()
        for fl in (fp, fe, fa, fi, fs):
            assert bool(fl[-64:].isnan().all())
        for w in range(E):
            want = hd.select(v[w], sa[w][:, 0], tau, q[w])
            for got, ref, k in zip((p, ev, am, si, sact), want, ("p", "eval_action", "argmax", "sample_idx", "sample_action")):
                assert torch.equal(got[w].reshape(-1), ref.reshape(-1)), (n, E, w, k)
        # without expo / p: the arg-max and the weighted mean alone
        fe2, ev2 = _padded((E, A), torch.float32)
        fa2, am2 = _padded((E,), torch.int32)
        rc = lab.m3pc_debug_select_batch(v.data_ptr(), sa.data_ptr(), n * H * A, H * A, E, n, A, tau, None, None, ev2.data_ptr(),
                                         am2.data_ptr(), None, None, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lab.m3pc_last_error()
        torch.cuda.synchronize()
        assert torch.equal(ev2, ev) and torch.equal(am2, am) and bool(fe2[-64:].isnan().all()) and bool(fa2[-64:].isnan().all())


def test_native_fp32_planning_keeps_the_reference_argmax():
    """The four hopper / weight seed 0 cases of g5_argmax.npz (captured from the reference) as one fp32 batch, native against
    lockstep=True (the bf16 form of this check: tests/test_batch_gpu.py)."""
    g5 = np.load(os.path.join(GD, "g5_argmax.npz"))
    N, H, T = (int(v) for v in g5["cfg"])
    dims = synth.Dims(11, 3, T)
    mk = lambda: HipPlanner(_cfg(T, N, H, 0.01, "rtg_guiding"), synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), None,
                            precision="fp32", max_windows=4, generator=torch.Generator(device="cuda"))
    py, nat = mk(), mk()
    hists, epss = [], []
    for ci in range(4):
        env, mode, wseed, hseed, pl = str(g5["cases"][ci]).split(":")
        assert env == "hopper" and wseed == "0"
        h = synth.make_history(dims, int(hseed))
        h["path_length"] = int(pl)
        hists.append(h)
        epss.append(synth.make_eps(N, dims, 100 + ci).reshape(N, T, 3))
    stack = torch.stack(epss).cuda()
    res = {}
    for p, mode in ((py, True), (nat, "native")):
        p._eps = lambda shape: stack
        p.generator.manual_seed(9)
        res[mode] = (p.action_sample_batch(hists, eval=True, rtg=3.0, lockstep=mode).clone(), p.last)
        torch.cuda.synchronize()
    _same(res[True], res["native"], "g5 fp32")
    for ci in range(4):
        w = nat.last["windows"][ci]
        assert int(w["argmax"].item()) == int(g5[f"argmax_{ci}"]), ci
        assert w["n_rescored"] is None and w["saturated"] is None
        assert np.abs(res["native"][0][ci].cpu().numpy() - g5[f"eval_action_{ci}"]).max() < 2e-2
    py.handle.close()
    nat.handle.close()


# ---------------------------------------------------------------------------------------------- 5. bf16x3
def test_bf16x3_native_equals_the_python_path_at_the_calibrated_bound(pairs):
    b = pairs("hopper-N625", precision="bf16x3")
    delta = b.dev[capi.PREC_BF16X3]
    assert 0 < delta < b.dev[capi.PREC_BF16]
    for E in (2, MAX_E):
        for ev in (True, False):
            want = b.run(b.py, True, E, 6000 + E, ev, delta=delta)
            got = b.run(b.nat, "native", E, 6000 + E, ev, delta=delta)
            _same(want, got, ("bf16x3", E, ev))
            assert all(w["n_rescored"] < b.N for w in want[1]["windows"])


# ---------------------------------------------------------------------------------------------- 6. state
def test_state_rules_and_the_single_window_call_behind_a_batch(pairs):
    b = pairs("hopper-N625")
    hd, N = b.nat.handle, b.N
    eps, expo = _variates(b, MAX_E, 7000)
    delta = b.dev[capi.PREC_BF16]
    cert = dict(delta=delta, grow_delta=False, kmin=KMIN1, kmax=128, rfirst=RFIRST1, rmax=32)
    batch = lambda E=MAX_E: hd.plan_steps_certified(b.mode, b.s[:E], b.a[:E], b.r[:E], RTGS[:E], eps[:E].contiguous(),
                                                    expo[:E].contiguous(), b.H, 0.6, 0.99, N, b.tau, **cert)
    single = lambda: hd.plan_step_certified(b.mode, b.s[1], b.a[1], b.r[1], eps[1], expo[1], b.H, RTGS[1], 0.6, 0.99, N, b.tau, **cert)
    before, rec0 = single()
    res0, recs0 = batch()
    torch.cuda.synchronize()
    # a single-window step right behind a batch call: the bits it gave before it
    after, rec1 = single()
    torch.cuda.synchronize()
    assert bytes(rec0) == bytes(rec1)
    for k in ("loc", "std", "sample_actions", "expect_return_low", "expect_return"):
        assert torch.equal(before[k], after[k]), k
    for x, y in zip(before["sel"], after["sel"]):
        assert torch.equal(x, y)
    # with a pipelined step begun the batch call is refused, and works again behind _end
    begun = hd.plan_step_certified_begin(b.mode, b.s[0], b.a[0], b.r[0], eps[0], expo[0], b.H, RTGS[0], 0.6, 0.99, N, b.tau, slot=1, **cert)
    with pytest.raises(capi.M3pcError, match=r"m3pc error %d: .*begun" % ESTATE):
        batch()
    hd.plan_step_certified_end(1)
    torch.cuda.synchronize()
    del begun
    # more windows than max_batch: refused, and the next valid call succeeds with the same bits
    six = lambda t: torch.cat([t, t[:1]]).contiguous()
    with pytest.raises(capi.M3pcError, match=r"m3pc error %d: .*max_batch" % EINVAL):
        hd.plan_steps_certified(b.mode, six(b.s), six(b.a), six(b.r), RTGS + [1.0], six(eps), six(expo), b.H, 0.6, 0.99, N, b.tau, **cert)
    res1, recs1 = batch()
    torch.cuda.synchronize()
    assert [bytes(r) for r in recs0] == [bytes(r) for r in recs1]
    for k, v in _flat(res0).items():
        if k != "list":
            assert torch.equal(v, _flat(res1)[k]), k
    # a first pass of more rows than one scoring call takes (5 x 627 > max(max_candidates = 5 N, max_rescore)): refused with
    # M3PC_ENOMEM before anything is enqueued
    with pytest.raises(capi.M3pcError, match=r"m3pc error -4: .*first pass"):
        hd.plan_steps_certified(b.mode, b.s, b.a, b.r, RTGS, eps, expo, b.H, 0.6, 0.99, N, b.tau, **dict(cert, kmin=N, kmax=900))
    # a low-precision pass without the certified re-score (rescore="topk"; "none", which lockstep=True serves by selecting on the
    # low-precision scores alone) is the Python path's: the native path refuses it and names lockstep=True, before anything runs
    for other in ("topk", "none"):
        b.nat.rescore = other
        try:
            with pytest.raises(ValueError, match="lockstep=True"):
                b.nat.action_sample_batch(b.hists[:2], rtg=RTGS[:2], lockstep="native")
        finally:
            b.nat.rescore = "bound"
    want = b.run(b.py, True, 2, 7100, True, delta=delta)
    got = b.run(b.nat, "native", 2, 7100, True, delta=delta)
    _same(want, got, "behind the refusals")


def test_a_calibrating_group_takes_the_python_path(pairs):
    """While the weight load's calibration windows are not used up, lockstep="native" runs the group through lockstep=True -- the
    one piece of code that calibrates -- and switches to the library call afterwards."""
    b = pairs("hopper-N625")
    runs = {}
    for p, mode in ((b.py, True), (b.nat, "native")):
        p._delta_fixed = None
        p._reset_calibration()
        p._cal_left = 3
        p._warned_saturated = True
        p.generator.manual_seed(8000)
        outs = []
        for _ in range(2):  # 3 of the first call's 5 windows calibrate; the second call plans under the calibrated bound
            outs.append((p.action_sample_batch(b.hists, eval=False, rtg=RTGS, lockstep=mode).clone(), p.last))
            torch.cuda.synchronize()
        runs[mode] = outs
        assert p._cal_left == 0 and p._delta0 > 0
    for want, got in zip(runs[True], runs["native"]):
        _same(want, got, "calibrating")
    assert f32(b.py._delta0) == f32(b.nat._delta0)


# ---------------------------------------------------------------------------------------------- 7. the C example
def test_c_example_plans_three_rounds_of_three_environments(pairs, tmp_path):
    """examples/lockstep_steps.c compiled with gcc -Wall -Werror against include/m3pc_hip.h, linked to the built library and run
    for three rounds of E = 3: every window's arg-max and multinomial index are what Handle.plan_steps_certified returns for the
    same seed, step indices and bound."""
    so = tmp_path / "liblockstep_steps.so"
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "lockstep_steps.c"), "-o", str(so), "-L", libdir,
                           "-l:" + os.path.basename(capi.LIB_PATH), "-Wl,-rpath," + libdir])
    b = pairs("hopper-N625")
    p, dims, hd = b.py, b.dims, b.py.handle
    N, T, H, A, tau = b.N, b.T, b.H, dims.action_dim, b.tau
    K, E, seed = 3, 3, 2025
    fp, vp = C.POINTER(C.c_float), C.c_void_p

    class IO(C.Structure):
        _fields_ = [("dims", C.POINTER(capi.Dims)), ("weights", C.POINTER(capi.NamedTensor)), ("n_weights", C.c_int),
                    ("tok_mean", fp * 4), ("tok_std", fp * 4), ("tok_dim", C.c_int * 4), ("tok_normalize", C.c_int * 4),
                    ("n_rounds", C.c_int), ("n_envs", C.c_int), ("states", vp), ("actions", vp), ("rewards", vp),
                    ("rtg", C.POINTER(C.c_double)), ("n", C.c_int), ("horizon", C.c_int), ("lmbda", C.c_double), ("discount", C.c_double),
                    ("temperature", C.c_float), ("seed", C.c_ulonglong), ("eps", vp), ("expo", vp),
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
    # K rounds of E windows: window (k, w) is window (k + w) % 5 of the shape, with its return-to-go
    pick = [(k + w) % MAX_E for k in range(K) for w in range(E)]
    wins = dict(states=b.s[pick].contiguous(), actions=b.a[pick].contiguous(), rewards=b.r[pick].contiguous())
    rtg = (C.c_double * (K * E))(*[RTGS[i] for i in pick])
    dev = dict(device="cuda")
    bufs = dict(eps=torch.empty((E, N, T * A), **dev), expo=torch.empty((E, N), **dev),
                sample_actions=torch.empty((K * E, N, H, A), **dev), scores_low=torch.empty((K * E, N), **dev),
                merged=torch.empty((K * E, N), **dev), eval_action=torch.empty((K * E, A), **dev),
                argmax=torch.full((K * E,), -1, dtype=torch.int32, **dev), sample_idx=torch.full((K * E,), -1, dtype=torch.int32, **dev),
                sample_action=torch.empty((K * E, A), **dev))
    for name, t in dict(**wins, **bufs).items():
        setattr(io, name, t.data_ptr())
    records = (capi.CertRecord * (K * E))()
    io.records, io.rtg = C.cast(records, C.POINTER(capi.CertRecord)), C.cast(rtg, C.POINTER(C.c_double))
    io.n_rounds, io.n_envs, io.n, io.horizon, io.lmbda, io.discount, io.temperature, io.seed = K, E, N, H, 0.6, 0.99, tau, seed
    torch.cuda.synchronize()
    lib = C.CDLL(str(so))
    lib.lockstep_steps.restype = C.c_int
    lib.lockstep_steps.argtypes = [C.POINTER(IO), C.c_int, vp]
    rc = lib.lockstep_steps(C.byref(io), torch.cuda.current_device(), vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, hd.lib.m3pc_last_error()
    torch.cuda.synchronize()
    assert io.delta > 0
    delta = io.delta
    for k in range(K):
        ids = pick[k * E : (k + 1) * E]
        var = [hd.draw_variates(seed, k * E + w, N, T * A) for w in range(E)]
        eps, q = torch.stack([v[0] for v in var]), torch.stack([v[1] for v in var])
        res, recs = hd.plan_steps_certified(capi.MODE_RTG, b.s[ids], b.a[ids], b.r[ids], [RTGS[i] for i in ids], eps, q, H, 0.6, 0.99, N,
                                            tau, delta=delta, grow_delta=True, kmin=6, kmax=128, rfirst=2, rmax=32)
        torch.cuda.synchronize()
        for w in range(E):
            t = k * E + w
            print(f"round {k} window {w}: C argmax {int(bufs['argmax'][t])} sample_idx {int(bufs['sample_idx'][t])}, binding "
                  f"{int(res['sel'][2][w])} {int(res['sel'][3][w])}; n_rescored {records[t].n_rescored} n_race {records[t].n_race}")
            assert records[t].certified == 1 and bytes(records[t]) == bytes(recs[w]), (k, w)
            assert int(bufs["argmax"][t]) == int(res["sel"][2][w]) and int(bufs["sample_idx"][t]) == int(res["sel"][3][w]), (k, w)
            assert torch.equal(bufs["merged"][t], res["expect_return"][w])
        delta = recs[-1].delta
    del keep, toks
