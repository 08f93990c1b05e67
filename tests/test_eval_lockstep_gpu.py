"""m3pc_plan_steps_certified_eval -- a lock-step batch of certified plan steps with the eval_action certificate per window -- on the
GPU: the report-only identity with m3pc_plan_steps_certified, every window's bound against a stand-alone m3pc_eval_bound on what the
call returned, a bound raised by a middle window (the later windows' blocks launched in advance are dropped), a finite and an
unreachable tolerance, ``action_sample_batch(lockstep="native")`` and ``evaluate_plan(lockstep="native")`` with ``eval_tol``.

Shapes: hopper rtg N=625 T=8 H=4 tau=0.01 and walker2d critic N=256 T=16 H=8 tau=1; E = 1 and 3 windows that differ in path length
and return-to-go."""
import types
import warnings

import numpy as np
import pytest
import torch

import eval_bound_ref as R
from m3pc_amd import capi, synth
from m3pc_amd.planner import HipPlanner
from m3pc_amd.rollout import evaluate_plan

pytestmark = pytest.mark.gpu
f32 = lambda x: float(np.float32(x))
INF = float("inf")
RTG = ("hopper", "rtg_guiding", 0.01, 625, 8, 4)
CRITIC = ("walker2d", "critic_lambda_guiding", 1.0, 256, 16, 8)
SHAPES = (RTG, CRITIC)
IDS = lambda s: s[0]
MAX_E = 3
PLS = [500, 37, 321]
RTGS = [3.0, 2.0, 2.5]
KMIN, KMAX, RFIRST, RMAX = 6, 128, 2, 32
TENSORS = ("sample_actions", "expect_return_low", "expect_return", "loc", "std")


def _cfg(T, N, H, tau, guidance):
    return types.SimpleNamespace(traj_length=T, action_samples=N, horizon=H, discount=0.99, temperature=tau, lmbda=0.6,
                                 plan_guidance=guidance, device="cuda")


def _planner(shape, precision="bf16", **kw):
    env, guidance, tau, N, T, H = shape
    S, A = synth.ENV_DIMS[env]
    dims = synth.Dims(S, A, T)
    qsd, om, os_ = synth.make_critic(dims, 0) if guidance != "rtg_guiding" else (None, None, None)
    p = HipPlanner(_cfg(T, N, H, tau, guidance), synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), qsd, om, os_,
                   precision=precision, max_windows=MAX_E, generator=torch.Generator(device="cuda").manual_seed(9), **kw)
    return p, dims


class Ctx:
    """One shape: a handle, three windows, their variates, the deviation one calibration returns on window 0, and the fp32
    lock-step call on them (computed once, shared, left unchanged)."""

    def __init__(self, shape):
        env, guidance, self.tau, self.N, self.T, self.H = shape
        self.mode = capi.MODE_RTG if guidance == "rtg_guiding" else capi.MODE_CRITIC
        self.p, self.dims = _planner(shape, rescore_delta=1.0)
        self.hd = hd = self.p.handle
        self.hists = []
        for i in range(MAX_E):
            h = synth.make_history(self.dims, i)
            h["path_length"] = PLS[i]
            self.hists.append(h)
        wins = [self.p.assemble_window(h, rtg=RTGS[i]) for i, h in enumerate(self.hists)]
        assert all(w[3] == self.H for w in wins)
        self.s = torch.stack([w[0] for w in wins]).contiguous()
        self.a = torch.stack([w[1] for w in wins]).contiguous()
        self.r = torch.stack([w[2] for w in wins]).contiguous()
        g = torch.Generator(device="cuda").manual_seed(4242)
        N, A = self.N, self.dims.action_dim
        self.eps = torch.randn((MAX_E, N, self.T, A), device="cuda", dtype=torch.float32, generator=g)
        self.expo = torch.stack([torch.empty((N,), dtype=torch.float32, device="cuda").exponential_(1, generator=g) for _ in range(MAX_E)])
        self.dev = {}
        for prec in (capi.PREC_BF16, capi.PREC_BF16X3):
            hd.policy_pass(self.mode, self.s[0], self.a[0], self.r[0], self.H, RTGS[0], slot=0)
            low = hd.candidate_pass(self.mode, self.s[0], self.a[0], self.r[0], self.eps[0].reshape(N, -1), self.H, 0.6, 0.99, N,
                                    precision=prec, slot=0)["expect_return"]
            self.dev[prec] = hd.calibrate_delta(self.mode, self.s[0], self.a[0], self.r[0], self.eps[0].reshape(N, -1), low, self.H, 0.6,
                                                0.99, N, factor=1.0, slot=0)
        torch.cuda.synchronize()
        self.fp32 = {E: self.call(E, 0.0, False, capi.PREC_FP32)[0] for E in (1, MAX_E)}
        torch.cuda.synchronize()

    def call(self, E, delta, grow, prec=capi.PREC_BF16, eval_tol=None, rmax=RMAX):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = self.hd.plan_steps_certified(self.mode, self.s[:E], self.a[:E], self.r[:E], RTGS[:E], self.eps[:E].contiguous(),
                                               self.expo[:E].contiguous(), self.H, 0.6, 0.99, self.N, self.tau, delta=delta,
                                               grow_delta=grow, kmin=KMIN, kmax=KMAX, rfirst=RFIRST if rmax else 0, rmax=rmax,
                                               precision=prec, eval_tol=eval_tol)
        torch.cuda.synchronize()
        return out

    def standalone(self, res, rec, w, rmax=RMAX):
        """m3pc_eval_bound on window w of what a call returned: its merged row, its lists, its record."""
        lst = res["list"][w, rmax - rec.n_race :].contiguous()
        n_listed = rec.n_rescored if rec.saturated else min(KMAX, self.N)
        st = self.hd.eval_bound(res["expect_return"][w], lst, rec.n_race, rec.n_rescored, n_listed, res["sample_actions"][w, :, 0], self.tau,
                                rec.delta, INF)
        torch.cuda.synchronize()
        return st.cpu().numpy()

    def close(self):
        self.hd.close()


@pytest.fixture(scope="module")
def ctxs():
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = Ctx(shape)
        return made[shape]

    yield get
    for c in made.values():
        c.close()


def _same_outputs(a, b, E, recs, what, rmax=RMAX):
    for k in TENSORS:
        assert torch.equal(a[k], b[k]), (what, k)
    for i, name in enumerate(("p", "eval_action", "argmax", "sample_idx", "sample_action")):
        assert torch.equal(a["sel"][i], b["sel"][i]), (what, name)
    for w in range(E):
        if not recs[w].everything:
            lo, hi = rmax - recs[w].n_race, rmax + recs[w].n_rescored
            assert torch.equal(a["list"][w, lo:hi], b["list"][w, lo:hi]), (what, "list", w)


@pytest.mark.parametrize("rmax", [0, RMAX])
@pytest.mark.parametrize("prec", ["bf16", "bf16x3"])
@pytest.mark.parametrize("E", [1, MAX_E])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_report_only_is_the_plain_call_and_the_bound_is_the_standalone_call(ctxs, shape, E, prec, rmax):
    """eval_tol = inf: every output buffer and every record is m3pc_plan_steps_certified's, bit for bit; every window's eval_bound
    is, bit for bit, m3pc_eval_bound on the returned merged row, lists and record.  Bounds: small (lists extended), calibrated
    (first pass enough), large (window set / every candidate)."""
    x = ctxs(shape)
    code = capi.PRECISIONS[prec]
    for mult in (0.5, 1.6, 24.0):
        delta = f32(mult * x.dev[code])
        base, recs0 = x.call(E, delta, False, code, rmax=rmax)
        res, recs, erecs = x.call(E, delta, False, code, eval_tol=INF, rmax=rmax)
        what = (shape[0], E, prec, rmax, mult)
        assert [bytes(r) for r in recs] == [bytes(r) for r in recs0], what
        _same_outputs(res, base, E, recs, what, rmax)
        for w in range(E):
            rec, erec = recs[w], erecs[w]
            assert rec.certified == 1 and erec.eval_certified == 1 and erec.n_eval == 0
            if rec.everything:
                assert (erec.eval_bound, erec.eval_rounds) == (0.0, 0)
                continue
            assert erec.eval_rounds == 1 and erec.need_eval_first == rec.n_rescored
            st = x.standalone(res, rec, w, rmax)
            assert np.float32(erec.eval_bound).view(np.uint32) == st[:1].view(np.uint32)[0], (what, w, erec.eval_bound, st[0])
        print(f"{what}: rounds {[r.rounds for r in recs]} n {[r.n_rescored for r in recs]} sat {[r.saturated for r in recs]} "
              f"all {[r.everything for r in recs]} bound {[e.eval_bound for e in erecs]}")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_a_bound_raised_by_a_window_reaches_the_later_windows(ctxs, shape):
    """grow_delta from a bound below the windows' deviations: a window raises delta, every later window is merged again under it
    (rounds >= 2), its block launched in advance under the old bound is dropped, and its eval_bound is still the stand-alone call's
    under the bound it came out with; the outputs and records stay the plain call's."""
    x = ctxs(shape)
    # the deviation each window's first merge shows (it does not depend on the bound); a window raises a bound below 1.5 x it.  Where
    # window 1 shows more than window 0, start between the two: the MIDDLE window is the one that raises
    _, probe = x.call(MAX_E, f32(1.6 * x.dev[capi.PREC_BF16]), False)
    d = [float(r.deviation) for r in probe]
    start = float(np.nextafter(np.float32(1.5 * d[0]), np.float32(np.inf))) if d[1] > 1.01 * d[0] else f32(0.25 * min(d))
    base, recs0 = x.call(MAX_E, start, True)
    res, recs, erecs = x.call(MAX_E, start, True, eval_tol=INF)
    print(f"{shape[0]}: first deviations {d}; delta {start:.4g} -> {[r.delta for r in recs]} rounds {[r.rounds for r in recs]} bound {[e.eval_bound for e in erecs]}")
    assert [bytes(r) for r in recs] == [bytes(r) for r in recs0]
    _same_outputs(res, base, MAX_E, recs, shape[0])
    raised = [w for w in range(MAX_E) if recs[w].delta > (recs[w - 1].delta if w else start)]
    assert raised and raised[0] < MAX_E - 1, [r.delta for r in recs]  # a window before the last raised the bound ...
    for w in range(raised[0] + 1, MAX_E):
        assert recs[w].rounds >= 2, (w, recs[w].rounds)  # ... and every later one was merged again under it
    for w in range(MAX_E):
        if recs[w].everything:
            continue
        st = x.standalone(res, recs[w], w)
        assert np.float32(erecs[w].eval_bound).view(np.uint32) == st[:1].view(np.uint32)[0], w
        assert erecs[w].eval_rounds == 1


@pytest.mark.parametrize("E", [1, MAX_E])
def test_a_finite_tolerance_is_reached_by_extension(ctxs, E):
    """Critic shape, bf16: the tolerance of tests/test_eval_bound_gpu.py:test_extension_reaches_the_tolerance, from the REFERENCE's
    bounds on window 0's report-only result (1.05 x bound(n') at n' = min(kmax, 4 n_rescored)).  Every window ends within it -- by
    more score entries or on fp32 scores for every candidate --, window 0 by an extension this certificate asked for; arg-max and
    draw are the fp32 lock-step call's."""
    x = ctxs(CRITIC)
    delta = f32(1.6 * x.dev[capi.PREC_BF16])
    rep, recs0, erecs0 = x.call(E, delta, False, eval_tol=INF)
    r0 = recs0[0]
    kmax = min(KMAX, x.N)
    npr = min(kmax, 4 * r0.n_rescored)
    lst = rep["list"][0, RMAX - r0.n_race : RMAX + kmax].cpu().numpy()
    ref = R.eval_bound(rep["expect_return"][0].cpu().numpy(), rep["sample_actions"][0, :, 0].cpu().numpy(), lst, r0.n_race, r0.n_rescored,
                       kmax, f32(x.tau), r0.delta)
    tol = f32(1.05 * float(ref["bounds"][npr - r0.n_rescored]))
    res, recs, erecs = x.call(E, delta, False, eval_tol=tol)
    print(f"tol {tol:.4g}: report-only n {[r.n_rescored for r in recs0]} bound {[e.eval_bound for e in erecs0]}; n {[r.n_rescored for r in recs]} "
          f"n_eval {[e.n_eval for e in erecs]} bound {[e.eval_bound for e in erecs]} all {[r.everything for r in recs]}")
    assert recs[0].n_rescored > r0.n_rescored and erecs[0].n_eval > 0 and not recs[0].everything
    f = x.fp32[E]
    for w in range(E):
        assert erecs[w].eval_bound <= tol and erecs[w].eval_certified == 1 and recs[w].certified == 1
        assert int(res["sel"][2][w]) == int(f["sel"][2][w]) and int(res["sel"][3][w]) == int(f["sel"][3][w]), w
        if not recs[w].everything:
            st = x.standalone(res, recs[w], w)
            assert np.float32(erecs[w].eval_bound).view(np.uint32) == st[:1].view(np.uint32)[0], w


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_an_unreachable_tolerance_scores_every_candidate_in_fp32(ctxs, shape):
    x = ctxs(shape)
    res, recs, erecs = x.call(MAX_E, f32(1.6 * x.dev[capi.PREC_BF16]), False, eval_tol=1e-9)
    f = x.fp32[MAX_E]
    for w in range(MAX_E):
        assert recs[w].everything == 1 and recs[w].n_rescored == x.N and recs[w].certified == 1
        assert erecs[w].eval_bound == 0.0 and erecs[w].eval_certified == 1 and erecs[w].need_eval_first == x.N and erecs[w].eval_rounds == 1
        assert int(res["sel"][2][w]) == int(f["sel"][2][w]) and int(res["sel"][3][w]) == int(f["sel"][3][w]), w


def test_fp32_precision_and_refusals(ctxs):
    x = ctxs(RTG)
    res, recs, erecs = x.call(MAX_E, 0.0, False, capi.PREC_FP32, eval_tol=1e-3)
    for w in range(MAX_E):
        e = erecs[w]
        assert (e.eval_bound, e.need_eval_first, e.n_eval, e.eval_rounds, e.eval_certified) == (0.0, 0, 0, 0, 1)
        assert recs[w].everything == 1 and recs[w].n_rescored == x.N
    assert torch.equal(res["sel"][1], x.fp32[MAX_E]["sel"][1])
    for tol in (0.0, -1.0, float("nan")):
        with pytest.raises(capi.M3pcError, match="eval_tol"):
            x.call(MAX_E, 1.0, False, eval_tol=tol)
    res2, _, _ = x.call(MAX_E, 0.0, False, capi.PREC_FP32, eval_tol=1e-3)  # (the handle is usable behind a refusal)
    assert torch.equal(res2["sel"][1], res["sel"][1])


# ---------------------------------------------------------------------------------------------- the planner and the rollout
def test_action_sample_batch_native_fills_the_eval_fields():
    p, dims = _planner(RTG, precision="bf16x3", native_step=True, eval_tol=1e-4, calibration_windows=2, calibration_factor=1.625)
    hists = []
    for i in range(MAX_E):
        h = synth.make_history(dims, i)
        h["path_length"] = PLS[i]
        hists.append(h)
    for rnd in range(2):  # (the first group calibrates, then runs the library call; the second runs it alone)
        out = p.action_sample_batch(hists, eval=True, rtg=RTGS, lockstep="native")
        torch.cuda.synchronize()
        assert out.shape == (MAX_E, dims.action_dim) and bool(torch.isfinite(out).all())
        for w, info in enumerate(p.last["windows"]):
            for k in ("eval_bound", "need_eval_first", "n_eval", "eval_rounds", "eval_certified"):
                assert k in info, (rnd, w, k)
            assert info["eval_bound"] <= 1e-4 and info["eval_certified"], (rnd, w, info["eval_bound"])
            assert torch.equal(out[w], info["eval_action"])
        print(f"round {rnd}: eval_bound {[i['eval_bound'] for i in p.last['windows']]} delta {p._delta:.4g}")
    assert p._cal_left == 0
    with pytest.raises(ValueError, match="lock-step"):
        p.action_sample_batch(hists, eval=True, rtg=RTGS, lockstep=True)
    with pytest.raises(ValueError, match="native"):
        p.action_sample_batch(hists, eval=True, rtg=RTGS, lockstep="onepass")
    p.handle.close()


def test_evaluate_plan_native_lockstep_stays_within_the_tolerance():
    """evaluate_plan(lockstep="native") on the toy environments of tests/test_rollout_gpu.py, bf16x3 with eval_tol = 1e-4: the dict
    gains eval_bound_max (<= eval_tol) and eval_steps_everything; without eval_tol it has neither."""
    from fake_learner import ToyEnv

    dims = synth.Dims(11, 3, 16)
    rtg_ref = np.linspace(3.0, 1.0, 1000)
    lengths = [6, 9, 7]
    cfg = types.SimpleNamespace(traj_length=16, action_samples=256, horizon=8, discount=0.99, temperature=0.01, lmbda=0.6,
                                plan_guidance="rtg_guiding", device="cuda")
    mk = lambda **kw: HipPlanner(cfg, synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), None, precision="bf16x3",
                                 generator=torch.Generator(device="cuda").manual_seed(3), max_batch=3, max_windows=3, **kw)
    p = mk(native_step=True, eval_tol=1e-4)
    envs = [ToyEnv(11, 3, i, length=lengths[i]) for i in range(3)]
    out = evaluate_plan(p, envs, rtg_ref, max_steps=9, lockstep="native")
    p.handle.close()
    print(f"eval_bound_max {out['eval_bound_max']:.4g} eval_steps_everything {out['eval_steps_everything']} of {out['plan_steps']}")
    assert out["plan_steps"] == sum(lengths) and out["lengths"] == [float(v) for v in lengths]
    assert 0.0 <= out["eval_bound_max"] <= 1e-4
    assert 0 <= out["eval_steps_everything"] <= out["plan_steps"]
    for tr, n in zip(out["trajectories"], lengths):
        assert float(np.abs(tr["actions"][:n]).max()) <= 1.0 and np.abs(tr["actions"][:n]).sum() > 0
    # the pipelined loop of a planner with eval_tol reports the same two figures; a planner without eval_tol neither
    q = mk(native_step=True, eval_tol=1e-4, pipeline_depth=3)
    out2 = evaluate_plan(q, [ToyEnv(11, 3, i, length=lengths[i]) for i in range(3)], rtg_ref, max_steps=9)
    q.handle.close()
    assert 0.0 <= out2["eval_bound_max"] <= 1e-4 and "eval_steps_everything" in out2
    n = mk(native_step=True)
    out3 = evaluate_plan(n, [ToyEnv(11, 3, i, length=lengths[i]) for i in range(3)], rtg_ref, max_steps=9, lockstep="native")
    n.handle.close()
    assert "eval_bound_max" not in out3 and "eval_steps_everything" not in out3
