"""The eval_action certificate on the GPU: eval_bound_kernel (m3pc_eval_bound) against the fp64 reference of
tests/eval_bound_ref.py, and m3pc_plan_step_certified_eval -- report-only identity with m3pc_plan_step_certified, soundness against
the fp32 step, extension to a tolerance, the every-candidate path for a tolerance the list cannot reach, fp32 precision -- then the
planner's eval_tol and the C example."""
import ctypes as C
import math
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import eval_bound_ref as R
from m3pc_amd import capi, synth
from m3pc_amd.planner import HipPlanner

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = lambda x: float(np.float32(x))
INF = float("inf")


# ------------------------------------------------------------------------------------------ 1. the kernel against the reference
@pytest.fixture(scope="module")
def handle():
    h = capi.Handle(11, 3, 8, n_embd=64, n_head=2, max_candidates=8)  # (m3pc_eval_bound reads the handle's device only)
    yield h
    h.close()


def _synthetic(n_total, A, stride_mult, lists, tau, seed):
    """Scores whose softmax weights fall by ~5 % per rank (|tau (m - max m)| <= 60), so that consecutive bound(n') differ by
    percents and a tolerance can sit clearly between two of them; a0 = tanh of normals in rows of stride_mult * A floats; the
    lists (r, n, n_listed) clipped to n_total, score entries in descending order of m (ties to the lower index), race entries
    random with one candidate planted in both parts (and, from r = 2 on, a second one that is a re-scored score entry)."""
    g = np.random.default_rng(seed)
    r0, n0, l0 = lists
    n_listed = min(l0, n_total)
    n = min(n0, n_listed)
    r = min(r0, n_total)
    z = -np.minimum(60.0, 0.05 * np.arange(n_total) + g.uniform(0.0, 0.02, n_total))
    m = np.empty(n_total, dtype=np.float32)
    m[g.permutation(n_total)] = (z / tau + 37.0).astype(np.float32)
    buf = np.zeros((n_total, stride_mult * A), dtype=np.float32)
    buf[:, :A] = np.tanh(g.normal(size=(n_total, A))).astype(np.float32)
    score = np.argsort(-m.astype(np.float64), kind="stable")[:n_listed]
    race = g.choice(n_total, size=r, replace=False) if r else np.zeros(0, dtype=np.int64)
    if r >= 1:
        race[0] = score[min(n + 1, n_listed - 1)]
    if r >= 2 and score[0] != race[0]:
        race[1] = score[0]
    lst = np.concatenate([race, score]).astype(np.int32)
    return m, buf, lst, r, n, n_listed


@pytest.mark.parametrize("n_total", [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 16384])
def test_kernel_against_fp64_reference(handle, n_total):
    """eval_bound, P_U and bound(n_listed) within 1e-3 relative of the fp64 reference (fp32 expf and argument rounding give about
    4e-6 per weight at these arguments; the margin covers expm1f at eps ~ 1e-4 and the cancellation in a - e); need_eval equal to
    the reference's for a tolerance that the reference's own bound(n') miss by more than 1e-2 relative on either side; delta = 0
    gives exactly 0; eval_tol = inf gives need_eval = n; the host block closes with the sequence number; two runs, same bits."""
    dev = handle.device
    worst = 0.0
    hs = capi.HostStats()
    checked_mid = 0
    for ci, (A, mult, lists, tau, delta) in enumerate((A, mult, lists, tau, delta) for A in (1, 3, 17) for mult in (1, 4)
                                                      for lists in ((0, 1, 1), (2, 8, 129), (64, 8, 960)) for tau in (0.01, 1.0)
                                                      for delta in (0.0, 0.012, 4.87)):
        tau32, delta32 = f32(tau), f32(delta)
        m, buf, lst, r, n, n_listed = _synthetic(n_total, A, mult, lists, tau32, 1000 * n_total + ci)
        ref = R.eval_bound_fast(m, buf[:, :A], lst, r, n, n_listed, tau32, delta32)
        b = ref["bounds"]
        md, bd, ld = torch.from_numpy(m).to(dev), torch.from_numpy(buf).to(dev), torch.from_numpy(lst).to(dev)
        a0 = bd[:, :A]
        assert a0.stride(0) == mult * A
        what = (n_total, A, mult, (r, n, n_listed), tau, delta)

        def run(tol, host=None, seq=0.0):
            st = torch.full((8,), float("nan"), device=dev)
            handle.eval_bound(md, ld, r, n, n_listed, a0, tau32, delta32, tol, stats=st, host_stats=host, seq=seq)
            return st

        seq = hs.next_seq()
        st = run(INF, hs.buf, seq)
        st2 = run(INF)
        torch.cuda.synchronize()
        got = st.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), st2.cpu().numpy().view(np.uint32)), what
        assert hs.np[4] == seq and np.array_equal(hs.np[[0, 1, 2, 3, 5, 6, 7]], got[[0, 1, 2, 3, 5, 6, 7]]), what
        for name, g_, w in (("eval_bound", got[0], ref["eval_bound"]), ("P_U", got[2], ref["P_U"]), ("bound(n_listed)", got[6], ref["bound_listed"])):
            if w == 0.0:
                assert g_ == 0.0, (what, name, g_)
            else:
                worst = max(worst, abs(float(g_) - w) / w)
                assert abs(float(g_) - w) <= 1e-3 * w, (what, name, float(g_), w)
        if delta == 0.0:
            assert got[0] == 0.0 and got[6] == 0.0, what
        assert int(got[1]) == n == ref["need_eval"], what  # (eval_tol = inf)
        assert int(got[7]) == ref["n_U"], what
        assert abs(float(got[5]) - ref["eps"]) <= 1e-6 * ref["eps"], what
        B = np.sort(ref["B"])
        if delta > 0 and B[-1] > 0 and (A == 1 or B[-2] < 0.99 * B[-1]):
            assert int(got[3]) == ref["k"], what
        assert 0 <= int(got[3]) < A
        if delta == 0.0:
            continue
        # a tolerance between two bounds that lie >= 5 % apart, as near the middle of the list as there is one
        ts = [t for t in range(1, len(b)) if b[t - 1] > 0 and b[t - 1] >= 1.05 * b[t]]
        if ts:
            t = min(ts, key=lambda t: abs(t - len(b) // 2))
            tol = f32(math.sqrt(b[t - 1] * b[t]) if b[t] > 0 else 0.5 * b[t - 1])  # (b[t] = 0: the last entry of U was listed)
            assert min(abs(b[t - 1] - tol), abs(b[t] - tol)) > 1e-2 * tol  # (on the reference alone: no off-by-one is excused)
            assert R.eval_bound_fast(m, buf[:, :A], lst, r, n, n_listed, tau32, delta32, tol)["need_eval"] == n + t
            got_t = run(tol).cpu().numpy()
            assert int(got_t[1]) == n + t, (what, tol, int(got_t[1]), n + t)
            assert got_t[0] == got[0]
            checked_mid += 1
        else:
            assert n_listed - n < 2 or n_total <= 2 or b[0] == 0.0, what  # (every longer list of these inputs has such a pair)
        if b[-1] > 0:  # the list cannot reach it
            tol = f32(0.5 * b[-1])
            assert int(run(tol).cpu()[1]) == n_total, what
    print(f"n_total {n_total}: largest relative deviation from the fp64 reference {worst:.3e}; {checked_mid} mid-list tolerances")
    assert checked_mid > 0 or n_total <= 2


# ------------------------------------------------------------------------------------------ 2. the certified step with the bound
def _cfg(T, N, H, tau, guidance):
    return types.SimpleNamespace(traj_length=T, action_samples=N, horizon=H, discount=0.99, temperature=tau, lmbda=0.6,
                                 plan_guidance=guidance, device="cuda")


def _planner(shape, precision="bf16", **kw):
    env, guidance, tau, N, T, H = shape
    S, A = synth.ENV_DIMS[env]
    dims = synth.Dims(S, A, T)
    qsd, om, os_ = synth.make_critic(dims, 0) if guidance != "rtg_guiding" else (None, None, None)
    p = HipPlanner(_cfg(T, N, H, tau, guidance), synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), qsd, om, os_,
                   precision=precision, **kw)
    return p, dims


RTG = ("hopper", "rtg_guiding", 0.01, 625, 8, 4)
CRITIC = ("walker2d", "critic_lambda_guiding", 1.0, 256, 16, 8)
KMIN, KMAX = 8, 128


def _mode(shape):
    return capi.MODE_RTG if shape[1] == "rtg_guiding" else capi.MODE_CRITIC


class Ctx:
    """One shape's handle, window and variates, and the fp32 step on them (computed once, shared, left unchanged)."""

    def __init__(self, shape):
        self.shape = shape
        env, guidance, self.tau, self.N, T, H = shape
        self.p, self.dims = _planner(shape)
        self.hd = self.p.handle
        N = self.N
        self.eps = synth.make_eps(N, self.dims, 1).cuda()
        self.q = torch.empty(N, dtype=torch.float32).exponential_(1, generator=torch.Generator().manual_seed(77)).cuda()
        hist = synth.make_history(self.dims, 0)
        hist["path_length"] = 500
        s, a, r, self.h, self.rtg = self.p.assemble_window(hist, rtg=3.0)
        self.win = (s.clone(), a.clone(), r.clone())
        self.mode = _mode(shape)
        self.deltas = {}
        res, rec = self.step(capi.PREC_FP32, 0, 0.0)
        torch.cuda.synchronize()
        self.f = res["expect_return"].cpu().numpy().astype(np.float64)
        self.e32 = res["sel"][1].cpu().numpy().astype(np.float64)
        self.argmax32, self.idx32 = int(res["sel"][2]), int(res["sel"][3])
        self.a0 = res["sample_actions"][:, 0].cpu().numpy().astype(np.float64)

    def delta(self, prec):
        if prec not in self.deltas:
            hd, (s, a, r) = self.hd, self.win
            hd.policy_pass(self.mode, s, a, r, self.h, self.rtg, slot=0)
            low = hd.candidate_pass(self.mode, s, a, r, self.eps, self.h, 0.6, 0.99, self.N, precision=prec, slot=0)["expect_return"]
            self.deltas[prec] = hd.calibrate_delta(self.mode, s, a, r, self.eps, low, self.h, 0.6, 0.99, self.N, factor=1.6, slot=0)
        return self.deltas[prec]

    def step(self, prec, rmax, delta, eval_tol=None):
        s, a, r = self.win
        return self.hd.plan_step_certified(self.mode, s, a, r, self.eps, self.q, self.h, self.rtg, 0.6, 0.99, self.N, self.tau, delta=delta,
                                           grow_delta=True, kmin=KMIN, kmax=KMAX, rfirst=2 if rmax else 0, rmax=rmax, precision=prec,
                                           slot=0, eval_tol=eval_tol)

    def slack(self, ev):
        """expm1(tau 2e-5 max|f|) max_jk |a0_jk - e_k|: 2e-5 is the project's fp32 forward parity between evaluation orders."""
        return math.expm1(self.tau * 2e-5 * np.abs(self.f).max()) * np.abs(self.a0 - ev[None, :]).max()


@pytest.fixture(scope="module")
def ctxs():
    c = {RTG: Ctx(RTG), CRITIC: Ctx(CRITIC)}
    yield c
    for x in c.values():
        x.hd.close()


CONFIGS = [(shape, prec, rmax) for shape in (RTG, CRITIC) for prec in ("bf16", "bf16x3") for rmax in (0, 32)]
_ids = lambda c: f"{c[0][0]}-{c[1]}-r{c[2]}"
REC_FIELDS = [n for n, _ in capi.CertRecord._fields_]


@pytest.mark.parametrize("cfg", CONFIGS, ids=_ids)
def test_report_only_is_the_certified_step_and_sound(ctxs, cfg):
    """eval_tol = inf: every output tensor and every field of the record are m3pc_plan_step_certified's; the eval record's bound is,
    bit for bit, a stand-alone m3pc_eval_bound on the returned merged vector and lists; and the bound holds against the fp32 step:
    max_k |eval_action_k - e32_k| <= eval_bound + slack."""
    shape, prec, rmax = cfg
    x = ctxs[shape]
    code = capi.PRECISIONS[prec]
    delta = x.delta(code)
    base, rec = x.step(code, rmax, delta)
    rep, rec2, erec = x.step(code, rmax, delta, eval_tol=INF)
    torch.cuda.synchronize()
    nl = rmax + min(KMAX + 1, x.N)  # (the list entries the rankings wrote)
    for k in ("loc", "std", "sample_actions", "expect_return_low", "expect_return"):
        assert torch.equal(base[k], rep[k]), k
    assert torch.equal(base["list"][:nl], rep["list"][:nl])
    for i, (t0, t1) in enumerate(zip(base["sel"], rep["sel"])):
        assert torch.equal(t0, t1), i
    for name in REC_FIELDS:
        v0, v1 = getattr(rec, name), getattr(rec2, name)
        assert np.array_equal(np.float32(v0).view(np.uint32), np.float32(v1).view(np.uint32)) if isinstance(v0, float) else v0 == v1, name
    assert not rec2.everything and rec2.certified == 1
    assert erec.eval_rounds == 1 and erec.n_eval == 0 and erec.eval_certified == 1 and erec.need_eval_first == rec2.n_rescored
    a0 = rep["sample_actions"][:, 0]
    st = x.hd.eval_bound(rep["expect_return"], rep["list"][rmax - rec2.n_race:].contiguous(), rec2.n_race, rec2.n_rescored,
                         rec2.n_rescored if rec2.saturated else min(KMAX, x.N), a0, x.tau, rec2.delta, INF)
    torch.cuda.synchronize()
    assert np.float32(erec.eval_bound).view(np.uint32) == st[:1].cpu().numpy().view(np.uint32)[0]
    ev = rep["sel"][1].cpu().numpy().astype(np.float64)
    err, slack = float(np.abs(ev - x.e32).max()), x.slack(ev)
    print(f"{_ids(cfg)}: delta {delta:.4g} -> {rec2.delta:.4g} n_rescored {rec2.n_rescored} n_race {rec2.n_race}; eval_bound "
          f"{erec.eval_bound:.4g}, |eval_action - fp32| {err:.4g}, slack {slack:.3g}, bound(kmax) {float(st[6]):.4g}, P_U {float(st[2]):.4g}")
    assert err <= erec.eval_bound + slack


def test_extension_reaches_the_tolerance(ctxs):
    """Critic shape, bf16: a tolerance 1.05 x the reference's bound(n') on the report-only run's merged vector at n' = min(kmax,
    4 n_rescored) makes the step re-score more score entries, because of this certificate, until the bound is within it; the
    arg-max and the draw stay the fp32 step's and eval_action is within tol + slack of it."""
    x = ctxs[CRITIC]
    rmax = 32
    delta = x.delta(capi.PREC_BF16)
    rep, rec0, erec0 = x.step(capi.PREC_BF16, rmax, delta, eval_tol=INF)
    torch.cuda.synchronize()
    kmax = min(KMAX, x.N)
    npr = min(kmax, 4 * rec0.n_rescored)
    lst = rep["list"][rmax - rec0.n_race : rmax + kmax].cpu().numpy()
    ref = R.eval_bound(rep["expect_return"].cpu().numpy(), rep["sample_actions"][:, 0].cpu().numpy(), lst, rec0.n_race, rec0.n_rescored,
                       kmax, f32(x.tau), rec0.delta)
    tol = 1.05 * float(ref["bounds"][npr - rec0.n_rescored])
    res, rec, erec = x.step(capi.PREC_BF16, rmax, delta, eval_tol=tol)
    torch.cuda.synchronize()
    ev = res["sel"][1].cpu().numpy().astype(np.float64)
    err, slack = float(np.abs(ev - x.e32).max()), x.slack(ev)
    print(f"report-only: n_rescored {rec0.n_rescored} eval_bound {erec0.eval_bound:.4g} (reference {ref['eval_bound']:.4g}); tol {tol:.4g} "
          f"(bound({npr})): n_rescored {rec.n_rescored} n_eval {erec.n_eval} need_eval_first {erec.need_eval_first} eval_rounds "
          f"{erec.eval_rounds} eval_bound {erec.eval_bound:.4g} everything {rec.everything}; |eval_action - fp32| {err:.4g} slack {slack:.3g}")
    assert rec.n_rescored > rec0.n_rescored
    assert erec.n_eval > 0
    assert erec.eval_bound <= tol
    assert erec.eval_certified == 1
    assert int(res["sel"][2]) == x.argmax32 and int(res["sel"][3]) == x.idx32
    assert err <= tol + slack


def test_unreachable_tolerance_scores_every_candidate_in_fp32(ctxs):
    x = ctxs[RTG]
    res, rec, erec = x.step(capi.PREC_BF16, 32, x.delta(capi.PREC_BF16), eval_tol=1e-9)
    p, ev, am, si, sa = x.hd.select(res["expect_return"], res["sample_actions"][:, 0], x.tau, x.q)
    torch.cuda.synchronize()
    print(f"eval_tol 1e-9: need_eval_first {erec.need_eval_first} everything {rec.everything} n_rescored {rec.n_rescored} eval_bound "
          f"{erec.eval_bound} eval_rounds {erec.eval_rounds}")
    assert rec.everything == 1 and rec.n_rescored == x.N and rec.certified == 1
    assert erec.eval_bound == 0.0 and erec.eval_certified == 1 and erec.need_eval_first == x.N
    assert torch.equal(res["sel"][1], ev)
    assert int(res["sel"][2]) == x.argmax32 and int(res["sel"][3]) == x.idx32


def test_fp32_precision_record(ctxs):
    x = ctxs[RTG]
    res, rec, erec = x.step(capi.PREC_FP32, 32, 0.0, eval_tol=1e-3)
    torch.cuda.synchronize()
    assert (erec.eval_bound, erec.need_eval_first, erec.n_eval, erec.eval_rounds, erec.eval_certified) == (0.0, 0, 0, 0, 1)
    assert rec.everything == 1 and rec.certified == 1 and rec.n_rescored == x.N
    assert int(res["sel"][2]) == x.argmax32


# ------------------------------------------------------------------------------------------ 3. the planner
def _hist(dims, t):
    h = synth.make_history(dims, t)
    h["path_length"] = [500, 37, 321][t]
    return h


def test_planner_eval_tol():
    """eval_tol = 1e-4 in bf16x3 leaves last["eval_bound"] <= 1e-4 on an evaluation step; eval_tol = None returns the bits of the
    default planner, and so does eval_tol = inf (report only); a plan_async ticket equals the serial result; misuse raises."""
    mk = lambda **kw: _planner(RTG, precision="bf16x3", calibration_windows=2, calibration_factor=1.625,
                               generator=torch.Generator(device="cuda").manual_seed(5), **kw)
    (pe, dims), (pn, _), (pi, _), (pd, _), (pa, _) = (mk(native_step=True, eval_tol=1e-4), mk(native_step=True), mk(native_step=True, eval_tol=INF),
                                                      mk(), mk(native_step=True, eval_tol=1e-4))
    for t in range(3):
        hist = _hist(dims, t)
        ae = pe.action_sample(hist, plan=True, eval=True, rtg=3.0)
        le = dict(pe.last)
        assert le["eval_bound"] <= 1e-4 and le["eval_certified"] and "need_eval_first" in le and "n_eval" in le
        an, ai, ad = (p.action_sample(hist, plan=True, eval=True, rtg=3.0) for p in (pn, pi, pd))
        assert "eval_bound" not in pn.last and "eval_bound" in pi.last
        assert torch.equal(an, ad) and torch.equal(ai, ad), t
        assert torch.equal(pn.last["argmax"], pd.last["argmax"]) and torch.equal(pn.last["sample_idx"], pd.last["sample_idx"])
        tk = pa.plan_async(hist, eval=True, rtg=3.0)
        aa = tk.result()
        torch.cuda.synchronize()
        print(f"step {t}: eval_bound {le['eval_bound']:.4g} n_rescored {le['n_rescored']} n_eval {le['n_eval']} need_eval_first "
              f"{le['need_eval_first']}; |eval_tol planner - default| {float((ae - ad).abs().max()):.3g}")
        assert torch.equal(aa, ae), t
        assert pa.last["eval_bound"] == le["eval_bound"]
    with pytest.raises(ValueError, match="lock-step"):
        pe.action_sample_batch([_hist(dims, 0)], eval=True, rtg=3.0, lockstep=True)
    with pytest.raises(ValueError, match="native_step"):
        _planner(RTG, precision="bf16x3", eval_tol=1e-4)
    for p in (pe, pn, pi, pd, pa):
        p.handle.close()


# ------------------------------------------------------------------------------------------ 4. the C example
def test_c_example_runs(tmp_path):
    """examples/certified_eval.c compiled against include/m3pc_hip.h, linked to the built library and run on the rtg shape in
    split bf16 with eval_tol = 1e-4: it returns 0 with a certified bound within the tolerance."""
    so = tmp_path / "libcertified_eval.so"
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "certified_eval.c"), "-o", str(so), "-L", libdir,
                           "-l:" + os.path.basename(capi.LIB_PATH), "-Wl,-rpath," + libdir])
    p, dims = _planner(RTG, precision="bf16x3")
    N, A = RTG[3], dims.action_dim
    eps = synth.make_eps(N, dims, 1).cuda().contiguous()
    q = torch.empty(N, dtype=torch.float32).exponential_(1, generator=torch.Generator().manual_seed(77)).cuda()
    hist = synth.make_history(dims, 0)
    hist["path_length"] = 500
    s, a, r, h, rtg = p.assemble_window(hist, rtg=3.0)
    fp, vp = C.POINTER(C.c_float), C.c_void_p

    class IO(C.Structure):
        _fields_ = [("dims", C.POINTER(capi.Dims)), ("weights", C.POINTER(capi.NamedTensor)), ("n_weights", C.c_int),
                    ("tok_mean", fp * 4), ("tok_std", fp * 4), ("tok_dim", C.c_int * 4), ("tok_normalize", C.c_int * 4),
                    ("states", vp), ("actions", vp), ("rewards", vp), ("eps", vp), ("expo", vp), ("n", C.c_int), ("horizon", C.c_int),
                    ("precision", C.c_int), ("rtg", C.c_double), ("lmbda", C.c_double), ("discount", C.c_double),
                    ("temperature", C.c_float), ("eval_tol", C.c_float),
                    ("sample_actions", vp), ("scores_low", vp), ("merged", vp), ("eval_action", vp), ("argmax", vp),
                    ("sample_idx", vp), ("sample_action", vp), ("record", capi.CertRecord), ("eval_record", capi.EvalRecord),
                    ("delta", C.c_float)]

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
    for name, t in dict(states=s, actions=a, rewards=r, eps=eps, expo=q, **outs).items():
        setattr(io, name, t.data_ptr())
    io.n, io.horizon, io.precision, io.rtg, io.lmbda, io.discount, io.temperature, io.eval_tol = N, h, capi.PREC_BF16X3, rtg, 0.6, 0.99, 0.01, 1e-4
    torch.cuda.synchronize()
    lib = C.CDLL(str(so))
    lib.certified_eval.restype = C.c_int
    lib.certified_eval.argtypes = [C.POINTER(IO), C.c_int, vp]
    rc = lib.certified_eval(C.byref(io), torch.cuda.current_device(), vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, p.handle.lib.m3pc_last_error()
    torch.cuda.synchronize()
    assert io.record.certified == 1 and io.delta > 0
    assert io.eval_record.eval_certified == 1 and io.eval_record.eval_bound <= 1e-4 and io.eval_record.eval_rounds >= 1
    assert 0 <= int(outs["argmax"].item()) < N
    del keep, toks
    p.handle.close()
