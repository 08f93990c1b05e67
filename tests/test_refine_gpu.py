"""CEM / MPPI refinement on the GPU (m3pc_refit_resample, m3pc_refine_plan, HipPlanner.cem_guiding(native=True)): the two
kernels of m3pc_amd/csrc/refine.hip against the fp64 restatement of tests/refine_ref.py at their edges, the loop link by link
(a chain that does not depend on how a near-tie at the elite boundary falls), end to end against the oracle's cem_guiding where
the oracle's own trace has a clear elite boundary, and what surrounds the call: library-drawn noise, warm start, state, the C
example.  All on the tiny model of tests/test_batch_gpu.py (T = 8, H = 4)."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import refine_ref as R
from m3pc_amd import capi, synth
from m3pc_amd.planner import HipPlanner
from oracle import mtm_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H, S, A = 8, 4, 11, 3
DIMS = synth.Dims(S, A, T, n_embd=64, n_head=2)
GUIDANCE = {"rtg": "rtg_guiding", "critic": "critic_lambda_guiding"}
MODE = {"rtg": capi.MODE_RTG, "critic": capi.MODE_CRITIC}
OUTPUTS = ("mean", "std", "candidates", "scores", "elites", "sample_action", "eval_action")


def _cfg(N, guidance, temp=1.0):
    return types.SimpleNamespace(traj_length=T, action_samples=N, horizon=H, discount=0.99, temperature=temp, lmbda=0.6,
                                 plan_guidance=guidance, device="cuda")


def _tiny(N=16, guidance="rtg_guiding", temp=1.0, **kw):
    qsd, om, os_ = synth.make_critic(DIMS, 0)
    return HipPlanner(_cfg(N, guidance, temp), synth.make_state_dict(DIMS, 0), synth.make_tokenizer_stats(DIMS, 0), qsd, om, os_,
                      n_embd=64, n_head=2, **kw)


@pytest.fixture(scope="module")
def planners():
    """Planners of the tiny model by (mode, N, precision), shared by the tests of this file that only read them."""
    cache = {}

    def get(mode, N, precision="fp32", **kw):
        key = (mode, N, precision, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = _tiny(N, GUIDANCE[mode], precision=precision, **kw)
        return cache[key]

    yield get
    for p in cache.values():
        p.handle.close()


@pytest.fixture(scope="module")
def world():
    """The CPU side, computed once: weights, statistics, the history (seed 0, path_length 100, rtg 3.0), the oracle's window and
    its policy mean.  Nothing in here is modified by a test."""
    sd, st = synth.make_state_dict(DIMS, 0), O.make_stats(synth.make_tokenizer_stats(DIMS, 0))
    hist = synth.make_history(DIMS, 0)
    hist["path_length"] = 100
    w = types.SimpleNamespace(sd=sd, st=st, critic=synth.make_critic(DIMS, 0), hist=hist, cem={})
    w.ocfg = lambda N: O.PlanCfg(T, H, N, n_head=2)
    w.win, w.h = O.assemble_window(w.ocfg(16), hist, 100, 3.0)
    loc, _ = O.policy_pass(sd, st, w.ocfg(16), w.win, w.h)
    w.mean0 = torch.tanh(loc[0, T - w.h:, 0, :])
    w.score = lambda mode, cand: O.plan_candidates(sd, st, w.ocfg(cand.shape[0]), w.win, w.h, cand, mode, 0.6, w.critic)

    def cem(mode, N, k, noise):
        if (mode, N, k) not in w.cem:
            w.cem[(mode, N, k)] = O.cem_guiding(sd, st, w.ocfg(N), w.win, w.h, 0.6, noise, mode, critic=w.critic, iterations=2, top_k=k)
        return w.cem[(mode, N, k)]

    w.cem_guiding = cem
    return w


def _noise(N, h=H, iterations=2):
    return torch.randn(iterations + 1, N, h, A, generator=torch.Generator().manual_seed(11))


def _window(p, world):
    s, a, r, h, rtg = p.assemble_window(world.hist, rtg=3.0)
    assert h == world.h
    return s.clone(), a.clone(), r.clone(), h, rtg


def _rebuild(mean, std, noise):
    """clamp(mean + std * noise, -1, 1) on the CPU in fp32, product and sum as two roundings."""
    return torch.clamp(mean[None] + std[None] * noise, -1.0, 1.0)


def _equal(a, b, what=""):
    for name in OUTPUTS:
        assert torch.equal(a[name], b[name]), (what, name)


# ---------------------------------------------------------------------------------------------- 1. refit / resample at their edges
GRID = [(1, 1), (64, 1), (64, 2), (65, 63), (130, 64), (130, 65), (625, 128), (1500, 1024), (1500, 1025), (1500, 1500), (16384, 4096)]


def refit_inputs(n, k, hz, a_dim):
    """cand uniform in [-1, 1] with about a tenth of the entries exactly +-1 and one column whose elites are all equal; elites an
    unsorted random subset; scores normal with sigma 8; noise standard normal.  -> numpy arrays and the equal column (t, a)."""
    rng = np.random.RandomState((1000003 * n + 1009 * k + 17 * hz + a_dim) % 2 ** 32)
    cand = rng.uniform(-1.0, 1.0, size=(n, hz, a_dim)).astype(np.float32)
    edge = rng.uniform(size=cand.shape)
    cand[edge < 0.05] = -1.0
    cand[edge > 0.95] = 1.0
    elites = rng.permutation(n)[:k].astype(np.int32)
    eq = (hz // 2, a_dim - 1)
    cand[elites, eq[0], eq[1]] = np.float32(0.3)
    scores = (8.0 * rng.normal(size=n)).astype(np.float32)
    noise = rng.normal(size=cand.shape).astype(np.float32)
    return cand, elites, scores, noise, eq


def _refit_case(hd, n, k, hz, weighting, tau, min_std=0.0):
    a_dim = hd.A
    cand, elites, scores, noise, eq = refit_inputs(n, k, hz, a_dim)
    mean_r, std_r, D = R.refit(cand, elites, scores, weighting, tau, min_std)
    one_hot = weighting == R.MPPI and tau > 1.0
    if one_hot and k > 1:  # every weight but the best elite's underflows in fp32 (and D <= 1e-6 in fp64 with it)
        e = np.sort(scores[elites].astype(np.float64))
        assert tau * (e[-1] - e[-2]) > 110.0 and D <= 1e-6
    elif k > 1:  # (k = 1: D is exactly 0 in either arithmetic)
        assert D >= 1e-3, D
    else:
        assert D == 0.0
    dev = dict(device="cuda")
    c, e_, s_, z = (torch.from_numpy(x).to(**dev) for x in (cand, elites, scores, noise))
    mean, std, out = hd.refit_resample(c, e_, s_, weighting, tau, min_std, noise=z)
    m, sd = mean.cpu(), std.cpu()
    err_m, err_s = float(np.abs(m.numpy() - mean_r).max()), float(np.abs(sd.numpy() - std_r).max())
    print(f"n {n} k {k} h {hz} A {a_dim} weighting {weighting} tau {tau} min_std {min_std}: D {D:.3e} |mean - ref| {err_m:.2e} |std - ref| {err_s:.2e}")
    assert torch.isfinite(m).all() and torch.isfinite(sd).all()
    assert err_m <= 1e-5 and err_s <= 1e-5
    assert float(sd[eq]) == float(np.float32(min_std)), "the all-equal column"
    assert float(m[eq]) == float(np.float32(0.3))
    if one_hot or k == 1:
        assert bool((sd == float(np.float32(min_std))).all())
    if min_std > 0:
        assert bool((sd >= float(np.float32(min_std))).all())
    # the resample, bit for bit, from the GPU's own distribution
    assert torch.equal(out.cpu(), _rebuild(m, sd, torch.from_numpy(noise)))
    # refit only; the same call again; the output aliased onto the input
    m2, s2 = hd.refit_resample(c, e_, s_, weighting, tau, min_std)
    m3, s3, o3 = hd.refit_resample(c, e_, s_, weighting, tau, min_std, noise=z)
    live = c.clone()
    m4, s4, o4 = hd.refit_resample(live, e_, s_, weighting, tau, min_std, noise=z, out=live)
    assert o4.data_ptr() == live.data_ptr()
    for mm, ss in ((m2, s2), (m3, s3), (m4, s4)):
        assert torch.equal(mm, mean) and torch.equal(ss, std)
    assert torch.equal(o3, out) and torch.equal(o4, out)


VARIANTS = [(R.CEM, 0.0, 0.0), (R.CEM, 0.0, 0.05), (R.MPPI, 0.01, 0.0), (R.MPPI, 0.25, 0.0), (R.MPPI, 0.25, 0.05), (R.MPPI, 1e4, 0.0)]


@pytest.fixture(scope="module")
def bare():
    """Handles without weights (m3pc_refit_resample needs none), by action dimension."""
    hs = {3: capi.Handle(S, 3, T, n_embd=64, n_head=2, max_candidates=16, critic_hidden=0),
          6: capi.Handle(17, 6, T, n_embd=64, n_head=2, max_candidates=16, critic_hidden=0)}
    yield hs
    for h in hs.values():
        h.close()


@pytest.mark.parametrize("n,k", GRID)
def test_refit_and_resample_at_their_edges(bare, n, k):
    """k = 1; k on both sides of a wave (63 / 64 / 65) and of what a workgroup keeps in registers (1024 / 1025); k = n; the
    largest n; horizon 1 (3 columns, an element count that is no multiple of 4 at odd n), 4, 8; both weightings."""
    for hz in (1, 4, 8):
        for weighting, tau, min_std in VARIANTS:
            _refit_case(bare[3], n, k, hz, weighting, tau, min_std)


@pytest.mark.parametrize("n,k", [(130, 65), (625, 128)])
def test_refit_and_resample_with_six_actions(bare, n, k):
    for hz in (1, 4, 8):
        for weighting, tau, min_std in VARIANTS:
            _refit_case(bare[6], n, k, hz, weighting, tau, min_std)


def test_refit_resample_refuses_what_the_header_rules_out(bare):
    hd = bare[3]
    c = torch.zeros((8, H, A), device="cuda")
    e = torch.arange(4, dtype=torch.int32, device="cuda")
    with pytest.raises(capi.M3pcError, match="horizon"):
        hd.refit_resample(torch.zeros((8, T + 1, A), device="cuda"), e)
    with pytest.raises(capi.M3pcError, match="scores"):
        hd.refit_resample(c, e, None, R.MPPI, 0.1)
    mean, std = hd.refit_resample(c, e)  # (the handle is still usable)
    assert float(mean.abs().max()) == 0.0 and float(std.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------- 2. the loop, link by link
def _check_chain(world, res, noise, N, k, iterations, score_ref, score_tol, weighting=R.CEM, tau=0.0, min_std=0.0, init_std=0.1,
                 init_mean=None, what=""):
    """Every link of one refine_plan call from its own outputs: candidates of `it` from (mean, std, noise)[it] -> scores[it]
    against `score_ref` on those candidates -> elites[it] the top_k of the returned scores -> mean / std [it + 1] the fp64 refit
    of those candidates on those elites; the final candidates and the two actions bit for bit."""
    out = {n: res[n].cpu() for n in OUTPUTS}
    mean, std = out["mean"], out["std"]
    assert mean.shape == std.shape == (iterations + 1, noise.shape[2], A)
    if init_mean is None:
        assert float((mean[0] - world.mean0).abs().max()) < 1e-5  # tanh of the oracle's policy loc over the last h steps
    else:
        assert torch.equal(mean[0], init_mean.cpu())
    assert bool((std[0] == float(np.float32(init_std))).all())
    for it in range(iterations):
        cand = _rebuild(mean[it], std[it], noise[it])
        ref = score_ref(cand)
        scale = max(1.0, float(ref.abs().max()))
        err = float((out["scores"][it] - ref).abs().max())
        top = R.top_k(out["scores"][it].numpy(), k)
        m, s, D = R.refit(cand.numpy(), out["elites"][it].numpy(), out["scores"][it].numpy(), weighting, tau, min_std)
        em, es = float(np.abs(mean[it + 1].numpy() - m).max()), float(np.abs(std[it + 1].numpy() - s).max())
        print(f"{what} it {it}: |scores - ref| {err:.3e} (scale {scale:.1f}) D {D:.3e} |mean - ref| {em:.2e} |std - ref| {es:.2e}")
        assert err <= score_tol * scale
        assert out["elites"][it].tolist() == top.tolist()
        if weighting == R.MPPI:
            assert D >= 1e-3
        assert em <= 1e-5 and es <= 1e-5
    assert torch.equal(out["candidates"], _rebuild(mean[-1], std[-1], noise[-1]))
    assert out["sample_action"].shape == (1, A) and out["eval_action"].shape == (A,)
    assert torch.equal(out["sample_action"], out["candidates"][0, 0][None]) and torch.equal(out["eval_action"], mean[-1][0])


CHAIN = [("rtg", 64, 16), ("rtg", 130, 65), ("critic", 64, 16), ("critic", 130, 65)]


@pytest.mark.parametrize("mode,N,k", CHAIN)
def test_the_loop_link_by_link(planners, world, mode, N, k):
    p = planners(mode, N)
    s, a, r, h, rtg = _window(p, world)
    noise = _noise(N)
    res = p.handle.refine_plan(MODE[mode], s, a, r, h, rtg, 0.6, 0.99, N, iterations=2, top_k=k, noise=noise.cuda())
    torch.cuda.synchronize()
    _check_chain(world, res, noise, N, k, 2, lambda cand: world.score(mode, cand), 5e-5, what=f"{mode} N {N} k {k}")


def test_the_loop_behind_a_pruned_policy_pass_and_without_the_optional_outputs(planners, world):
    """M3PC_PLAN_PRUNED_POLICY: the policy head at the h action tokens only; the same chain, mean[0] on the oracle's policy mean.
    And the call with scores / elites / sample_action / eval_action passed as NULL: the required outputs keep their bits."""
    mode, N, k = "rtg", 130, 65
    p = planners(mode, N)
    s, a, r, h, rtg = _window(p, world)
    noise = _noise(N)
    res = p.handle.refine_plan(MODE[mode], s, a, r, h, rtg, 0.6, 0.99, N, iterations=2, top_k=k, noise=noise.cuda(), pruned=True)
    torch.cuda.synchronize()
    _check_chain(world, res, noise, N, k, 2, lambda cand: world.score(mode, cand), 5e-5, what="pruned policy pass")
    full = p.handle.refine_plan(MODE[mode], s, a, r, h, rtg, 0.6, 0.99, N, iterations=2, top_k=k, noise=noise.cuda())
    bare_ = p.handle.refine_plan(MODE[mode], s, a, r, h, rtg, 0.6, 0.99, N, iterations=2, top_k=k, noise=noise.cuda(), want_trace=False,
                                 want_actions=False)
    torch.cuda.synchronize()
    assert set(bare_.keys()) == {"mean", "std", "candidates"}
    for name in bare_:
        assert torch.equal(bare_[name], full[name]), name


def test_critic_scoring_without_critic_weights_is_refused_up_front(world):
    p = HipPlanner(_cfg(64, "rtg_guiding"), synth.make_state_dict(DIMS, 0), synth.make_tokenizer_stats(DIMS, 0), None, n_embd=64, n_head=2)
    s, a, r, h, rtg = _window(p, world)
    with pytest.raises(capi.M3pcError, match="m3pc error -2.*critic"):
        p.handle.refine_plan(capi.MODE_CRITIC, s, a, r, h, rtg, 0.6, 0.99, 64, iterations=2, top_k=16)
    res = p.handle.refine_plan(capi.MODE_RTG, s, a, r, h, rtg, 0.6, 0.99, 64, iterations=2, top_k=16)  # (still usable)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(res["scores"]).all())
    p.handle.close()


# ---------------------------------------------------------------------------------------------- 3. end to end against the oracle
@pytest.mark.parametrize("mode,N,k", [("rtg", 130, 65), ("critic", 64, 16)])
def test_refine_plan_matches_the_oracle_where_its_elite_boundary_is_clear(planners, world, mode, N, k):
    noise = _noise(N)
    ref = world.cem_guiding(mode, N, k, noise)
    for it, e in enumerate(ref["trace"]):  # the oracle's own k-th and (k+1)-th scores are more than twice the score tolerance apart
        srt = torch.sort(e["expect_return"], descending=True).values
        scale = max(1.0, float(e["expect_return"].abs().max()))
        gap = float(srt[k - 1] - srt[k])
        print(f"{mode} N {N} k {k} it {it}: elite boundary gap {gap / scale:.3e} x scale")
        assert gap > 1e-4 * scale
    p = planners(mode, N)
    s, a, r, h, rtg = _window(p, world)
    res = p.handle.refine_plan(MODE[mode], s, a, r, h, rtg, 0.6, 0.99, N, iterations=2, top_k=k, noise=noise.cuda())
    torch.cuda.synchronize()
    for it, e in enumerate(ref["trace"]):
        assert set(res["elites"][it].cpu().tolist()) == set(e["top"].tolist())
        assert float((res["mean"][it + 1].cpu() - e["mean"]).abs().max()) <= 1e-5
        assert float((res["std"][it + 1].cpu() - e["std"]).abs().max()) <= 1e-5
    assert float((res["eval_action"].cpu() - ref["eval_action"]).abs().max()) <= 1e-5
    assert float((res["sample_action"].cpu() - ref["sample_action"]).abs().max()) <= 1e-5


# ---------------------------------------------------------------------------------------------- 4. native=True against native=False
@pytest.mark.parametrize("mode,N,k", [("critic", 64, 16), ("rtg", 130, 65)])
def test_native_cem_guiding_against_the_python_loop(planners, world, mode, N, k):
    p = planners(mode, N)
    s, a, r, h, rtg = _window(p, world)
    traj = {"states": s[None], "actions": a[None], "rewards": r[None], "_rtg": rtg}
    noise = _noise(N).cuda()
    sa0, ev0 = p.cem_guiding(traj, h, iterations=2, top_k=k, noise=noise)
    last0 = p.last
    sa1, ev1 = p.cem_guiding(traj, h, iterations=2, top_k=k, noise=noise, native=True)
    last1 = p.last
    torch.cuda.synchronize()
    assert sa1.shape == sa0.shape == (1, A) and ev1.shape == ev0.shape == (A,)
    assert set(last1.keys()) == set(last0.keys()) and len(last1["cem"]) == 2
    for it in range(2):
        g, e = last1["cem"][it], last0["cem"][it]
        assert set(g.keys()) == set(e.keys())
        scale = max(1.0, float(e["expect_return"].abs().max()))
        assert float((g["expect_return"] - e["expect_return"]).abs().max()) <= 5e-5 * scale
        assert set(g["top"].cpu().tolist()) == set(e["top"].cpu().tolist())
        assert float((g["mean"] - e["mean"]).abs().max()) <= 1e-5 and float((g["std"] - e["std"]).abs().max()) <= 1e-5
    # the native leg's candidates are the rebuild from its own last distribution, bit for bit; the two actions as in test 3
    assert torch.equal(last1["candidates"].cpu(), _rebuild(last1["cem"][-1]["mean"].cpu(), last1["cem"][-1]["std"].cpu(), noise[-1].cpu()))
    assert torch.equal(sa1, last1["candidates"][0, 0][None]) and torch.equal(ev1, last1["cem"][-1]["mean"][0])
    assert float((sa1 - sa0).abs().max()) <= 1e-5 and float((ev1 - ev0).abs().max()) <= 1e-5
    for kw in (dict(weighting="mppi"), dict(temperature=0.5), dict(min_std=0.01), dict(init_mean=ev0.new_zeros((h, A)))):
        with pytest.raises(ValueError):
            p.cem_guiding(traj, h, iterations=2, top_k=k, noise=noise, **kw)
    with pytest.raises(ValueError):
        p.cem_guiding(traj, h, iterations=2, top_k=k, noise=noise, native=True, weighting="softmax")


# ---------------------------------------------------------------------------------------------- 5. MPPI
def test_the_mppi_loop_link_by_link(planners, world):
    mode, N, k = "rtg", 130, 65
    p = planners(mode, N)
    s, a, r, h, rtg = _window(p, world)
    noise = _noise(N)
    res = p.handle.refine_plan(MODE[mode], s, a, r, h, rtg, 0.6, 0.99, N, iterations=2, top_k=k, weighting=capi.REFINE_MPPI,
                               temperature=0.01, noise=noise.cuda())
    torch.cuda.synchronize()
    _check_chain(world, res, noise, N, k, 2, lambda cand: world.score(mode, cand), 5e-5, weighting=R.MPPI, tau=0.01, what="mppi")
    # through the planner: the weighting reaches the call (cfg.temperature = 1.0 would give other weights)
    traj = {"states": s[None], "actions": a[None], "rewards": r[None], "_rtg": rtg}
    p.cem_guiding(traj, h, iterations=2, top_k=k, noise=noise.cuda(), native=True, weighting="mppi", temperature=0.01)
    assert torch.equal(p.last["cem"][1]["mean"], res["mean"][2]) and torch.equal(p.last["candidates"], res["candidates"])


# ---------------------------------------------------------------------------------------------- 6. bf16 / bf16x3
@pytest.mark.parametrize("precision,tol", [("bf16", 2e-2), ("bf16x3", 5e-5)])
@pytest.mark.parametrize("mode,N,k", CHAIN)
def test_the_low_precision_loop_link_by_link(planners, world, mode, N, k, precision, tol):
    """The chain of test 2 with the scoring in bf16 / split bf16: the scores against the fp32 scores of the same candidates, the
    elites exactly the top_k of the returned (low-precision) scores, the refit the fp64 refit of those."""
    p = planners(mode, N, precision)
    s, a, r, h, rtg = _window(p, world)
    noise = _noise(N)
    res = p.handle.refine_plan(MODE[mode], s, a, r, h, rtg, 0.6, 0.99, N, iterations=2, top_k=k, noise=noise.cuda(),
                               precision=capi.precision_code(precision))
    torch.cuda.synchronize()

    def fp32_scores(cand):
        return p.handle.score_actions(MODE[mode], s, a, r, cand.cuda(), None, h, 0.6, 0.99, precision=capi.PREC_FP32).cpu()

    _check_chain(world, res, noise, N, k, 2, fp32_scores, tol, what=f"{precision} {mode} N {N} k {k}")


# ---------------------------------------------------------------------------------------------- 7. library-drawn noise
@pytest.mark.parametrize("N,hz", [(130, 4), (65, 1)])
def test_library_drawn_noise_is_draw_variates(planners, world, N, hz):
    """noise = NULL with (seed, step) = (1234, 7) against the same call fed m3pc_draw_variates' array.  N = 130, h = 4: 1560
    elements per iteration, a multiple of 4; N = 65, h = 1: 195, so the slices of iterations 1 and 2 start inside a generator
    block."""
    p = planners("rtg", 130)
    s, a, r, h, rtg = _window(p, world)
    k = N // 2
    drawn, _ = p.handle.draw_variates(1234, 7, 3 * N, hz * A, want_expo=False)
    a1 = p.handle.refine_plan(capi.MODE_RTG, s, a, r, hz, rtg, 0.6, 0.99, N, iterations=2, top_k=k, noise=drawn.reshape(3, N, hz, A))
    a2 = p.handle.refine_plan(capi.MODE_RTG, s, a, r, hz, rtg, 0.6, 0.99, N, iterations=2, top_k=k, seed=1234, step=7)
    a3 = p.handle.refine_plan(capi.MODE_RTG, s, a, r, hz, rtg, 0.6, 0.99, N, iterations=2, top_k=k, seed=1234, step=8)
    torch.cuda.synchronize()
    _equal(a1, a2, f"N {N} h {hz}")
    assert not torch.equal(a3["candidates"], a2["candidates"])
    noise = drawn.reshape(3, N, hz, A).cpu()
    assert torch.equal(a2["candidates"].cpu(), _rebuild(a2["mean"][-1].cpu(), a2["std"][-1].cpu(), noise[-1]))
    assert 0.9 < float(noise.std()) < 1.1


def test_native_cem_guiding_on_the_library_variates(world):
    """HipPlanner(variates="library", seed=...): cem_guiding(native=True) without noise takes (seed, the planner's step index) and
    advances the index; each call equals Handle.refine_plan fed m3pc_draw_variates' array of that (seed, step), bit for bit."""
    N, k, seed = 130, 65, 4321
    p = _tiny(N, "rtg_guiding", variates="library", seed=seed)
    s, a, r, h, rtg = _window(p, world)
    traj = {"states": s[None], "actions": a[None], "rewards": r[None], "_rtg": rtg}
    for step in range(2):
        assert p._step_index == step
        sa, ev = p.cem_guiding(traj, h, iterations=2, top_k=k, native=True)
        last = p.last
        assert p._step_index == step + 1
        drawn, _ = p.handle.draw_variates(seed, step, 3 * N, h * A, want_expo=False)
        want = p.handle.refine_plan(capi.MODE_RTG, s, a, r, h, rtg, 0.6, 0.99, N, iterations=2, top_k=k, noise=drawn.reshape(3, N, h, A))
        torch.cuda.synchronize()
        assert torch.equal(sa, want["sample_action"]) and torch.equal(ev, want["eval_action"])
        assert torch.equal(last["candidates"], want["candidates"])
        for it in range(2):
            assert torch.equal(last["cem"][it]["expect_return"], want["scores"][it]) and torch.equal(last["cem"][it]["top"], want["elites"][it])
            assert torch.equal(last["cem"][it]["mean"], want["mean"][it + 1]) and torch.equal(last["cem"][it]["std"], want["std"][it + 1])
    # a plan step after it still plans (the step index the refinement took has no entry in the certificate history)
    ev = p.action_sample(world.hist, plan=True, eval=True, rtg=3.0)
    assert ev.shape == (A,) and bool(torch.isfinite(ev).all()) and p._step_index > 2
    p.handle.close()


# ---------------------------------------------------------------------------------------------- 8. warm start
def test_warm_start(planners, world):
    mode, N, k = "rtg", 130, 65
    p = planners(mode, N)
    s, a, r, h, rtg = _window(p, world)
    noise = _noise(N)
    init = (torch.rand(h, A, generator=torch.Generator().manual_seed(3)) - 0.5).cuda()
    res = p.handle.refine_plan(MODE[mode], s, a, r, h, rtg, 0.6, 0.99, N, iterations=2, top_k=k, noise=noise.cuda(), init_mean=init)
    torch.cuda.synchronize()
    assert torch.equal(res["mean"][0], init)
    _check_chain(world, res, noise, N, k, 2, lambda cand: world.score(mode, cand), 5e-5, init_mean=init, what="warm start")

    def pair():  # the example's pattern: the second refinement starts from the first one's final mean, nothing read back between
        one = p.handle.refine_plan(MODE[mode], s, a, r, h, rtg, 0.6, 0.99, N, iterations=2, top_k=k, seed=5, step=40)
        two = p.handle.refine_plan(MODE[mode], s, a, r, h, rtg, 0.6, 0.99, N, iterations=2, top_k=k, seed=5, step=41, init_mean=one["mean"][-1])
        return one, two

    (a1, a2), (b1, b2) = pair(), pair()
    torch.cuda.synchronize()
    assert torch.equal(a2["mean"][0], a1["mean"][-1])
    assert float((a1["mean"][0].cpu() - world.mean0).abs().max()) < 1e-5
    _equal(a1, b1, "first call")
    _equal(a2, b2, "warm-started call")
    assert not torch.equal(a2["candidates"], a1["candidates"])


# ---------------------------------------------------------------------------------------------- 9. state
def test_refine_plan_is_refused_while_a_pipelined_step_is_begun(planners, world):
    N, k = 64, 16
    p = planners("rtg", N, "bf16", rescore_delta=1.0)
    hd = p.handle
    s, a, r, h, rtg = _window(p, world)
    eps = synth.make_eps(N, DIMS, 1).cuda().reshape(N, -1).contiguous()
    q = torch.empty(N, dtype=torch.float32).exponential_(1, generator=torch.Generator().manual_seed(77)).cuda()
    cert = dict(delta=1.0, kmin=8, kmax=32, rfirst=2, rmax=16)
    step = (capi.MODE_RTG, s, a, r, eps, q, h, rtg, 0.6, 0.99, N, 0.01)
    noise = _noise(N).cuda()
    refine = lambda: hd.refine_plan(capi.MODE_RTG, s, a, r, h, rtg, 0.6, 0.99, N, iterations=2, top_k=k, noise=noise,
                                    precision=capi.PREC_BF16)
    twin, trec = hd.plan_step_certified(*step, slot=0, **cert)
    first = refine()
    torch.cuda.synchronize()
    res = hd.plan_step_certified_begin(*step, slot=1, **cert)
    with pytest.raises(capi.M3pcError, match="m3pc error -2"):
        refine()
    rec = hd.plan_step_certified_end(1)
    torch.cuda.synchronize()
    for name in ("loc", "std", "sample_actions", "expect_return_low", "expect_return"):
        assert torch.equal(res[name], twin[name]), name
    for t0, t1 in zip(res["sel"], twin["sel"]):
        assert torch.equal(t0, t1)
    for name, _ in capi.CertRecord._fields_:
        assert getattr(rec, name) == getattr(trec, name), name
    again = refine()
    torch.cuda.synchronize()
    _equal(first, again, "the call made twice")
    # bad arguments leave the handle usable too
    with pytest.raises(capi.M3pcError, match="top_k"):
        hd.refine_plan(capi.MODE_RTG, s, a, r, h, rtg, 0.6, 0.99, N, iterations=2, top_k=N + 1, noise=noise)
    with pytest.raises(capi.M3pcError, match="max_candidates"):
        hd.refine_plan(capi.MODE_RTG, s, a, r, h, rtg, 0.6, 0.99, N + 1, iterations=2, top_k=k)
    _equal(first, refine(), "after refused calls")


# ---------------------------------------------------------------------------------------------- 10. the C example
def test_c_example_refines_twice_with_a_warm_start(tmp_path, planners, world):
    """examples/refine_plan.c compiled with gcc -Wall -Werror against include/m3pc_hip.h, linked to the built library and run:
    its two refinements (library-drawn noise, the second warm-started) equal Handle.refine_plan on the same inputs bit for bit."""
    so = tmp_path / "librefine_plan.so"
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "refine_plan.c"), "-o", str(so), "-L", libdir,
                           "-l:" + os.path.basename(capi.LIB_PATH), "-Wl,-rpath," + libdir])
    N, k, iters = 130, 65, 2
    p = planners("rtg", N)
    s, a, r, h, rtg = _window(p, world)
    fp, vp = C.POINTER(C.c_float), C.c_void_p

    class IO(C.Structure):
        _fields_ = [("dims", C.POINTER(capi.Dims)), ("weights", C.POINTER(capi.NamedTensor)), ("n_weights", C.c_int),
                    ("tok_mean", fp * 4), ("tok_std", fp * 4), ("tok_dim", C.c_int * 4), ("tok_normalize", C.c_int * 4),
                    ("states", vp * 2), ("actions", vp * 2), ("rewards", vp * 2), ("n", C.c_int), ("horizon", C.c_int),
                    ("precision", C.c_int), ("iterations", C.c_int), ("top_k", C.c_int), ("weighting", C.c_int),
                    ("temperature", C.c_float), ("init_std", C.c_float), ("min_std", C.c_float),
                    ("rtg", C.c_double), ("lmbda", C.c_double), ("discount", C.c_double), ("seed", C.c_ulonglong), ("step", C.c_ulonglong),
                    ("mean", vp * 2), ("std", vp * 2), ("candidates", vp * 2), ("sample_action", vp * 2), ("eval_action", vp * 2)]

    sd = synth.make_state_dict(DIMS, 0)
    arr, keep = capi._named(sd)
    io = IO()
    io.dims, io.weights, io.n_weights = C.pointer(p.handle.dims), C.cast(arr, C.POINTER(capi.NamedTensor)), len(sd)
    toks = []
    for key, name in enumerate(capi.KEYS):
        t = p.tokenizer_manager.tokenizers[name]
        m, sdv = t._data_mean.float().contiguous().reshape(-1), t._data_std.float().contiguous().reshape(-1)
        toks.append((m, sdv))
        io.tok_mean[key], io.tok_std[key] = C.cast(m.data_ptr(), fp), C.cast(sdv.data_ptr(), fp)
        io.tok_dim[key], io.tok_normalize[key] = m.numel(), int(bool(t.normalize))
    dev = dict(device="cuda")
    outs = [dict(mean=torch.empty((iters + 1, h, A), **dev), std=torch.empty((iters + 1, h, A), **dev),
                 candidates=torch.empty((N, h, A), **dev), sample_action=torch.empty((1, A), **dev), eval_action=torch.empty(A, **dev))
            for _ in range(2)]
    for c in range(2):
        io.states[c], io.actions[c], io.rewards[c] = s.data_ptr(), a.data_ptr(), r.data_ptr()
        for name, t in outs[c].items():
            getattr(io, name)[c] = t.data_ptr()
    io.n, io.horizon, io.precision, io.iterations, io.top_k, io.weighting = N, h, capi.PREC_FP32, iters, k, capi.REFINE_MPPI
    io.temperature, io.init_std, io.min_std, io.rtg, io.lmbda, io.discount, io.seed, io.step = 0.01, 0.1, 0.01, rtg, 0.6, 0.99, 2 ** 40 + 9, 2 ** 33
    torch.cuda.synchronize()
    lib = C.CDLL(str(so))
    lib.refine_plan.restype = C.c_int
    lib.refine_plan.argtypes = [C.POINTER(IO), C.c_int, vp]
    rc = lib.refine_plan(C.byref(io), torch.cuda.current_device(), vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, p.handle.lib.m3pc_last_error()
    torch.cuda.synchronize()
    kw = dict(iterations=iters, top_k=k, weighting=capi.REFINE_MPPI, temperature=0.01, init_std=0.1, min_std=0.01, seed=2 ** 40 + 9)
    one = p.handle.refine_plan(capi.MODE_RTG, s, a, r, h, rtg, 0.6, 0.99, N, step=2 ** 33, **kw)
    two = p.handle.refine_plan(capi.MODE_RTG, s, a, r, h, rtg, 0.6, 0.99, N, step=2 ** 33 + 1, init_mean=one["mean"][-1], **kw)
    torch.cuda.synchronize()
    for c, want in enumerate((one, two)):
        for name, t in outs[c].items():
            assert torch.equal(t, want[name]), (c, name)
    assert bool((one["std"][1:] >= float(np.float32(0.01))).all())
    del keep, toks
