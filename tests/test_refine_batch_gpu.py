"""CEM / MPPI refinement of a lock-step batch of windows as one call (m3pc_refine_plans, Handle.refine_plans,
HipPlanner.cem_guiding_batch, HipPlanner(refine=...)): the batched refit / resample / top-k / variates kernels link by link against
what the library itself returns for one window, the shifted warm start, the refusals, the single call and the oracle where the
oracle's own elite boundary is clear, the planner's warm-start memory and the C example.  All on the tiny model of
tests/test_refine_gpu.py (T = 8, H = 4, S = 11, A = 3, n_embd = 64, n_head = 2); planners are built with max_batch = max_windows = E."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import refine_ref as R
import test_refine_gpu as G
from m3pc_amd import capi, synth
from m3pc_amd.planner import HipPlanner
from m3pc_amd.rollout import evaluate_plan
from oracle import mtm_oracle as O

pytestmark = pytest.mark.gpu
ROOT = G.ROOT
T, H, S, A, DIMS, MODE, GUIDANCE = G.T, G.H, G.S, G.A, G.DIMS, G.MODE, G.GUIDANCE
_rebuild = G._rebuild
OUTPUTS = G.OUTPUTS
RTGS = (3.0, 3.5, 4.0)
LMBDA, DISCOUNT = 0.6, 0.99


def _tiny(N, guidance="rtg_guiding", E=3, **kw):
    return G._tiny(N, guidance, max_batch=E, max_windows=E, **kw)


@pytest.fixture(scope="module")
def planners():
    """Planners of the tiny model by (mode, N, precision, E), shared by the tests of this file that only read them."""
    cache = {}

    def get(mode, N, precision="fp32", E=3, **kw):
        key = (mode, N, precision, E, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = _tiny(N, GUIDANCE[mode], E, precision=precision, **kw)
        return cache[key]

    yield get
    for p in cache.values():
        p.handle.close()


def _history(seed, path_length=100):
    hist = synth.make_history(DIMS, seed)
    hist["path_length"] = path_length
    return hist


def _windows(p, seeds, rtgs=None):
    """(states (E,T,S), actions (E,T,A), rewards (E,T,1), h, [rtg]) of the histories of ``seeds`` at path_length 100."""
    rtgs = [RTGS[i % 3] for i in range(len(seeds))] if rtgs is None else rtgs
    parts, rt = [], []
    for seed, g in zip(seeds, rtgs):
        s, a, r, h, rtg = p.assemble_window(_history(seed), rtg=g)
        assert h == H
        parts.append((s.clone(), a.clone(), r.clone()))
        rt.append(rtg)
    return tuple(torch.stack([q[i] for q in parts]).contiguous() for i in range(3)) + (H, rt)


def _noise(N, E, h=H, iterations=2, seed=11, ties=True):
    """(iterations+1, E, N, h, A) normals; ties: rows 5 and N-1 of every window repeat rows 3 and 7 (N > 8), in every iteration,
    so that two pairs of candidates of a window are equal and their scores tie exactly."""
    z = torch.randn(iterations + 1, E, N, h, A, generator=torch.Generator().manual_seed(seed))
    if ties and N > 8:
        z[:, :, 5] = z[:, :, 3]
        z[:, :, N - 1] = z[:, :, 7]
    return z


def _cpu(res):
    return {n: res[n].cpu() for n in OUTPUTS if n in res}


def _equal(a, b, what=""):
    for name in OUTPUTS:
        assert torch.equal(a[name], b[name]), (what, name)


def _check_links(hd, mode, precision, win, res, noise, N, k, iterations, weighting, tau, min_std=0.0, init_std=0.1, windows=None,
                 loc=None, ties=True, what=""):
    """Every link of one refine_plans call from its own outputs and from what the library returns for the same rows."""
    s, a, r, h_win, rtgs = win
    E, hz = s.shape[0], noise.shape[3]
    out = _cpu(res)
    mean, std = out["mean"], out["std"]
    assert mean.shape == std.shape == (iterations + 1, E, hz, A)
    windows = range(E) if windows is None else windows
    if loc is not None:
        for w in windows:
            assert float((mean[0, w] - torch.tanh(loc[w, T - hz:])).abs().max()) < 1e-5, (what, w)
    assert bool((std[0] == float(np.float32(init_std))).all())
    widx = (torch.arange(E * N, dtype=torch.int32) // N).cuda()
    for it in range(iterations):
        cand = torch.stack([_rebuild(mean[it, w], std[it, w], noise[it, w]) for w in range(E)])  # (E, N, hz, A)
        # the same call on the same rows in the same workspace regime
        again = hd.score_actions(MODE[mode], s, a, r, cand.reshape(E * N, hz, A).cuda(), widx, hz, LMBDA, DISCOUNT,
                                 precision=capi.precision_code(precision)).cpu().reshape(E, N)
        assert torch.equal(again, out["scores"][it]), (what, it)
        for w in windows:
            sc, el = out["scores"][it, w], out["elites"][it, w]
            if ties and N > 8:
                assert float(sc[5]) == float(sc[3]) and float(sc[N - 1]) == float(sc[7]), (what, it, w)
            assert el.tolist() == R.top_k(sc.numpy(), k).tolist(), (what, it, w)
            one = hd.refit_resample(cand[w].cuda(), el.cuda(), sc.cuda(), weighting, tau, min_std)
            assert torch.equal(one[0].cpu(), mean[it + 1, w]) and torch.equal(one[1].cpu(), std[it + 1, w]), (what, it, w)
            m, sd, D = R.refit(cand[w].numpy(), el.numpy(), sc.numpy(), weighting, tau, min_std)
            em, es = float(np.abs(mean[it + 1, w].numpy() - m).max()), float(np.abs(std[it + 1, w].numpy() - sd).max())
            print(f"{what} it {it} window {w}: D {D:.3e} |mean - ref| {em:.2e} |std - ref| {es:.2e}")
            assert em <= 1e-5 and es <= 1e-5, (what, it, w)
    for w in windows:
        assert torch.equal(out["candidates"][w], _rebuild(mean[-1, w], std[-1, w], noise[-1, w])), (what, w)
        assert torch.equal(out["sample_action"][w], out["candidates"][w, 0, 0]) and torch.equal(out["eval_action"][w], mean[-1, w, 0])


def _policy_loc(hd, mode, win, hz):
    s, a, r, _, rtgs = win
    loc = torch.empty((s.shape[0], T, A), device="cuda")
    hd.policy_pass_batch(MODE[mode], s, a, r, hz, rtgs, loc=loc, std=torch.empty_like(loc))
    return loc.cpu()


def _call(hd, mode, win, hz, N, k, precision="fp32", **kw):
    s, a, r, _, rtgs = win
    res = hd.refine_plans(MODE[mode], s, a, r, hz, rtgs, LMBDA, DISCOUNT, N, top_k=k, precision=capi.precision_code(precision), **kw)
    torch.cuda.synchronize()
    return res


# ---------------------------------------------------------------------------------------------- 1. link by link
SHAPES = [(130, 65, H), (65, 1, 1), (1500, 1025, H)]


@pytest.mark.parametrize("weighting,tau", [(R.CEM, 0.0), (R.MPPI, 0.01)])
@pytest.mark.parametrize("mode,precision", [("rtg", "fp32"), ("rtg", "bf16"), ("critic", "fp32")])
@pytest.mark.parametrize("N,k,hz", SHAPES)
def test_the_batched_loop_link_by_link(planners, N, k, hz, mode, precision, weighting, tau):
    """E = 3 windows of three histories.  (130, 65): k on both sides of a wave; (65, 1) at h = 1: 195 elements per window, so the
    blocks of windows 1 and 2 are not 16-byte aligned and every window takes the scalar path; (1500, 1025): one elite more than a
    workgroup keeps in registers, and the ranking by blocks at its largest."""
    p = planners(mode, N, precision)
    win = _windows(p, (0, 1, 2))
    noise = _noise(N, 3, hz)
    loc = _policy_loc(p.handle, mode, win, hz)
    res = _call(p.handle, mode, win, hz, N, k, precision, iterations=2, weighting=weighting, temperature=tau, noise=noise.cuda())
    _check_links(p.handle, mode, precision, win, res, noise, N, k, 2, weighting, tau, loc=loc,
                 what=f"{mode} {precision} N {N} k {k} h {hz} weighting {weighting}")


# ---------------------------------------------------------------------------------------------- 2. the top-k regimes
@pytest.mark.parametrize("N,k", [(2048, 64), (2049, 64), (2049, 65)])
def test_the_three_top_k_regimes_through_the_loop(planners, N, k):
    """n = 2048: the ranking by blocks at its limit; 2049 with k = 64: the selection; 2049 with k = 65: the bitonic sort."""
    p = planners("rtg", N, "fp32", E=2)
    win = _windows(p, (0, 1))
    noise = _noise(N, 2, iterations=1)
    res = _cpu(_call(p.handle, "rtg", win, H, N, k, iterations=1, noise=noise.cuda()))
    for w in range(2):
        sc = res["scores"][0, w]
        assert float(sc[5]) == float(sc[3]) and float(sc[N - 1]) == float(sc[7])
        assert res["elites"][0, w].tolist() == R.top_k(sc.numpy(), k).tolist(), w


# ---------------------------------------------------------------------------------------------- 3. more than 64 windows
def test_more_than_64_windows(planners):
    """E = 65 crosses the 64 windows a launch of the batched resample / variates kernels carries in its arguments."""
    E, N, k = 65, 16, 4
    p = planners("rtg", N, "fp32", E=E)
    win = _windows(p, tuple(range(E)), rtgs=[3.0 + 0.01 * w for w in range(E)])
    noise = _noise(N, E)
    loc = _policy_loc(p.handle, "rtg", win, H)
    res = _call(p.handle, "rtg", win, H, N, k, iterations=2, noise=noise.cuda())
    _check_links(p.handle, "rtg", "fp32", win, res, noise, N, k, 2, R.CEM, 0.0, windows=(0, 63, 64), loc=loc, what="E 65")
    # library noise: window w's variates are those of its own step
    steps = [1000 + 3 * w for w in range(E)]
    drawn = _cpu(_call(p.handle, "rtg", win, H, N, k, iterations=2, seed=9, steps=steps))
    for w in (0, 63, 64):
        z, _ = p.handle.draw_variates(9, steps[w], 3 * N, H * A, want_expo=False)
        z = z.reshape(3, N, H, A).cpu()
        assert torch.equal(drawn["candidates"][w], _rebuild(drawn["mean"][-1, w], drawn["std"][-1, w], z[-1])), w


# ---------------------------------------------------------------------------------------------- 4. the shift
def test_the_shifted_warm_start(planners):
    N, k, h = 130, 65, H
    p = planners("rtg", N)
    win = _windows(p, (0, 1, 2))
    noise = _noise(N, 3)
    loc = _policy_loc(p.handle, "rtg", win, h)
    pol = torch.tanh(loc[:, T - h:])
    init = (torch.rand(3, h + 1, A, generator=torch.Generator().manual_seed(3)) * 1.8 - 0.9)
    res = _call(p.handle, "rtg", win, h, N, k, iterations=2, noise=noise.cuda(), init_mean=init.cuda(), init_rows=[h + 1, h, 0], init_offset=1)
    m0 = res["mean"][0].cpu()
    assert torch.equal(m0[0], init[0, 1:h + 1])
    assert torch.equal(m0[1, :h - 1], init[1, 1:h]) and float((m0[1, h - 1] - pol[1, h - 1]).abs().max()) < 1e-5
    assert not torch.equal(m0[1, h - 1], init[1, h])
    cold = _call(p.handle, "rtg", win, h, N, k, iterations=2, noise=noise.cuda())
    assert torch.equal(m0[2], cold["mean"][0, 2].cpu()) and float((m0[2] - pol[2]).abs().max()) < 1e-5
    _check_links(p.handle, "rtg", "fp32", win, res, noise, N, k, 2, R.CEM, 0.0, what="shifted warm start")
    # offset 0, every row given: the caller's mean as it is
    res = _call(p.handle, "rtg", win, h, N, k, iterations=2, noise=noise.cuda(), init_mean=init[:, :h].contiguous().cuda())
    assert torch.equal(res["mean"][0].cpu(), init[:, :h])
    # h = 1, offset 1, one row: nothing of it is left, the whole mean comes from the policy head
    loc1 = _policy_loc(p.handle, "rtg", win, 1)
    res = _call(p.handle, "rtg", win, 1, N, k, iterations=2, noise=_noise(N, 3, 1).cuda(), init_mean=init[:, :1].contiguous().cuda(),
                init_rows=[1, 1, 1], init_offset=1)
    assert float((res["mean"][0].cpu() - torch.tanh(loc1[:, T - 1:])).abs().max()) < 1e-5
    cold1 = _call(p.handle, "rtg", win, 1, N, k, iterations=2, noise=_noise(N, 3, 1).cuda())
    _equal(res, cold1, "h = 1")


# ---------------------------------------------------------------------------------------------- 5. library noise
@pytest.mark.parametrize("N,hz", [(130, H), (65, 1)])
def test_library_drawn_noise_per_window(planners, N, hz):
    p = planners("rtg", 130)
    win = _windows(p, (0, 0, 2), rtgs=[3.0, 3.0, 4.0])  # windows 0 and 1: the same history and return-to-go
    k, seed, steps = N // 2, 1234, [7, 7, 9]
    init = torch.zeros(3, hz, A).cuda()
    res = _cpu(_call(p.handle, "rtg", win, hz, N, k, iterations=2, seed=seed, steps=steps, init_std=0.3, init_mean=init))
    z = [p.handle.draw_variates(seed, st, 3 * N, hz * A, want_expo=False)[0].reshape(3, N, hz, A).cpu() for st in steps]
    assert torch.equal(z[0], z[1]) and not torch.equal(z[0], z[2])
    # the first candidates of windows 0 and 1 are equal: the same noise on the same distribution
    fed = _cpu(_call(p.handle, "rtg", win, hz, N, k, iterations=2, noise=torch.stack(z, dim=1).contiguous().cuda(), init_std=0.3, init_mean=init))
    _equal(res, fed, "fed the drawn noise")
    first = torch.stack([_rebuild(res["mean"][0, w], res["std"][0, w], z[w][0]) for w in range(3)])
    assert torch.equal(first[0], first[1]) and not torch.equal(first[0], first[2])
    assert torch.equal(res["scores"][0, 0], res["scores"][0, 1])
    for w in range(3):
        assert torch.equal(res["candidates"][w], _rebuild(res["mean"][-1, w], res["std"][-1, w], z[w][-1])), w
    # steps = NULL: the refine step + w
    a1 = _cpu(_call(p.handle, "rtg", win, hz, N, k, iterations=2, seed=seed, step=40))
    a2 = _cpu(_call(p.handle, "rtg", win, hz, N, k, iterations=2, seed=seed, steps=[40, 41, 42]))
    _equal(a1, a2, "steps = NULL")
    assert not torch.equal(a1["candidates"][0], a1["candidates"][1])


# ---------------------------------------------------------------------------------------------- 6. the single call, the oracle
# history seeds per case, picked on the CPU: with rtg 3.0 / 3.5 / 4.0 and slice w of _noise(N, 3, ties=False) the oracle's own k-th and
# (k+1)-th scores are more than 1e-4 of the score scale apart in both iterations (asserted below)
CLEAR = [("rtg", 130, 65, (0, 1, 2)), ("critic", 64, 16, (0, 1, 4))]


@pytest.fixture(scope="module")
def oracle():
    """The oracle's cem_guiding per (mode, N, k, history seed, window slot), computed once on the CPU."""
    sd, st = synth.make_state_dict(DIMS, 0), O.make_stats(synth.make_tokenizer_stats(DIMS, 0))
    critic = synth.make_critic(DIMS, 0)
    cache = {}

    def get(mode, N, k, seed, slot):
        key = (mode, N, k, seed, slot)
        if key not in cache:
            cfg = O.PlanCfg(T, H, N, n_head=2)
            win, h = O.assemble_window(cfg, _history(seed), 100, RTGS[slot])
            ref = O.cem_guiding(sd, st, cfg, win, h, LMBDA, _noise(N, 3, ties=False)[:, slot], mode, critic=critic, iterations=2, top_k=k)
            for it, e in enumerate(ref["trace"]):
                srt = torch.sort(e["expect_return"], descending=True).values
                scale = max(1.0, float(e["expect_return"].abs().max()))
                gap = float(srt[k - 1] - srt[k])
                print(f"{mode} N {N} k {k} history {seed} window {slot} it {it}: elite boundary gap {gap / scale:.3e} x scale")
                assert gap > 1e-4 * scale
            cache[key] = ref
        return cache[key]

    return get


@pytest.mark.parametrize("mode,N,k,seeds", CLEAR)
def test_a_batch_of_one_against_the_single_call(planners, oracle, mode, N, k, seeds):
    oracle(mode, N, k, seeds[0], 0)  # (the boundary of this window's trace is clear)
    p = planners(mode, N)
    win = _windows(p, seeds[:1])
    noise = _noise(N, 3, ties=False)[:, :1].contiguous()
    s, a, r, h, rtgs = win
    one = p.handle.refine_plan(MODE[mode], s[0], a[0], r[0], h, rtgs[0], LMBDA, DISCOUNT, N, iterations=2, top_k=k, noise=noise[:, 0].contiguous().cuda())
    res = _call(p.handle, mode, win, h, N, k, iterations=2, noise=noise.cuda(), init_offset=0)
    assert float((res["mean"][:, 0] - one["mean"]).abs().max()) <= 1e-5 and float((res["std"][:, 0] - one["std"]).abs().max()) <= 1e-5
    for it in range(2):
        assert set(res["elites"][it, 0].cpu().tolist()) == set(one["elites"][it].cpu().tolist())
    assert float((res["sample_action"] - one["sample_action"]).abs().max()) <= 1e-5
    assert float((res["eval_action"][0] - one["eval_action"]).abs().max()) <= 1e-5


@pytest.mark.parametrize("mode,N,k,seeds", CLEAR)
def test_every_window_of_a_batch_against_the_oracle(planners, oracle, mode, N, k, seeds):
    p = planners(mode, N)
    win = _windows(p, seeds)
    noise = _noise(N, 3, ties=False)
    res = _cpu(_call(p.handle, mode, win, H, N, k, iterations=2, noise=noise.cuda()))
    for w, seed in enumerate(seeds):
        ref = oracle(mode, N, k, seed, w)
        for it, e in enumerate(ref["trace"]):
            assert set(res["elites"][it, w].tolist()) == set(e["top"].tolist()), (w, it)
            assert float((res["mean"][it + 1, w] - e["mean"]).abs().max()) <= 1e-5, (w, it)
            assert float((res["std"][it + 1, w] - e["std"]).abs().max()) <= 1e-5, (w, it)
        assert float((res["eval_action"][w] - ref["eval_action"]).abs().max()) <= 1e-5
        assert float((res["sample_action"][w] - ref["sample_action"].reshape(-1)).abs().max()) <= 1e-5


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_handle_usable(planners):
    N, k, E = 64, 16, 3
    p = planners("rtg", N, "bf16", rescore_delta=1.0)
    hd = p.handle
    win = _windows(p, (0, 1, 2))
    s, a, r, h, rtgs = win
    noise = _noise(N, E).cuda()
    init = torch.zeros(E, h, A).cuda()
    good = lambda: _cpu(_call(hd, "rtg", win, h, N, k, "bf16", iterations=2, noise=noise))
    first = good()

    def refused(code, match=None, mode="rtg", n=N, windows=win, **kw):
        kw = {**dict(iterations=2, noise=noise, top_k=k), **kw}
        ss, aa, rr, _, rt = windows
        with pytest.raises(capi.M3pcError, match=f"m3pc error {code}" + (f".*{match}" if match else "")):
            hd.refine_plans(MODE.get(mode, mode), ss, aa, rr, kw.pop("hz", h), rt, LMBDA, DISCOUNT, n, precision=capi.PREC_BF16, **kw)
        _equal(first, good(), f"after {code} {match} {kw.keys()}")

    # every check of m3pc_refine_plan
    refused(-1, "iterations", iterations=0, noise=None)
    refused(-1, "iterations", iterations=capi.REFINE_MAX_ITER + 1, noise=None)
    refused(-1, "top_k", top_k=N + 1)
    refused(-1, "top_k", top_k=0)
    refused(-1, "weighting", weighting=2)
    refused(-1, "temperature", weighting=capi.REFINE_MPPI, temperature=-1.0)
    refused(-1, "min_std", min_std=float("nan"))
    refused(-1, "init_std", init_std=float("inf"))
    refused(-1, "horizon", hz=T + 1, noise=None)
    refused(-1, "mode", mode=capi.MODE_NOISE)
    refused(-1, None, hz=0, noise=None)  # (the binding's empty outputs are null pointers: refused as such)
    # the batch's own
    empty = (s[:0], a[:0], r[:0], h, [])
    refused(-1, "n_windows", windows=empty, noise=None)
    refused(-1, "init_offset", init_offset=-1)
    refused(-1, "init_rows", init_mean=init, init_rows=[0, h + 1, 0])
    refused(-1, "init_rows", init_mean=init, init_rows=[-1, 0, 0])
    big = tuple(torch.cat([t, t[:1]]) for t in (s, a, r)) + (h, rtgs + [3.0])
    refused(-4, "max_batch", windows=big, n=16, top_k=4, noise=None)  # (M3PC_ENOMEM, as m3pc_policy_pass_batch)
    refused(-4, "max_candidates", n=N + 1, noise=None)
    # through the raw prototype: what the binding cannot express (args->returns, args->flags, init_stride < 1)
    out = {n_: torch.empty_like(first[n_], device="cuda") for n_ in ("mean", "std", "candidates")}

    def raw(returns=None, flags=0, stride=h):
        args = hd._args(capi.MODE_RTG, capi.PREC_BF16, h, N, 0, N, LMBDA, DISCOUNT, 0.0, 0, returns)
        args.flags = flags
        ref = capi.RefineArgs(2, k, capi.REFINE_CEM, 0.0, 0.1, 0.0, 0, 0, 0, 0)
        return hd.lib.m3pc_refine_plans(hd._h, C.byref(args), C.byref(ref), E, capi._ptr(s), capi._ptr(a), capi._ptr(r),
                                        (C.c_double * E)(*rtgs), capi._ptr(init), stride, None, 0, capi._ptr(noise), None,
                                        capi._ptr(out["mean"]), capi._ptr(out["std"]), capi._ptr(out["candidates"]), None, None, None, None,
                                        capi._stream(hd.device))

    assert raw(returns=torch.zeros(T, device="cuda")) == -1
    assert raw(flags=capi.PLAN_PRUNED_POLICY) == -1
    assert raw(stride=0) == -1
    _equal(first, good(), "after the raw refusals")
    # state: a pipelined certified step begun
    eps = synth.make_eps(N, DIMS, 1).cuda().reshape(N, -1).contiguous()
    q = torch.empty(N, dtype=torch.float32).exponential_(1, generator=torch.Generator().manual_seed(77)).cuda()
    hd.plan_step_certified_begin(capi.MODE_RTG, s[0], a[0], r[0], eps, q, h, rtgs[0], LMBDA, DISCOUNT, N, 0.01, slot=1, delta=1.0, kmin=8,
                                 kmax=32, rfirst=2, rmax=16)
    with pytest.raises(capi.M3pcError, match="m3pc error -2"):
        _call(hd, "rtg", win, h, N, k, "bf16", iterations=2, noise=noise)
    hd.plan_step_certified_end(1)
    torch.cuda.synchronize()
    _equal(first, good(), "after the state refusal")


def test_critic_scoring_without_critic_weights_is_refused_up_front():
    p = HipPlanner(G._cfg(64, "rtg_guiding"), synth.make_state_dict(DIMS, 0), synth.make_tokenizer_stats(DIMS, 0), None, n_embd=64,
                   n_head=2, max_batch=3, max_windows=3)
    win = _windows(p, (0, 1, 2))
    noise = _noise(64, 3).cuda()
    first = _cpu(_call(p.handle, "rtg", win, H, 64, 16, iterations=2, noise=noise))
    with pytest.raises(capi.M3pcError, match="m3pc error -2.*critic"):
        _call(p.handle, "critic", win, H, 64, 16, iterations=2, noise=noise)
    _equal(first, _cpu(_call(p.handle, "rtg", win, H, 64, 16, iterations=2, noise=noise)), "after the refusal")
    p.handle.close()


# ---------------------------------------------------------------------------------------------- 8. the planner
REFINE = dict(iterations=2, top_k=16, weighting="mppi", warm=True)


def _advance(hist, steps=1):
    hist = dict(hist)
    hist["path_length"] = int(hist["path_length"]) + steps
    return hist


def test_the_planner_keeps_a_shifted_warm_start():
    N = 64
    p = _tiny(N, E=2, refine=REFINE, variates="library", seed=5)
    hist = _history(0, 100)
    steps = []
    for t in range(3):
        ev = p.action_sample(_advance(hist, t), plan=True, eval=True, rtg=3.0)
        assert ev.shape == (A,) and bool(torch.isfinite(ev).all())
        steps.append(p.last["windows"][0])
    assert not steps[0]["warm"] and steps[0]["init_rows"] == 0 and steps[0]["horizon"] == H
    for prev, cur in zip(steps, steps[1:]):
        assert cur["warm"] and cur["init_rows"] == H
        assert torch.equal(cur["mean0"][:H - 1], prev["mean"][1:])
        assert not torch.equal(cur["mean0"][H - 1], prev["mean"][H - 1])
    sa = p.action_sample(_advance(hist, 3), plan=True, eval=False, rtg=3.0)
    assert sa.shape == (1, A) and p.last["windows"][0]["warm"]
    # a path_length that jumps, a repeated step and a weight load are cold starts
    p.action_sample(_advance(hist, 5), plan=True, eval=True, rtg=3.0)
    assert not p.last["windows"][0]["warm"]
    p.action_sample(_advance(hist, 5), plan=True, eval=True, rtg=3.0)
    assert not p.last["windows"][0]["warm"]
    p.action_sample(_advance(hist, 6), plan=True, eval=True, rtg=3.0)
    assert p.last["windows"][0]["warm"]
    p.load_state_dict(synth.make_state_dict(DIMS, 0))
    p.action_sample(_advance(hist, 7), plan=True, eval=True, rtg=3.0)
    assert not p.last["windows"][0]["warm"]
    with pytest.raises(ValueError):
        p.plan_async(hist, eval=True, rtg=3.0)
    p.handle.close()
    with pytest.raises(ValueError):
        G._tiny(N, "noise_adding_lambda", refine=REFINE)


def test_the_shrinking_horizon_of_an_episode_start_takes_every_row_from_the_previous_mean():
    """path_length < T - H: the effective horizon is T - path_length, one less per step, so the shifted plan fills every row."""
    N = 64
    p = _tiny(N, E=2, refine=REFINE, variates="library", seed=5)
    hist = _history(0, 1)
    p.action_sample(hist, plan=True, eval=True, rtg=3.0)
    first = p.last["windows"][0]
    assert first["horizon"] == T - 1 and not first["warm"]
    p.action_sample(_advance(hist), plan=True, eval=True, rtg=3.0)
    second = p.last["windows"][0]
    assert second["horizon"] == T - 2 and second["warm"] and second["init_rows"] == T - 1
    assert torch.equal(second["mean0"], first["mean"][1:])
    p.handle.close()


def test_action_sample_batch_groups_by_horizon_and_equals_cem_guiding_batch():
    N, E = 64, 3
    kw = dict(E=E, refine=dict(REFINE, warm=False), variates="library", seed=21)
    p, twin = _tiny(N, **kw), _tiny(N, **kw)
    hists = [_history(0, 100), _history(1, 2), _history(2, 100)]  # horizons H, T - 2, H
    rtgs = [3.0, 3.5, 4.0]
    out = p.action_sample_batch(hists, eval=True, rtg=rtgs)
    info = p.last["windows"]
    assert out.shape == (E, A) and [w["horizon"] for w in info] == [H, T - 2, H]
    sample = p.action_sample_batch(hists, eval=False, rtg=rtgs)  # (the step index has moved on: other noise)
    assert sample.shape == (E, A) and not torch.equal(sample, out)
    # the twin: one cem_guiding_batch per horizon group, shortest horizon first, on the same step indices
    for hz, ids in ((H, [0, 2]), (T - 2, [1])):
        trajs = []
        for i in ids:
            s, a, r, h, rtg = twin.assemble_window(hists[i], rtg=rtgs[i])
            assert h == hz
            trajs.append({"states": s.clone()[None], "actions": a.clone()[None], "rewards": r.clone()[None], "_rtg": rtg})
        sa, ev = twin.cem_guiding_batch(trajs, hz, iterations=2, top_k=16, weighting="mppi")
        assert len(twin.last["cem"]) == len(ids) and len(twin.last["cem"][0]) == 2
        for j, i in enumerate(ids):
            assert torch.equal(ev[j], out[i]), i
            assert torch.equal(twin.last["cem"][j][-1]["mean"], info[i]["mean"]) and torch.equal(twin.last["candidates"][j], info[i]["candidates"])
    p.handle.close()
    twin.handle.close()


def test_a_lockstep_rollout_by_refinement_keeps_the_warm_starts_of_the_environments_that_go_on():
    from fake_learner import ToyEnv

    dims = synth.Dims(11, 3, 16)
    cfg = G.types.SimpleNamespace(traj_length=16, action_samples=64, horizon=8, discount=0.99, temperature=0.01, lmbda=0.6,
                                  plan_guidance="rtg_guiding", device="cuda")
    p = HipPlanner(cfg, synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), None, max_batch=2, max_windows=2,
                   refine=REFINE, variates="library", seed=3)
    lengths = [3, 7]
    seen = []
    real = p.action_sample_batch

    def spy(*args, **kw):
        out = real(*args, **kw)
        seen.append((list(kw["keys"]), [w["warm"] for w in p.last["windows"]]))
        return out

    p.action_sample_batch = spy
    with pytest.raises(ValueError):
        evaluate_plan(p, [ToyEnv(11, 3, 0, length=2)], np.linspace(3.0, 1.0, 100), max_steps=2)  # (the pipelined loop: no ticket form)
    p.reset_warm_start()
    seen.clear()
    out = evaluate_plan(p, [ToyEnv(11, 3, i, length=lengths[i]) for i in range(2)], np.linspace(3.0, 1.0, 100), max_steps=7, lockstep=True)
    p.handle.close()
    assert out["plan_steps"] == sum(lengths) and out["lengths"] == [float(v) for v in lengths]
    assert seen[0] == ([0, 1], [False, False]) and seen[1] == ([0, 1], [True, True])
    # environment 0 has ended: environment 1 is alone in the round, under its own key, and still warm
    assert all(s == ([1], [True]) for s in seen[3:]) and len(seen) == 7
    for tr, n in zip(out["trajectories"], lengths):
        assert float(np.abs(tr["actions"][:n]).max()) <= 1.0 and np.abs(tr["actions"][:n]).sum() > 0


def test_a_planner_without_refine_plans_as_before():
    N = 64
    make = lambda **kw: _tiny(N, E=1, generator=torch.Generator(device="cuda").manual_seed(8), **kw)
    a, b = make(), make(refine=None)
    hist = _history(0)
    for eval_ in (True, False):
        assert torch.equal(a.action_sample(hist, plan=True, eval=eval_, rtg=3.0), b.action_sample(hist, plan=True, eval=eval_, rtg=3.0))
    assert "windows" not in a.last
    a.handle.close()
    b.handle.close()


# ---------------------------------------------------------------------------------------------- 9. the C example
def test_c_example_refines_three_windows_twice_with_a_shifted_warm_start(tmp_path, planners):
    """examples/refine_plans.c compiled with gcc -Wall -Werror against include/m3pc_hip.h, linked to the built library and run: its
    two rounds (library-drawn noise, the second warm-started with init_offset = 1) equal Handle.refine_plans bit for bit."""
    so = tmp_path / "librefine_plans.so"
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "refine_plans.c"), "-o", str(so), "-L", libdir,
                           "-l:" + os.path.basename(capi.LIB_PATH), "-Wl,-rpath," + libdir])
    N, k, iters, E = 130, 65, 2, 3
    p = planners("rtg", N)
    wins = [_windows(p, (0, 1, 2)), _windows(p, (3, 4, 5))]
    h = H
    fp, vp = C.POINTER(C.c_float), C.c_void_p

    class IO(C.Structure):
        _fields_ = [("dims", C.POINTER(capi.Dims)), ("weights", C.POINTER(capi.NamedTensor)), ("n_weights", C.c_int),
                    ("tok_mean", fp * 4), ("tok_std", fp * 4), ("tok_dim", C.c_int * 4), ("tok_normalize", C.c_int * 4),
                    ("n_windows", C.c_int), ("states", vp * 2), ("actions", vp * 2), ("rewards", vp * 2),
                    ("rtg", C.POINTER(C.c_double) * 2), ("n", C.c_int), ("horizon", C.c_int),
                    ("precision", C.c_int), ("iterations", C.c_int), ("top_k", C.c_int), ("weighting", C.c_int),
                    ("temperature", C.c_float), ("init_std", C.c_float), ("min_std", C.c_float),
                    ("lmbda", C.c_double), ("discount", C.c_double), ("seed", C.c_ulonglong), ("step", C.c_ulonglong),
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
    outs = [dict(mean=torch.empty((iters + 1, E, h, A), **dev), std=torch.empty((iters + 1, E, h, A), **dev),
                 candidates=torch.empty((E, N, h, A), **dev), sample_action=torch.empty((E, A), **dev), eval_action=torch.empty((E, A), **dev))
            for _ in range(2)]
    rt = [(C.c_double * E)(*wins[c][4]) for c in range(2)]
    for c in range(2):
        io.states[c], io.actions[c], io.rewards[c] = (t.data_ptr() for t in wins[c][:3])
        io.rtg[c] = C.cast(rt[c], C.POINTER(C.c_double))
        for name, t in outs[c].items():
            getattr(io, name)[c] = t.data_ptr()
    io.n_windows, io.n, io.horizon, io.precision, io.iterations, io.top_k, io.weighting = E, N, h, capi.PREC_FP32, iters, k, capi.REFINE_MPPI
    io.temperature, io.init_std, io.min_std, io.lmbda, io.discount, io.seed, io.step = 0.01, 0.1, 0.01, LMBDA, DISCOUNT, 2 ** 40 + 9, 2 ** 33
    torch.cuda.synchronize()
    lib = C.CDLL(str(so))
    lib.refine_plans.restype = C.c_int
    lib.refine_plans.argtypes = [C.POINTER(IO), C.c_int, vp]
    rc = lib.refine_plans(C.byref(io), torch.cuda.current_device(), vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, p.handle.lib.m3pc_last_error()
    torch.cuda.synchronize()
    kw = dict(iterations=iters, weighting=capi.REFINE_MPPI, temperature=0.01, init_std=0.1, min_std=0.01, seed=2 ** 40 + 9)
    one = _call(p.handle, "rtg", wins[0], h, N, k, steps=[2 ** 33 + w for w in range(E)], **kw)
    two = _call(p.handle, "rtg", wins[1], h, N, k, steps=[2 ** 33 + E + w for w in range(E)], init_mean=one["mean"][-1], init_offset=1, **kw)
    for c, want in enumerate((one, two)):
        for name, t in outs[c].items():
            assert torch.equal(t, want[name]), (c, name)
    assert torch.equal(two["mean"][0][:, :h - 1], one["mean"][-1][:, 1:])
    del keep, toks
