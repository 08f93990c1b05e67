"""m3pc_draw_variates on the device against its float64 restatement (tests/variates_ref.py): values, slices, determinism, guard
elements, optional outputs, and one certified plan step planned on the library's variates."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import variates_ref as V
from m3pc_amd import capi, synth
from m3pc_amd.planner import HipPlanner

pytestmark = pytest.mark.gpu
SEED, STEP = 1234, 7
SHAPES = [(1, 3), (5, 7), (625, 24), (1024, 96)]
NAN = float("nan")


@pytest.fixture(scope="module")
def handle():
    h = capi.Handle(11, 3, 8, max_candidates=64)
    yield h
    h.close()


@pytest.fixture(scope="module")
def whole(handle):
    """{shape: (device eps, device expo, float64 eps, float64 expo)} of (SEED, STEP): computed once, left unchanged."""
    out = {}
    for n, row in SHAPES:
        e, q = handle.draw_variates(SEED, STEP, n, row)
        out[(n, row)] = (e, q, V.eps(SEED, STEP, n, row), V.expo(SEED, STEP, n))
    torch.cuda.synchronize()
    return out


def _slices(n):
    return [(b, c) for b, c in ((0, n), (3, 2), (n - 1, 1)) if b >= 0 and b + c <= n]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_values_against_the_float64_restatement(whole, shape):
    """eps to 1e-5 absolute (|z| <= 6.7: logf, sqrtf and the sine / cosine to a few ulp give under 4e-6), expo to 1e-6 relative."""
    e, q, e64, q64 = whole[shape]
    assert e.shape == shape and q.shape == (shape[0],)
    de = float(np.abs(e.cpu().numpy().astype(np.float64) - e64).max())
    dq = float((np.abs(q.cpu().numpy().astype(np.float64) - q64) / q64).max())
    print(f"{shape}: max |eps - ref| {de:.3g}, max rel |expo - ref| {dq:.3g}, max |z| {float(e.abs().max()):.3f}, min q {float(q.min()):.3g}")
    assert float(e.abs().max()) <= 6.7
    assert de <= 1e-5
    assert dq <= 1e-6
    assert float(q.min()) > 0.0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("guard", [4, 1], ids=["aligned", "unaligned"])
def test_slices_equal_the_whole_array_and_guards_stay(handle, whole, shape, guard):
    """Rows [b, b + c) drawn alone are the same rows of the whole array bit for bit (a slice edge inside a Philox block at
    (5, 7)), into 16-byte aligned and unaligned outputs; the NaN-filled elements before and after both outputs stay NaN."""
    n, row = shape
    e, q = whole[shape][:2]
    for b, c in _slices(n):
        eb = torch.full((guard + c * row + 5,), NAN, device="cuda")
        qb = torch.full((guard + c + 5,), NAN, device="cuda")
        handle.draw_variates(SEED, STEP, n, row, n_begin=b, n_count=c, eps=eb[guard : guard + c * row], expo=qb[guard : guard + c])
        torch.cuda.synchronize()
        assert torch.equal(eb[guard : guard + c * row].view(c, row), e[b : b + c]), (shape, b, c)
        assert torch.equal(qb[guard : guard + c], q[b : b + c]), (shape, b, c)
        for buf, m in ((eb, c * row), (qb, c)):
            assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + m :]).all()), (shape, b, c)


def test_same_bits_twice_and_other_values_for_another_step_or_seed(handle, whole):
    n, row = 625, 24
    e, q = whole[(n, row)][:2]
    e2, q2 = handle.draw_variates(SEED, STEP, n, row)
    assert torch.equal(e, e2) and torch.equal(q, q2)
    for seed, step in ((SEED, STEP + 1), (SEED + 1, STEP), (SEED + (1 << 32), STEP), (SEED, STEP + (1 << 32))):
        e3, q3 = handle.draw_variates(seed, step, n, row)
        assert float((e3 == e).float().mean()) < 1e-3 and float((q3 == q).float().mean()) < 1e-2, (seed, step)
        assert float(np.abs(e3.cpu().numpy() - V.eps(seed, step, n, row)).max()) <= 1e-5


def test_null_outputs_are_accepted_and_bad_ranges_refused(handle, whole):
    n, row = 5, 7
    e, q = whole[(n, row)][:2]
    e2, none = handle.draw_variates(SEED, STEP, n, row, want_expo=False)
    none2, q2 = handle.draw_variates(SEED, STEP, n, row, want_eps=False)
    assert none is None and none2 is None and torch.equal(e2, e) and torch.equal(q2, q)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert handle.lib.m3pc_draw_variates(handle._h, 1, 1, 0, 4, 3, None, None, st) == 0
    for b, c, r in ((-1, 4, 3), (0, 0, 3), (0, 4, 0)):
        assert handle.lib.m3pc_draw_variates(handle._h, 1, 1, b, c, r, None, None, st) == -1, (b, c, r)


def test_certified_step_on_library_variates_follows_the_fp32_planner(handle):
    """One certified bf16 step at (hopper, rtg, N 625, T 8, H 4) on the variates the library draws for step 3: certified, and on
    the arg-max and the multinomial index of the fp32 planner on the same variates."""
    N, T, H, tau = 625, 8, 4, 0.01
    S, A = synth.ENV_DIMS["hopper"]
    dims = synth.Dims(S, A, T)
    cfg = types.SimpleNamespace(traj_length=T, action_samples=N, horizon=H, discount=0.99, temperature=tau, lmbda=0.6,
                                plan_guidance="rtg_guiding", device="cuda")
    mk = lambda prec: HipPlanner(cfg, synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), None, precision=prec)
    p, pb = mk("fp32"), mk("bf16")  # (the fp32 planner for the reference; the bf16 planner's handle has the re-score workspaces)
    hd = pb.handle
    eps, q = hd.draw_variates(99, 3, N, T * A)
    hist = synth.make_history(dims, 0)
    hist["path_length"] = 500
    s, a, r, h, rtg = p.assemble_window(hist, rtg=3.0)
    s, a, r = s.clone(), a.clone(), r.clone()
    p._draw_expo = lambda: q
    p._guide(capi.MODE_RTG, s, a, r, rtg, h, 0.6, eps=eps.view(N, 1, T, 1, A))
    want = (int(p.last["argmax"]), int(p.last["sample_idx"]))
    hd.policy_pass(capi.MODE_RTG, s, a, r, h, rtg, slot=0)
    low = hd.candidate_pass(capi.MODE_RTG, s, a, r, eps, h, 0.6, 0.99, N, precision=capi.PREC_BF16, slot=0)["expect_return"]
    delta = hd.calibrate_delta(capi.MODE_RTG, s, a, r, eps, low, h, 0.6, 0.99, N, factor=1.6, slot=0)
    res, rec = hd.plan_step_certified(capi.MODE_RTG, s, a, r, eps, q, h, rtg, 0.6, 0.99, N, tau, delta=delta, grow_delta=True,
                                      kmin=8, kmax=128, rfirst=2, rmax=32, precision=capi.PREC_BF16, slot=0)
    torch.cuda.synchronize()
    got = (int(res["sel"][2]), int(res["sel"][3]))
    print(f"library variates: fp32 planner {want}, certified bf16 step {got}, n_rescored {rec.n_rescored} n_race {rec.n_race}")
    assert rec.certified == 1
    assert got == want
    p.handle.close()
    pb.handle.close()


def test_planner_draws_its_steps_from_the_library():
    """HipPlanner(variates="library", seed=...): step t -- serial or pipelined -- plans on the rows of (seed, t); the default
    planner keeps torch's generator."""
    N, T, H = 64, 8, 4
    S, A = synth.ENV_DIMS["hopper"]
    dims = synth.Dims(S, A, T)
    cfg = types.SimpleNamespace(traj_length=T, action_samples=N, horizon=H, discount=0.99, temperature=0.01, lmbda=0.6,
                                plan_guidance="rtg_guiding", device="cuda")
    p = HipPlanner(cfg, synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), None, precision="fp32",
                   variates="library", seed=4242)
    hist = synth.make_history(dims, 0)
    hist["path_length"] = 500
    p.action_sample(hist, plan=True, eval=False, rtg=3.0)              # step 0, serial
    infos = [dict(p.last)]
    infos.append(dict(p.plan_async(hist, rtg=3.0).pair() and p.last))  # step 1, pipelined
    torch.cuda.synchronize()
    for t, last in enumerate(infos):
        eps, q = p.handle.draw_variates(4242, t, N, T * A)
        assert torch.equal(last["eps"].reshape(N, T * A), eps) and torch.equal(last["expo"], q), t
    with pytest.raises(ValueError):
        HipPlanner(cfg, synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), None, variates="numpy")
    p.handle.close()
