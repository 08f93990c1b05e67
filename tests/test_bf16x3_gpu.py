"""The split-bf16 precision tier (M3PC_PREC_BF16X3, csrc/gemm_x3.hip) on the GPU: the kernel against an fp64 product, the
generic forward and the golden plan steps against the fp32 bars, shard / pipeline exactness, the planner against the fp32
planner, and the bf16 -> bf16x3 fallback.  Every call with precision 2 failed with M3PC_EINVAL before the tier existed."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from m3pc_amd import capi, synth
from m3pc_amd.planner import HipPlanner
from hip_util import lab_library, make_handle, maxerr, window_dev
from oracle import mtm_oracle as O

pytestmark = pytest.mark.gpu
GD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
X3 = capi.PREC_BF16X3


def _assert_close(got, ref, tol, what):
    s = max(float(np.abs(ref.detach().cpu().double().numpy() if torch.is_tensor(ref) else np.asarray(ref)).max()), 1e-6)
    e = maxerr(got, ref)
    assert e <= tol * s, f"{what}: max err {e:.3e} > {tol:.1e} * scale {s:.3e}"


# ------------------------------------------------------------------------------------ kernel
def _gemm_x3(lib, A, W, bias, R, out, gelu, variant):
    fn = lib.m3pc_debug_gemm
    fn.restype = C.c_int
    vp, i = C.c_void_p, C.c_int
    fn.argtypes = [i, vp, vp, vp, vp, vp, i, i, i, i, i, i, vp]
    M, K = A.shape
    N = W.shape[0]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = fn(2, A.data_ptr(), W.data_ptr(), bias.data_ptr() if bias is not None else None, R.data_ptr() if R is not None else None,
            out.data_ptr(), M, N, K, gelu, 1, variant, st)
    assert rc == 0, lib.m3pc_last_error()
    torch.cuda.synchronize()


def _ref(A, W, bias, R, gelu):
    """fp64 C and the elementwise bound sum_k |a_k w_k| of the product."""
    A64, W64 = A.double(), W.double()
    c = A64 @ W64.T + (bias.double() if bias is not None else 0.0)
    if gelu:
        c = torch.nn.functional.gelu(c)
    if R is not None:
        c = c + R.double()
    return c, A64.abs() @ W64.abs().T


@pytest.mark.parametrize("K,N", [(512, 512), (512, 1536), (512, 2048), (2048, 512)])
@pytest.mark.parametrize("epi", ["bias", "gelu", "res", "none"])
def test_x3_gemm_against_fp64(K, N, epi):
    """|C - C_fp64| <= 3e-5 sum_k |a_k w_k| elementwise, on every row, at the step's shapes, ragged M, every epilogue; split-K (variant 0 on few
    rows) included.  And the result of a row does not depend on the row count (128x128 against 64x64 tiles, no split)."""
    lib = lab_library()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(K + N)
    M = 20000 + 77
    A = torch.randn(M, K, device=dev, generator=g)
    W = torch.randn(N, K, device=dev, generator=g) / K ** 0.5
    bias = torch.randn(N, device=dev, generator=g) if epi != "none" else None
    R = torch.randn(M, N, device=dev, generator=g) if epi == "res" else None
    gelu = int(epi == "gelu")
    out = torch.full((M, N), float("nan"), device=dev)
    _gemm_x3(lib, A, W, bias, R, out, gelu, 1)
    assert bool(torch.isfinite(out).all())
    for r0 in range(0, M, 4096):  # every row
        r1 = min(M, r0 + 4096)
        ref, bound = _ref(A[r0:r1], W, bias, R[r0:r1] if R is not None else None, gelu)
        err = (out[r0:r1].double() - ref).abs()
        assert bool((err <= 3e-5 * bound + 1e-30).all()), (r0, float((err / bound).max()))
    # a shard's row count: 300 + 5 rows take 64x64 tiles (the full problem took 128x128 where N allows): identical bits
    Ms = 305
    small = torch.full((Ms, N), float("nan"), device=dev)
    _gemm_x3(lib, A[:Ms].contiguous(), W, bias, R[:Ms].contiguous() if R is not None else None, small, gelu, 1)
    assert torch.equal(small, out[:Ms])
    # split-K (the few-row fp32 passes' shape: the debug entry's workspace, variant 0): same accuracy bar
    few = torch.full((Ms, N), float("nan"), device=dev)
    _gemm_x3(lib, A[:Ms].contiguous(), W, bias, R[:Ms].contiguous() if R is not None else None, few, gelu, 0)
    ref_s, bound_s = _ref(A[:Ms], W, bias, R[:Ms] if R is not None else None, gelu)
    assert bool(((few.double() - ref_s).abs() <= 3e-5 * bound_s + 1e-30).all())


# ------------------------------------------------------------------------------------ generic forward
MASKS = {"rcbc": O.rcbc_mask, "fd": O.fd_mask, "pi": O.pi_mask, "fid": O.fid_mask}


@pytest.mark.parametrize("d,nh,T,B", [(64, 2, 8, 3), (512, 4, 8, 2), (512, 4, 16, 1), (128, 2, 8, 3), (512, 8, 8, 2)])  # (head width 64: 128 / 2, 512 / 8)
@pytest.mark.parametrize("mask_name,idx_frac", [("rcbc", 0.5), ("fd", 0.5), ("pi", 0.5), ("fid", 0.25), ("rcbc", 0.0)])
def test_forward_x3_matches_oracle(d, nh, T, B, mask_name, idx_frac):
    """test_hip_parity.py::test_forward_matches_oracle's grid in x3: 2e-4 of scale (fp32 is held to 2e-5, bf16 to 5e-2)."""
    dims = synth.Dims(11, 3, T, n_embd=d, n_head=nh)
    h, sd, stats, _ = make_handle(dims, max_candidates=8, max_batch=4)
    idx = int(T * idx_frac)
    masks = MASKS[mask_name](T, idx)
    g = torch.Generator().manual_seed(3)
    toks = {k: torch.randn(B, T, 1, f, generator=g) for k, f in dims.feat.items()}
    ref = O.mtm_forward(sd, toks, masks, nh)
    out = h.forward([toks[k][:, :, 0].cuda() for k in synth.KEYS], [masks[k] for k in synth.KEYS], precision=X3)
    torch.cuda.synchronize()
    for k in ("states", "rewards", "returns"):
        _assert_close(out[k], ref[k][:, :, 0], 2e-4, f"{mask_name} {k}")
    _assert_close(out["actions"][0], ref["actions"][0][:, :, 0], 2e-4, "mu")
    _assert_close(out["actions"][1], ref["actions"][1][:, :, 0], 2e-4, "std")
    h.close()


# ------------------------------------------------------------------------------------ goldens, raw x3 pass
def _full(name, max_c):
    g = np.load(os.path.join(GD, f"g2_{name}.npz"))
    S, A, T, H, N = [int(v) for v in g["cfg"]]
    dims = synth.Dims(S, A, T)
    h, sd, stats, critic = make_handle(dims, max_candidates=max_c, max_batch=1)
    cfg = O.PlanCfg(T, H, N, 0.99, float(g["temperature"]), 0.6)
    win, hh = O.assemble_window(cfg, synth.make_history(dims, 0), 500, 3.0)
    return g, dims, h, cfg, win


def _check_golden(g, h, er, a0, cfg):
    scale = max(float(er.abs().max()), 1.0)
    got = (er - er.max()).cpu().numpy()
    err = np.abs(got - g["expect_return_shifted"]).max()
    assert err <= 1e-4 * scale, f"expect_return err {err:.3e} vs scale {scale:.3e}"
    p, ev, am = h.select(er, a0, cfg.temperature)
    assert int(am.item()) == int(g["argmax"])
    ref = g["expect_return_shifted"]
    assert set(torch.topk(er, 8).indices.tolist()) == set(np.argsort(-ref, kind="stable")[:8].tolist())
    assert maxerr(ev, g["eval_action"]) <= 1e-4


@pytest.mark.parametrize("name", ["c1", "c2s", "c2"])
def test_g2_rtg_x3_vs_reference_golden(name):
    g, dims, h, cfg, win = _full(name, 1024)
    N, H = cfg.action_samples, cfg.horizon
    eps = synth.make_eps(N, dims, 1)[:, 0, :, 0, :].cuda()
    s, a, r = window_dev(win)
    res = h.plan_step(capi.MODE_RTG, s, a, r, eps, H, 3.0, 0.6, 0.99, N, precision=X3)
    _check_golden(g, h, res["expect_return"], res["sample_actions"][:, 0], cfg)
    h.close()


def test_g2_critic_x3_vs_reference_golden():
    g, dims, h, cfg, win = _full("c3", 1024)
    N, H = cfg.action_samples, cfg.horizon
    eps = synth.make_eps(N, dims, 1)[:, 0, :, 0, :].cuda()
    s, a, r = window_dev(win)
    ers, a0s = [], []
    for b in range(0, N, 1024):
        res = h.plan_step(capi.MODE_CRITIC, s, a, r, eps, H, 3.0, 0.6, 0.99, N, n_begin=b, n_count=1024, precision=X3)
        ers.append(res["expect_return"].clone())
        a0s.append(res["sample_actions"][:, 0].contiguous())
    _check_golden(g, h, torch.cat(ers), torch.cat(a0s), cfg)
    h.close()


def test_x3_sharding_is_exact_and_profiled():
    """Scores over [0, N) and over two shards are identical bits; the x3 GEMMs are reported under their own precision."""
    dims = synth.Dims(11, 3, 32)
    h, sd, stats, critic = make_handle(dims, max_candidates=1024, max_batch=1)
    cfg = O.PlanCfg(32, 16, 1024)
    win, hh = O.assemble_window(cfg, synth.make_history(dims, 0), 500, 3.0)
    eps = synth.make_eps(1024, dims, 1)[:, 0, :, 0, :].cuda()
    s, a, r = window_dev(win)
    h.profile_enable(True)
    full = h.plan_step(capi.MODE_RTG, s, a, r, eps, 16, 3.0, 0.6, 0.99, 1024, precision=X3)["expect_return"].clone()
    n_x3, ms_x3, fl_x3 = h.profile_read(X3, reset=False)
    assert n_x3 > 0 and fl_x3 > 0
    h.profile_read(-1)
    h.profile_enable(False)
    parts = [h.plan_step(capi.MODE_RTG, s, a, r, eps, 16, 3.0, 0.6, 0.99, 1024, n_begin=b, n_count=512,
                         precision=X3)["expect_return"].clone() for b in (0, 512)]
    assert torch.equal(full, torch.cat(parts))
    # and the x3 pass did not leave the fp32 pass's cached tables in x3 arithmetic: fp32 after x3 equals fp32 on a fresh handle
    f_after = h.plan_step(capi.MODE_RTG, s, a, r, eps, 16, 3.0, 0.6, 0.99, 1024)["expect_return"].clone()
    h2, *_ = make_handle(dims, max_candidates=1024, max_batch=1)
    f_fresh = h2.plan_step(capi.MODE_RTG, s, a, r, eps, 16, 3.0, 0.6, 0.99, 1024)["expect_return"].clone()
    assert torch.equal(f_after, f_fresh)
    h.close()
    h2.close()


# ------------------------------------------------------------------------------------ planner
def _cfg(T, N, H, tau=0.01, guidance="rtg_guiding"):
    return types.SimpleNamespace(traj_length=T, action_samples=N, horizon=H, discount=0.99, temperature=tau, lmbda=0.6,
                                 plan_guidance=guidance, device="cuda")


def _window(dims, i):
    h = synth.make_history(dims, i % 11)
    h["path_length"] = [500, 37, 321, 998, 640, 77, 250, 123, 864][i % 9] if i < 9 else 33 + (i * 37) % 960
    return h


@pytest.mark.parametrize("env,guidance,tau,N", [("hopper", "rtg_guiding", 0.01, 1024), ("walker2d", "critic_lambda_guiding", 1.0, 4096)],
                         ids=["C2", "C3"])
@pytest.mark.parametrize("weights", ["recipe", "trained_x2"])
def test_x3_planner_follows_the_fp32_planner(env, guidance, tau, N, weights):
    """16 steps: the bf16x3 planner's arg-max and drawn index are the fp32 planner's, eval_action within 1e-4, and its calibrated
    delta is at most 1/100 of the bf16 planner's on the same weights."""
    T, H = 32, 16
    S, A = synth.ENV_DIMS[env]
    dims = synth.Dims(S, A, T)
    sd, st = synth.make_state_dict(dims, 1), synth.make_tokenizer_stats(dims, 1)
    if weights == "trained_x2":
        sd, st = synth.trained_like(sd, st, seed=1, linear_scale=2.0, returns_std_scale=0.1)
    mode = capi.MODE_RTG if guidance == "rtg_guiding" else capi.MODE_CRITIC
    qsd, om, os_ = synth.make_critic(dims, 1) if mode == capi.MODE_CRITIC else (None, None, None)
    mk = lambda prec: HipPlanner(_cfg(T, N, H, tau, guidance), sd, st, qsd, om, os_, precision=prec, auto_fp32=False,
                                 generator=torch.Generator(device="cuda").manual_seed(1))
    px, pf, pb = mk("bf16x3"), mk("fp32"), mk("bf16")
    for t in range(16):
        hist = _window(dims, t)
        eps = synth.make_eps(N, dims, 500 + t).cuda()
        s, a, r, h, g = px.assemble_window(hist, rtg=3.0 + 0.25 * (t % 5))
        px._guide(mode, s, a, r, g, h, 0.6, eps=eps)
        pf._guide(mode, s, a, r, g, h, 0.6, eps=eps)
        pb._guide(mode, s, a, r, g, h, 0.6, eps=eps)
        lx, lf = px.last, pf.last
        assert lx["certified"]
        assert int(lx["argmax"].item()) == int(lf["argmax"].item()), t
        assert int(lx["sample_idx"].item()) == int(lf["sample_idx"].item()), t
        assert maxerr(lx["eval_action"], lf["eval_action"]) <= 1e-4, t
    assert px._delta is not None and pb._delta is not None
    assert px._delta <= pb._delta / 100, (px._delta, pb._delta)
    for p in (px, pf, pb):
        p.handle.close()


def test_x3_pipelined_equals_serial():
    """plan_async at depth 3 in x3 returns the serial run's actions bit for bit."""
    N, T, H = 1024, 32, 16
    dims = synth.Dims(11, 3, T)
    sd, st = synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0)
    mk = lambda: HipPlanner(_cfg(T, N, H), sd, st, None, precision="bf16x3", generator=torch.Generator(device="cuda").manual_seed(5),
                            pipeline_depth=3)
    n = 10
    ps = mk()
    serial = [ps.action_sample(_window(dims, t), plan=True, eval=(t % 2 == 0), rtg=3.0).clone() for t in range(n)]
    ps.handle.close()
    pp = mk()
    got, flight = [None] * n, []
    for t in range(n):
        flight.append((t, pp.plan_async(_window(dims, t), eval=(t % 2 == 0), rtg=3.0)))
        while len(flight) > 3:
            i, tk = flight.pop(0)
            got[i] = tk.result().clone()
    for i, tk in flight:
        got[i] = tk.result().clone()
    for t in range(n):
        assert torch.equal(got[t], serial[t]), t
    pp.handle.close()


def test_goal_actions_x3_close_to_fp32_on_g3():
    g = np.load(os.path.join(GD, "g3_zeroshot.npz"))
    T, S, A = 8, 11, 3
    dims = synth.Dims(S, A, T)
    cfg = types.SimpleNamespace(traj_length=T, action_samples=1, horizon=4, discount=0.99, temperature=1.0, lmbda=0.6,
                                plan_guidance="rtg_guiding", index_jump=4)
    p = HipPlanner(cfg, synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), None, goal_batch=64)
    for pl in (0, 2, 37, 997):
        hist = synth.make_history(dims, 0)
        hist["observations"] = g[f"obs_pl{pl}"]
        hist["path_length"] = pl
        s, a, r, h, _ = p.assemble_goal_window(hist, rtg=2.5)
        s, a = s.clone().expand(16, -1, -1).contiguous(), a.clone().expand(16, -1, -1).contiguous()
        ef = p.goal_actions(s, a, h, eval=True, precision="fp32")
        ex = p.goal_actions(s, a, h, eval=True, precision="bf16x3")
        torch.cuda.synchronize()
        assert maxerr(ex, ef) <= 1e-4, pl
        assert np.abs(ex[0].cpu().numpy() - g[f"action_piid_sample_pl{pl}_eval_action"][0]).max() <= 1e-4
    p.handle.close()


def test_fallback_to_bf16x3_on_weights_that_make_the_certificate_expensive():
    """test_certificate_gpu.py's fallback weights (every Linear x 4): with fallback="bf16x3" the saturated bf16 planner switches
    to x3 (not fp32), at the same step as the fp32 fallback, and its actions stay the fp32 planner's.  A weight load returns it
    to bf16."""
    N, T, H = 1024, 32, 16
    dims = synth.Dims(11, 3, T)
    sd0, st0 = synth.make_state_dict(dims, 2), synth.make_tokenizer_stats(dims, 2)
    sd4, st4 = synth.trained_like(sd0, st0, seed=2, linear_scale=4.0, returns_std_scale=0.1)
    pb = HipPlanner(_cfg(T, N, H), sd4, st4, None, precision="bf16", fallback="bf16x3",
                    generator=torch.Generator(device="cuda").manual_seed(1))
    pf = HipPlanner(_cfg(T, N, H), sd4, st4, None, precision="fp32", generator=torch.Generator(device="cuda").manual_seed(1))
    switched_at = None
    with pytest.warns(UserWarning, match="planning in bf16x3"):
        for t in range(4 + capi.SLOTS + 6):
            hist = _window(dims, t)
            eps = synth.make_eps(N, dims, 300 + t).cuda()
            pb._eps = pf._eps = lambda shape: eps
            ab = pb.action_sample(hist, plan=True, eval=True, rtg=3.0)
            af = pf.action_sample(hist, plan=True, eval=True, rtg=3.0)
            assert int(pb.last["argmax"].item()) == int(pf.last["argmax"].item())
            assert int(pb.last["sample_idx"].item()) == int(pf.last["sample_idx"].item())
            assert not pb.fp32_fallback
            if pb.precision == capi.PREC_BF16X3:
                switched_at = t if switched_at is None else switched_at
                assert pb.fallback_precision == "bf16x3" and pb.last["certified"]
                # (eval_action: 1.2e-4 measured.  With every Linear x 4 two fp32 evaluation orders of one score already differ by up
                # to 5e-4 of its scale -- test_certificate_gpu.py's trained-like sweep holds re-scores to 1e-3 -- and the merged vector's
                # un-re-scored entries are x3 scores)
                assert maxerr(ab, af) <= 5e-4
    assert switched_at == 3 + capi.SLOTS
    pb.load_state_dict(sd0)
    assert pb.precision == capi.PREC_BF16 and pb.fallback_precision is None and not pb.fp32_fallback
    pb.handle.close()
    pf.handle.close()

