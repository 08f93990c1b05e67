"""GPU parity: libm3pc_hip.so (through the C ABI / ctypes) against the oracle and the committed golden
vectors.  Everything here needs a real MI355X:  python -m pytest tests -m gpu

Tolerances (fp32 path): the oracle runs MKL fp32 on the CPU, the HIP path accumulates every product as an
exact fp32 fma chain on the matrix cores (v_mfma_f32_32x32x2_f32); the two differ by summation order only.
Measured agreement is ~1e-6 relative per GEMM; the tests allow 2e-5 of the tensor's scale, the same bar the
oracle itself is held to against the reference (tests/test_oracle_golden.py).
bf16 path: operands rounded to bf16 (8 significant bits) -> tolerances are stated per test.
"""
import os

import numpy as np
import pytest
import torch

from m3pc_amd import capi, synth
from oracle import mtm_oracle as O

from hip_util import make_handle, maxerr, window_dev

pytestmark = pytest.mark.gpu
GD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _scale(x):
    return float(np.abs(np.asarray(x.detach().cpu() if torch.is_tensor(x) else x)).max())


def _assert_close(got, ref, tol, what):
    s = max(_scale(ref), 1e-6)
    e = maxerr(got, ref)
    assert e <= tol * s, f"{what}: max err {e:.3e} > {tol:.1e} * scale {s:.3e}"


# ------------------------------------------------------------------------------------ generic forward
MASKS = {"rcbc": O.rcbc_mask, "fd": O.fd_mask, "pi": O.pi_mask, "fid": O.fid_mask}


@pytest.mark.parametrize("d,nh,T,B", [(64, 2, 8, 3), (512, 4, 8, 2), (512, 4, 16, 1), (128, 2, 8, 3), (512, 8, 8, 2)])  # (head width 64: 128 / 2, 512 / 8)
@pytest.mark.parametrize("mask_name,idx_frac", [("rcbc", 0.5), ("fd", 0.5), ("pi", 0.5), ("fid", 0.25), ("rcbc", 0.0)])
def test_forward_matches_oracle(d, nh, T, B, mask_name, idx_frac):
    dims = synth.Dims(11, 3, T, n_embd=d, n_head=nh)
    h, sd, stats, _ = make_handle(dims, max_candidates=8, max_batch=4)
    idx = int(T * idx_frac)
    masks = MASKS[mask_name](T, idx)
    g = torch.Generator().manual_seed(3)
    toks = {k: torch.randn(B, T, 1, f, generator=g) for k, f in dims.feat.items()}
    ref = O.mtm_forward(sd, toks, masks, nh)
    out = h.forward([toks[k][:, :, 0].cuda() for k in synth.KEYS], [masks[k] for k in synth.KEYS])
    torch.cuda.synchronize()
    for k in ("states", "rewards", "returns"):
        _assert_close(out[k], ref[k][:, :, 0], 2e-5, f"{mask_name} {k}")
    _assert_close(out["actions"][0], ref["actions"][0][:, :, 0], 2e-5, "mu")
    _assert_close(out["actions"][1], ref["actions"][1][:, :, 0], 2e-5, "std")
    h.close()


def test_forward_bf16_close_to_oracle():
    """bf16 operands: 8-bit mantissas through 3 transformer layers; head outputs (O(1) values) agree with
    the fp32 oracle to 5e-2 of scale."""
    _forward_bf16_close(512, 4)


@pytest.mark.parametrize("d,nh", [(128, 2), (512, 8)])
def test_forward_bf16_head_width_64_close_to_oracle(d, nh):
    """The same at head width 64: n_embd 128 / n_head 2 (the default omtmConfig, m3pc_amd/mtm.py) and 512 / 8."""
    _forward_bf16_close(d, nh)


def _forward_bf16_close(d, nh):
    dims = synth.Dims(11, 3, 8, n_embd=d, n_head=nh)
    h, sd, stats, _ = make_handle(dims, max_candidates=8, max_batch=4)
    masks = O.fd_mask(8, 4)
    g = torch.Generator().manual_seed(3)
    toks = {k: torch.randn(2, 8, 1, f, generator=g) for k, f in dims.feat.items()}
    ref = O.mtm_forward(sd, toks, masks, nh)
    out = h.forward([toks[k][:, :, 0].cuda() for k in synth.KEYS], [masks[k] for k in synth.KEYS],
                    precision=capi.PREC_BF16)
    for k in ("states", "rewards", "returns"):
        _assert_close(out[k], ref[k][:, :, 0], 5e-2, f"bf16 {k}")
    h.close()


def test_forward_bf16_many_rows_takes_the_matrix_core_heads():
    """Round 6: with >= 2048 rows per key the heads' last Linear runs as head_out_mfma_kernel on bf16 hidden rows (17-wide
    states head included).  Same forward, 2 rows (the row-per-wave kernel on fp32 hidden rows) against 96 sequences (the MFMA
    kernel): the shared sequences agree to bf16 noise, and both stay within the bf16 tolerance of the fp32 oracle."""
    T, B = 32, 96  # 96 x 32 = 3072 rows per key
    dims = synth.Dims(17, 6, T)
    h, sd, stats, _ = make_handle(dims, max_candidates=8, max_batch=B)
    masks = O.fd_mask(T, 16)
    g = torch.Generator().manual_seed(5)
    toks = {k: torch.randn(B, T, 1, f, generator=g) for k, f in dims.feat.items()}
    ins = [toks[k][:, :, 0].cuda() for k in synth.KEYS]
    big = h.forward(ins, [masks[k] for k in synth.KEYS], precision=capi.PREC_BF16)
    small = h.forward([x[:2].contiguous() for x in ins], [masks[k] for k in synth.KEYS], precision=capi.PREC_BF16)
    ref = O.mtm_forward(sd, {k: v[:8] for k, v in toks.items()}, masks, 4)
    for k in ("states", "rewards", "returns"):
        _assert_close(big[k][:8], ref[k][:, :, 0], 5e-2, f"bf16 many rows {k}")
        _assert_close(big[k][:2], small[k], 5e-2, f"bf16 many rows vs few rows {k}")
        assert torch.isfinite(big[k]).all()
    h.close()


# ------------------------------------------------------------------------------------ tokenizer
def test_tokenizer_roundtrip_and_f64():
    dims = synth.Dims(11, 3, 8, n_embd=64, n_head=2)
    h, sd, stats, _ = make_handle(dims, 8, 2)
    x = torch.randn(5, 8, 11)
    ref = O.tok_encode(x, stats["states"])[:, :, 0]
    got = h.tokenize(capi.STATES, x.cuda())
    assert torch.equal(got.cpu(), ref), "fp32 tokenize must be bit-exact (same IEEE sub/div)"
    back = h.detokenize(capi.STATES, got)
    assert torch.equal(back.cpu(), O.tok_decode(ref.unsqueeze(2), stats["states"]))
    r64 = torch.from_numpy(3.0 * np.ones((1, 8, 1)))
    got64 = h.tokenize(capi.RETURNS, r64.cuda())
    assert torch.equal(got64.cpu(), O.tok_encode(r64, stats["returns"])[:, :, 0])
    a = torch.rand(2, 8, 3)
    assert torch.equal(h.tokenize(capi.ACTIONS, a.cuda()).cpu(), a)  # actions are not normalised
    h.close()


# ------------------------------------------------------------------------------------ G1 tiny plan step
@pytest.fixture(scope="module")
def tiny():
    dims = synth.Dims(11, 3, 8, n_embd=64, n_head=2)
    h, sd, stats, critic = make_handle(dims, max_candidates=16, max_batch=1)
    yield dict(dims=dims, h=h, sd=sd, stats=stats, critic=critic, g=np.load(os.path.join(GD, "g1_tiny.npz")))
    h.close()


MODES = {"rtg": capi.MODE_RTG, "critic": capi.MODE_CRITIC, "noise": capi.MODE_NOISE}


@pytest.mark.parametrize("mode,temp", [("rtg", 0.01), ("critic", 1.0), ("noise", 1.0)])
@pytest.mark.parametrize("pl", [0, 3, 100, 998])
def test_g1_plan_step_vs_reference_golden(tiny, mode, temp, pl):
    g, dims, h = tiny["g"], tiny["dims"], tiny["h"]
    N, H, T = 16, 4, 8
    cfg = O.PlanCfg(T, H, N, 0.99, temp, 0.6, n_head=2)
    win, hh = O.assemble_window(cfg, synth.make_history(dims, 0), pl, 3.0)
    pre = f"{mode}_pl{pl}_"
    if mode == "noise":
        eps = torch.randn((N, hh, 3), generator=torch.Generator().manual_seed(123))
    else:
        eps = torch.from_numpy(g["eps"])[:, 0, :, 0, :]  # (N,T,A)
    s, a, r = window_dev(win)
    res = h.plan_step(MODES[mode], s, a, r, eps.cuda(), hh, 3.0, 0.6, 0.99, N, want_debug=True)
    torch.cuda.synchronize()
    _assert_close(res["loc"], g[pre + "loc"].reshape(T, 3), 2e-5, "loc")
    _assert_close(res["std"], g[pre + "std"].reshape(T, 3), 2e-5, "std")
    _assert_close(res["sample_actions"], g[pre + "sample_actions"], 2e-5, "sample_actions")
    _assert_close(res["pred_rewards"], g[pre + "dec_rewards"][:, T - hh:, 0], 2e-5, "rewards")
    if mode == "rtg":
        _assert_close(res["pred_boot"], 1000 * g[pre + "dec_returns"][:, T - hh:, 0], 2e-5, "boot")
    er = res["expect_return"]
    ref_shift = g[pre + "expect_return"]
    scale = float(er.abs().max())
    got_shift = (er - er.max()).cpu().numpy()
    assert np.abs(got_shift - ref_shift).max() <= 2e-5 * max(scale, 1.0), np.abs(got_shift - ref_shift).max()
    p, ev, am = h.select(er, res["sample_actions"][:, 0], temp)
    assert int(am.item()) == int(np.argmax(ref_shift))
    _assert_close(p, g[pre + "p"], 1e-4, "p")
    _assert_close(ev, g[pre + "eval_action"], 2e-5, "eval_action")


# ------------------------------------------------------------------------------------ G2 full size, fp32
def _full(name, max_c):
    g = np.load(os.path.join(GD, f"g2_{name}.npz"))
    S, A, T, H, N = [int(v) for v in g["cfg"]]
    dims = synth.Dims(S, A, T)
    h, sd, stats, critic = make_handle(dims, max_candidates=max_c, max_batch=1)
    cfg = O.PlanCfg(T, H, N, 0.99, float(g["temperature"]), 0.6)
    win, hh = O.assemble_window(cfg, synth.make_history(dims, 0), 500, 3.0)
    return g, dims, h, cfg, win


@pytest.mark.parametrize("name", ["c1", "c2s", "c2"])
def test_g2_rtg_fp32_vs_reference_golden(name):
    g, dims, h, cfg, win = _full(name, 1024)
    N, H, T = cfg.action_samples, cfg.horizon, cfg.traj_length
    eps = synth.make_eps(N, dims, 1)[:, 0, :, 0, :].cuda()
    s, a, r = window_dev(win)
    res = h.plan_step(capi.MODE_RTG, s, a, r, eps, H, 3.0, 0.6, 0.99, N, want_debug=True)
    _assert_close(res["loc"], g["loc"].reshape(T, -1), 2e-5, "loc")
    _assert_close(res["std"], g["std"].reshape(T, -1), 2e-5, "std")
    rows = g["rows"]
    _assert_close(res["sample_actions"][rows], g["sample_actions_rows"], 2e-5, "sample_actions")
    _assert_close(res["pred_rewards"][rows], g["dec_rewards_rows"][:, :, 0], 5e-5, "rewards")
    _assert_close(res["pred_boot"][rows], 1000 * g["dec_returns_rows"][:, :, 0], 5e-5, "returns")
    er = res["expect_return"]
    scale = float(er.abs().max())
    got = (er - er.max()).cpu().numpy()
    err = np.abs(got - g["expect_return_shifted"]).max()
    assert err <= 5e-5 * scale, f"expect_return err {err:.3e} vs scale {scale:.3e}"
    p, ev, am = h.select(er, res["sample_actions"][:, 0], cfg.temperature)
    assert int(am.item()) == int(g["argmax"]), "argmax must be bit-exact"
    assert set(torch.topk(er, 8).indices.tolist()) == set(g["top32"][:8].tolist())
    _assert_close(p, g["p"], 1e-3, "p")
    _assert_close(ev, g["eval_action"], 1e-4, "eval_action")
    # the reference's multinomial draw, replayed on the gathered p with the stored seed
    idx = torch.multinomial(p.cpu(), 1, generator=torch.Generator().manual_seed(77))
    assert int(idx) == int(g["sample_idx"].reshape(-1)[0])
    h.close()


def test_g2_critic_fp32_vs_reference_golden():
    """C3 walker2d critic_lambda_guiding N=4096: all candidates, in 4 shards of 1024 (the sharded API)."""
    g, dims, h, cfg, win = _full("c3", 1024)
    N, H, T = cfg.action_samples, cfg.horizon, cfg.traj_length
    eps = synth.make_eps(N, dims, 1)[:, 0, :, 0, :].cuda()
    s, a, r = window_dev(win)
    ers, a0s = [], []
    for b in range(0, N, 1024):
        res = h.plan_step(capi.MODE_CRITIC, s, a, r, eps, H, 3.0, 0.6, 0.99, N, n_begin=b, n_count=1024)
        ers.append(res["expect_return"])
        a0s.append(res["sample_actions"][:, 0].contiguous())
    er, a0 = torch.cat(ers), torch.cat(a0s)
    got = (er - er.max()).cpu().numpy()
    err = np.abs(got - g["expect_return_shifted"]).max()
    assert err <= 2e-5, f"expect_return err {err:.3e}"
    p, ev, am = h.select(er, a0, cfg.temperature)
    assert int(am.item()) == int(g["argmax"])
    _assert_close(ev, g["eval_action"], 1e-4, "eval_action")
    h.close()


def test_g2_c4_blocks_fp32_vs_reference_golden():
    """C4 halfcheetah N=16384 H=32 T=64: the three candidate blocks the reference was run on."""
    g, dims, h, cfg, win = _full("c4", 512)
    N, H, T = cfg.action_samples, cfg.horizon, cfg.traj_length
    eps = synth.make_eps(N, dims, 1)[:, 0, :, 0, :].cuda()
    s, a, r = window_dev(win)
    for bi, (b0, b1) in enumerate(g["blocks"]):
        res = h.plan_step(capi.MODE_RTG, s, a, r, eps, H, 3.0, 0.6, 0.99, N, n_begin=int(b0), n_count=int(b1 - b0),
                          want_debug=True)
        _assert_close(res["pred_rewards"], g["dec_rewards_blocks"][bi], 5e-5, "rewards")
        _assert_close(res["pred_boot"], 1000 * g["dec_returns_blocks"][bi], 5e-5, "returns")
        er = res["expect_return"]
        got = (er - er.max()).cpu().numpy()
        err = np.abs(got - g["expect_return_shifted_blocks"][bi]).max()
        assert err <= 5e-5 * float(er.abs().max()), err
    h.close()


# ------------------------------------------------------------------------------------ bf16 candidate pass
def test_c2_bf16_screen_quality():
    """BASELINE config 2 in bf16: scores are 1000 x predicted returns; bf16 operand rounding perturbs them.
    Stated bar: |E_bf16 - E_ref| <= 1% of the score range-scale, the reference argmax stays inside the bf16
    top-32, eval_action (softmax-weighted mean at temperature 0.01) within 5e-3."""
    g, dims, h, cfg, win = _full("c2", 1024)
    N, H, T = cfg.action_samples, cfg.horizon, cfg.traj_length
    eps = synth.make_eps(N, dims, 1)[:, 0, :, 0, :].cuda()
    s, a, r = window_dev(win)
    res = h.plan_step(capi.MODE_RTG, s, a, r, eps, H, 3.0, 0.6, 0.99, N, precision=capi.PREC_BF16)
    er = res["expect_return"]
    got = (er - er.max()).cpu().numpy()
    ref = g["expect_return_shifted"]
    err = np.abs((got - got.mean()) - (ref - ref.mean())).max()
    scale = float(er.abs().max())
    assert err <= 1e-2 * scale, f"bf16 expect_return err {err:.3f} vs scale {scale:.1f}"
    top = torch.topk(er, 32).indices.tolist()
    assert int(g["argmax"]) in top
    p, ev, am = h.select(er, res["sample_actions"][:, 0], cfg.temperature)
    _assert_close(ev, g["eval_action"], 5e-3, "eval_action")
    h.close()


def test_c4_block_bf16_screen_quality():
    """T=64 / H=32 shapes in bf16 (halfcheetah dims): exercises the two-chunk attention kernel with two query / key
    segments (64 shared + 33 own tokens in the first layer) and the pre-reduced masked-key block at Lk = 97.
    Bar: 3 % of the score scale (the T=32 study measured up to 2.9 %), reference block arg-max inside the bf16 top-32."""
    g, dims, h, cfg, win = _full("c4", 512)
    N, H, T = cfg.action_samples, cfg.horizon, cfg.traj_length
    eps = synth.make_eps(N, dims, 1)[:, 0, :, 0, :].cuda()
    s, a, r = window_dev(win)
    b0, b1 = (int(x) for x in g["blocks"][0])
    res = h.plan_step(capi.MODE_RTG, s, a, r, eps, H, 3.0, 0.6, 0.99, N, n_begin=b0, n_count=b1 - b0, precision=capi.PREC_BF16)
    er = res["expect_return"]
    got = (er - er.max()).cpu().numpy()
    ref = g["expect_return_shifted_blocks"][0]
    err = np.abs((got - got.mean()) - (ref - ref.mean())).max()
    scale = float(er.abs().max())
    assert err <= 3e-2 * scale, f"bf16 expect_return err {err:.3f} vs scale {scale:.1f}"
    assert int(np.argmax(ref)) in torch.topk(er, 32).indices.tolist()
    h.close()


def test_c3_critic_bf16_screen_quality():
    """critic_lambda_guiding in bf16 (walker2d dims, N=4096): per-candidate decoder queries (no shared query table),
    first-layer history sharing on, twin-Q on bf16-decoded states.  Same bar as the rtg screen."""
    g, dims, h, cfg, win = _full("c3", 4096)
    N, H, T = cfg.action_samples, cfg.horizon, cfg.traj_length
    eps = synth.make_eps(N, dims, 1)[:, 0, :, 0, :].cuda()
    s, a, r = window_dev(win)
    res = h.plan_step(capi.MODE_CRITIC, s, a, r, eps, H, 3.0, 0.6, 0.99, N, precision=capi.PREC_BF16)
    er = res["expect_return"]
    got = (er - er.max()).cpu().numpy()
    ref = g["expect_return_shifted"]
    err = np.abs((got - got.mean()) - (ref - ref.mean())).max()
    scale = max(float(er.abs().max()), float(np.abs(ref).max()), 1.0)
    assert err <= 3e-2 * scale, f"bf16 critic expect_return err {err:.4f} vs scale {scale:.2f}"
    assert int(g["argmax"]) in torch.topk(er, 32).indices.tolist()
    h.close()


# ------------------------------------------------------------------------------------ edge shapes vs the oracle
# (the oracle runs on the CPU: one case at the shipped N=625, the critic one at N=250 -- the same kernels, less oracle time)
@pytest.mark.parametrize("T,H,N,mode", [(8, 4, 625, "rtg"), (8, 4, 250, "critic"), (8, 1, 37, "rtg"), (8, 8, 130, "critic"),
                                        (16, 5, 1, "rtg"), (8, 4, 64, "noise")])
def test_odd_shapes_match_oracle(T, H, N, mode):
    """The reference's shipped planning config (N=625, H=4, T=8, finetune_omtm/config.yaml:5,77-78) and ragged
    cases: horizon 1, horizon == T (no history), a single candidate, candidate counts that are not tile
    multiples.  fp32 path against the oracle on identical eps."""
    dims = synth.Dims(11, 3, T)
    h, sd, stats, critic = make_handle(dims, max_candidates=N, max_batch=1)
    cfg = O.PlanCfg(T, H, N, 0.99, 1.0 if mode != "rtg" else 0.01, 0.6)
    win, hh = O.assemble_window(cfg, synth.make_history(dims, 3), 300, 2.0)
    assert hh == H
    if mode == "noise":
        eps = torch.randn((N, H, 3), generator=torch.Generator().manual_seed(5))
        dev_eps = eps.cuda()
    else:
        eps = synth.make_eps(N, dims, 9)
        dev_eps = eps[:, 0, :, 0, :].cuda()
    ref = O.guiding(sd, stats, cfg, win, H, 0.6, eps, mode, critic=critic)
    s, a, r = window_dev(win)
    res = h.plan_step(MODES[mode], s, a, r, dev_eps, H, 2.0, 0.6, 0.99, N)
    _assert_close(res["sample_actions"], ref["sample_actions"], 2e-5, "sample_actions")
    scale = max(float(ref["expect_return"].abs().max()), 1.0)
    assert float((res["expect_return"].cpu() - ref["expect_return"]).abs().max()) <= 5e-5 * scale
    p, ev, am = h.select(res["expect_return"], res["sample_actions"][:, 0], cfg.temperature)
    assert int(am.item()) == ref["argmax"]
    _assert_close(ev, ref["eval_action"], 1e-4, "eval_action")
    h.close()


@pytest.mark.parametrize("mode", ["rtg", "critic"])
def test_head_width_64_plan_step_matches_oracle(mode):
    """n_embd 128 / n_head 2 (head width 64: the default omtmConfig, m3pc_amd/mtm.py): one fp32 plan step per mode against the
    oracle, at test_odd_shapes_match_oracle's bars.  (The GEMM chains, not the fused layer tail, which needs n_embd 512.)"""
    T, H, N = 8, 4, 130
    dims = synth.Dims(11, 3, T, n_embd=128, n_head=2)
    h, sd, stats, critic = make_handle(dims, max_candidates=N, max_batch=1)
    cfg = O.PlanCfg(T, H, N, 0.99, 1.0 if mode != "rtg" else 0.01, 0.6, n_head=2)
    win, hh = O.assemble_window(cfg, synth.make_history(dims, 3), 300, 2.0)
    assert hh == H
    eps = synth.make_eps(N, dims, 9)
    ref = O.guiding(sd, stats, cfg, win, H, 0.6, eps, mode, critic=critic)
    s, a, r = window_dev(win)
    res = h.plan_step(MODES[mode], s, a, r, eps[:, 0, :, 0, :].cuda(), H, 2.0, 0.6, 0.99, N)
    _assert_close(res["sample_actions"], ref["sample_actions"], 2e-5, "sample_actions")
    scale = max(float(ref["expect_return"].abs().max()), 1.0)
    assert float((res["expect_return"].cpu() - ref["expect_return"]).abs().max()) <= 5e-5 * scale
    p, ev, am = h.select(res["expect_return"], res["sample_actions"][:, 0], cfg.temperature)
    assert int(am.item()) == ref["argmax"]
    _assert_close(ev, ref["eval_action"], 1e-4, "eval_action")
    h.close()


@pytest.mark.parametrize("hidden", [64, 128, 96])
def test_critic_widths_match_oracle(hidden):
    """TwinQ at other hidden widths (finetune_omtm/model.py:146-171): 64 / 128 run the fp32 matrix-core kernel (256 is every
    other critic test), 96 the scalar one; 130 rows = four whole 32-row tiles and a ragged one."""
    T, H, N = 8, 4, 130
    dims = synth.Dims(11, 3, T)
    h = capi.Handle(dims.state_dim, dims.action_dim, dims.traj_length, dims.n_embd, dims.n_head, dims.n_enc_layer,
                    dims.n_dec_layer, max_candidates=N, max_batch=1, critic_hidden=hidden)
    sd = synth.make_state_dict(dims, 0)
    h.load_weights(sd)
    tstats = synth.make_tokenizer_stats(dims, 0)
    for k, name in enumerate(synth.KEYS):
        h.set_tokenizer(k, tstats[name]["mean"], tstats[name]["std"], normalize=(name != "actions"))
    critic = synth.make_critic(dims, 0, hidden=hidden)
    h.set_critic(*critic)
    cfg = O.PlanCfg(T, H, N, 0.99, 1.0, 0.6)
    win, hh = O.assemble_window(cfg, synth.make_history(dims, 3), 300, 2.0)
    eps = synth.make_eps(N, dims, 9)
    ref = O.guiding(sd, O.make_stats(tstats), cfg, win, H, 0.6, eps, "critic", critic=critic)
    s, a, r = window_dev(win)
    res = h.plan_step(MODES["critic"], s, a, r, eps[:, 0, :, 0, :].cuda(), H, 2.0, 0.6, 0.99, N)
    scale = max(float(ref["expect_return"].abs().max()), 1.0)
    assert float((res["expect_return"].cpu() - ref["expect_return"]).abs().max()) <= 5e-5 * scale
    p_, ev, am = h.select(res["expect_return"], res["sample_actions"][:, 0], cfg.temperature)
    assert int(am.item()) == ref["argmax"]
    h.close()


@pytest.mark.parametrize("T,H,N,mode", [(8, 4, 625, "rtg"), (8, 4, 320, "critic"), (16, 8, 300, "rtg")])
def test_few_tile_bf16_passes_match_oracle(T, H, N, mode):
    """bf16 candidate passes of 16..96 fused-tail tiles (the reference's shipped N=625 / H=4 / T=8 config among them) take the
    four-workgroups-per-tile form of the fused layer tail + its reduce launch (DESIGN.md section 4 "Small problems"): scores
    within the bf16 tolerance of the oracle, shards of the candidates bit-identical to the whole."""
    dims = synth.Dims(11, 3, T)
    h, sd, stats, critic = make_handle(dims, max_candidates=N, max_batch=1)
    cfg = O.PlanCfg(T, H, N, 0.99, 1.0 if mode != "rtg" else 0.01, 0.6)
    win, hh = O.assemble_window(cfg, synth.make_history(dims, 3), 300, 2.0)
    eps = synth.make_eps(N, dims, 9)
    dev_eps = eps[:, 0, :, 0, :].cuda()
    ref = O.guiding(sd, stats, cfg, win, H, 0.6, eps, mode, critic=critic)
    s, a, r = window_dev(win)
    res = h.plan_step(MODES[mode], s, a, r, dev_eps, H, 2.0, 0.6, 0.99, N, precision=capi.PREC_BF16)
    scale = max(float(ref["expect_return"].abs().max()), 1.0)
    d = res["expect_return"].cpu() - ref["expect_return"]
    assert float((d - d.median()).abs().max()) <= 3e-2 * scale, float((d - d.median()).abs().max()) / scale
    # two shards: the same bits (the kernel choice goes by n_total, not by the shard)
    n0 = N // 2
    parts = [h.plan_step(MODES[mode], s, a, r, dev_eps, H, 2.0, 0.6, 0.99, N, b0, cnt, precision=capi.PREC_BF16)["expect_return"]
             for b0, cnt in ((0, n0), (n0, N - n0))]
    assert torch.equal(torch.cat(parts), res["expect_return"])
    h.close()


# ------------------------------------------------------------------------------------ properties at full size
def test_sharding_is_exact():
    """Scoring candidates in shards gives bit-identical scores to one call (candidates are independent)."""
    dims = synth.Dims(11, 3, 32)
    h, sd, stats, critic = make_handle(dims, max_candidates=1024, max_batch=1)
    cfg = O.PlanCfg(32, 16, 1024)
    win, hh = O.assemble_window(cfg, synth.make_history(dims, 0), 500, 3.0)
    eps = synth.make_eps(1024, dims, 1)[:, 0, :, 0, :].cuda()
    s, a, r = window_dev(win)
    for prec in (capi.PREC_FP32, capi.PREC_BF16):
        full = h.plan_step(capi.MODE_RTG, s, a, r, eps, 16, 3.0, 0.6, 0.99, 1024, precision=prec)["expect_return"].clone()
        parts = [h.plan_step(capi.MODE_RTG, s, a, r, eps, 16, 3.0, 0.6, 0.99, 1024, n_begin=b, n_count=256,
                             precision=prec)["expect_return"].clone() for b in range(0, 1024, 256)]
        assert torch.equal(full, torch.cat(parts))
    h.close()


def test_select_properties():
    dims = synth.Dims(11, 3, 8, n_embd=64, n_head=2)
    h, *_ = make_handle(dims, 8, 1)
    g = torch.Generator().manual_seed(0)
    er = (torch.randn(5000, generator=g) * 30).cuda()
    a0 = torch.rand(5000, 4, 3, generator=g).cuda()
    p, ev, am = h.select(er, a0[:, 0], 0.05)
    cfg = O.PlanCfg(8, 4, 5000, temperature=0.05)
    pr, evr = O.select(cfg, er.cpu(), a0[:, 0].cpu())
    assert int(am.item()) == int(torch.argmax(er))
    assert abs(float(p.sum()) - 1.0) < 1e-5
    _assert_close(p, pr, 1e-5, "p")
    _assert_close(ev, evr, 1e-5, "eval_action")
    # the multinomial draw: argmax(p / Exp(1)) with the caller's generator == torch.multinomial(p, 1)
    for seed in (5, 6, 7):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        ref_idx = torch.multinomial(p, 1, generator=gen)
        gen.manual_seed(seed)
        expo = torch.empty(5000, device="cuda").exponential_(1, generator=gen)
        _, _, _, si, sa = h.select(er, a0[:, 0], 0.05, expo)
        assert int(si.item()) == int(ref_idx.item())
        assert torch.equal(sa[0], a0[int(ref_idx.item()), 0])
    h.close()


def test_rescore_topk_replaces_exactly_the_k_best():
    """bf16 scores for all candidates, then fp32 re-scores of the top-k written in place: the touched
    entries equal the fp32 plan_step's scores bit for bit, the others keep their bf16 value."""
    dims = synth.Dims(11, 3, 16)
    h, sd, stats, critic = make_handle(dims, max_candidates=256, max_batch=1)
    cfg = O.PlanCfg(16, 8, 256)
    win, hh = O.assemble_window(cfg, synth.make_history(dims, 0), 500, 3.0)
    eps = synth.make_eps(256, dims, 1)[:, 0, :, 0, :].cuda()
    s, a, r = window_dev(win)
    f32 = h.plan_step(capi.MODE_RTG, s, a, r, eps, 8, 3.0, 0.6, 0.99, 256)["expect_return"].clone()
    b16 = h.plan_step(capi.MODE_RTG, s, a, r, eps, 8, 3.0, 0.6, 0.99, 256, precision=capi.PREC_BF16)["expect_return"]
    before = b16.clone()
    top = h.rescore_topk(capi.MODE_RTG, s, a, r, eps, b16, 16, 8, 3.0, 0.6, 0.99).long()
    assert set(top.tolist()) == set(torch.topk(before, 16).indices.tolist())
    # same fp32 arithmetic; the 16-candidate pass splits K over blocks, so sums associate differently
    assert float((b16[top] - f32[top]).abs().max()) <= 2e-5 * float(f32.abs().max())
    rest = torch.ones(256, dtype=torch.bool, device="cuda")
    rest[top] = False
    assert torch.equal(b16[rest], before[rest])
    h.close()


def test_errors_are_reported():
    dims = synth.Dims(11, 3, 8, n_embd=64, n_head=2)
    h = capi.Handle(11, 3, 8, 64, 2, max_candidates=4, max_batch=1)
    z = torch.zeros(8, 11).cuda()
    with pytest.raises(capi.M3pcError, match="weights not loaded"):
        h.plan_step(capi.MODE_RTG, z, torch.zeros(8, 3).cuda(), torch.zeros(8, 1).cuda(), torch.zeros(4, 8, 3).cuda(),
                    4, 1.0, 0.6, 0.99, 4)
    with pytest.raises(capi.M3pcError, match="missing"):
        h.load_weights({"pos_embed": torch.zeros(8, 64)})
    h.close()
