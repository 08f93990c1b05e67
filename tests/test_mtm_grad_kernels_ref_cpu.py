"""The references of tests/mtm_grad_kernels_ref.py, tested themselves (no GPU): each float64 reference agrees with torch autograd in
float64; the float32 restatement of every operation (the shadow an EV carries, or torch's float32) stays inside the operation's own
bound; the `int` regimes are exact in float64 and float32; the bit-for-bit restatements reproduce hand-computed cases; seeded errors of
the kind the GPU suite is for exceed the bounds; and every refusal of the m3pc_debug_mg_* hooks comes before any HIP call."""
import ctypes as C
import re
import os

import numpy as np
import pytest
import torch

import attn_ref as AR
import gemm_ref as GM
import mtm_grad_kernels_ref as R
import mtm_loss_ref as LR
from mtm_grad_kernels_ref import EV, F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gen(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g)


def inside(ev, what, floor=R.TINY):
    ratio = float(((ev.s.double() - ev.v).abs() / (ev.e + floor)).max())
    assert ratio <= 1, f"{what}: the float32 restatement is {ratio:.3g} bounds from float64"
    return ratio


# ------------------------------------------------------------------------------------------------ the header and the ids
def test_the_header_lists_the_fifteen_ids_of_the_source():
    hdr = open(os.path.join(ROOT, "include", "m3pc_hip_debug.h")).read()
    block = hdr[hdr.index("MTM-gradient kernel ids"):hdr.index("(end of the MTM-gradient kernel ids)")]
    ids = {int(n): k for n, k in re.findall(r"(\d+) (mg_[a-z0-9_]+_kernel(?:<[a-z]+>)?)", block)}
    assert sorted(ids) == list(range(1, 16))
    src = open(os.path.join(ROOT, "m3pc_amd", "csrc", "mtm_grad.hip")).read()
    kernels = set(re.findall(r"__global__ __launch_bounds__\(256\) void (mg_[a-z0-9_]+_kernel)", src))
    assert len(kernels) == 14 and {k.split("<")[0] for k in ids.values()} == kernels
    picks = [int(n) for n in re.findall(r"M3PC_MG_PICK\((\d+)\)", src)]
    assert sorted(picks) == list(range(1, 16))
    # every launch of the file goes through a launcher that records its id
    assert src.count("hipLaunchKernelGGL(") == 15
    assert set(R.KID.values()) == set(ids)


# ------------------------------------------------------------------------------------------------ the product
@pytest.mark.parametrize("splitk", [False, True])
def test_gemm_int_regime_is_exact_in_both_precisions(splitk):
    t = R.gemm_inputs("int", 33, 65, 200, seed=1, bias=True, bias2=True, pos_T=5, res=True, gelu_aux=True, c0=True)
    r = R.mg_gemm_ref(t, pos_T=5, splitk=splitk)
    assert torch.equal(r["C"], r["C32"].double())
    assert torch.equal(r["C"] * 2, (r["C"] * 2).round())  # (gelu' = 0.5 halves an integer)
    aux = EV(t["gelu_aux"])
    gp = R.ev_gelu_grad(aux)
    assert set(gp.s.unique().tolist()) == {0.5, 1.0}


@pytest.mark.parametrize("regime", ["randn", "offset", "spike"])
def test_gemm_float32_stays_inside_the_bound(regime):
    for K in (1, 3, 17, 200):
        t = R.gemm_inputs(regime, 33, 31, K, seed=K, bias=True, bias2=True, pos_T=5, res=True, gelu_aux=True, c0=True)
        r = R.mg_gemm_ref(t, pos_T=5, gelu_out=True)
        assert float(((r["C32"].double() - r["C"]).abs() / r["E"]).max()) <= 1, (regime, K)
        assert float(((r["G32"].double() - r["G"]).abs() / r["EG"]).max()) <= 1, (regime, K)


def test_gemm_forms_are_dx_and_dw_of_a_linear():
    rn = gen(3)
    X, W, dY = rn(9, 12).double().requires_grad_(), rn(7, 12).double().requires_grad_(), rn(9, 7)
    (X @ W.T * dY.double()).sum().backward()
    dx = R.mg_gemm_ref({"A": dY, "W": W.detach().T.contiguous().float()})           # dX (M, N) = dY (M, K) W (K, N): "W" is B^T = W^T
    dw = R.mg_gemm_ref({"A": dY.T.contiguous(), "W": X.detach().T.contiguous().float()}, splitk=True)  # dW = dY^T X
    assert torch.allclose(dx["C"], X.grad, rtol=1e-6, atol=1e-6) and torch.allclose(dw["C"], W.grad, rtol=1e-6, atol=1e-6)


def test_the_bound_catches_a_dropped_tail_term_and_a_dropped_partial():
    t = R.gemm_inputs("spike", 33, 31, 200, seed=5)
    r = R.mg_gemm_ref(t, splitk=True)
    A, W = t["A"].double(), t["W"].double()
    for k in (199, R.SPIKE_K2):
        bad = r["C"] - A[:, k:k + 1] @ W[:, k:k + 1].T
        assert float(((bad - r["C"]).abs() / r["E"]).min()) > 100
    t = R.gemm_inputs("randn", 8, 8, 64, seed=6, bias=True, bias2=True)
    r = R.mg_gemm_ref(t)
    assert float(((r["C"] - t["bias2"].double() - r["C"]).abs() / r["E"]).median()) > 100  # bias2 dropped
    t = R.gemm_inputs("randn", 8, 8, 64, seed=7, gelu_aux=True)
    r = R.mg_gemm_ref(t)
    x = t["gelu_aux"].double()
    cdf_only = GM.gemm_ref(t["A"], t["W"])["acc"] * 0.5 * (1 + torch.erf(x * R.C_SQRT_HALF))
    assert float(((cdf_only - r["C"]).abs() / r["E"]).median()) > 100                      # gelu' without x pdf


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("regime", ["randn", "offset"])
@pytest.mark.parametrize("d", [64, 192, 1024])
def test_layernorm_references(regime, d):
    from elementwise_ref import ln_inputs
    x, g, b, _, _ = ln_inputs(regime, 5, d, False, "cpu", d)
    y32, m32, r32 = R.ln_fwd32(x, g, b)
    m64, r64 = R.ln_stats64(x)
    dm, dr = R.ln_stat_bound(x)
    assert bool(((y32.double() - GM.layernorm64(x, g, b)).abs() <= GM.ln_bound(x, g, b)).all())
    assert bool(((m32.double() - m64).abs() <= dm).all()) and bool(((r32.double() - r64).abs() <= dr).all())
    # backward: float64 against autograd, the float32 shadow inside the bound
    dy = gen(d + 1)(5, d)
    xg = x.double().requires_grad_()
    (GM.layernorm64(xg, g, b) * dy.double()).sum().backward()
    ref = R.ln_bwd64(x, dy, g, m64, r64)
    assert torch.allclose(ref, xg.grad, rtol=1e-9, atol=1e-9 * float(xg.grad.abs().max()))
    ev = R.ln_bwd_ref(x, dy, g, m64.float(), r64.float(), dx0=gen(d + 2)(5, d))
    inside(ev, f"ln_bwd {regime} d={d}")
    ev0 = R.ln_bwd_ref(x, dy, g, m64.float(), r64.float())
    assert torch.allclose(ev0.v, ref, rtol=1e-4, atol=1e-5 * float(ref.abs().max()))  # (the statistics rounded to float32)
    # seeded: without the xhat * s2 term; with eps 1e-6 (randn rows of small variance feel it)
    gg = dy.double() * g.double()
    xh = (x.double() - m64[:, None]) * r64[:, None]
    no_s2 = r64[:, None] * (gg - gg.mean(-1, keepdim=True))
    assert float(((no_s2 - ev0.v).abs() / ev0.bound()).median()) > 10


def test_the_layernorm_bound_tells_eps_1e_6():
    x = 0.01 * gen(1)(4, 64)
    g, b = torch.ones(64), torch.zeros(64)
    c = x.double() - x.double().mean(-1, keepdim=True)
    y6 = c * torch.rsqrt((c * c).mean(-1, keepdim=True) + 1e-6)
    assert float(((y6 - GM.layernorm64(x, g, b)).abs() / GM.ln_bound(x, g, b)).median()) > 100


# ------------------------------------------------------------------------------------------------ column sums
def test_colsum_restatement_on_a_hand_computed_case():
    # two sequences of L = 3 rows, the run j0 = 1, n = 2, sel = 0b10: the rows (s, j = 1): buffer rows 2 and 5, compact rows 1 and 3
    dY = np.arange(12, dtype=F).reshape(6, 2) + 1          # buffer rows
    X = np.array([[0, 0], [0, 0], [3, 5], [0, 0], [0, 0], [7, 1]], F)
    st = np.array([[9, 9], [1, 2], [9, 9], [3, 0.5]], F)
    o0, o1 = R.colsum_ref(dY, 0, X, st, 2, 3, 1, 2, 0b10, 2)
    assert o0.tolist() == [5 + 11, 6 + 12]
    assert o1.tolist() == [5 * (3 - 1) * 2 + 11 * (7 - 3) * 0.5, 6 * (5 - 1) * 2 + 12 * (1 - 3) * 0.5]
    dYc = np.array([[0, 0], [5, 6], [0, 0], [11, 12]], F)  # the same rows, compact
    c0, c1 = R.colsum_ref(dYc, 1, X, st, 2, 3, 1, 2, 0b10, 2)
    assert c0.tolist() == o0.tolist() and c1.tolist() == o1.tolist()
    assert R.colsum_ref(dY, 0, None, None, 2, 3, 1, 2, 0b10, 2)[1] is None
    # float64 accumulation: 2^24 + 1 + 1 is exact there and rounds once; a float32 chain would lose both ones
    big = np.array([[2.0 ** 24], [1.0], [1.0]], F)
    assert R.colsum_ref(big, 0, None, None, 3, 1, 0, 1, 1, 1)[0][0] == F(2.0 ** 24 + 2)
    # chunks of 64: rows 0..63 and 64 land in different partials, the total is the same
    ones = np.ones((65, 1), F)
    assert R.colsum_ref(ones, 0, None, None, 65, 1, 0, 1, 1, 1)[0][0] == 65


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("regime", AR.REGIMES)
def test_attention_references(regime):
    B, L, nh, hd = 2, 9, 2, 32
    d = nh * hd
    t = AR.make_inputs(regime, B, L, L, nh, hd, dtype=0, seed=11)
    QKV = torch.cat([t["q"], t["k1"], t["v1"]], -1)
    scale = hd ** -0.5
    dO = gen(12)(B, L, d)
    P, EP, O, EO = R.attn_fwd_ref(QKV, nh, scale)
    p32, o32 = R.attn_fwd32(QKV, nh, scale)
    assert float(((p32.double() - P).abs() / EP).max()) <= 1 and float(((o32.double() - O).abs() / EO).max()) <= 1
    # float64 against autograd
    qkv = QKV.double().requires_grad_()
    q, k, v = R.split_qkv(qkv, d)
    (AR.attention_ref(q, k, v, nh, scale)["O"] * dO.double()).sum().backward()
    dqkv, ds64, p64 = R.attn_bwd64(QKV, dO, nh, scale)
    assert torch.allclose(dqkv, qkv.grad, rtol=1e-9, atol=1e-9 * float(qkv.grad.abs().max()))
    # the kernels' references on the P they are given
    Pf = P.float()
    dv = R.attn_col_ref(Pf, dO, nh, 1.0)
    ds, dq = R.attn_row_ref(Pf, dO, QKV, nh, scale)
    dk = R.attn_col_ref(ds.s, t["q"], nh, scale)
    for ev, name in ((dv, "dV"), (ds, "dS"), (dq, "dQ"), (dk, "dK")):
        inside(ev, f"{regime} {name}")
    tol = lambda x: 1e-5 * float(x.abs().max()) + 1e-30
    assert torch.allclose(dv.v, dqkv[..., 2 * d:], rtol=1e-4, atol=tol(dv.v))
    if regime in ("randn", "offset"):  # (peaked, same: dS and dQ are what the rounding of P to float32 leaves of a cancellation)
        assert torch.allclose(dq.v, dqkv[..., :d], rtol=1e-4, atol=tol(dq.v)) and torch.allclose(ds.v, ds64, rtol=1e-4, atol=tol(ds64))
        assert torch.allclose(dk.v, dqkv[..., d:2 * d], rtol=1e-3, atol=10 * tol(dk.v))
    # seeded: alpha not applied (dK), dot not subtracted (dS)
    if regime == "randn":
        assert float(((dk.v / scale - dk.v).abs() / dk.bound()).median()) > 100
        dp = R.heads(dO.double(), nh) @ R.heads(t["v1"].double(), nh).transpose(-1, -2)
        assert float(((Pf.double() * dp - ds.v).abs() / ds.bound()).median()) > 100


# ------------------------------------------------------------------------------------------------ token layout
def test_token_restatements_on_a_hand_computed_case():
    T, B, d = 3, 1, 2
    bits, kept, eoff, Le = R.mask_bits([[], [2], [0, 2], []], T)
    assert (bits, kept, eoff, Le) == ([0, 4, 5, 0], [0, 1, 2, 0], [0, 0, 1, 3], 3)
    assert R.enc_rows(bits, T) == [(1, 2), (2, 0), (2, 2)]
    tok = [np.zeros((1, 3, 1), F), np.array([[[9, 9], [9, 9], [2, 3]]], F), np.array([[[4], [9], [5]]], F), np.zeros((1, 3, 1), F)]
    W = [np.zeros((2, 1), F), np.array([[1, 10], [100, 1000]], F), np.array([[2], [3]], F), np.zeros((2, 1), F)]
    bias = [np.zeros(2, F), np.array([0.5, 0.25], F), np.array([1, 2], F), np.zeros(2, F)]
    pdim = [np.zeros(2, F), np.array([8, 16], F), np.array([32, 64], F), np.zeros(2, F)]
    pos = np.array([[1000, 2000], [0, 0], [3000, 4000]], F)
    X = R.embed_ref(tok, W, bias, pdim, pos, bits, B, T, d)
    assert X[0].tolist() == [[2 + 30 + 0.5 + 8 + 3000, 200 + 3000 + 0.25 + 16 + 4000], [8 + 1 + 32 + 1000, 12 + 2 + 64 + 2000],
                             [10 + 1 + 32 + 3000, 15 + 2 + 64 + 4000]]
    # float32 order: (a + bias) + pdim + pos, every step rounded -- 2^24 + 1 absorbs, the order shows
    tok1 = [np.array([[[1]]], F)] + [np.zeros((1, 1, 1), F)] * 3
    W1 = [np.array([[2.0 ** 24]], F)] + [np.zeros((1, 1), F)] * 3
    one = [np.array([1.0], F)] + [np.zeros(1, F)] * 3
    assert R.embed_ref(tok1, W1, one, one, np.array([[-2.0 ** 24]], F), [1, 0, 0, 0], 1, 1, 1)[0, 0, 0] == 0.0
    mtok = [np.array([-1, -1], F), np.array([-2, -2], F), np.array([-3, -3], F), np.array([-4, -4], F)]
    src = np.array([[[1, 1], [2, 2], [3, 3]]], F)
    Z = R.gather_ref(src, mtok, bits, B, T, d)
    assert Z[0, :, 0].tolist() == [-1, -1, -1, -2, -2, 1, 2, -3, 3, -4, -4, -4]
    assert np.array_equal(R.scatter_ref(Z, bits, B, T, d), src)
    assert R.tokv_ref(tok[2], bits[2], T).tolist() == [[4], [5]] and R.tokv_ref(tok[1], bits[1], T).tolist() == [[2, 3]]


# ------------------------------------------------------------------------------------------------ std, the loss backward
def test_std_reference():
    ls = torch.cat([torch.linspace(-12, 12, 4001), torch.tensor([-30.0, 30.0])])
    ev = R.std_ref(ls)
    inside(ev, "std")
    assert torch.allclose(ev.v, torch.exp(-5 + 3.5 * (torch.tanh(ls.double()) + 1)))
    assert abs(float(ev.v[-2]) - np.exp(-5.0)) < 1e-12 and abs(float(ev.v[-1]) - np.exp(2.0)) < 1e-12  # the ends
    assert float((ev.bound() / ev.v).max()) < 200 * R.U32  # the bound is a few dozen ulp, not a guess
    three = torch.exp(-5 + 3.0 * (torch.tanh(ls.double()) + 1))
    assert float(((three - ev.v).abs() / ev.bound()).median()) > 1000


@pytest.mark.parametrize("flags,loss_keys", [(R.CLIP_ACTIONS, 1), (R.NORM_L2, 15), (R.CLIP_ACTIONS, 6), (R.NORM_L2, 0)])
@pytest.mark.parametrize("shape", [(1, 4, 11, 3), (3, 8, 17, 6), (5, 4, 1, 1)])
def test_loss_backward_reference(shape, flags, loss_keys):
    B, T, S, A = shape
    pred, mu, ls, tgt, eps = R.loss_inputs(B, T, S, A, 1, bool(flags & R.CLIP_ACTIONS))
    mask = R.loss_masks(T, 3)
    hidden = T - bin(mask[1]).count("1")
    inv_cnt = float(F(1.0 / (B * hidden * A)))
    sd = R.std_ref(ls).v.float()
    dpred, dmu, dls = R.loss_bwd_ref(pred, mu, sd, ls, tgt, eps, mask, B, T, S, A, flags, loss_keys, 0.1, inv_cnt)
    for ev, name in list(zip(dpred, ("dstates", "drewards", "dreturns"))) + [(dmu, "dmu"), (dls, "dls")]:
        ok = torch.isfinite(ev.v)
        assert LR.same_specials(ev.v.numpy(), ev.s.double().numpy()), name
        assert float(((ev.s.double() - ev.v).abs()[ok] / ev.bound()[ok]).max()) <= 1, name
    # float64 against autograd of the header's total (the float32 clip bounds), where the total is finite
    if S > 1 or not flags & R.NORM_L2:
        leaves = [p.double().requires_grad_() for p in pred] + [mu.double().requires_grad_(), ls.double().requires_grad_()]
        total = R.loss_total64(leaves[:3], leaves[3], leaves[4], tgt, eps, mask, B, T, S, A, flags, loss_keys, 0.1)
        assert bool(torch.isfinite(total))
        total.backward()
        for ev, leaf, name in zip(dpred + [dmu, dls], leaves, ("dstates", "drewards", "dreturns", "dmu", "dls")):
            g = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
            assert torch.allclose(ev.v, g, rtol=2e-5, atol=2e-6 * max(1.0, float(g.abs().max()))), (name, float((ev.v - g).abs().max()))


def test_loss_backward_specials_and_seeded_errors():
    B, T, S, A = 2, 4, 1, 2
    pred, mu, ls, tgt, eps = R.loss_inputs(B, T, S, A, 2, False)
    tgt[0][3, 0] = 0.0                                              # NORM_L2 of a width-1 zero target: 0 / 0
    sd = R.std_ref(ls).v.float()
    dpred, dmu, dls = R.loss_bwd_ref(pred, mu, sd, ls, tgt, eps, R.loss_masks(T, 3), B, T, S, A, R.NORM_L2, 15, 0.1, float(F(1 / (B * 2 * A))))
    assert bool(torch.isnan(dpred[0].v[3, 0])) and int(torch.isnan(dpred[0].v).sum()) == 1
    # every action visible: inv_cnt = inf never reaches a visible row
    mask = R.loss_masks(T, 3, all_visible=True)
    dpred, dmu, dls = R.loss_bwd_ref(pred, mu, sd, ls, tgt, eps, mask, B, T, S, A, R.CLIP_ACTIONS, 15, 0.1, float("inf"))
    assert bool(torch.isfinite(dmu.v).all()) and not bool(dls.v.any()) and all(bool(torch.isfinite(p.v).all()) for p in dpred)
    # seeded: 3.0 for 3.5 in d log_std
    mask = R.loss_masks(T, 3)
    _, dmu, dls = R.loss_bwd_ref(pred, mu, sd, ls, tgt, eps, mask, B, T, S, A, R.CLIP_ACTIONS, 1, 0.1, float(F(1 / (B * 2 * A))))
    nz = dls.v != 0
    assert float(((dls.v * (3.0 / 3.5) - dls.v).abs()[nz] / dls.bound()[nz]).median()) > 1000


# ------------------------------------------------------------------------------------------------ the hooks' refusals
def test_every_bad_argument_is_refused_before_any_hip_call():
    """The refusals make no HIP call: they return M3PC_EINVAL on a machine without a device (every pointer below is host memory the
    hooks never read)."""
    import mtm_grad_lab as ML
    try:
        lib = ML.lab()
    except Exception as e:  # no hipcc here: the lab library cannot be built
        pytest.skip(f"the lab library cannot be built: {e}")
    err = lib.m3pc_last_error
    buf = C.create_string_buffer(1 << 16)
    p = C.addressof(buf)
    picked = (C.c_int * 2)(7, 7)
    pk = C.cast(picked, ML.pi)

    def refused(fn, a, word, what):
        a.picked = pk
        picked[0] = picked[1] = 7
        rc = getattr(lib, fn)(C.byref(a))
        assert rc == -1 and word in err(), (what, rc, err())
        assert picked[0] == 0 and picked[1] == 0, what

    for fn in ML.HOOKS:
        assert getattr(lib, fn)(None) == -1 and b"null arguments" in err(), fn

    # ---- the product
    def gemm(**kw):
        a = ML.GemmArgs()
        a.A = ML.Op(p, 8, 1, (0, 0, 0), 0, 64)
        a.B = ML.Op(p, 8, 1, (0, 0, 0), 0, 64)
        a.C, a.ldc, a.c_len, a.M, a.N, a.K = p, 8, 64, 8, 8, 8
        for k, v in kw.items():
            o = a
            *path, leaf = k.split("__")
            for q in path:
                o = getattr(o, q)
            setattr(o, leaf, v)
        return a
    G = "m3pc_debug_mg_gemm"
    refused(G, gemm(C=None), b"required", "null C")
    refused(G, gemm(A__p=None), b"required", "null A")
    refused(G, gemm(B__p=None), b"required", "null B")
    for dim in ("M", "N", "K"):
        refused(G, gemm(**{dim: 0}), b">= 1", dim)
    refused(G, gemm(M=9), b"operand A", "A row 8 beyond 64 floats")
    refused(G, gemm(N=9), b"operand B", "B row 8 beyond 64 floats")
    refused(G, gemm(K=9), b"operand A", "k = 8 beyond the last row")
    refused(G, gemm(A__s_o=-8), b"operand A", "negative stride")
    refused(G, gemm(A__map=(2, 1, 0)), b"operand A", "gstride < rpg")
    refused(G, gemm(A__map=(2, 4, 0)), b"operand A", "the row map leaves the buffer")
    refused(G, gemm(B__map=(2, 4, 0), B__map_k=1, B__s_o=1, B__s_k=8), b"operand B", "the k map leaves the buffer")
    refused(G, gemm(A__s_o=1 << 40, A__len=1 << 62), b"operand A", "an index beyond int")
    refused(G, gemm(ldc=7), b"ldc", "ldc < N")
    refused(G, gemm(c_len=63), b"of C", "C too short")
    refused(G, gemm(cmap=(4, 8, 0)), b"of C", "cmap leaves C")
    refused(G, gemm(bias2=p), b"bias2", "bias2 alone")
    refused(G, gemm(pos=p, pos_T=0), b"pos_T", "pos_T 0")

    # ---- LayerNorm
    def ln(**kw):
        a = ML.LnArgs()
        a.X, a.x_rows, a.g, a.b, a.Y, a.st, a.dY, a.dX, a.rows, a.d = p, 4, p, p, p, p, p, p, 4, 64
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    Lh = "m3pc_debug_mg_layernorm"
    for f in ("X", "g", "st"):
        refused(Lh, ln(**{f: None}), b"required", f)
    refused(Lh, ln(Y=None), b"forward needs", "Y")
    refused(Lh, ln(b=None), b"forward needs", "b")
    refused(Lh, ln(backward=1, dY=None), b"backward needs", "dY")
    refused(Lh, ln(backward=1, dX=None), b"backward needs", "dX")
    refused(Lh, ln(rows=0), b"rows", "rows 0")
    refused(Lh, ln(d=0), b"rows", "d 0")
    refused(Lh, ln(rows=1 << 22, d=1 << 10, x_rows=1 << 22), b"rows", "rows d beyond int")
    refused(Lh, ln(xmap=(2, 1, 0)), b"row map", "bad map")
    refused(Lh, ln(rows=5), b"x_rows", "row 4 of 4")
    refused(Lh, ln(xmap=(2, 4, 1)), b"x_rows", "mapped row 6 of 4")

    # ---- column sums
    def cs(**kw):
        a = ML.ColsumArgs()
        a.dY, a.ldy, a.nseq, a.L, a.j0, a.n, a.sel, a.C, a.part, a.part_doubles, a.buf_rows, a.out0 = p, 8, 3, 4, 1, 3, 7, 8, p, 16, 12, p
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    Ch = "m3pc_debug_mg_colsum"
    for f in ("dY", "out0", "part"):
        refused(Ch, cs(**{f: None}), b"required", f)
    refused(Ch, cs(X=p), b"come together", "X without st")
    refused(Ch, cs(st=p), b"come together", "st without X")
    refused(Ch, cs(out1=p), b"come together", "out1 without X")
    refused(Ch, cs(nseq=0), b"nseq", "nseq 0")
    refused(Ch, cs(n=0), b"nseq", "n 0")
    refused(Ch, cs(n=65, L=80, buf_rows=1000, part_doubles=1000), b"nseq", "n 65")
    refused(Ch, cs(j0=-1), b"beyond L", "j0 < 0")
    refused(Ch, cs(j0=2), b"beyond L", "j0 + n > L")
    refused(Ch, cs(C=0), b"ldy", "C 0")
    refused(Ch, cs(ldy=7), b"ldy", "ldy < C")
    refused(Ch, cs(buf_rows=11), b"buf_rows", "the last row is 11")
    refused(Ch, cs(part_doubles=15), b"chunks", "one chunk of 2 C = 16 doubles")
    refused(Ch, cs(nseq=22, buf_rows=88, part_doubles=31), b"chunks", "66 rows: two chunks, 32 doubles")
    refused(Ch, cs(nseq=1 << 30, L=64, n=64, j0=0, buf_rows=1 << 40, part_doubles=1 << 40), b"buf_rows", "nseq n beyond int")

    # ---- attention
    def at(**kw):
        a = ML.AttnArgs()
        a.QKV, a.P, a.O, a.dO, a.dQKV, a.B, a.L, a.d, a.nh, a.hd, a.scale = p, p, p, p, p, 1, 4, 64, 2, 32, 0.25
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    Ah = "m3pc_debug_mg_attention"
    refused(Ah, at(which=4), b"which", "which 4")
    refused(Ah, at(which=-1), b"which", "which -1")
    for L in (0, -1, 257, 1 << 20):
        refused(Ah, at(L=L), b"LDS", f"L {L}")
    refused(Ah, at(nh=3), b"against d", "nh hd != d")
    refused(Ah, at(hd=0), b"against d", "hd 0")
    refused(Ah, at(B=0), b"against d", "B 0")
    refused(Ah, at(B=1 << 20, L=256), b"exceed int", "B nh L L")
    refused(Ah, at(B=1 << 16, L=256, d=1024, nh=1, hd=1024), b"exceed int", "B L 3 d")
    for which, f in ((0, "QKV"), (0, "P"), (0, "O"), (1, "dO"), (1, "P"), (1, "dQKV"), (2, "QKV"), (2, "dO"), (2, "dQKV"), (3, "QKV"), (3, "dQKV")):
        refused(Ah, at(which=which, **{f: None}), b"is null", f"which {which} without {f}")

    # ---- token layout
    def tk(**kw):
        a = ML.TokensArgs()
        for k in range(4):
            a.tok[k] = a.W[k] = a.bias[k] = a.pdim[k] = a.mtok[k] = p
            a.feat[k] = 2
        a.bits[:] = (0b101, 0b010, 0, 0b111)
        a.kept[:] = (2, 1, 0, 3)
        a.eoff[:] = (0, 2, 3, 3)
        a.pos, a.B, a.T, a.d, a.Le, a.X, a.src, a.dst, a.out = p, 1, 3, 4, 6, p, p, p, p
        for k, v in kw.items():
            if isinstance(v, tuple) and k in ("bits", "kept", "eoff", "feat", "mtok", "tok"):
                getattr(a, k)[v[0]] = v[1]
            else:
                setattr(a, k, v)
        return a
    Th = "m3pc_debug_mg_tokens"
    refused(Th, tk(which=4), b"which", "which 4")
    for T in (0, 65):
        refused(Th, tk(T=T), b"outside [1, 64]", f"T {T}")
    refused(Th, tk(B=0), b"outside [1, 64]", "B 0")
    refused(Th, tk(bits=(2, 0b1000), kept=(2, 1)), b"at or above T", "bit 3 at T = 3")
    refused(Th, tk(kept=(0, 1)), b"inconsistent", "kept != popcount")
    refused(Th, tk(eoff=(1, 1)), b"inconsistent", "eoff not the prefix sum")
    refused(Th, tk(Le=5), b"Le", "Le != sum")
    a = tk()
    a.bits[:] = (0, 0, 0, 0)
    a.kept[:] = (0, 0, 0, 0)
    a.eoff[:] = (0, 0, 0, 0)
    a.Le = 0
    refused(Th, a, b"Le", "no token kept")
    refused(Th, tk(B=1 << 22, d=1 << 10), b"exceeds int", "B 4 T d")
    refused(Th, tk(which=0, X=None), b"embed needs", "embed without X")
    refused(Th, tk(which=0, tok=(1, None)), b"embed needs", "embed without a kept key's tokens")
    refused(Th, tk(which=0, feat=(0, 0)), b"embed needs", "feat 0")
    refused(Th, tk(which=1, mtok=(2, None)), b"gather needs", "gather without a mask token")
    refused(Th, tk(which=1, src=None), b"gather needs", "gather without src")
    refused(Th, tk(which=2, dst=None), b"scatter needs", "scatter without dst")
    refused(Th, tk(which=3, key=2), b"tokv needs", "tokv of a fully hidden key")
    refused(Th, tk(which=3, key=4), b"tokv needs", "key 4")
    refused(Th, tk(which=3, key=0, out=None), b"tokv needs", "tokv without out")

    # ---- std, the loss backward
    for args in ((None, p, 4), (p, None, 4), (p, p, 0)):
        picked[0] = picked[1] = 7
        assert lib.m3pc_debug_mg_std(args[0], args[1], args[2], None, pk) == -1 and b"debug_mg_std" in err() and picked[0] == 0

    def lb(**kw):
        a = ML.LossBwdArgs()
        for j in range(3):
            a.pred[j] = a.dpred[j] = p
        for k in range(4):
            a.tgt[k] = p
        a.mu = a.sd = a.ls = a.eps = a.dmu = a.dls = p
        a.batch, a.T, a.S, a.A, a.loss_keys = 2, 4, 3, 2, 15
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(a, k)[v[0]] = v[1]
            else:
                setattr(a, k, v)
        return a
    Bh = "m3pc_debug_mg_loss_bwd"
    for f in ("mu", "sd", "ls", "eps", "dmu", "dls"):
        refused(Bh, lb(**{f: None}), b"null pointer", f)
    refused(Bh, lb(pred=(1, None)), b"null pointer", "pred[1]")
    refused(Bh, lb(dpred=(2, None)), b"null pointer", "dpred[2]")
    refused(Bh, lb(tgt=(3, None)), b"null pointer", "tgt[3]")
    for f in ("batch", "S", "A", "T"):
        refused(Bh, lb(**{f: 0}), b"outside [1, 64]", f)
    refused(Bh, lb(T=65), b"outside [1, 64]", "T 65")
    refused(Bh, lb(mask=(1, 0b10000)), b"at or above T", "mask bit 4 at T = 4")
    refused(Bh, lb(flags=4), b"unknown flag", "flags 4")
    refused(Bh, lb(loss_keys=16), b"loss_keys", "loss_keys 16")
    refused(Bh, lb(batch=1 << 24, S=1 << 10), b"exceeds int", "batch T (S + 2 + A)")
