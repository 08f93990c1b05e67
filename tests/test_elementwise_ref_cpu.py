"""tests/elementwise_ref.py without a GPU: the float64 references against torch's own float64 operations and the oracle's twinq and
td_lambda; every bound against a plain float32 torch evaluation of the same operation (an honest float32 implementation must pass
its own bound); the `int` inputs really exact in float32; critic_pack's layout (m3pc_debug_critic_pack) against the index formulas of
the comment above critic_mfma_kernel; and what every elementwise hook of include/m3pc_hip_debug.h refuses before it would launch."""
import ctypes as C
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elementwise_ref as R
import test_elementwise_edges_gpu as E
from oracle import mtm_oracle as O

CPU = "cpu"
EINVAL = -1  # M3PC_EINVAL (include/m3pc_hip.h)
REGIMES = E.REGIMES


def ratio(out, ref, bound):
    return float(((out.double() - ref).abs() / bound).max())


# ------------------------------------------------------------------------------------------------ references are torch in float64
U64 = 2.0 ** -53  # float64 unit roundoff


def agree64(a, b, bound32):
    """Two float64 evaluations of one operation agree within twice the operation's own derived bound taken at float64 roundoff: every
    bound of elementwise_ref is a sum of terms k u |.| (convex in u), so bound(U32) U64 / U32 >= bound(U64), once for either side."""
    return bool(((a - b).abs() <= 2 * bound32 * (U64 / R.U32)).all())


def test_references_are_torch_in_float64():
    rn, ri, _ = R.gen(CPU, 1)
    x, g, b = rn(7, 192).double(), rn(192).double(), rn(192).double()
    assert agree64(R.layernorm64(x, g, b), F.layer_norm(x, (192,), g, b, 1e-5), R.ln_bound(x, g, b))
    x, W, bb, mean, stdv = R.head_inputs("randn", 5, 64, 17, CPU, 2)
    v, B = R.head_out_ref(x, W, bb, mean, stdv)
    assert agree64(v, F.linear(x.double(), W.double(), bb.double()) * stdv.double() + mean.double(), B)
    x, Wmu, bmu, Wls, bls, lnp = R.actor_inputs("randn", 5, 256, 5, CPU, 3, True)
    mu, Emu, sd, Esd = R.actor_ref(x, Wmu, bmu, Wls, bls, lnp)
    xn = F.layer_norm(x.double(), (256,), lnp[0].double(), lnp[1].double(), 1e-5)
    assert agree64(mu, F.linear(xn, Wmu.double(), bmu.double()), Emu)
    ls = -5.0 + 0.5 * (2.0 - (-5.0)) * (torch.tanh(F.linear(xn, Wls.double(), bls.double())) + 1.0)
    assert agree64(sd, torch.exp(ls), Esd)


def _qsd(nets, dtype):
    sd = {}
    for q, (W1, b1, W2, b2, W3, b3) in zip(("q1", "q2"), nets):
        for li, (W, b) in zip((0, 2, 4), ((W1, b1), (W2, b2), (W3[None], b3))):
            sd[f"{q}.net.{li}.weight"], sd[f"{q}.net.{li}.bias"] = W.to(dtype), b.to(dtype)
    return sd


def test_critic_reference_is_the_oracles_twinq():
    states, actions, om, os_, nets = R.critic_inputs("randn", 33, 17, 6, 128, CPU, 4)
    ref, B = R.critic_ref(states, actions, om, os_, nets, R.critic_n3(False, 128))
    d = torch.float64
    assert agree64(ref, O.twinq(_qsd(nets, d), om.to(d), os_.to(d), states.to(d), actions.to(d)), B)


def test_td_lambda_restatement_is_the_oracles_loop():
    """td_lambda_ref against the oracle's td_lambda.  The oracle accumulates in float32 whatever it is given (its `values` and `er` are
    float32 tensors) and sums each step's values in torch's own order, so the two agree within the roundings of two float32 evaluations.
    Per evaluation and step t: the running product gamma^(k + 1) (at most h roundings on a term), the product with it (1), the sum of
    t + 1 terms in any order (at most h), the two weights (2), and the accumulation into the result over h steps (at most h):
    (3 h + 3) u on M = sum_t sum_k |term|, with every weight at most 1."""
    rn, _, _ = R.gen(CPU, 5)
    for h in (1, 2, 7, 64):
        for lmbda in (0.0, 0.95, 1.0):
            rewards, boot = rn(9, h), rn(9, h)
            cfg = types.SimpleNamespace(discount=0.99)
            er, _ = R.td_lambda_ref(rewards.numpy(), boot.numpy(), 1.0, 0.99, lmbda)
            want = O.td_lambda(cfg, rewards, boot, lmbda)
            assert want.dtype == torch.float32
            disc = float(np.float32(0.99)) ** torch.arange(1, h + 1, dtype=torch.float64)
            r, b = rewards.abs().double() * disc, boot.abs().double() * disc
            M = sum(r[:, :t].sum(1) + b[:, t] for t in range(h))
            bound = 2 * (3 * h + 3) * R.U32 * M
            assert bool(((torch.from_numpy(er).double() - want.double()).abs() <= bound).all()), (h, lmbda)


# ------------------------------------------------------------------------------------------------ float32 passes its own bound
def ln_f32(x, g, b):
    """The kernels' LayerNorm in float32, step by step: sum * fl(1 / d), the variance of the centred values, rsqrt(var + 1e-5)."""
    inv_d = torch.tensor(1.0) / x.shape[-1]
    mean = x.sum(-1, keepdim=True) * inv_d
    c = x - mean
    rstd = torch.rsqrt((c * c).sum(-1, keepdim=True) * inv_d + 1e-5)
    return c * rstd * g + b


@pytest.mark.parametrize("regime", REGIMES)
def test_float32_layernorm_passes_its_bound(regime):
    for d, double in ((64, False), (192, True), (1024, True)):
        x, g1, b1, g2, b2 = R.ln_inputs(regime, 9, d, double, CPU, 11 + d)
        norm = R.ln_int_ref if regime == "int" else R.layernorm64
        y1 = ln_f32(x, g1, b1)
        ref, B = norm(x, g1, b1), R.ln_bound(x, g1, b1)
        if regime != "int":
            assert ratio(F.layer_norm(x, (d,), g1, b1, 1e-5), ref, B) <= 1
        if regime == "int":
            assert torch.equal(y1.double(), ref), "the int rows are not exact in float32"
        else:
            assert ratio(y1, ref, B) <= 1
        if double:
            y2 = ln_f32(y1, g2, b2)
            ref2, B2 = norm(y1, g2, b2), R.ln_bound(y1, g2, b2)
            if regime == "int":
                assert torch.equal(y2.double(), ref2) and float(y2.abs().max()) <= 24
                assert torch.equal(y2.to(torch.bfloat16).double(), ref2)
            else:
                assert ratio(y2, ref2, B2) <= 1
                assert ratio(y2.to(torch.bfloat16).float(), ref2, R.bf16_out_bound(ref2, B2)) <= 1


def test_int_layernorm_rows_have_a_power_of_two_rstd():
    for d in E.LN_D:
        x = R.ln_int_rows(33, d, CPU, d)
        m = x.mean(1, keepdim=True)
        assert torch.equal(m, m.round()) and torch.equal(((x - m) ** 2).mean(1), torch.full((33,), 256.0))
        assert float(torch.rsqrt(torch.tensor(256.0) + 1e-5)) == R.LN_INT_RSTD  # (fp32 absorbs the eps)
        inv_d = torch.tensor(1.0) / d  # the kernel's mean: sum * fl(1 / d)
        assert torch.equal(x.sum(1, keepdim=True) * inv_d, m) and torch.equal(((x - m) ** 2).sum(1) * inv_d, torch.full((33,), 256.0))


@pytest.mark.parametrize("regime", REGIMES)
def test_float32_head_out_passes_its_bound(regime):
    for d, D, mfma in ((64, 1, False), (1024, 32, False), (512, 17, True)):
        x, W, b, mean, stdv = R.head_inputs(regime, 9, d, D, CPU, 21 + d, bf16_rows=mfma)
        ref, B = R.head_out_ref(x, W, b, mean, stdv, mfma=mfma)
        if mfma:  # the kernel's split: x (bf16) times hi, then lo, accumulated in float32
            hi = W.to(torch.bfloat16).float()
            lo = (W - hi).to(torch.bfloat16).float()
            acc = x @ lo.T + x @ hi.T
        else:
            acc = x @ W.T
        y = (acc + b) * stdv + mean
        if regime == "int":
            assert torch.equal(y.double(), ref), "the int inputs are not exact in float32"
        else:
            assert ratio(y, ref, B) <= 1


@pytest.mark.parametrize("regime", REGIMES)
def test_float32_critic_passes_its_bound(regime):
    for S, A, H in ((1, 1, 64), (26, 6, 256), (32, 32, 96)):
        states, actions, om, os_, nets = R.critic_inputs(regime, 19, S, A, H, CPU, 31 + H)
        ref, B = R.critic_ref(states, actions, om, os_, nets, R.critic_n3(False, H))
        q = O.twinq(_qsd(nets, torch.float32), om, os_, states, actions)
        if regime == "int":
            assert torch.equal(q.double(), ref), "the int inputs are not exact in float32"
            assert float(ref.abs().max()) < 2 ** 24
        else:
            assert ratio(q, ref, B) <= 1


@pytest.mark.parametrize("regime", REGIMES)
def test_float32_actor_head_passes_its_bound(regime):
    for d, A, ln in ((64, 9, False), (256, 4, True), (1024, 8, True), (512, 32, False)):
        x, Wmu, bmu, Wls, bls, lnp = R.actor_inputs(regime, 9, d, A, CPU, 41 + d, ln)
        mu, Emu, sd, Esd = R.actor_ref(x, Wmu, bmu, Wls, bls, lnp, norm=R.ln_int_ref if regime == "int" else R.layernorm64)
        xn = ln_f32(x, lnp[0], lnp[1]) if ln else x
        m32 = F.linear(xn, Wmu, bmu)
        s32 = torch.exp(-5.0 + 3.5 * (torch.tanh(F.linear(xn, Wls, bls)) + 1.0))
        if regime == "int":
            assert torch.equal(m32.double(), mu), "the int inputs are not exact in float32"
        else:
            assert ratio(m32, mu, Emu) <= 1
        assert ratio(s32, sd, Esd) <= 1


def test_float32_embed_row_passes_its_bound():
    rn, _, _ = R.gen(CPU, 51)
    x, WT, Et = rn(9, 32), rn(32, 320), rn(9, 320)
    ref, B = R.embed_ref(x, WT, Et)
    assert ratio(x @ WT + Et, ref, B) <= 1


def test_bit_for_bit_restatements_are_the_operations():
    """The float32 restatements against the same operations in float64, within their own roundings (counted beside each bound)."""
    rng = np.random.default_rng(0)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    d64 = lambda a: a.astype(np.float64)
    T, A, idx, n = 6, 3, 2, 5
    hist, loc, sd, eps = np.tanh(f(T, A)), f(T, A), np.abs(f(T, A)) + 0.1, f(n + 2, T, A)
    tanh_r = lambda x: np.tanh(d64(x)).astype(np.float32)  # (a float64 tanh rounded once: within u |tanh| of the function)
    cand, sa = R.sample_ref(hist, loc, sd, eps, 0, T, A, idx, T - idx, 1, n, tanh=tanh_r)
    assert np.array_equal(cand[:, :idx], np.broadcast_to(hist[:idx], (n, idx, A)))
    prod = d64(sd[idx:]) * d64(eps[1:n + 1, idx:])
    arg = d64(loc[idx:]) + prod
    # the product and the sum round once each (the argument moves by u |sd e| + u |arg|, |tanh'| <= 1), the result once (u |tanh| <= u)
    bound = R.U32 * (np.abs(prod) + np.abs(arg)) * (1 + R.U32) + R.U32
    assert (np.abs(cand[:, idx:] - np.tanh(arg)) <= bound).all() and np.array_equal(sa, cand[:, idx:])
    mean, stdv = f(17), np.abs(f(17)) + 0.5
    x = f(4, 7, 17)
    tk = R.tokenize_ref(x, mean, stdv, True)
    # x - mean, / stdv, * stdv round once each on x - mean (3 u |x - mean|), + mean once on the result (u |x|); second order in (1 + 4 u)
    bound = R.U32 * (3 * np.abs(d64(x) - d64(mean)) + np.abs(d64(x))) * (1 + 4 * R.U32)
    assert (np.abs(d64(R.detokenize_ref(tk, mean, stdv, True)) - d64(x)) <= bound).all()
    assert np.array_equal(R.tokenize_ref(x.astype(np.float64), mean, stdv, False), x)
    p, out = R.overlay_ref(tk, x, 7, 2, mean, stdv, True)
    assert np.array_equal(out[:, [3, 6]], x[:, [3, 6]]) and np.array_equal(out[:, [0, 1, 2, 4, 5]], p[:, [0, 1, 2, 4, 5]])
    pq = f(4, 7, 17)  # (two rows more than the five overlay rows: unused)
    out = R.overlay_rows_ref(pq, x, 7, 2)
    assert np.array_equal(out[:, [0, 1, 2, 4, 5]], pq[:, :5]) and np.array_equal(out[:, [3, 6]], x[:, [3, 6]])
    g = R.gather_ref(f(2, 3, 64), np.zeros((2, 64), np.float32), [1, -2])
    assert g.shape == (2, 2, 64) and not g[:, 1].any()


# ------------------------------------------------------------------------------------------------ critic_pack
@pytest.mark.parametrize("hidden,SA", [(64, 2), (128, 23), (256, 32), (64, 32)])
def test_critic_pack_layout(hidden, SA):
    lib = E.lab()
    fp = C.POINTER(C.c_float)
    n1, n2 = E.ll(), E.ll()
    assert lib.m3pc_debug_critic_pack(None, None, SA, hidden, None, None, C.byref(n1), C.byref(n2)) == 0
    NT, NG = hidden // 32, hidden // 8
    assert n1.value == NT * 4 * 256 and n2.value == NT * NG * 256 + 1024
    W1 = np.arange(1, hidden * SA + 1, dtype=np.float32)  # (every element its own value: a wrong index shows)
    W2 = -np.arange(1, hidden * hidden + 1, dtype=np.float32)
    w1f, w2f = np.full(n1.value, np.nan, np.float32), np.full(n2.value, np.nan, np.float32)
    p = lambda a: a.ctypes.data_as(fp)
    assert lib.m3pc_debug_critic_pack(p(W1), p(W2), SA, hidden, p(w1f), p(w2f), None, None) == 0, lib.m3pc_last_error()
    i1, i2 = R.critic_pack_index(hidden, SA)
    assert np.array_equal(w1f, np.where(i1 >= 0, W1[np.maximum(i1, 0)], np.float32(0)))
    assert np.array_equal(w2f[:len(i2)], W2[i2]) and not w2f[len(i2):].any() and len(w2f) - len(i2) == 1024
    for bad in ((0, hidden), (33, hidden), (SA, 96), (SA, 32)):
        assert lib.m3pc_debug_critic_pack(p(W1), p(W2), bad[0], bad[1], p(w1f), p(w2f), None, None) != 0


# ------------------------------------------------------------------------------------------------ refusals
A16 = 0x10000000  # fake, 16-byte aligned addresses: a refused call never follows them


def _ptrs(a, names, step=0x100000):
    for i, n in enumerate(names):
        setattr(a, n, A16 + i * step)


def _ln():
    a = E.LnArgs()
    _ptrs(a, ("X", "g1", "b1", "Yf", "Yb"))
    a.ldx, a.rows, a.d = 512, 5, 512
    return a


def _head():
    a = E.HeadArgs()
    _ptrs(a, ("X", "W", "b", "Y"))
    a.ldx, a.rows, a.d, a.D, a.ldy = 512, 4096, 512, 17, 17
    return a


def _actor():
    a = E.ActorArgs()
    _ptrs(a, ("X", "Wmu", "bmu", "Wls", "bls", "mu", "sd"))
    a.ldx, a.rows, a.d, a.A = 512, 5, 512, 4
    return a


def _critic():
    a = E.CriticArgs()
    _ptrs(a, ("states", "actions", "om", "os", "q"))
    for i, n in enumerate(("W1", "b1", "W2", "b2", "W3", "b3")):
        setattr(a, n, (E.vp * 2)(A16 * 2 + i * 0x1000, A16 * 3 + i * 0x1000))
    a.rows, a.S, a.A, a.hidden = 5, 17, 6, 256
    return a


def _sample():
    a = E.SampleArgs()
    _ptrs(a, ("hist_actions", "loc", "sd", "eps", "cand"))
    a.mode, a.T, a.A, a.idx, a.h, a.n_begin, a.n_count, a.eps_rows, a.hist_windows = 0, 8, 3, 2, 6, 0, 16, 16, 1
    return a


def _score():
    a = E.ScoreArgs()
    _ptrs(a, ("rewards", "boot", "expect_return"))
    a.n, a.h, a.boot_scale, a.gamma, a.lmbda = 5, 4, 1.0, 0.99, 0.6
    return a


_SRC = (C.c_int * 3)(1, -2, 0)


def _gather():
    a = E.GatherArgs()
    _ptrs(a, ("Xe", "table", "out"))
    a.rowsrc, a.xe_bstride, a.rows_per_batch, a.batch, a.d, a.xe_rows, a.table_rows = C.cast(_SRC, E.vp), 2 * 512, 3, 2, 512, 2, 2
    return a


def _embed():
    a = E.EmbedArgs()
    a.tokmap, a.X, a.batch, a.L, a.d, a.T = A16, A16 * 2, 2, 3, 320, 4
    return a


REFUSALS = [
    ("m3pc_debug_layernorm", _ln, [("d % 64", {"d": 96, "ldx": 96}), ("d > 1024", {"d": 1088, "ldx": 1088}), ("d < 64", {"d": 0}), ("ldx < d", {"ldx": 508}),
                                   ("rows < 1", {"rows": 0}), ("no output", {"Yf": None, "Yb": None}), ("g2 alone", {"g2": A16}), ("null g1", {"g1": None}),
                                   ("X off 16 bytes", {"X": A16 + 4}), ("Yf off 16 bytes", {"Yf": A16 + 8}), ("Yb off 8 bytes", {"Yb": A16 + 4}),
                                   ("g2 off 16 bytes", {"g2": A16 + 4, "b2": A16}), ("row map", {"xmap": (3, 2, 0)}), ("row map offset", {"xmap": (3, 5, -1)})]),
    ("m3pc_debug_head_out", _head, [("d % 64", {"d": 500, "ldx": 500}), ("d > 1024", {"d": 2048, "ldx": 2048}), ("D > 32", {"D": 33, "ldy": 33}), ("D < 1", {"D": 0}),
                                    ("ldx < d", {"ldx": 256}), ("ldy < D", {"ldy": 16}), ("mean alone", {"mean": A16}), ("rows < 1", {"rows": 0}),
                                    ("bf16 rows alone below 2048 rows", {"X": None, "Xb": A16, "rows": 2047}), ("bf16 rows alone at d 256", {"X": None, "Xb": A16, "d": 256, "ldx": 256}),
                                    ("Xb off 16 bytes", {"Xb": A16 + 2}), ("bf16 ldx % 8", {"Xb": A16, "ldx": 516}), ("no rows", {"X": None}), ("row map", {"ymap": (-1, 0, 0)})]),
    ("m3pc_debug_actor_head", _actor, [("d % 64", {"d": 100, "ldx": 100}), ("d > 1024", {"d": 1280, "ldx": 1280}), ("A < 1", {"A": 0}), ("A > 32", {"A": 33}),
                                       ("ldx < d", {"ldx": 256}), ("ln_g alone", {"ln_g": A16}), ("ln at A 9", {"A": 9, "ln_g": A16, "ln_b": A16}),
                                       ("ln at d 192", {"d": 192, "ldx": 192, "ln_g": A16, "ln_b": A16}), ("X off 16 bytes", {"X": A16 + 4}),
                                       ("Wls off 16 bytes", {"Wls": A16 + 8}), ("ldx % 4", {"ldx": 514}), ("null mu", {"mu": None}), ("rows < 1", {"rows": 0})]),
    ("m3pc_debug_critic", _critic, [("S > 32", {"S": 33}), ("A > 32", {"A": 33}), ("S < 1", {"S": 0}), ("hidden > 256", {"hidden": 288}), ("hidden < 1", {"hidden": 0}),
                                    ("rows < 1", {"rows": 0}), ("null q", {"q": None}), ("null W2 of network 1", {"W2": (A16, None)}),
                                    ("b1 off 16 bytes", {"b1": (A16 + 4, A16)}), ("W3 off 16 bytes", {"W3": (A16, A16 + 8)})]),
    ("m3pc_debug_sample", _sample, [("mode", {"mode": 3}), ("idx > T", {"idx": 9}), ("idx < 0", {"idx": -1}), ("h < T - idx", {"h": 5}), ("A < 1", {"A": 0}),
                                    ("n_count < 1", {"n_count": 0}), ("rows outside eps", {"n_begin": 1}), ("null cand", {"cand": None}), ("null eps", {"eps": None}),
                                    ("idx > 0 without history", {"hist_actions": None}), ("mode 0 without sd", {"sd": None}), ("mode 1 without loc", {"mode": 1, "loc": None}),
                                    ("windows without widx", {"hist_windows": 2})]),
    ("m3pc_debug_score", _score, [("n < 1", {"n": 0}), ("h < 1", {"h": 0}), ("null boot", {"boot": None}), ("scatter_out without its index", {"scatter_out": A16})]),
    ("m3pc_debug_gather_rows", _gather, [("d % 64", {"d": 100}), ("d > 1024", {"d": 2048}), ("no output", {"out": None}), ("own row outside Xe", {"xe_rows": 1}),
                                         ("table row outside the table", {"table_rows": 1}), ("table row without a table", {"table": None}),
                                         ("xe_bstride % 4", {"xe_bstride": 1026}), ("xe_bstride below xe_rows d", {"xe_bstride": 512}), ("out off 16 bytes", {"out": A16 + 4}), ("batch < 1", {"batch": 0})]),
    ("m3pc_debug_embed", _embed, [("d % 64", {"d": 100}), ("d > 1024", {"d": 1088}), ("d < 64", {"d": 0}), ("Xb at d 320", {"X": None, "Xb": A16}),
                                  ("n_indep at d 320", {"n_indep": 1}), ("x_first_only at d 192", {"d": 192, "x_first_only": 1}),
                                  ("n_sh at d 960", {"d": 960, "n_indep": 2, "n_sh": 1, "ln_g": A16, "ln_b": A16, "Hb": A16, "Hb_sh": A16}),
                                  ("x_compact at d 64", {"d": 64, "x_compact": 1})]),
]


@pytest.mark.parametrize("fn,base,edits", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_hooks_refuse_before_they_launch(fn, base, edits):
    """Every edit of an acceptable argument structure is refused with M3PC_EINVAL and `picked` 0.  The pointers are fake: a call that
    got past its checks would fault, so a pass also shows that nothing was launched."""
    lib = E.lab()
    for what, edit in edits:
        a = base()
        for k, v in edit.items():
            setattr(a, k, (type(getattr(a, k)))(*v) if isinstance(v, tuple) else v)
        picked = (E.ci * 1)(-1)
        if hasattr(a, "picked"):
            a.picked = C.cast(picked, E.pi)
        rc = getattr(lib, fn)(C.byref(a))
        assert rc == EINVAL, (fn, what, rc)
        assert lib.m3pc_last_error(), (fn, what)
        if hasattr(a, "picked"):
            assert picked[0] == 0, (fn, what, picked[0])


def test_embed_ex_refuses_before_it_launches():
    """m3pc_debug_embed_ex: m3pc_debug_embed's refusals, and Hf without the norm's vectors, with n_sh, or off 16 bytes."""
    lib = E.lab()

    def run(d=512, **kw):
        ex = E.EmbedExArgs()
        ex.base.tokmap, ex.base.X, ex.base.batch, ex.base.L, ex.base.d, ex.base.T = A16, A16 * 2, 2, 3, d, 4
        picked = (E.ci * 1)(-1)
        ex.picked = C.cast(picked, E.pi)
        for k, v in kw.items():
            setattr(ex if k == "Hf" else ex.base, k, v)
        return lib.m3pc_debug_embed_ex(C.byref(ex)), picked[0]

    for what, kw in (("Hf without ln_g", dict(Hf=A16)), ("Hf off 16 bytes", dict(Hf=A16 + 4, ln_g=A16, ln_b=A16)),
                     ("Hf with n_sh", dict(Hf=A16, ln_g=A16, ln_b=A16, n_indep=2, n_sh=1, Hb=A16, Hb_sh=A16)),
                     ("d % 64", dict(d=100)), ("Xb at d 320", dict(d=320, X=None, Xb=A16))):
        assert run(**kw) == (EINVAL, 0), what


def test_overlay_hooks_refuse_before_they_launch():
    lib = E.lab()
    picked = (E.ci * 1)(-1)
    ok = dict(pred=A16, sin=A16 * 2, out=A16 * 3, windows=4, T=7, D=17, idx=2)
    for what, edit in (("null pred", {"pred": None}), ("windows < 1", {"windows": 0}), ("T < 1", {"T": 0}), ("D < 1", {"D": 0}), ("idx < 0", {"idx": -1}),
                       ("idx > T - 1", {"idx": 7})):
        k = dict(ok, **edit)
        assert lib.m3pc_debug_goal_overlay(k["pred"], k["sin"], k["out"], k["windows"], k["T"], k["D"], k["idx"], A16, A16, 1, None, picked) == EINVAL, what
        assert lib.m3pc_debug_goal_overlay_rows(k["pred"], k["sin"], k["out"], k["windows"], k["T"], k["D"], k["idx"], 7, None, picked) == EINVAL, what
        assert picked[0] == 0
    assert lib.m3pc_debug_goal_overlay(A16, A16 * 2, A16 * 3, 4, 7, 17, 2, None, A16, 1, None, picked) == EINVAL  # normalize without mean
    assert lib.m3pc_debug_goal_overlay_rows(A16, A16 * 2, A16 * 3, 4, 7, 17, 2, 4, None, picked) == EINVAL  # 5 overlay rows, nq 4


def test_case_table_matches_the_header():
    want = E.header_ids()
    assert set(want) == set(range(1, 28)) and E.case_ids() == set(want)
    assert want[10] == "layernorm_rows_kernel<2, 2>" and want[14] == "head_out_mfma_kernel" and want[22] == "critic_mfma_kernel<8>"
    # the named pair of the LayerNorm dispatch: 8192 rows of d = 512 take the rows kernel, 8191 do not
    assert E.ln_kernel(512, 512, 8192) == 10 and E.ln_kernel(512, 512, 8191) == 8 and E.ln_kernel(512, 513, 8192) == 7
    names = [c["name"] for cs in (E.LN_CASES, E.HEAD_CASES, E.CRITIC_CASES, E.ACTOR_CASES, E.EMBED_CASES, E.SAMPLE_CASES, E.OVERLAY_CASES) for c in cs]
    assert len(names) == len(set(names))
