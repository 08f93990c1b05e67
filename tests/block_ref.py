"""Float64 restatement of the fused layer tail and of the fused decoder input (m3pc_amd/csrc/block_fused.hip, BlockP / SplitReduceP /
KvFusedP in csrc/kernels.h; hooks m3pc_debug_block_ex / m3pc_debug_kv_fused_ex of include/m3pc_hip_debug.h), the input regimes the
kernel-level tests run, and the checks both tests/test_block_edges_gpu.py (the kernels) and tests/test_block_ref_cpu.py (an fp32 torch
restatement with seeded bugs) apply.

What a launch computes, for logical row r < M (d = 512, ff = 2048; bf16 operands, fp32 accumulation):

    R[r]  = res[r]                                    res_L > 0: res[r % res_L] when r % res_L < res_nshared (the shared leading rows
                                                      of a sequence are stored once, in sequence 0)
          | rowtab[w], w = r % rt_mod                 w < res_nu: rowtab[rt_mod + (r / rt_mod) res_nu + w], the row's own, behind the table
    X'    = R + bo + O[r] Wo^T
    a     = bf16(LayerNorm2(X'))                      eps 1e-5, biased variance
    pre   = a W1^T + b1;  hid = bf16(gelu(pre))
    X''   = X' + b2 + hid W2^T                        -> Xout (fp32; bf16(X'') when x_bf16 -- everything behind it still takes the fp32 value)
    y     = LN_A(X'');  y = LN_B[s](y)                s = (r % out_mod) / out_grp (out_mod 0: s = 0); only when lnB is given
    Hout[hrow(r)] = bf16(y)                           hrow = s (M / out_mod) out_grp + (r / out_mod) out_grp + r % out_grp (out_mod 0: r)
    QKV[r] = bf16(bf16(LN_A(X'')) Wqkv^T + bqkv)
    head_s[i] = detok(hw2_s . gelu(Wh_s bf16(y) + hb1_s) + hb2_s)    i-th row of group s; detok(v) = v std_s + mean_s
    split: slab_0 + slab_1 + slab_2 + slab_3 = X'' (fp32 additions of fp32 partials), then the reduce's own LayerNorm(s) of the sum
    kv_fused: y = Z[map(r)] We^T + rowtab[r % rt_mod];  K|V[map(r)] = bf16(bf16(LayerNorm(y)) Wkv^T + bkv)

The regimes (make_params / make_rows):
  first   every operand in front of X'' is a small integer bf16 holds and W2 = 0: X'' = X' + b2 exactly (|sums| < 2^24), the kernel's
          Xout must EQUAL the reference.  Owns the O rows, the out-proj, bo, b2, every residual source, the row clamp, the store mapping,
          the split slabs and their sum.
  second  as first in front of X', and every LayerNorm has gain 0 and a small-integer bias (fmaf(t, 0, b) = b for any finite t), W1,
          W2, Wqkv, Wh, hw2 are integers and b1 / hb1 make every GELU argument an integer p with 8 <= |p| <= 64: the tail's GELU
          returns p for p >= 8 and -4e-12 or -0 for p <= -8, so every output is an integer (+ 1e-8) whatever the hardware's rcp / exp2
          round to.  Held to SECOND_TOL = 2^-10; a wrong term moves an element by at least 1.  Owns FFN1 / FFN2, b1, the split form's
          stage offsets, the Q|K|V projection, bqkv, the heads and their de-tokeniser, the reduce's LayerNorm path, kv_fused's K|V.
  random  N(0, 1) rows, N(0, 1) / sqrt(fan-in) weights: X'' against the float64 chain at X_RTOL * max|X''| (two bf16 roundings sit in
          the middle of the chain: a worst-case element-wise bound through both comes out near 2 for values near 3), everything behind
          X'' stage-wise from the kernel's OWN X'' with derived bounds (ln_bound) or, where a bf16 rounding of LayerNorm rows sits in
          front of a product, the absolute tolerances QKV_TOL / HEAD_RTOL.

ln_bound extends gemm_ref.ln_bound (see its derivation there) by
  one_pass   the fused tail's LayerNorms take var = max(E[x^2] - mean^2, 0) from one pass: the fp32 sum of squares, its scaling, mean^2
             and the subtraction round relative to v + m^2 instead of v, dv = 2 |m| dm + dm^2 + (d + 4) u (v + m^2); and the centred value
             is fma(x, rstd, -mean rstd), whose second operand is rounded once: dc = dm + u |m|.
  dx         the LayerNorm is fed x + e, |e| <= dx element-wise (LN_B on the kernel's fp32 LN_A rows, which differ from the float64
             LN_A by its bound): the exact LayerNorm moves by |g| r (dx + mean dx) + |c r g| dv_in / (2 (v + eps)), dv_in = mean(2 |c| dc_in
             + dc_in^2), with r taken at the lowest variance the errors allow; the rounding terms are taken on the enlarged magnitudes."""
import torch

import gemm_ref as G
from gemm_ref import U16, U32, gelu64, layernorm64, map_rows  # noqa: F401  (re-exported)

D, FF = 512, 2048
SECOND_TOL = 2.0 ** -10
X_RTOL = 2e-3          # tests/test_block_fused_gpu.py::test_block_fused_matches_torch
QKV_TOL = 6e-2         # ...::test_block_fused_with_next_qkv
HEAD_RTOL = 3e-2       # ...::test_block_fused_with_scalar_output_heads
KV_TOL = (0.06, 4e-3)  # ...::test_kv_fused_matches_reference (max, mean)
GELU_TAIL_ERR = 2.6e-5  # the kernel comment's bound on |tail gelu - x Phi(x)|
REGIMES = ("first", "second", "random")
_C = [float(torch.tensor(c, dtype=torch.float32)) for c in (-2.3011212, -0.10677572, 0.001014263)]  # (the kernel's float literals)


def rb(t):
    """float64 -> nearest bf16 (through fp32, as the kernels round an fp32 value) -> float64."""
    return t.float().to(torch.bfloat16).double()


def half_ulp_bf16(t):
    """Half a bf16 ulp at magnitude t >= 0 (8 significant bits: 2^(floor(log2 t) - 8)): what one rounding to nearest adds to a value of at
    most that magnitude."""
    _, e = torch.frexp(t.double())  # t = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(t, dtype=torch.float64), e - 9)


def quiet_row(prm):
    """A residual row for the `first` regime that, with an all-zero O row, makes X'' = R + bo + b2 eight ones among zeros: variance 0.015,
    where eps and the variance's divisor show (a LayerNorm of N(0, 1) rows cannot tell eps 1e-5 from 1e-6)."""
    e = torch.zeros_like(prm["p"]["bo"])
    e[5::64] = 1.0
    return e - prm["p"]["bo"] - prm["p"]["b2"]


def gelu_tail_f64(x):
    """The fused tail's GELU formula in float64: x / (1 + exp2(x (C0 + C1 s + C2 s^2))), s = min(x^2, 50)."""
    s = torch.clamp(x * x, max=50.0)
    return x / (1.0 + torch.exp2(x * (_C[0] + s * (_C[1] + s * _C[2]))))


def ln_bound(x, g, b, one_pass=False, dx=None):
    """Element-wise bound on |fp32 LayerNorm(x + e) - layernorm64(x)|, |e| <= dx (module docstring)."""
    if not one_pass and dx is None:
        return G.ln_bound(x, g, b)
    x, g, b = x.double(), g.double(), b.double()
    d = x.shape[-1]
    mean = lambda t: t.mean(-1, keepdim=True)
    m = mean(x)
    c = x - m
    v = mean(c * c)
    dx = torch.zeros_like(x) if dx is None else dx.double()
    dc_in = dx + mean(dx)
    dv_in = mean(2 * c.abs() * dc_in + dc_in * dc_in)
    ax, ac, am, vv = x.abs() + dx, c.abs() + dc_in, m.abs() + mean(dx), v + dv_in
    dm = (d + 1) * U32 * mean(ax)
    if one_pass:
        dc = dm + U32 * am
        dv = 2 * am * dm + dm * dm + (d + 4) * U32 * (vv + am * am)
    else:
        dc = dm + U32 * ac
        dv = mean(2 * ac * dc) + (d + 4) * U32 * vv
    vlo = torch.clamp(v - dv_in - dv, min=0.0)
    r = torch.rsqrt(vlo + G.LN_EPS)
    dr = (dv + dv_in) / (2 * (vlo + G.LN_EPS)) + 4 * U32
    y = c * torch.rsqrt(v + G.LN_EPS) * g + b
    return g.abs() * r * (dc + dc_in) + ac * r * g.abs() * (dr + 2 * U32) + U32 * (y.abs() + g.abs() * r * dc_in)


def residual_index(M, res_L=0, res_nshared=0, rt_mod=0, res_nu=0, device="cpu"):
    """Row of `res` (rt_mod 0) or of `rowtab` that logical row r takes its residual from."""
    r = torch.arange(M, device=device)
    if rt_mod:
        w = r % rt_mod
        return torch.where(w < res_nu, rt_mod + (r // rt_mod) * res_nu + w, w)
    if res_L > 0:
        return torch.where(r % res_L < res_nshared, r % res_L, r)
    return r


def group_of(M, out_mod, out_grp, device="cpu"):
    """(sel, hrow): row group and physical Hout row of every logical row."""
    r = torch.arange(M, device=device)
    if not out_mod:
        return torch.zeros_like(r), r
    w = r % out_mod
    sel = w // out_grp
    return sel, sel * (M // out_mod) * out_grp + (r // out_mod) * out_grp + w % out_grp


def behind(X, prm, lnA=True, lnB=False, out_mod=0, out_grp=0, qkv=False, heads=False, detok=False, one_pass=True):
    """Everything behind X'' = X (float64 LayerNorms of THIS X): lnA, y (LN_B on top where asked), sel, hrow, H = bf16(y) and its bound
    Hb (the fp32 LayerNorm(s), one- or two-pass, and the bf16 rounding), qkv, heads [2 x (M / 2)]."""
    X = X.double()
    M, dev = X.shape[0], X.device
    p = prm["p"]
    out = {}
    if not lnA:
        return out
    yA = layernorm64(X, p["gA"], p["bA"])
    E = ln_bound(X, p["gA"], p["bA"], one_pass=one_pass)
    y = yA
    sel, hrow = group_of(M, out_mod, out_grp, dev)
    if lnB:
        B = prm["lnB"]
        ys = [layernorm64(yA, B[2 * s], B[2 * s + 1]) for s in range(2)]
        Es = [ln_bound(yA, B[2 * s], B[2 * s + 1], one_pass=one_pass, dx=E) for s in range(2)]
        y = torch.where(sel[:, None] == 0, ys[0], ys[1])
        E = torch.where(sel[:, None] == 0, Es[0], Es[1])
    out.update(lnA=yA, y=y, sel=sel, hrow=hrow, H=rb(y), Hb=E + half_ulp_bf16(y.abs() + E))
    if qkv:
        out["qkv"] = rb(rb(yA) @ prm["W"]["qkv"].double().T + prm["bqkv"].double())
    if heads:
        h, yb = prm["heads"], rb(y)
        out["heads"] = []
        for s in range(2):
            hid = gelu64(yb[sel == s] @ prm["W"]["h"][s].double().T + h["hb1"][s].double())
            v = hid @ h["hw2"][s].double() + h["hb2"][s].double()
            out["heads"].append(v * h["hstd"][s].double() + h["hmean"][s].double() if detok else v)
    return out


def tail_ref(prm, O, src, res_L=0, res_nshared=0, rt_mod=0, res_nu=0, x_bf16=False, **kw):
    """Every stage of the tail in float64 with the kernel's bf16 rounding points.  src: the physical residual rows (rt_mod 0) or the
    row table with the rows of their own behind it; kw: behind()'s."""
    d_ = lambda t: t.double()
    W, p = prm["W"], prm["p"]
    M = O.shape[0]
    R = d_(src)[residual_index(M, res_L, res_nshared, rt_mod, res_nu, O.device)]
    x1 = R + d_(p["bo"]) + d_(O) @ d_(W["o"]).T
    a = rb(layernorm64(x1, p["g2"], p["be2"]))
    pre = a @ d_(W["1"]).T + d_(p["b1"])
    hid = rb(gelu64(pre))
    x2 = x1 + d_(p["b2"]) + hid @ d_(W["2"]).T
    out = dict(R=R, x1=x1, a=a, pre=pre, hid=hid, x2=x2, xout=rb(x2) if x_bf16 else x2)
    out.update(behind(x2, prm, **kw))
    return out


def kv_ref(prm, Z, M, rmap, rt_mod, group, tab):
    """One group of kv_fused: y, bf16(LayerNorm(y)), K|V (bf16) and the physical rows of Z / KV."""
    prow = map_rows(rmap, M, Z.device)
    y = Z.double()[prow] @ prm["We"][group].double().T + tab.double()[torch.arange(M, device=Z.device) % rt_mod]
    ln = rb(layernorm64(y, prm["ln_g"], prm["ln_b"]))
    return dict(prow=prow, y=y, ln=ln, KV=rb(ln @ prm["Wkv"].double().T + prm["bkv"].double()))


# ------------------------------------------------------------------------------------------------ inputs
def _gen(device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=device, generator=g)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, device=device, generator=g).float()
    return rn, ri


def _gelu_args(ri, n):
    """n integers p with 8 <= |p| <= 64."""
    return ri(8, 64, n) * (2 * ri(0, 1, n) - 1)


def make_params(regime, device="cpu", seed=0):
    """Weights (float32 tensors holding bf16 values) and vectors of one regime, shared by every case: W {o, 1, 2, qkv, h}, p {bo, b1,
    b2, g2, be2, gA, bA}, lnB [g0, b0, g1, b1], bqkv, heads {hb1, hw2 (2, 512), hb2, hmean, hstd (2)}, and kv_fused's We [2], Wkv,
    ln_g, ln_b, bkv."""
    rn, ri = _gen(device, seed)
    bf = lambda t: t.to(torch.bfloat16).float()
    W = {"o": bf(rn(D, D) / D ** 0.5), "1": bf(rn(FF, D) / D ** 0.5), "2": bf(rn(D, FF) / FF ** 0.5), "qkv": bf(rn(3 * D, D) / D ** 0.5),
         "h": bf(rn(2, D, D) / D ** 0.5)}
    p = {"bo": 0.1 * rn(D), "b1": 0.1 * rn(FF), "b2": 0.1 * rn(D), "g2": 1 + 0.1 * rn(D), "be2": 0.1 * rn(D), "gA": 1 + 0.1 * rn(D),
         "bA": 0.1 * rn(D)}
    lnB = [1 + 0.1 * rn(D), 0.1 * rn(D), 1 + 0.1 * rn(D), 0.1 * rn(D)]
    bqkv = 0.1 * rn(3 * D)
    heads = {"hb1": 0.1 * rn(2, D), "hw2": rn(2, D) / D ** 0.5, "hb2": 0.1 * rn(2), "hmean": rn(2), "hstd": rn(2).abs() + 0.5}
    kv = {"We": [bf(rn(D, D) / D ** 0.5) for _ in range(2)], "Wkv": bf(rn(2 * D, D) / D ** 0.5), "ln_g": 1 + 0.1 * rn(D), "ln_b": 0.1 * rn(D),
          "bkv": 0.1 * rn(2 * D)}
    if regime in ("first", "second"):
        W["o"], p["bo"], p["b2"] = ri(-2, 2, D, D), ri(-64, 64, D), ri(-64, 64, D)
    if regime == "first":
        W["2"] = torch.zeros(D, FF, device=device)
    elif regime == "second":
        W["1"], W["2"], W["qkv"], W["h"] = ri(-2, 2, FF, D), ri(-2, 2, D, FF), ri(-2, 2, 3 * D, D), ri(-2, 2, 2, D, D)
        z = torch.zeros(D, device=device)
        p["g2"], p["be2"], p["gA"], p["bA"] = z, ri(-2, 2, D), z.clone(), ri(-2, 2, D)
        lnB = [z.clone(), ri(-2, 2, D), z.clone(), ri(-2, 2, D)]
        p["b1"] = _gelu_args(ri, FF) - W["1"] @ p["be2"]
        bqkv = ri(-64, 64, 3 * D)
        heads = {"hb1": torch.stack([_gelu_args(ri, D) - W["h"][s] @ lnB[2 * s + 1] for s in range(2)]), "hw2": ri(-2, 2, 2, D),
                 "hb2": ri(-8, 8, 2), "hmean": ri(-8, 8, 2), "hstd": torch.tensor([0.5, 0.25], device=device)}
        kv.update(Wkv=ri(-2, 2, 2 * D, D), ln_g=z.clone(), ln_b=ri(-2, 2, D), bkv=ri(-64, 64, 2 * D))
    elif regime != "random":
        raise ValueError(regime)
    return dict(regime=regime, W=W, p=p, lnB=lnB, bqkv=bqkv, heads=heads, **kv)


def make_rows(regime, M, n_src, device="cpu", seed=0, x_bf16=False):
    """O (M, 512) and n_src residual / table rows: integers in the exact regimes (O in [-4, 4], rows within +-64), N(0, 1) otherwise
    (bf16 values for O, and for the rows of a bf16 residual stream)."""
    rn, ri = _gen(device, seed)
    if regime == "random":
        O, src = rn(M, D).to(torch.bfloat16).float(), rn(n_src, D)
        return O, (src.to(torch.bfloat16).float() if x_bf16 else src)
    return ri(-4, 4, M, D), ri(-64, 64, n_src, D)


# ------------------------------------------------------------------------------------------------ checks
def _worst(err, bnd, what):
    ratio = err / bnd
    w = float(ratio.max())
    if not w <= 1:
        i = int(torch.nan_to_num(ratio, nan=float("inf")).flatten().argmax())
        n = err.shape[-1] if err.dim() > 1 else 1
        raise AssertionError(f"{what}: err / bound {w:.3g} at row {i // n} column {i % n} (err {float(err.flatten()[i]):.3g}, "
                             f"bound {float(bnd.flatten()[i]):.3g})")
    return w


def _equal(got, want, what):
    bad = ~(got.double() == want)
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        n = got.shape[-1] if got.dim() > 1 else 1
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ from the exact result, first at row {i // n} column {i % n} "
                             f"(got {float(got.flatten()[i])}, want {float(want.flatten()[i])})")


def check_tail(regime, prm, ref, out, what, x_bf16=False, one_pass=True, **kw):
    """The checks of one launch.  ref: tail_ref of its inputs; out: what the kernel (or a restatement) produced, logical rows: X (X''
    as stored: fp32, or bf16 values for x_bf16; None when the form stores none), Xown (the fp32 X'' of the same inputs, from this launch
    or its companion), H (logical rows, i.e. Hout[hrow]), QKV, heads [2].  kw: behind()'s (of this launch, or of the reduce: one_pass
    False).  Returns {stage: largest err / bound} of the random regime ('exact' counts as 0)."""
    res = {}
    def fin(t, n):
        assert bool(torch.isfinite(t).all()), f"{what}: non-finite {n} (a poisoned element was read)"
    X, Xown = out.get("X"), out["Xown"].double()
    fin(Xown, "X''")
    if regime == "first":
        _equal(Xown, ref["x2"], f"{what} X''")
        if X is not None:
            _equal(X, ref["xout"], f"{what} Xout")
    elif regime == "second":
        _worst((Xown - ref["x2"]).abs(), torch.full_like(Xown, SECOND_TOL), f"{what} X''")
        if X is not None:
            # (bf16 rows: the fp32 value is the integer itself once it is 1 or more -- its rounding must be the reference's)
            bnd = torch.where(ref["x2"].abs() < 1, SECOND_TOL, 1e-30) if x_bf16 else torch.full_like(Xown, SECOND_TOL)
            _worst((X.double() - ref["xout"]).abs(), bnd, f"{what} Xout")
    else:
        tol = X_RTOL * float(ref["x2"].abs().max())
        res["X"] = _worst((Xown - ref["x2"]).abs(), torch.full_like(Xown, tol), f"{what} X''")
        if X is not None:
            _equal(X, rb(Xown) if x_bf16 else Xown, f"{what} Xout against the fp32 X'' of the same inputs")
    # behind X'': from the reference X'' where it is exact, from the kernel's own otherwise
    own = behind(ref["x2"] if regime != "random" else Xown, prm, one_pass=one_pass, **kw)
    if out.get("H") is not None:
        H = out["H"].double()
        fin(H, "Hout")
        bnd = torch.full_like(H, SECOND_TOL) if regime == "second" else own["Hb"]
        res["H"] = _worst((H - (own["H"] if regime == "second" else own["y"])).abs(), bnd, f"{what} Hout")
    if out.get("QKV") is not None:
        Q = out["QKV"].double()
        fin(Q, "QKV")
        if regime == "second":
            _equal(Q, own["qkv"], f"{what} QKV")
        else:
            res["QKV"] = _worst((Q - own["qkv"]).abs(), torch.full_like(Q, QKV_TOL), f"{what} QKV")
    if out.get("heads") is not None:
        for s in range(2):
            got, want = out["heads"][s].double(), own["heads"][s]
            fin(got, f"head {s}")
            tol = SECOND_TOL if regime == "second" else HEAD_RTOL * max(1.0, float(want.abs().max()))
            res[f"head{s}"] = _worst((got - want).abs(), torch.full_like(got, tol), f"{what} head {s}")
    return res


def check_kv(regime, ref, got, what):
    """K|V rows of one group (logical order) against kv_ref."""
    got = got.double()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite K|V"
    if regime == "second":
        _equal(got, ref["KV"], f"{what} K|V")
        return 0.0
    err = (got - ref["KV"]).abs()
    assert float(err.mean()) <= KV_TOL[1], (what, float(err.mean()))
    return _worst(err, torch.full_like(err, KV_TOL[0]), f"{what} K|V")
