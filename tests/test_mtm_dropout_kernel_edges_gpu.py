"""Every kernel of m3pc_amd/csrc/mtm_dropout.hip at its edges, each alone through its lab hook (include/m3pc_hip_debug.h:
m3pc_debug_mtm_keep, m3pc_debug_mg_gemm_drop, m3pc_debug_mg_attention_drop, m3pc_debug_mg_drop_rows -- the launchers m3pc_mtm_grad goes
through), against the host mirror of the keep masks (tests/mtm_dropout_ref.py) and float64.

What is exact here and why: a mask is bits; the product's dropout is ONE rounded multiplication of the value the launch without
dropout stores (and one rounded addition of the residual behind it), so the expected output is computed in float32 from that launch's
own output, in the order m3pc_amd/csrc/mtm_grad.h states; the stored probabilities keep their bits and carry the mask in the sign.
What is held to a bound: O, dV, dS, dQ, dK, by the running error analysis of tests/mtm_grad_kernels_ref.py (class EV and attn_col_ref)
evaluated on the dropped operands.  test_every_dropout_kernel_has_a_case checks that the cases reach the six ids of the header's
"MTM-dropout kernel ids"."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mtm_dropout_ref as DR
import mtm_grad_kernels_ref as R
import mtm_grad_lab as ML
import mtm_loss_ref as LR
from mtm_grad_kernels_ref import EV, KID
from test_mtm_grad_kernel_edges_gpu import DEV, NAN, SENT, P, _bits, attn_inputs, nan_rows, owned, p_buffer, same, sent, third

pytestmark = pytest.mark.gpu
ci, vp, u64 = C.c_int, C.c_void_p, C.c_ulonglong
DKID = {"gemm_drop": 16, "attn_fwd_drop": 17, "attn_col_drop": 18, "attn_row_drop": 19, "drop_rows": 20, "keep": 21}
WORST, REACHED = {}, set()
SEED, DRAW = 0x1234567890ABCDEF, 2 ** 32 + 7  # (both words of the key and of the draw are in use)


class Drop(C.Structure):
    _fields_ = [("p", C.c_double), ("seed", u64), ("draw", u64), ("site", ci)]


class GemmDropArgs(C.Structure):
    _fields_ = [("g", ML.GemmArgs), ("drop", Drop)]


class AttnDropArgs(C.Structure):
    _fields_ = [("a", ML.AttnArgs), ("drop", Drop)]


class DropRowsArgs(C.Structure):
    _fields_ = [("dX", vp), ("dY", vp), ("R", ci), ("C", ci), ("drop", Drop), ("stream", vp), ("picked", ML.pi)]


@pytest.fixture(scope="module")
def lib():
    lab = ML.lab()
    for name, st in (("m3pc_debug_mg_gemm_drop", GemmDropArgs), ("m3pc_debug_mg_attention_drop", AttnDropArgs), ("m3pc_debug_mg_drop_rows", DropRowsArgs)):
        fn = getattr(lab, name)
        fn.restype, fn.argtypes = ci, [C.POINTER(st)]
    lab.m3pc_debug_mtm_keep.restype, lab.m3pc_debug_mtm_keep.argtypes = ci, [C.POINTER(Drop), ci, C.c_longlong, ci, vp, vp, ML.pi]
    return lab


def call(lib, fn, a, inner, want, what, *args):
    """Runs a hook, checks its return code and the kernel id it reports (inner: the structure that holds stream / picked)."""
    picked = (ci * 2)(-1, -1)
    st = torch.cuda.current_stream().cuda_stream
    if a is None:
        rc = getattr(lib, fn)(*args, st, C.cast(picked, ML.pi))
    else:
        inner.picked, inner.stream = C.cast(picked, ML.pi), st
        rc = getattr(lib, fn)(C.byref(a))
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a device error: nothing more is started on that device
        pytest.exit(f"{what}: {e}", returncode=3)
    if rc != 0:
        msg = lib.m3pc_last_error()
        if b"HIP" in msg or b"hip" in msg:
            pytest.exit(f"{what}: {msg}", returncode=3)
        raise AssertionError((what, msg))
    assert picked[0] == want and picked[1] == 1 << want, f"{what}: the launcher reports kernel {picked[0]} (set {picked[1]:#x}), the case is for {want}"
    REACHED.add(want)


def hold(kid, key, out, ref, bound, what):
    out, ref = out.double(), ref.double()
    assert LR.same_specials(out.cpu().numpy(), ref.cpu().numpy()), f"{what}: {key} has NaN / inf where the reference has none (or the reverse)"
    ratio = float(((out - ref).abs() / bound.expand_as(ref)).max())
    WORST[(kid, key)] = max(WORST.get((kid, key), 0.0), ratio)
    print(f"{what}: {key} err / bound {ratio:.3g}")
    assert ratio <= 1, f"{what}: {key} err / bound {ratio:.3g}"


def mirror(site, shape, p):
    return torch.from_numpy(DR.keep(SEED, DRAW, site, shape, p)).to(DEV)


def att_mirror(site, R_, C_, p, seed=SEED, draw=DRAW):
    """R_ attention rows of C_ keys: the leading rows of a (1, nh, C_, C_) site."""
    nh = -(-R_ // C_)
    return DR.keep(seed, draw, site, (1, nh, C_, C_), p).reshape(-1, C_)[:R_]


def f32(x):
    return torch.tensor(x, dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------------------------------------ the mask itself
@pytest.mark.parametrize("attention", [0, 1])
@pytest.mark.parametrize("extent", [(1, 1), (3, 5), (33, 96), (140, 64)])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_bytes_equal_the_mirror(lib, extent, attention, p):
    R_, C_ = extent
    site = 7 + 4 * attention
    buf = torch.full((R_ * C_ + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    d = Drop(p, SEED, DRAW, site)
    call(lib, "m3pc_debug_mtm_keep", None, None, DKID["keep"], f"keep {extent} {attention}", C.byref(d), attention, R_, C_, buf.data_ptr())
    want = att_mirror(site, R_, C_, p) if attention else DR.keep(SEED, DRAW, site, (R_, C_), p)
    got = buf[:R_ * C_].reshape(R_, C_).cpu().numpy()
    assert np.array_equal(got, want.astype(np.uint8)), f"{int((got != want).sum())} of {got.size} keep bytes differ from the mirror"
    assert bool((buf[R_ * C_:] == 0x5A).all()), "written beyond the extent"


def test_keep_refusals(lib):
    buf = torch.zeros(64, dtype=torch.uint8, device=DEV)
    for d, R_, C_ in ((Drop(1.0, 1, 0, 0), 4, 4), (Drop(float("nan"), 1, 0, 0), 4, 4), (Drop(0.1, 1, 0, 256), 4, 4), (Drop(0.1, 1, 0, -1), 4, 4),
                      (Drop(0.1, 1, 0, 0), 0, 4), (Drop(0.1, 1, 0, 0), 4, 0)):
        picked = (ci * 2)(7, 7)
        assert lib.m3pc_debug_mtm_keep(C.byref(d), 0, R_, C_, buf.data_ptr(), None, C.cast(picked, ML.pi)) == -1 and picked[0] == 0
    assert lib.m3pc_debug_mtm_keep(None, 0, 4, 4, buf.data_ptr(), None, None) == -1
    assert not bool(buf.any())


# ------------------------------------------------------------------------------------------------ the product's epilogue
GEMM_SHAPES = [(M, N, K) for M in (1, 31, 33, 140) for N in (3, 64, 96) for K in (16, 40)]


def gemm_run(lib, A, W, p, site, bias=None, res=None, gelu_aux=None, gelu_out=False, splitk=0, want=None):
    """C (M, N) [and gelu_out] of the product hook on contiguous operands, C with a padded ld and a guard row."""
    M, K = A.shape
    N = W.shape[0]
    ldc = N + 3
    a = GemmDropArgs()
    g = a.g
    none = (ci * 3)(0, 0, 0)
    g.A = ML.Op(A.data_ptr(), K, 1, none, 0, A.numel())
    g.B = ML.Op(W.data_ptr(), K, 1, none, 0, W.numel())
    Cb = sent(M, ldc)
    Gb = sent(M, ldc) if gelu_out else None
    pad = lambda x: None if x is None else nan_rows(x, ldc)
    resb, auxb = pad(res), pad(gelu_aux)
    g.C, g.ldc, g.c_len, g.cmap, g.M, g.N, g.K = P(Cb), ldc, Cb.numel(), none, M, N, K
    g.bias, g.res, g.gelu_aux, g.gelu_out, g.splitk = P(bias), P(resb), P(auxb), P(Gb), splitk
    a.drop = Drop(p, SEED, DRAW, site)
    before, gbefore = Cb.clone(), (None if Gb is None else Gb.clone())
    call(lib, "m3pc_debug_mg_gemm_drop", a, a.g, want if want is not None else (DKID["gemm_drop"] if p > 0 else KID["gemm"]), f"gemm {M}x{N}x{K} p {p}")
    rows = torch.arange(M, device=DEV)
    out = owned(Cb, before, rows, slice(0, N), "C")
    return out, (None if Gb is None else owned(Gb, gbefore, rows, slice(0, N), "gelu_out"))


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_epilogue_is_one_rounded_multiplication(lib, M, N, K, p):
    g = torch.Generator(device=DEV).manual_seed(1000 * M + 10 * N + K)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    A, W, bias, res, aux = rn(M, K), rn(N, K), rn(N), rn(M, N), 1.5 * rn(M, N)
    site = 4 * 9 + 3
    keep, sc = mirror(site, (M, N), p), f32(DR.scale(p))
    zero = torch.zeros((), device=DEV)
    # forward, no residual: where(keep, fl(Y scale), 0) on the Y of the same launch without dropout
    Y, _ = gemm_run(lib, A, W, 0.0, site, bias=bias)
    out, _ = gemm_run(lib, A, W, p, site, bias=bias)
    want = torch.where(keep, Y * sc, zero)
    assert torch.equal(_bits(out), _bits(want)), f"{int((out != want).sum())} elements differ"
    assert bool((out[~keep] == 0).all()) and (p != 0.5 or torch.equal(out[keep], 2 * Y[keep]))
    # with the residual: one more rounded addition, behind the mask
    out, _ = gemm_run(lib, A, W, p, site, bias=bias, res=res)
    assert torch.equal(_bits(out), _bits(want + res)), "the residual is added behind the mask"
    # with gelu_out: C stays the undropped pre-activation, the stored GELU is masked
    Y2, G0 = gemm_run(lib, A, W, 0.0, site, bias=bias, gelu_out=True)
    out, G = gemm_run(lib, A, W, p, site, bias=bias, gelu_out=True)
    assert torch.equal(_bits(Y2), _bits(Y)) and torch.equal(_bits(out), _bits(Y))
    assert torch.equal(_bits(G), _bits(torch.where(keep, G0 * sc, zero)))
    # backward form: ((acc) k) gelu'(aux); gelu'(aux) as the kernel computes it: the same epilogue on an accumulator of exactly 1
    one_a, one_w = torch.zeros(M, K, device=DEV), torch.zeros(N, K, device=DEV)
    one_a[:, 0], one_w[:, 0] = 1.0, 1.0
    gp, _ = gemm_run(lib, one_a, one_w, 0.0, site, gelu_aux=aux)
    acc, _ = gemm_run(lib, A, W, 0.0, site)
    out, _ = gemm_run(lib, A, W, p, site, gelu_aux=aux)
    assert torch.equal(_bits(out), _bits(torch.where(keep, acc * sc, zero) * gp))
    # another site, another draw: another mask
    other, _ = gemm_run(lib, A, W, p, site + 1, bias=bias)
    if M * N >= 64:
        assert not torch.equal(other == 0, ~keep) and torch.equal(other == 0, ~mirror(site + 1, (M, N), p))


def test_the_split_k_product_has_no_dropout_form(lib):
    A, W = torch.randn(40, 33, device=DEV), torch.randn(40, 31, device=DEV)  # (K = 40 rows, M = 33, N = 31: dW = A^T W)
    a = GemmDropArgs()
    g = a.g
    none = (ci * 3)(0, 0, 0)
    g.A, g.B = ML.Op(A.data_ptr(), 1, 33, none, 1, A.numel()), ML.Op(W.data_ptr(), 1, 31, none, 1, W.numel())
    Cb = sent(33, 31)
    g.C, g.ldc, g.c_len, g.cmap, g.M, g.N, g.K, g.splitk = P(Cb), 31, Cb.numel(), none, 33, 31, 40, 1
    a.drop = Drop(0.0, SEED, DRAW, 3)
    call(lib, "m3pc_debug_mg_gemm_drop", a, a.g, KID["gemm_split"], "split-k through the dropout hook, p 0")
    plain = Cb.clone()
    Cb.fill_(SENT)
    call(lib, "m3pc_debug_mg_gemm", a.g, a.g, KID["gemm_split"], "split-k through the plain hook")
    assert torch.equal(_bits(plain), _bits(Cb))
    a.drop = Drop(0.1, SEED, DRAW, 3)
    picked = (ci * 2)(7, 7)
    a.g.picked = C.cast(picked, ML.pi)
    assert lib.m3pc_debug_mg_gemm_drop(C.byref(a)) == -1 and b"split-k" in lib.m3pc_last_error() and picked[0] == 0


# ------------------------------------------------------------------------------------------------ attention
def _att_cases():
    cs = []
    for L in (1, 5, 63, 64, 65, 256):
        for hd in (8, 128):
            nh = 2 if hd == 8 else 1
            e = DR.ATT_EDGE
            edge = L == e["L"] and hd == 8
            c = dict(L=L, hd=hd, nh=nh, d=nh * hd, B=1 if L == 256 else 2, regime="randn", p=0.5 if L <= 5 else 0.1, edge=edge,
                     seed=e["seed"] if edge else SEED, draw=e["draw"] if edge else DRAW, site=e["site"] if edge else 4 * (L % 7))
            assert not edge or (c["B"], c["nh"], c["p"]) == (e["B"], e["nh"], e["p"])
            c["name"] = f"att_L{L}_hd{hd}_B{c['B']}_p{c['p']}"
            cs.append(c)
    return cs


ATT_CASES = _att_cases()


def att_args(which, c, p, QKV=None, Pb=None, O=None, dO=None, dQKV=None):
    a = AttnDropArgs()
    x = a.a
    x.which, x.QKV, x.P, x.O, x.dO, x.dQKV = which, P(QKV), P(Pb), P(O), P(dO), P(dQKV)
    x.B, x.L, x.d, x.nh, x.hd, x.scale = c["B"], c["L"], c["d"], c["nh"], c["hd"], c["hd"] ** -0.5
    a.drop = Drop(p, c["seed"], c["draw"], c["site"])
    return a


@pytest.mark.parametrize("c", ATT_CASES, ids=[c["name"] for c in ATT_CASES])
def test_attention_with_the_mask_in_the_sign_bit(lib, c):
    B, L, d, nh, p = c["B"], c["L"], c["d"], c["nh"], c["p"]
    what, scale = c["name"], c["hd"] ** -0.5
    QKV, dO = attn_inputs(c, 31 * L + d + nh)
    rows = torch.arange(B * L, device=DEV)
    qkv2, do2 = nan_rows(QKV.reshape(B * L, 3 * d), 3 * d), nan_rows(dO.reshape(B * L, d), d)
    keep_np = DR.keep(c["seed"], c["draw"], c["site"], (B, nh, L, L), p)
    keep = torch.from_numpy(keep_np).to(DEV)
    kf = keep.float() * f32(DR.scale(p))  # k, exact in float32
    run = lambda which, a, want, tag: call(lib, "m3pc_debug_mg_attention_drop", a, a.a, want, f"{what} {tag}")
    # ---- forward: the launch without dropout gives the probabilities; with it |P| keeps their bits and the sign carries the mask
    P0, n = p_buffer(torch.full((B, nh, L, L), SENT, device=DEV), SENT)
    O0 = sent(B * L, d)
    run(0, att_args(0, c, 0.0, qkv2, P0, O0), KID["attn_fwd"], "fwd p 0")
    Pb, _ = p_buffer(torch.full((B, nh, L, L), SENT, device=DEV), SENT)
    O = sent(B * L, d)
    pb, ob, qb = Pb.clone(), O.clone(), qkv2.clone()
    run(0, att_args(0, c, p, qkv2, Pb, O), DKID["attn_fwd_drop"], "fwd")
    same(qkv2, qb, what)
    assert torch.equal(_bits(Pb[n:]), _bits(pb[n:])), f"{what}: P written beyond (B, nh, L, L)"
    Pd = Pb[:n].reshape(B, nh, L, L)
    assert torch.equal(_bits(Pd.abs()), _bits(P0[:n].reshape(B, nh, L, L))), f"{what}: |P| is not the undropped probability bit for bit"
    assert torch.equal(torch.signbit(Pd), ~keep), f"{what}: the sign bits are not the mirror's dropped elements"
    Pref, EP, _, _ = R.attn_fwd_ref(QKV, nh, scale)
    Vh = R.heads(QKV[..., 2 * d:], nh)
    o = (EV(Pref, EP, Pref.float()) * EV(kf)).dot(EV(Vh), "bhij,bhje->bhie")
    Oout = owned(O, ob, rows, slice(0, d), what + " O").reshape(B, L, d)
    hold(DKID["attn_fwd_drop"], "O", Oout, R.unheads(o.v), R.unheads(o.bound()), what)
    gone = ~keep.any(-1)  # (B, nh, L): query rows with every key dropped
    if c["edge"]:
        assert bool(gone.any()) and bool(keep.all(-1).any()), "the fixture has an all-dropped and an all-kept row"
    Oh = R.heads(Oout, nh)
    assert not bool(Oh[gone].any()), f"{what}: an all-dropped row gives an exactly zero O row"
    # ---- dV = (|P| k)^T dO on the float64 softmax rounded to float32 and signed by the mask
    Pin = Pref.float()
    Psigned = torch.where(keep, Pin, -Pin)
    Pb, n = p_buffer(Psigned)
    dQKV = sent(B * L, 3 * d)
    pb, db, dob = Pb.clone(), dQKV.clone(), do2.clone()
    run(1, att_args(1, c, p, None, Pb, None, do2, dQKV), DKID["attn_col_drop"], "dV")
    same(Pb, pb, what)
    same(do2, dob, what)
    ev = R.attn_col_ref(Pin * kf, dO, nh, 1.0)  # (Pin * kf in float32 is the kernel's one rounded product: an exact operand)
    hold(DKID["attn_col_drop"], "dV", owned(dQKV, db, rows, third(d, 2), what + " dV").reshape(B, L, d), ev.v, ev.bound(), what)
    # ---- dP = (dO V^T) k, dS = |P| (dP - sum dP |P|) over P, dQ = dS K scale
    dQKV = sent(B * L, 3 * d)
    db = dQKV.clone()
    run(2, att_args(2, c, p, qkv2, Pb, None, do2, dQKV), DKID["attn_row_drop"], "row")
    same(qkv2, qb, what)
    same(do2, dob, what)
    assert torch.equal(_bits(Pb[n:]), _bits(pb[n:])), f"{what}: dS written beyond (B, nh, L, L)"
    Kh, dOh = R.heads(QKV[..., d:2 * d], nh), R.heads(dO, nh)
    dp = EV(dOh).dot(EV(Vh), "bhie,bhje->bhij") * EV(kf)
    pe = EV(Pin)
    ds = pe * (dp - (dp * pe).esum(-1, True))
    dq = ds.dot(EV(Kh), "bhij,bhje->bhie") * EV(f32(scale))
    hold(DKID["attn_row_drop"], "dS", Pb[:n].reshape(B, nh, L, L), ds.v, ds.bound(), what)
    hold(DKID["attn_row_drop"], "dQ", owned(dQKV, db, rows, third(d, 0), what + " dQ").reshape(B, L, d), R.unheads(dq.v), R.unheads(dq.bound()), what)
    # ---- dK = dS^T Q scale: the launch without dropout, whatever p says
    dsin = ds.v.float()
    Sb, n = p_buffer(dsin)
    dQKV = sent(B * L, 3 * d)
    sb, db = Sb.clone(), dQKV.clone()
    run(3, att_args(3, c, p, qkv2, Sb, None, None, dQKV), KID["attn_col"], "dK")
    same(Sb, sb, what)
    ev = R.attn_col_ref(dsin, QKV[..., :d], nh, scale)
    hold(KID["attn_col"], "dK", owned(dQKV, db, rows, third(d, 1), what + " dK").reshape(B, L, d), ev.v, ev.bound(), what)


# ------------------------------------------------------------------------------------------------ dY = dX k over rows
@pytest.mark.parametrize("extent", [(1, 1), (5, 3), (140, 64), (33, 2048)])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_drop_rows_is_exact(lib, extent, p):
    R_, C_ = extent
    n, site = R_ * C_, 4 * 2 + 1
    g = torch.Generator(device=DEV).manual_seed(R_ + C_)
    xbuf, ybuf = torch.full((n + 8,), NAN, device=DEV), torch.full((n + 8,), SENT, device=DEV)
    x = xbuf[1:1 + n]  # (a base 4 bytes off 16-byte alignment, in and out)
    x.copy_(torch.randn(n, device=DEV, generator=g))
    assert x.data_ptr() % 16 == 4
    a = DropRowsArgs(x.data_ptr(), ybuf[1:].data_ptr(), R_, C_, Drop(p, SEED, DRAW, site))
    xb = xbuf.clone()
    call(lib, "m3pc_debug_mg_drop_rows", a, a, DKID["drop_rows"], f"drop_rows {extent}")
    assert torch.equal(_bits(torch.nan_to_num(xbuf, 7.0)), _bits(torch.nan_to_num(xb, 7.0))), "the input was written"
    keep = mirror(site, (R_, C_), p)
    want = torch.where(keep, x.reshape(R_, C_) * f32(DR.scale(p)), torch.zeros((), device=DEV))
    assert torch.equal(_bits(ybuf[1:1 + n].reshape(R_, C_)), _bits(want))
    assert bool((ybuf[:1] == SENT).all()) and bool((ybuf[1 + n:] == SENT).all()), "written beyond the rows"
    # in place, as nothing forbids
    a = DropRowsArgs(x.data_ptr(), x.data_ptr(), R_, C_, Drop(p, SEED, DRAW, site))
    call(lib, "m3pc_debug_mg_drop_rows", a, a, DKID["drop_rows"], f"drop_rows {extent} in place")
    assert torch.equal(_bits(x.reshape(R_, C_)), _bits(want))
    picked = (ci * 2)(7, 7)
    a = DropRowsArgs(x.data_ptr(), x.data_ptr(), R_, C_, Drop(0.0, SEED, DRAW, site), None, C.cast(picked, ML.pi))
    assert lib.m3pc_debug_mg_drop_rows(C.byref(a)) == -1 and picked[0] == 0, "p = 0: m3pc_mtm_grad makes no such launch"


# ------------------------------------------------------------------------------------------------ closing
def test_every_dropout_kernel_has_a_case():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "m3pc_hip_debug.h")).read()
    block = hdr[hdr.index("MTM-dropout kernel ids"):hdr.index("(end of the MTM-dropout kernel ids)")]
    ids = {int(n): k for n, k in re.findall(r"(\d+) (mg_[a-z0-9_]+_kernel)", block)}
    assert ids == {v: f"mg_{k}_kernel" for k, v in DKID.items()}
    names = {**ids, KID["attn_col"]: "mg_attn_col_kernel"}
    print("\nlargest err / bound per kernel and output:")
    for (kid, key), v in sorted(WORST.items()):
        print(f"  {kid:2d} {names[kid]:24s} {key:10s} {v:.3g}")
    if REACHED:  # (run alone, this test has nothing to say)
        assert set(ids) <= REACHED, f"the cases reach {sorted(REACHED)}, the header lists {sorted(ids)}"
