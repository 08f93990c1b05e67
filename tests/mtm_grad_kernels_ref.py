"""References and bounds for the kernels of m3pc_amd/csrc/mtm_grad.hip, each alone (the hooks m3pc_debug_mg_* of
include/m3pc_hip_debug.h; tests/test_mtm_grad_kernel_edges_gpu.py).  Everything is float64 torch / numpy.  Reused as they stand:
gemm_ref.gemm_ref / bound / ln_bound / map_rows, attn_ref.attention_ref / bound / make_inputs, and TANHF_ULPS / EXPF_ULPS of
elementwise_ref.py.  The library is built with -ffp-contract=off: a product and the addition behind it round separately.

BIT FOR BIT (float32 / float64 numpy in the kernel's own order)
  embed_ref      the dot over f ascending from 0.f, every product and sum rounded to float32, then ((a + bias) + pdim) + pos
  gather_ref, scatter_ref, tokv_ref   copies; enc_rows is enc_row_token's table
  colsum_ref     rows in chunks of 64 ascending, chunks ascending, float64 sums; dy * xhat is a float32 product with
                 xhat = (x - mean) * rstd in float32; one rounding to float32 at the end

RUNNING ERROR ANALYSIS (class EV).  Where no bound of an earlier suite applies, the reference is evaluated by EV: a value carries its
float64 value v, a bound e on |fp32 value - v|, and a float32 shadow s computed by the same operations (the "float32 restatement";
tests/test_mtm_grad_kernels_ref_cpu.py holds |s - v| <= e).  With u = 2^-24 and the standard model fl(a op b) = (a op b)(1 + t),
|t| <= u, every operation propagates first-order terms AND the products of errors:
  a + b, a - b   e = (ea + eb) + u (|v| + ea + eb)
  a * b          e = (|a| eb + |b| ea + ea eb), then + u (|v| + that)
  a / b          e = (ea + |v| eb) / (|b| - eb), then + u (|v| + that)
  scale(c)       c a power of two: exact, e = |c| ea
  fn(f, lip, k)  a library function within k ulp (1 ulp <= 2 u |f|) whose derivative is at most lip on [a - ea, a + ea]:
                 e = lip ea + 2 k u (|v| + lip ea)
  esum(n terms)  added in any order by at most n roundings per term: e = sum ei + g_n (sum |vi| + sum ei), g_n = n u / (1 - n u).
                 (A lane's chain starts from 0.f, whose addition is exact, and a 64-lane butterfly adds six more: never more than n.)
  dot(einsum)    rounded products of two EVs summed like esum over the contracted extent
A final floor of 2^-126 covers results that underflow.  ulp counts: tanhf 5, expf 3 (elementwise_ref.py), erff 16 (gemm_ref.py),
log1pf 2 (the same table of the OpenCL C specification).  No bound reads a device result.

mg_gemm_kernel   acc: gemm_ref.bound(dtype 0, K, S_split) -- n = K + S_split roundings in ANY order, S_split = 4 for the split form
                 (three additions of partial tiles), so neither the order of the two products inside one MFMA nor the split-K order
                 matters.  Epilogue by EV in the kernel's order: add = bias + bias2; v = acc + add; + pos; + res; * gelu'(aux) with
                 gelu'(x) = 0.5 (1 + erff(x c)) + x (c' expf(-0.5 x x)); + C (accumulate); gelu_out = 0.5 v (1 + erff(v c)) on the
                 kernel's own v (EV carries E through the formula).  `int` regime: every
                 operand, epilogue term and partial sum is a small integer and gelu_aux is 0 or 10, where gelu' is exactly 0.5 or 1:
                 the result must EQUAL the reference (gelu_out is held to its bound: erff is not exact).
LayerNorm fwd    Y: gemm_ref.ln_bound.  st: ln_stat_bound, the dm and r dr of ln_bound's derivation (the mean: d additions in any
                 order and the division; rstd: dv / (2 (v + eps)) + 4 u relative -- here sqrtf and a division, both correctly rounded).
LayerNorm bwd    by EV from x, dy, g and the (mean, rstd) it is GIVEN (the float64 statistics rounded to float32 are its inputs).
attention fwd    O: attn_ref.bound (its budget per weight, (hd + 4) Amax u + 4 u, covers this kernel's scores: q * scale and every
                 product rounded, hd - 1 additions).  P: p ((2 hd + 8) Amax + Lk + 16) u -- a weight is off by the score's
                 (hd + 1) Amax u, the subtraction of the maximum 2 Amax u and expf's 3 ulp = 6 u; twice that (the weight and the
                 normaliser) and (Lk + 2) u for the sum and the division, rounded up -- + 2^-126 for weights that underflow.
attention col    a dot of L rounded products (EV.dot) times alpha.
attention row    by EV from the P it is given: dp, dot = sum dp p, dS = p (dp - dot), dQ = (sum dS K) scale.
mg_std_kernel    exp(-5 + 3.5 (tanh(ls) + 1)) by EV.
mg_loss_bwd_kernel  by EV at the float32 clip bounds (mtm_grad_ref.loss_total(f32_clip=True)): the action branch near |a| -> 1 is
                 ill-conditioned in a, but a is an exact input and log1pf(+-ac) is within 2 ulp of a value of size <= 14.
                 Specials (NORM_L2 of a zero target: NaN) are compared with mtm_loss_ref.same_specials; the bound holds where
                 the reference is finite."""
import math

import numpy as np
import torch

import attn_ref as AR
import gemm_ref as GM
from elementwise_ref import EXPF_ULPS, TANHF_ULPS
from gemm_ref import U32, map_rows  # noqa: F401

F = np.float32
ERFF_ULPS = 16
LOG1PF_ULPS = 2
TINY = 2.0 ** -126
C_SQRT_HALF = 0.70710678118654752440
C_INV_SQRT_2PI = 0.39894228040143267794
NORM_L2, CLIP_ACTIONS = 1, 2
KID = {"gemm": 1, "gemm_split": 2, "ln_fwd": 3, "ln_bwd": 4, "colsum": 5, "colsum_fin": 6, "attn_fwd": 7, "attn_col": 8, "attn_row": 9,
       "embed": 10, "gather": 11, "scatter": 12, "tokv": 13, "std": 14, "loss_bwd": 15}


def gam(n):
    return n * U32 / (1 - n * U32)


# ------------------------------------------------------------------------------------------------ running error analysis
class EV:
    """(v, e, s): float64 value, bound on |fp32 value - v|, float32 shadow by the same operations."""
    __slots__ = ("v", "e", "s")

    def __init__(self, v, e=None, s=None):
        if isinstance(v, EV):
            self.v, self.e, self.s = v.v, v.e, v.s
            return
        v = torch.as_tensor(v)
        if e is None and s is None:  # an input or an exact constant: what float32 holds of it
            self.s = v.to(torch.float32)
            self.v = self.s.double()
            self.e = torch.zeros_like(self.v)
        else:
            self.v, self.e, self.s = v.double(), e, (v.to(torch.float32) if s is None else s)

    @staticmethod
    def const(c):
        """A literal of the source, rounded to float32 by the compiler: the analysis is against the real number."""
        s = torch.tensor(c, dtype=torch.float32)
        return EV(torch.tensor(c, dtype=torch.float64), (s.double() - c).abs(), s)

    def _r(self, v, e0, s):
        return EV(v, e0 + U32 * (v.abs() + e0), s)

    def __add__(self, o):
        o = EV(o)
        return self._r(self.v + o.v, self.e + o.e, self.s + o.s)

    def __sub__(self, o):
        o = EV(o)
        return self._r(self.v - o.v, self.e + o.e, self.s - o.s)

    def __mul__(self, o):
        o = EV(o)
        return self._r(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e, self.s * o.s)

    def __truediv__(self, o):
        o = EV(o)
        v = self.v / o.v
        return self._r(v, (self.e + v.abs() * o.e) / (o.v.abs() - o.e).clamp_min(0.0), self.s / o.s)

    def __neg__(self):
        return EV(-self.v, self.e, -self.s)

    def scale(self, c):
        assert math.frexp(abs(c))[0] == 0.5, c
        return EV(self.v * c, self.e * abs(c), self.s * c)

    def fn(self, f, lip, ulps):
        v = f(self.v)
        e0 = lip * self.e
        return EV(v, e0 + 2 * ulps * U32 * (v.abs() + e0), f(self.s))

    def esum(self, dim, keepdim=False):
        n = self.v.shape[dim]
        se = self.e.sum(dim, keepdim)
        return EV(self.v.sum(dim, keepdim), se + gam(n) * (self.v.abs().sum(dim, keepdim) + se), self.s.sum(dim, keepdim))

    def dot(self, o, eq):
        """einsum(eq) of two EVs: rounded products, added in any order; n = the contracted extent."""
        o = EV(o)
        a, b = self.v.abs(), o.v.abs()
        es = lambda x, y: torch.einsum(eq, x, y)
        S = es(a, b)
        n = es(torch.ones_like(a), torch.ones_like(b)).max().item()
        X = es(a, o.e) + es(self.e, b) + es(self.e, o.e)
        se = X + U32 * (S + X)
        return EV(es(self.v, o.v), se + gam(n) * (S + se), es(self.s, o.s))

    def bound(self):
        return self.e + TINY


def ev_tanh(x):
    return x.fn(torch.tanh, 1.0, TANHF_ULPS)


def ev_exp(x):
    return x.fn(torch.exp, torch.exp(x.v + x.e), EXPF_ULPS)


def ev_erf(x):
    return x.fn(torch.erf, 2.0 / math.sqrt(math.pi), ERFF_ULPS)


def ev_gelu_grad(x):
    """gelu_grad_exact: cdf + x * pdf."""
    cdf = (ev_erf(x * EV.const(C_SQRT_HALF)) + 1.0).scale(0.5)
    pdf = EV.const(C_INV_SQRT_2PI) * ev_exp(x.scale(-0.5) * x)
    return cdf + x * pdf


def ev_gelu(x):
    """gelu_exact: 0.5f * x * (1.0f + erff(x * c))."""
    return x.scale(0.5) * (ev_erf(x * EV.const(C_SQRT_HALF)) + 1.0)


# ------------------------------------------------------------------------------------------------ the product
GEMM_REGIMES = ("int", "randn", "offset", "spike")
SPIKE_K2 = 16 * 3 + 15  # the last k of wavefront 3's first block in the split form


def gemm_inputs(regime, M, N, K, device="cpu", seed=0, bias=False, bias2=False, pos_T=0, res=False, gelu_aux=False, c0=False):
    """Logical A (M, K), W (N, K) = B^T and the epilogue terms the case uses.  Regimes of gemm_ref.make_inputs (fp32 operands); the
    spike regime carries a second large term at k = SPIKE_K2 where K reaches it; offset at odd K is the even K + 1 cut back.
    int: gelu_aux in {0, 10} (gelu' exactly 0.5, 1), C0 integers."""
    Ke = K + (K % 2 if regime == "offset" else 0)
    t = GM.make_inputs(regime, M, N, Ke, dtype=0, bias=bias, rt_mod=pos_T, res=res, device=device, seed=seed)
    t["A"], t["W"] = t["A"][:, :K].contiguous(), t["W"][:, :K].contiguous()
    g = torch.Generator(device=device).manual_seed(seed + 4099)
    rn = lambda *s: torch.randn(*s, device=device, generator=g)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, device=device, generator=g).float()
    if regime == "spike" and K - 1 > SPIKE_K2:
        t["A"][:, SPIKE_K2] = torch.sign(rn(M)) * 4 * K ** 0.5 * (1 + 0.1 * rn(M))
        t["W"][:, SPIKE_K2] = torch.sign(rn(N)) * (1 + 0.1 * rn(N))
    t["pos"] = t.pop("rowtab")
    integer = regime == "int"
    t["bias2"] = (ri(-64, 64, N) if integer else rn(N)) if bias2 else None
    t["gelu_aux"] = (10.0 * ri(0, 1, M, N) if integer else 1.5 * rn(M, N)) if gelu_aux else None
    t["c0"] = (ri(-64, 64, M, N) if integer else rn(M, N)) if c0 else None
    return t


def mg_gemm_ref(t, pos_T=1, splitk=False, gelu_out=False):
    """t: gemm_inputs' dict (logical tensors).  Returns C (M, N) float64, its bound E, and with gelu_out G, EG."""
    A, W = t["A"], t["W"]
    M, K = A.shape
    ref = GM.gemm_ref(A, W)
    v = EV(ref["acc"], GM.bound(ref, 0, K, S_split=4 if splitk else 1), A @ W.T)
    if t.get("bias") is not None:
        add = EV(t["bias"]) if t.get("bias2") is None else EV(t["bias"]) + EV(t["bias2"])
        v = v + add
    if t.get("pos") is not None:
        v = v + EV(t["pos"][torch.arange(M, device=A.device) % pos_T])
    if t.get("res") is not None:
        v = v + EV(t["res"])
    if t.get("gelu_aux") is not None:
        v = v * ev_gelu_grad(EV(t["gelu_aux"]))
    if t.get("c0") is not None:
        v = v + EV(t["c0"])
    out = {"C": v.v, "E": v.bound(), "C32": v.s}
    if gelu_out:
        g = ev_gelu(v)  # (the kernel's gelu reads its own v: EV carries E through the formula)
        out["G"], out["EG"], out["G32"] = g.v, g.bound(), g.s
    return out


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_stats64(x):
    x = x.double()
    m = x.mean(-1)
    c = x - m[:, None]
    v = (c * c).mean(-1)
    return m, torch.rsqrt(v + GM.LN_EPS)


def ln_stat_bound(x):
    """Bounds on the fp32 (mean, rstd) of a row: the dm and r * dr of gemm_ref.ln_bound's derivation."""
    x = x.double()
    d = x.shape[-1]
    m = x.mean(-1, keepdim=True)
    c = x - m
    v = (c * c).mean(-1, keepdim=True)
    dm = (d + 1) * U32 * x.abs().mean(-1, keepdim=True)
    dc = dm + U32 * c.abs()
    dv = (2 * c.abs() * dc).mean(-1, keepdim=True) + (d + 4) * U32 * v
    dr = dv / (2 * (v + GM.LN_EPS)) + 4 * U32
    return dm[:, 0] + TINY, (torch.rsqrt(v + GM.LN_EPS) * dr)[:, 0] + TINY


def ln_fwd32(x, g, b):
    """The float32 restatement of mg_ln_fwd_kernel (sums in torch's order)."""
    x = x.float()
    d = x.shape[-1]
    m = x.sum(-1, keepdim=True) / float(d)
    c = x - m
    r = 1.0 / torch.sqrt((c * c).sum(-1, keepdim=True) / float(d) + torch.tensor(1e-5, dtype=torch.float32))
    return c * r * g.float() + b.float(), m[:, 0], r[:, 0]


def ln_bwd_ref(x, dy, g, mean, rstd, dx0=None):
    """dx = rstd ((g' - mean(g')) - xhat mean(g' xhat)), g' = dy g, xhat = (x - mean) rstd, from the statistics GIVEN (float32
    values: inputs of the kernel); + dx0 with accumulate.  Returns an EV over (rows, d)."""
    x, dy, g = EV(x), EV(dy), EV(g)
    mean, rstd = EV(mean.reshape(-1, 1)), EV(rstd.reshape(-1, 1))
    d = float(x.v.shape[-1])
    gg = dy * g
    xh = (x - mean) * rstd
    s1 = gg.esum(-1, True) / d
    s2 = (gg * xh).esum(-1, True) / d
    v = rstd * ((gg - s1) - xh * s2)
    return v if dx0 is None else EV(dx0) + v


def ln_bwd64(x, dy, g, mean, rstd):
    x, dy, g = x.double(), dy.double(), g.double()
    gg = dy * g
    xh = (x - mean.double()[:, None]) * rstd.double()[:, None]
    return rstd.double()[:, None] * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True))


# ------------------------------------------------------------------------------------------------ column sums
def colsum_rows(nseq, L, j0, n, sel):
    """(compact row q, buffer row) of every selected (s, j), in the kernel's order."""
    return [(s * n + j, s * L + j0 + j) for s in range(nseq) for j in range(n) if (sel >> j) & 1]


def colsum_ref(dY, dy_compact, X, st, nseq, L, j0, n, sel, C):
    """float32 numpy arrays as the kernel sees them: dY (rows, ldy), X (buffer rows, C) or None, st (nseq n, 2).  Returns out0,
    out1 (float32; out1 None without X) in the kernel's order: chunks of 64 compact rows, float64 sums, one final rounding."""
    total = nseq * n
    chunks = (total + 63) // 64
    part = np.zeros((chunks, 2, C), np.float64)
    for q, br in colsum_rows(nseq, L, j0, n, sel):
        dy = dY[q if dy_compact else br, :C].astype(F)
        part[q // 64, 0] += dy.astype(np.float64)
        if X is not None:
            xh = ((X[br, :C].astype(F) - F(st[q, 0])).astype(F) * F(st[q, 1])).astype(F)
            part[q // 64, 1] += (dy * xh).astype(F).astype(np.float64)
    a = np.zeros((2, C), np.float64)
    for k in range(chunks):
        a += part[k]
    return a[0].astype(F), (a[1].astype(F) if X is not None else None)


# ------------------------------------------------------------------------------------------------ attention
def split_qkv(QKV, d):
    return QKV[..., :d], QKV[..., d:2 * d], QKV[..., 2 * d:]


def heads(x, nh):
    """(B, L, d) -> (B, nh, L, hd)"""
    B, L, d = x.shape
    return x.reshape(B, L, nh, d // nh).transpose(1, 2)


def unheads(x):
    B, nh, L, hd = x.shape
    return x.transpose(1, 2).reshape(B, L, nh * hd)


def attn_fwd_ref(QKV, nh, scale):
    """QKV (B, L, 3 d).  Returns P (B, nh, L, L), its bound, O (B, L, d), its bound (attn_ref.bound, fp32 kernels)."""
    d = QKV.shape[-1] // 3
    q, k, v = split_qkv(QKV, d)
    ref = AR.attention_ref(q, k, v, nh, scale)
    hd, Lk = d // nh, k.shape[1]
    Amax = heads(ref["Amax"], nh)[..., :1]  # (B, nh, L, 1): the same for every column of a head
    EP = ref["p"] * ((2 * hd + 8) * Amax + Lk + 16) * U32 + TINY
    return ref["p"], EP, ref["O"], AR.bound(ref, 0) + TINY


def attn_fwd32(QKV, nh, scale):
    d = QKV.shape[-1] // 3
    q, k, v = (heads(t.float(), nh) for t in split_qkv(QKV, d))
    p = torch.softmax((q * F(scale)) @ k.transpose(-1, -2), -1)
    return p, unheads(p @ v)


def attn_col_ref(Mx, Z, nh, alpha):
    """out[b, j, h, e] = alpha sum_i Mx[b, h, i, j] Z[b, i, h, e]: Mx (B, nh, L, L), Z (B, L, d).  EV over (B, L, d)."""
    out = EV(Mx).dot(EV(heads(Z, nh)), "bhij,bhie->bhje")
    out = out * EV(torch.tensor(alpha, dtype=torch.float32)) if alpha != 1.0 else out
    return EV(unheads(out.v), unheads(out.e), unheads(out.s))


def attn_row_ref(P, dO, QKV, nh, scale):
    """dS (B, nh, L, L) and dQ (B, L, d) as EV, from the P given."""
    d = QKV.shape[-1] // 3
    _, k, v = split_qkv(QKV, d)
    Kh, Vh, dOh = heads(k, nh), heads(v, nh), heads(dO, nh)
    dp = EV(dOh).dot(EV(Vh), "bhie,bhje->bhij")
    p = EV(P)
    dot = (dp * p).esum(-1, True)
    ds = p * (dp - dot)
    dq = ds.dot(EV(Kh), "bhij,bhje->bhie")
    dq = dq * EV(torch.tensor(scale, dtype=torch.float32))
    return ds, EV(unheads(dq.v), unheads(dq.e), unheads(dq.s))


def attn_bwd64(QKV, dO, nh, scale):
    """float64 dQKV (B, L, 3 d) and dS of softmax attention, written out (the CPU test holds it to autograd)."""
    d = QKV.shape[-1] // 3
    q, k, v = (heads(t.double(), nh) for t in split_qkv(QKV, d))
    dOh = heads(dO.double(), nh)
    p = torch.softmax(q @ k.transpose(-1, -2) * scale, -1)
    dv = p.transpose(-1, -2) @ dOh
    dp = dOh @ v.transpose(-1, -2)
    ds = p * (dp - (dp * p).sum(-1, keepdim=True))
    return torch.cat([unheads(ds @ k * scale), unheads(ds.transpose(-1, -2) @ q * scale), unheads(dv)], -1), ds, p


# ------------------------------------------------------------------------------------------------ token layout
def mask_bits(vis, T):
    """vis: per key the visible timesteps.  Returns bits, kept, eoff, Le."""
    bits = [sum(1 << t for t in set(v)) for v in vis]
    assert all(b >> T == 0 for b in bits)
    kept = [bin(b).count("1") for b in bits]
    eoff = [sum(kept[:k]) for k in range(4)]
    return bits, kept, eoff, sum(kept)


def enc_rows(bits, T):
    """[(key, timestep)] of encoder row j: the keys in order, the visible timesteps of each ascending."""
    return [(k, t) for k in range(4) for t in range(T) if (bits[k] >> t) & 1]


def embed_ref(tok, W, bias, pdim, pos, bits, B, T, d):
    """numpy float32: tok[k] (B, T, F_k), W[k] (d, F_k), bias[k] / pdim[k] (d), pos (T, d).  X (B, Le, d), bit for bit."""
    rows = enc_rows(bits, T)
    X = np.zeros((B, len(rows), d), F)
    for j, (k, t) in enumerate(rows):
        a = np.zeros((B, d), F)
        for f in range(W[k].shape[1]):
            a = (a + (tok[k][:, t, f][:, None] * W[k][None, :, f]).astype(F)).astype(F)
        X[:, j] = (((a + bias[k][None]).astype(F) + pdim[k][None]).astype(F) + pos[t][None]).astype(F)
    return X


def gather_ref(src, mtok, bits, B, T, d):
    """src (B, Le, d) -> dst (B, 4 T, d): the encoder row of a visible token, the key's mask token of a hidden one."""
    dst = np.zeros((B, 4 * T, d), F)
    for k in range(4):
        dst[:, k * T:(k + 1) * T] = mtok[k][None, None]
    for j, (k, t) in enumerate(enc_rows(bits, T)):
        dst[:, k * T + t] = src[:, j]
    return dst


def scatter_ref(src, bits, B, T, d):
    """src (B, 4 T, d) -> dst (B, Le, d)."""
    rows = enc_rows(bits, T)
    return np.stack([src[:, k * T + t] for k, t in rows], 1) if rows else np.zeros((B, 0, d), F)


def tokv_ref(tok_k, bits_k, T):
    """tok_k (B, T, F) -> (B kept, F): the visible rows, compact."""
    ts = [t for t in range(T) if (bits_k >> t) & 1]
    return tok_k[:, ts].reshape(-1, tok_k.shape[-1])


# ------------------------------------------------------------------------------------------------ std, the loss backward
def std_ref(ls):
    """exp(-5 + 3.5 (tanh(ls) + 1)) as EV."""
    return ev_exp((ev_tanh(EV(ls)) + 1.0) * 3.5 + (-5.0))


def loss_bwd_ref(pred, mu, sd, ls, tgt, eps, mask, batch, T, S, A, flags, loss_keys, entropy_reg, inv_cnt):
    """pred: [states (B T, S), rewards (B T, 1), returns (B T, 1)], tgt: the four keys' token rows, mask: four bit sets; all float32
    torch tensors of (B T, width).  inv_cnt: the float32 value the kernel is given.  Returns dpred (three EV), dmu, dls (EV)."""
    rows = batch * T
    dev = mu.device
    dpred = []
    for j, k in enumerate((0, 2, 3)):
        D = S if j == 0 else 1
        if not (loss_keys >> k) & 1:
            z = torch.zeros(rows, D, device=dev)
            dpred.append(EV(z))
            continue
        tv = EV(tgt[k])
        if flags & NORM_L2:
            sq = EV(tgt[k]) * EV(tgt[k])                       # float32 products
            n2 = EV(sq.v.sum(-1, keepdim=True), sq.e.sum(-1, keepdim=True), sq.s.double().sum(-1, keepdim=True).float())  # float64 sum
            n2 = EV(n2.v, n2.e + U32 * (n2.v.abs() + n2.e), n2.s)                                                        # (float)n2
            root = n2.fn(torch.sqrt, 0.5 / torch.sqrt((n2.v - n2.e).clamp_min(TINY)), 0.5)                              # sqrtf: correctly rounded
            tv = tv / root
        g = ((EV(pred[j]) - tv).scale(2.0)) / EV(torch.tensor(float(rows * D), dtype=torch.float32))
        dpred.append(g)
    t_of_row = torch.arange(rows, device=dev) % T
    vis = torch.tensor([(mask[1] >> t) & 1 for t in range(T)], dtype=torch.bool, device=dev)[t_of_row][:, None].expand(rows, A)
    a = tgt[1]
    # visible
    th = ev_tanh(EV(mu))
    one = 1.0
    gv = ((th - EV(a)).scale(2.0) * (-(th * th) + one)) / EV(torch.tensor(float(rows * A), dtype=torch.float32))
    if not (loss_keys >> 1) & 1:
        gv = EV(torch.zeros(rows, A, device=dev))
    # hidden
    ac = a
    if flags & CLIP_ACTIONS:
        lo, hi = F(-1.0 + 1e-6), F(1.0 - 1e-6)
        ac = torch.where(torch.isnan(a), a, a.clamp(float(lo), float(hi)))
    l1 = EV(ac).fn(torch.log1p, 1.0, LOG1PF_ULPS)   # (ac is exact: the Lipschitz factor multiplies a zero error)
    l2 = EV(-ac).fn(torch.log1p, 1.0, LOG1PF_ULPS)
    z = (l1 - l2).scale(0.5)
    sdv, epsv, muv = EV(sd), EV(eps), EV(mu)
    dz = z - muv
    var = sdv * sdv
    thu = ev_tanh(muv + epsv * sdv)
    er = EV(torch.tensor(entropy_reg, dtype=torch.float32))
    ic = EV(torch.tensor(inv_cnt, dtype=torch.float32))
    inv_sd = EV(torch.ones((), device=dev)) / sdv
    dmu_h = ((er.scale(2.0) * thu) - dz / var) * ic
    dsd_h = (er * ((thu.scale(2.0) * epsv) - inv_sd) - ((dz * dz) / (var * sdv) - inv_sd)) * ic
    pick = lambda m, x, y: EV(torch.where(m, x.v, y.v), torch.where(m, x.e, y.e), torch.where(m, x.s, y.s))
    zero = EV(torch.zeros(rows, A, device=dev))
    dmu = pick(vis, gv, dmu_h)
    dsd = pick(vis, zero, dsd_h)
    tl = ev_tanh(EV(ls))
    dls = ((dsd * sdv) * 3.5) * (-(tl * tl) + one)
    return dpred, dmu, dls


def loss_inputs(B, T, S, A, seed, clip):
    """As tests/test_mtm_loss_kernel_gpu.py::_inputs: ls across saturation at both ends, |mu| to 8, target actions exactly +-1 at a
    hidden and a visible timestep with the clip (strictly inside without)."""
    rng = np.random.RandomState(1000 * seed + 7 * B + T + S)
    f = lambda *sh: torch.from_numpy(rng.normal(size=sh).astype(F))
    mu = rng.uniform(-8, 8, size=(B * T, A)).astype(F)
    ls = rng.uniform(-4, 4, size=(B * T, A)).astype(F)
    act = rng.uniform(-0.95, 0.95, size=(B * T, A)).astype(F)
    mu[0, 0], mu[T - 1, 0], mu[-1, -1] = 8.0, -8.0, 8.0
    ls[0, 0], ls[T - 1, 0], ls[-1, -1] = -20.0, 20.0, -20.0
    ls[-T // 2, -1] = 20.0
    if clip:
        act[0, 0], act[T - 1, 0], act[-T, -1], act[-1, -1] = 1.0, -1.0, -1.0, 1.0
    pred = [f(B * T, S), f(B * T, 1), f(B * T, 1)]
    tgt = [f(B * T, S), torch.from_numpy(act), f(B * T, 1), f(B * T, 1)]
    return pred, torch.from_numpy(mu), torch.from_numpy(ls), tgt, f(B * T, A)


def loss_masks(T, seed, all_visible=False):
    rng = np.random.RandomState(seed + T)
    bits = []
    for k in range(4):
        m = (rng.uniform(size=T) < 0.5).astype(np.uint8)
        m[0], m[T - 1] = 1, 0                       # (T == 1: the one timestep is hidden)
        bits.append(sum(int(v) << t for t, v in enumerate(m)))
    if all_visible:
        bits[1] = (1 << T) - 1
    return bits


def loss_total64(pred, mu, ls, tgt, eps, mask, batch, T, S, A, flags, loss_keys, entropy_reg):
    """The float64 total of the header from the head outputs (mtm_grad_ref.loss_total at the float32 clip bounds), for autograd."""
    import mtm_grad_ref as GR
    sd = torch.exp(-5.0 + 3.5 * (torch.tanh(ls) + 1.0))
    sh = lambda x, D: x.reshape(batch, T, 1, D)
    out = {"states": sh(pred[0], S), "rewards": sh(pred[1], 1), "returns": sh(pred[2], 1), "actions": (sh(mu, A), sh(sd, A))}
    tokens = {"states": sh(tgt[0], S), "actions": sh(tgt[1], A), "rewards": sh(tgt[2], 1), "returns": sh(tgt[3], 1)}
    masks = {k: np.array([(mask[i] >> t) & 1 for t in range(T)], np.float64) for i, k in enumerate(GR.KEYS)}
    total, _ = GR.loss_total(out, tokens, masks, eps.reshape(batch, T, A), entropy_reg, flags, loss_keys, torch.float64, True)
    return total
