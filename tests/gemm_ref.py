"""Float64 restatement of the library's GEMM (m3pc_debug_gemm_ex, include/m3pc_hip_debug.h) and an element-wise bound on what the
fp32, bf16 and split-bf16 kernels may differ from it.

What the hook computes, for logical row r < M and column c < N (a row map {rpg, gstride, off} sends r to the physical row
(r / rpg) gstride + r % rpg + off; rpg 0 is the identity):

    a    = A[amap(r)]                               (a_ln_*: LayerNorm of that row first, eps 1e-5, biased variance)
    acc  = sum_k a_k W[c, k]
    pre  = acc + bias[c] + rowtab[r % rt_mod, c]
    v    = gelu(pre)                                 (exact-erf GELU; without gelu v = pre)
    C[cmap(r), c] = v + res[cmap(r), c]
    ln_out[r] = LayerNorm(C row)                     (optional, fp32 output only)

The bound, per output element, with u = 2^-24 (fp32 unit roundoff), u16 = 2^-8 (bf16), S = sum_k |a_k W_ck|.  Every term is a
rounding point that can be read off the kernels (gemm.hip, gemm_x3.hip, gemm_glds.hip, gemm_big.hip, gemm_line.hip,
gemm_f32_direct.hip, gemm_epilogue.h); each later term is taken on |reference value| + the error so far:

  accumulation   E0 = n u S / (1 - n u)
      bf16 operands: products are exact in fp32, n = K + S_split fp32 additions in any order (S_split: the slabs of a split-K
      launch, or the 16 K slices of the few-row kernel; 1 otherwise).  fp32 operands: v_mfma_f32_32x32x2_f32 is a chain of
      fmas, one rounding each: the same count.  (The multi-term adder inside a bf16 MFMA is taken to round no worse than the
      chain of fp32 additions it replaces.)
      split-bf16 (dtype 2): a = a_hi + a_lo + da with |a_lo| <= u16 |a|, |da| <= u16^2 |a|, the same for w, and the kernel sums
      a_hi w_hi + a_hi w_lo + a_lo w_hi = a w - (a dw + w da - da dw) - a_lo w_lo: at most (3 u16^2 + u16^4) |a w| per product,
      and n = 3 K + S_split additions of terms whose absolute sum is at most (1 + u16)^2 S.
      a_ln_*: the fp32 LayerNorm of the operand row moves a_k by at most ln_bound(row)_k; E0 gains sum_k ln_bound_k |W_ck|.
  bias, rowtab   one fp32 rounding of the result each: E += u (|value| + E)
  GELU           E = L E + G(pre) with L = 1.13 >= max |gelu'| (1.1289 at x = sqrt 2) and G the error of the kernel's formula
      fp32 / split-bf16 operands (0.5 x (1 + erff(x / sqrt 2))): G = 12 u |x| -- erff within 16 ulp (the OpenCL bound; <= 16 u on
      |erf| <= 1, times |x| / 2), the rounded argument 0.24 u |x|, the rounding of 1 + erf u |x|, two multiplications 2 u |x|.
      bf16 operands (gelu_fast: Abramowitz-Stegun 7.1.26 on v_rcp_f32 and v_exp_f32):
      G = |x| / 2 (AS_ERR + 16 u) + u |gelu(x)| -- AS_ERR = 1.5e-7 is the polynomial's stated error on erf (gelu_fast_f64 over
      gelu_grid(): 1.4e-7 measured, see test_gemm_ref_cpu.py::test_gelu_fast_formula_error), and 16 u is the stated allowance for
      what a CPU cannot measure: 1 ulp each for the hardware rcp and exp2, the rounded exponent argument (<= 0.37 * 3 u on p e)
      and the five fp32 roundings of the polynomial, all on values <= 1.
  residual       one fp32 rounding: E += u (|value| + E)
  bf16 output    one rounding to nearest even: E += u16 (|value| + E)

LayerNorm (ln_bound: ln_out is held to it against the float64 LayerNorm of the kernel's OWN fp32 C, a_ln_* through E0), for a row x
of d values with float64 mean m, centred c = x - m, variance v, r = (v + eps)^-1/2:
      dm = (d + 1) u mean|x|                       the fp32 mean: d additions in any order, one multiplication
      dc = dm + u |c|                              x - mean
      dv = mean(2 |c| dc) + (d + 4) u v            the fp32 variance: squares, d additions, one multiplication
      dr = dv / (2 (v + eps)) + 4 u                relative error of rsqrtf(v + eps) (<= 2 ulp) and the addition of eps
      dy = |g| r dc + |c r g| (dr + 2 u) + u |y|   (c r) g + b

The bound is a worst case: sums are ~sqrt(n) random walks, so err / bound of an honest kernel sits well below 1.  At K = 2048 it
cannot show one dropped term -- that is what the `int` regime is for: every operand and partial sum is an integer below 2^24, so
any summation order, any split and the hi / lo split are exact and the kernel must EQUAL the reference (rounded to bf16 for bf16
output)."""
import math

import torch

U32 = 2.0 ** -24
U16 = 2.0 ** -8
GELU_LIP = 1.13
AS_ERR = 1.5e-7
GELU_FAST_ULPS = 16
ERFF_TERM = 12
LN_EPS = 1e-5


def map_rows(rmap, M, device="cpu"):
    """Physical row of every logical row r < M under {rpg, gstride, off} (None / rpg 0: identity)."""
    r = torch.arange(M, device=device)
    if rmap is None or rmap[0] == 0:
        return r
    rpg, gstride, off = rmap
    return (r // rpg) * gstride + r % rpg + off


def layernorm64(x, g, b, unbiased=False):
    x = x.double()
    m = x.mean(-1, keepdim=True)
    c = x - m
    v = (c * c).sum(-1, keepdim=True) / (x.shape[-1] - (1 if unbiased else 0))
    return c * torch.rsqrt(v + LN_EPS) * g.double() + b.double()


def ln_bound(x, g, b):
    """Element-wise bound on |fp32 LayerNorm(x) - layernorm64(x)| (see the module docstring)."""
    x, g, b = x.double(), g.double(), b.double()
    d = x.shape[-1]
    m = x.mean(-1, keepdim=True)
    c = x - m
    v = (c * c).mean(-1, keepdim=True)
    r = torch.rsqrt(v + LN_EPS)
    dm = (d + 1) * U32 * x.abs().mean(-1, keepdim=True)
    dc = dm + U32 * c.abs()
    dv = (2 * c.abs() * dc).mean(-1, keepdim=True) + (d + 4) * U32 * v
    dr = dv / (2 * (v + LN_EPS)) + 4 * U32
    y = c * r * g + b
    return g.abs() * r * dc + (c * r * g).abs() * (dr + 2 * U32) + U32 * y.abs()


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def gelu_fast_f64(x):
    """The formula of gelu_fast (device_util.h) in float64: what the polynomial alone costs."""
    ax = x.abs() * 0.70710678118654752440
    t = 1.0 / (0.3275911 * ax + 1.0)
    p = t * 1.061405429 - 1.453152027
    p = t * p + 1.421413741
    p = t * p - 0.284496736
    p = t * p + 0.254829592
    p = p * t
    e = torch.exp2(-ax * ax * 1.44269504088896340736)
    erf_abs = 1.0 - p * e
    hx = 0.5 * x
    return hx.abs() * erf_abs + hx


def gelu_grid():
    return torch.linspace(-12.0, 12.0, 2_400_001, dtype=torch.float64)


def gemm_ref(A, W, M=None, bias=None, rowtab=None, rt_mod=1, gelu=False, res=None, amap=None, cmap=None, a_ln=None, ln=None,
             gelu_after_res=False, row0=0):
    """A (physical rows, K), W (N, K), bias (N), rowtab (>= rt_mod, N), res (physical rows of C, N): any float dtype on any device,
    columns already cut to K / N; computed in float64 there.  M logical rows (default: A's rows).  a_ln / ln: (g, b) pairs.
    Returns a dict: C (M, N) logical rows, crow (M,) their physical rows, S, pre (the GELU's argument, None without gelu), the
    magnitudes the bound needs, dA (a_ln: the operand's LayerNorm bound, folded into S-like term SA), ln (function: C -> float64
    LayerNorm of its rows) when ln is given.  row0: the tensors hold logical rows row0 .. row0 + M of a larger problem (identity
    maps; a chunked check).  gelu_after_res is a seeded bug of the bound's own test."""
    f = lambda t: None if t is None else t.double()
    A, W, bias, rowtab, res = map(f, (A, W, bias, rowtab, res))
    M = A.shape[0] if M is None else M
    dev = A.device
    arow, crow = map_rows(amap, M, dev), map_rows(cmap, M, dev)
    a = A[arow]
    SA = None
    if a_ln is not None:
        dA = ln_bound(a, a_ln[0], a_ln[1])
        a = layernorm64(a, a_ln[0], a_ln[1])
        SA = dA @ W.abs().T
    acc = a @ W.T
    S = a.abs() @ W.abs().T
    out = {"acc": acc, "S": S, "SA": SA, "crow": crow, "bias": None, "rt": None, "pre": None, "g": None, "K": A.shape[1]}
    v = acc
    if bias is not None:
        v = v + bias
        out["bias"] = v
    if rowtab is not None:
        v = v + rowtab[(row0 + torch.arange(M, device=dev)) % rt_mod]
        out["rt"] = v
    r = res[crow] if res is not None else None
    if gelu and not gelu_after_res:
        out["pre"] = v
        v = gelu64(v)
        out["g"] = v
    if r is not None:
        v = v + r
        out["res"] = True
    if gelu and gelu_after_res:
        v = gelu64(v)
    out["C"] = v
    if ln is not None:
        out["ln"] = lambda C: layernorm64(C, ln[0], ln[1])
    return out


def bound(ref, dtype, K, S_split=1, f32out=True):
    """Element-wise bound (M, N) on |C_kernel - ref["C"]| for dtype 0 (fp32 operands), 1 (bf16) or 2 (split-bf16)."""
    S = ref["S"]
    if dtype == 2:
        n = 3 * K + S_split
        E = n * U32 / (1 - n * U32) * (1 + U16) ** 2 * S + (3 * U16 ** 2 + U16 ** 4) * S
    else:
        n = K + S_split
        E = n * U32 / (1 - n * U32) * S
    if ref["SA"] is not None:
        E = E + ref["SA"] * (1 + n * U32)
    for key in ("bias", "rt"):
        if ref[key] is not None:
            E = E + U32 * (ref[key].abs() + E)
    if ref["pre"] is not None:
        x, g = ref["pre"], ref["g"]
        if dtype == 1:
            G = 0.5 * x.abs() * (AS_ERR + GELU_FAST_ULPS * U32) + U32 * g.abs()
        else:
            G = ERFF_TERM * U32 * x.abs()
        E = GELU_LIP * E + G
    if ref.get("res"):
        E = E + U32 * (ref["C"].abs() + E)
    if not f32out:
        E = E + U16 * (ref["C"].abs() + E)
    return E


REGIMES = ("int", "randn", "spike", "offset")


def make_inputs(regime, M, N, K, dtype=1, bias=True, rt_mod=0, res=False, spike_k=None, device="cpu", seed=0):
    """Logical inputs of one case, float32 tensors holding values the operand type represents (bf16-rounded for dtype 1):
    A (M, K), W (N, K), bias (N) / rowtab (rt_mod, N) / res (M, N) or None.
      int:    A, W uniform in {-3 .. 3}, bias / rowtab / res integers in +-64: every partial sum is an integer below 2^24 (K <= 2048:
              9 K + 192), so the result is exact in fp32 under any summation order, any split-K and the hi / lo split (lo = 0);
      randn:  A ~ N(0, 1), W ~ N(0, 1) K^-1/2, epilogue terms N(0, 1);
      spike:  randn, and k = spike_k (default K - 1) carries most of every row's S: A[:, k] = +-4 sqrt K (1 + 0.1 N) (a sign per
              row), W[:, k] = +-(1 + 0.1 N) (a sign per column): |a_k w_k| ~ 4 sqrt K against ~0.64 sqrt K for the rest together;
      offset: A = 100 + N(0, 1), W in pairs w_{2j+1} = -w_{2j} + 0.01 N K^-1/2: |C| is a hundredth of S."""
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=device, generator=g)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, device=device, generator=g).float()
    if regime == "int":
        t = {"A": ri(-3, 3, M, K), "W": ri(-3, 3, N, K), "bias": ri(-64, 64, N) if bias else None,
             "rowtab": ri(-64, 64, rt_mod, N) if rt_mod else None, "res": ri(-64, 64, M, N) if res else None}
        return t
    A, W = rn(M, K), rn(N, K) / K ** 0.5
    if regime == "spike":
        k = K - 1 if spike_k is None else spike_k
        A[:, k] = torch.sign(rn(M)) * 4 * K ** 0.5 * (1 + 0.1 * rn(M))
        W[:, k] = torch.sign(rn(N)) * (1 + 0.1 * rn(N))
    elif regime == "offset":
        A = A + 100.0
        W[:, 1::2] = -W[:, 0::2] + 0.01 * rn(N, K // 2) / K ** 0.5
    elif regime != "randn":
        raise ValueError(regime)
    t = {"A": A, "W": W, "bias": rn(N) if bias else None, "rowtab": rn(rt_mod, N) if rt_mod else None,
         "res": rn(M, N) if res else None}
    if dtype == 1:
        t["A"], t["W"] = t["A"].to(torch.bfloat16).float(), t["W"].to(torch.bfloat16).float()
    return t
