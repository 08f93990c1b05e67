"""Float64 restatements of the kernels of m3pc_amd/csrc/elementwise.hip (the hooks m3pc_debug_layernorm, _head_out, _actor_head,
_critic, _embed of include/m3pc_hip_debug.h), element-wise bounds on what the fp32 / bf16 kernels may differ from them, and float32
restatements in the kernels' own operation order of the kernels that are held bit for bit (sample, score, gather_rows, tokenise,
de-tokenise, the goal overlays).  layernorm64, ln_bound, map_rows, U32 and U16 are those of tests/gemm_ref.py.

u = U32 = 2^-24, u16 = U16 = 2^-8.  Every term below is a rounding point read off the kernel; each later term is taken on
|reference value| + the error so far.  The bounds are worst cases (sums are ~sqrt(n) random walks): an honest kernel sits well below 1.

LayerNorm (layernorm_kernel, layernorm_vec_kernel, layernorm_rows_kernel<NV, 2>, and the fused norm of actor_head_kernel): two passes
over registers, mean = sum * fl(1 / d), variance from the centred values, rsqrtf(var + 1e-5f), (x - mean) * rstd * g + b.  The fused
norms of embed_kernel and embed_rows_kernel DIVIDE instead (tot / (float)d for the mean and for the variance: one correctly rounded
division where the others round fl(1 / d) and a product); embed_kernel adds the partial sums of its blockDim / 64 waves through LDS in
wave order.  ln_bound covers both: its (d + 1) u on the mean and (d + 4) u on the variance allow d - 1 additions in any order and
two roundings behind them, of which the division uses one.
  int            ln_int_ref: the exact fp32 result of rows whose variance is 256 (fp32 absorbs the eps; rstd = 2^-4)
  single norm    ln_bound(x, g1, b1) against layernorm64(x, g1, b1)          (gemm_ref.py derives it: d - 1 additions, fl(1 / d) and
                 one multiplication are its (d + 1) u; rsqrtf within 2 ulp)
  double norm    the same bound applied twice: the second norm is held to ln_bound(y1, g2, b2) against layernorm64(y1, g2, b2) of
                 the kernel's OWN fp32 first stage y1 -- the same launch without g2 / b2, whose first stage is the same instructions --
                 and y1 itself is held to the single-norm bound
  bf16 output    one rounding to nearest even: + u16 (|y| + E)

head_out_kernel: lane l multiplies its d / 64 columns into one fma chain, a 6-step butterfly adds the 64 lanes:
  accumulation   E = (d + 7) u S,  S = sum_k |x_k w_k|           (d / 64 fmas + 6 additions <= d + 7 roundings of partial sums <= S)
  bias           E += u (|v| + E)
  de-tokeniser   v * stdv, + mean, one rounding each (__fmul_rn, __fadd_rn): E = E |stdv| + u (|v stdv| + E |stdv|), E += u (|v'| + E)
head_out_mfma_kernel: X is bf16 and taken exactly; w = hi + lo + dw with hi = bf16(w), lo = bf16(w - hi), |lo| <= u16 |w|,
|dw| <= u16^2 |w|; two accumulation chains (lo, then hi, per k-step) run into ONE fp32 accumulator:
  accumulation   E = U16^2 S + n u (1 + u16) S / (1 - n u),  n = 2 d   (d products of each chain, exact in fp32, added in any order;
                 the terms' absolute sum is at most (1 + u16) S; the multi-term adder of a bf16 MFMA is taken to round no worse than
                 the chain of fp32 additions it replaces, as in gemm_ref.py)
  bias, de-tokeniser as above.

Critic (critic_kernel / critic_mfma_kernel<NT>), per network, z = [(s - om) / os | a]:
  input          two roundings (subtraction, division): dz = 2 u |z| (1 + u) on the state features, 0 on the actions
  layer 1        an fma chain of S + A terms and the bias (the matrix-core kernel starts from the bias and pads to 32 features with
                 exact zeros: the same count): E1 = sum |W1| dz + (S + A + 1) u (sum |W1 z| + |b1|)
  ReLU           Lipschitz constant 1: E1 carries over
  layer 2        an fma chain of `hidden` terms and the bias: E2 = sum |W2| E1 + (hidden + 1) u (sum |W2| (h1 + E1) + |b2|)
  ReLU           E2 carries over
  w3 dot         scalar kernel: a rounded product per unit, a 6-step butterfly, 4 partial sums and b3: n3 = 1 + 6 + 4 = 11;
                 matrix-core kernel: an fma chain of 16, the half-wave exchange, NT tile sums and b3: n3 = 16 + 1 + NT + 1;
                 E3 = sum |w3| E2 + n3 u (sum |w3| (h2 + E2) + |b3|)
  min            |min(a, b) - min(a', b')| <= max(Ea, Eb)

Actor head (actor_head_kernel<4|8>, actor_head_small_kernel): x = the row, or its fp32 LayerNorm (x moves by at most ln_bound):
  two dots       E = sum |w| dx + (d + 7) u S, then the bias: E += u (|v| + E)        (mu is done here)
  tanhf          |tanh'| <= 1: E_t = E + TANHF_ULPS u |tanh|
  affine         a = t + 1, m = 3.5 a, ls = m - 5, one rounding each (0.5f * (2 - -5) folds to 3.5f exactly)
  expf           E_sd = sd (exp(E_ls) - 1) + EXPF_ULPS u sd
  TANHF_ULPS = 5 and EXPF_ULPS = 3 are the OpenCL full-profile bounds of tanh and exp (OpenCL C specification, "Relative error as
  ULPs"), which the ROCm device library that implements tanhf / expf is written to -- the same source gemm_ref.py names for erff's 16.

embed_kernel (d % 256 != 0) and embed_rows_kernel: acc = fma chain over the token's D features, + E[t] (one rounding); with the fused
norm, the LayerNorm of the kernel's OWN fp32 row is held to ln_bound in fp32 (Hf) and with the bf16 output term (Hb); in the `int`
regime to ln_int_ref (sum / d and 256 d / d are exact divisions).  No normalisation, no window index
(the hook passes neither).
  row            E = (D + 1) u (sum |x_f W_f| + |E_t|)

Bit for bit (float32 numpy, the kernel's operation order):
  sample_ref          cand / sample_actions of sample_kernel; tanh is passed in (the device library's tanhf has no bit-exact CPU
                      twin: the GPU test passes torch.tanh on the device, the same library function; the CPU test np.tanh)
  td_lambda_ref       the O(h^2) loop of oracle/mtm_oracle.py::td_lambda, every sum left to right -- NOT score_kernel's running form
  gather_ref, tokenize_ref, detokenize_ref, overlay_ref, overlay_rows_ref"""
import numpy as np
import torch

from gemm_ref import LN_EPS, U16, U32, layernorm64, ln_bound, map_rows  # noqa: F401  (re-exported for the tests)

TANHF_ULPS = 5   # OpenCL full-profile bound of tanh (see the module docstring)
EXPF_ULPS = 3    # OpenCL full-profile bound of exp
LN_INT_RSTD = 1.0 / 16.0  # the `int` rows' variance is 256 = 4^4, above which fp32 absorbs the eps of 1e-5: rstd = 2^-4


def gen(device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=device, generator=g)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, device=device, generator=g).float()
    return rn, ri, g


def bf16_out_bound(y, E):
    return E + U16 * (y.abs() + E)


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_int_rows(rows, d, device, seed):
    """Rows whose fp32 mean is an integer m and whose variance is exactly 256 (rstd = 2^-4 exactly: 256 + 1e-5 rounds to 256): the
    centred values are a permutation, per row, of either d / 2 times +-16 or of d / 8 times +-32 and 3 d / 4 zeros."""
    rn, ri, g = gen(device, seed)
    a = torch.cat([torch.full((d // 2,), 16.0), torch.full((d // 2,), -16.0)])
    b = torch.cat([torch.full((d // 8,), 32.0), torch.full((d // 8,), -32.0), torch.zeros(d - 2 * (d // 8))])
    pat = torch.stack([a, b]).to(device)
    which = torch.randint(0, 2, (rows,), device=device, generator=g)
    perm = torch.rand(rows, d, device=device, generator=g).argsort(1)
    c = pat[which].gather(1, perm)
    return c + ri(-40, 40, rows, 1)


def ln_int_ref(x, g, b):
    """What an fp32 LayerNorm of ln_int_rows must give exactly: the mean and the variance 256 are exact, 256 + 1e-5 rounds to 256 in fp32
    (the eps is below half an ulp of 256), rsqrtf(256) = 2^-4, and (x - mean) 2^-4 g + b is a small integer.  (The float64 norm keeps the
    eps and differs from this by 2e-8 |y|: in this regime the reference is the exact fp32 result.)"""
    x, g, b = x.double(), g.double(), b.double()
    return (x - x.mean(-1, keepdim=True)) * LN_INT_RSTD * g + b


def ln_inputs(regime, rows, d, double, device, seed):
    """x (rows, d) and g1, b1, g2, b2 (g2 / b2 None without `double`).
      int:    ln_int_rows; g, b integers in +-8 -- and g1 = 16, b1 = 3 in front of a second norm, so that its input is again such a row:
              every value, sum and product is a small integer or a power of two and the result is exact, in bf16 too (|y| <= 24);
      randn:  x ~ N(0, 1) with a scale per row in [0.1, 10], g ~ 1 + 0.3 N, b ~ N;
      offset: the randn rows moved by 300 row standard deviations (|mean| >> sd)."""
    rn, ri, _ = gen(device, seed + 7919)
    if regime == "int":
        x = ln_int_rows(rows, d, device, seed)
        g1, b1 = (torch.full((d,), 16.0, device=device), torch.full((d,), 3.0, device=device)) if double else (ri(-8, 8, d), ri(-8, 8, d))
        return x, g1, b1, (ri(-8, 8, d) if double else None), (ri(-8, 8, d) if double else None)
    sc = 10.0 ** (2 * torch.rand(rows, 1, device=device, generator=torch.Generator(device=device).manual_seed(seed)) - 1)
    x = rn(rows, d) * sc
    if regime == "offset":
        x = x + 300.0 * sc * torch.sign(rn(rows, 1))
    elif regime != "randn":
        raise ValueError(regime)
    p = [1 + 0.3 * rn(d), rn(d)] + ([1 + 0.3 * rn(d), rn(d)] if double else [None, None])
    return (x, *p)


# ------------------------------------------------------------------------------------------------ head_out
def detok_bound(v, E, stdv, mean):
    """(v stdv) + mean, one rounding each; returns (value, bound)."""
    v2 = v * stdv
    E = E * stdv.abs() + U32 * (v2.abs() + E * stdv.abs())
    v3 = v2 + mean
    return v3, E + U32 * (v3.abs() + E)


def head_out_ref(x, W, b, mean=None, stdv=None, mfma=False):
    """x (rows, d) -- bf16-representable for the matrix-core kernel --, W (D, d), b (D): float64 result and bound (rows, D)."""
    x, W, b = x.double(), W.double(), b.double()
    d = x.shape[1]
    acc, S = x @ W.T, x.abs() @ W.abs().T
    if mfma:
        n = 2 * d
        E = U16 ** 2 * S + n * U32 * (1 + U16) * S / (1 - n * U32)
    else:
        E = (d + 7) * U32 * S
    v = acc + b
    E = E + U32 * (v.abs() + E)
    if mean is not None:
        v, E = detok_bound(v, E, stdv.double(), mean.double())
    return v, E


def head_inputs(regime, rows, d, D, device, seed, bf16_rows=False):
    """x, W, b, mean, stdv.  int: x, W in {-3 .. 3}, b, mean integers in +-64, stdv a power of two in {1/2, 1, 2, 4}: every partial sum
    is an integer below 9 d + 64 < 2^24 and the de-tokeniser is exact; randn: x ~ N, W ~ N d^-1/2; offset: x = 100 + N, W in pairs
    w_{2j+1} = -w_{2j} + 0.01 N d^-1/2 (|y| a hundredth of S), as gemm_ref.make_inputs."""
    rn, ri, g = gen(device, seed)
    if regime == "int":
        return ri(-3, 3, rows, d), ri(-3, 3, D, d), ri(-64, 64, D), ri(-64, 64, D), 2.0 ** ri(-1, 2, D)
    x, W = rn(rows, d), rn(D, d) / d ** 0.5
    if regime == "offset":
        x = x + 100.0
        W[:, 1::2] = -W[:, 0::2] + 0.01 * rn(D, d // 2) / d ** 0.5
    elif regime != "randn":
        raise ValueError(regime)
    if bf16_rows:
        x = x.to(torch.bfloat16).float()
    return x, W, rn(D), rn(D), 0.5 + torch.rand(D, device=device, generator=g)


# ------------------------------------------------------------------------------------------------ critic
def critic_ref(states, actions, om, os_, nets, n3):
    """nets: two tuples (W1 (H, S + A), b1, W2 (H, H), b2, W3 (H,), b3 (1,)) in torch layout.  Float64 q (rows,) and its bound."""
    f = lambda t: t.double()
    z = (f(states) - f(om)) / f(os_)
    dz = torch.cat([2 * U32 * z.abs() * (1 + U32), torch.zeros_like(f(actions))], 1)
    z = torch.cat([z, f(actions)], 1)
    SA = z.shape[1]
    qs, Es = [], []
    for W1, b1, W2, b2, W3, b3 in nets:
        W1, b1, W2, b2, W3, b3 = map(f, (W1, b1, W2, b2, W3, b3))
        H = W1.shape[0]
        p1 = z @ W1.T + b1
        E1 = dz @ W1.abs().T + (SA + 1) * U32 * (z.abs() @ W1.abs().T + b1.abs())
        h1 = p1.clamp(min=0)
        p2 = h1 @ W2.T + b2
        E2 = E1 @ W2.abs().T + (H + 1) * U32 * ((h1 + E1) @ W2.abs().T + b2.abs())
        h2 = p2.clamp(min=0)
        q = h2 @ W3 + b3
        E3 = E2 @ W3.abs() + n3 * U32 * ((h2 + E2) @ W3.abs() + b3.abs())
        qs.append(q)
        Es.append(E3)
    return torch.minimum(qs[0], qs[1]), torch.maximum(Es[0], Es[1])


def critic_n3(mfma, hidden):
    return 16 + 1 + hidden // 32 + 1 if mfma else 11


def critic_inputs(regime, rows, S, A, H, device, seed):
    """states, actions, om, os, nets.  int: states, om, actions integers (z in +-3 after os in {1, 2}), weights in {-1, 0, 1}, biases
    integers in +-4: |layer 1| <= 64 * 3 + 4, |layer 2| <= 256 * 196 + 4, |q| <= 256 * 50180 + 4 < 2^24 -- exact in any order;
    randn: N(0, 1) data, weights N fan_in^-1/2; offset: states = 50 + N with om = 50 (the centring cancels two digits)."""
    rn, ri, g = gen(device, seed)
    if regime == "int":
        os_ = 2.0 ** ri(0, 1, S)
        om = ri(-5, 5, S)
        states = om + os_ * ri(-3, 3, rows, S)
        actions = ri(-3, 3, rows, A)
        nets = [(ri(-1, 1, H, S + A), ri(-4, 4, H), ri(-1, 1, H, H), ri(-4, 4, H), ri(-1, 1, H), ri(-4, 4, 1)) for _ in range(2)]
        return states, actions, om, os_, nets
    om, os_ = rn(S), 0.5 + torch.rand(S, device=device, generator=g)
    states, actions = rn(rows, S) * os_ + om, torch.tanh(rn(rows, A))
    if regime == "offset":
        om = om + 50.0
        states = states + 50.0
    elif regime != "randn":
        raise ValueError(regime)
    nets = [(rn(H, S + A) / (S + A) ** 0.5, 0.1 * rn(H), rn(H, H) / H ** 0.5, 0.1 * rn(H), rn(H) / H ** 0.5, 0.1 * rn(1)) for _ in range(2)]
    return states, actions, om, os_, nets


def critic_pack_index(hidden, SA):
    """The index formulas of the comment above critic_mfma_kernel, as (gather index into W1 or -1 for a zero, gather index into W2):
      W1F[t][g < 4][lane][j]            = W1[32 t + (lane & 31)][2 (4 g + j) + (lane >> 5)]       (features >= SA: zero)
      W2F[u][g < hidden / 8][lane][j]   = W2[32 u + (lane & 31)][8 g + 4 (lane >> 5) + j]         (+ 1024 floats of zeros)"""
    NT, NG = hidden // 32, hidden // 8
    lane, j = np.arange(64)[:, None], np.arange(4)[None, :]
    w1 = np.empty((NT, 4, 64, 4), np.int64)
    for t in range(NT):
        for g in range(4):
            f = 2 * (4 * g + j) + (lane >> 5)
            w1[t, g] = np.where(f < SA, (32 * t + (lane & 31)) * SA + f, -1)
    w2 = np.empty((NT, NG, 64, 4), np.int64)
    for u in range(NT):
        for g in range(NG):
            w2[u, g] = (32 * u + (lane & 31)) * hidden + 8 * g + 4 * (lane >> 5) + j
    return w1.reshape(-1), w2.reshape(-1)


# ------------------------------------------------------------------------------------------------ actor head
def actor_ref(x, Wmu, bmu, Wls, bls, ln=None, norm=layernorm64):
    """x (rows, d) fp32 rows (already mapped).  Returns mu, E_mu, sd, E_sd in float64.  norm: ln_int_ref in the `int` regime."""
    f = lambda t: t.double()
    xd = f(x)
    d = xd.shape[1]
    dx = torch.zeros_like(xd)
    if ln is not None:
        dx = ln_bound(xd, ln[0], ln[1])
        xd = norm(xd, ln[0], ln[1])
    out = []
    for W, b in ((f(Wmu), f(bmu)), (f(Wls), f(bls))):
        v = xd @ W.T + b
        E = dx @ W.abs().T + (d + 7) * U32 * ((xd.abs() + dx) @ W.abs().T)
        out.append((v, E + U32 * (v.abs() + E)))
    (mu, Emu), (s, Es) = out
    t = torch.tanh(s)
    Et = Es + TANHF_ULPS * U32 * t.abs()
    a = t + 1
    Ea = Et + U32 * a
    m = 3.5 * a
    Em = 3.5 * Ea + U32 * m
    ls = m - 5
    Els = Em + U32 * ls.abs()
    sd = torch.exp(ls)
    return mu, Emu, sd, sd * torch.expm1(Els) + EXPF_ULPS * U32 * sd * torch.exp(Els)


def actor_inputs(regime, nrows, d, A, device, seed, ln):
    """x, Wmu, bmu, Wls, bls, (ln_g, ln_b) or None.  int (mu only is exact; sd goes through tanhf / expf and is held to its bound): without
    the norm x, Wmu in {-3 .. 3}, bmu integers; with it x = ln_int_rows, ln_g, ln_b small integers, so the normalised row is integer."""
    rn, ri, _ = gen(device, seed)
    lnp = None
    if regime == "int":
        x = ln_int_rows(nrows, d, device, seed) if ln else ri(-3, 3, nrows, d)
        if ln:
            lnp = (ri(-2, 2, d), ri(-2, 2, d))
        return x, ri(-3, 3, A, d), ri(-8, 8, A), rn(A, d) / d ** 0.5 / (3.0 if ln else 1.0), rn(A), lnp
    x = rn(nrows, d)
    if regime == "offset":
        x = x + 100.0
    elif regime != "randn":
        raise ValueError(regime)
    if ln:
        lnp = (1 + 0.3 * rn(d), rn(d))
    Wmu, Wls = rn(A, d) / d ** 0.5, rn(A, d) / d ** 0.5
    if regime == "offset" and not ln:
        Wmu[:, 1::2] = -Wmu[:, 0::2] + 0.01 * rn(A, d // 2) / d ** 0.5
        Wls[:, 1::2] = -Wls[:, 0::2] + 0.01 * rn(A, d // 2) / d ** 0.5
    return x, Wmu, rn(A), Wls, rn(A), lnp


# ------------------------------------------------------------------------------------------------ embed_kernel
def embed_ref(x, WT, Et):
    """x (rows, D) token features, WT (D, d), Et (rows, d) the table rows: float64 row and bound."""
    x, WT, Et = x.double(), WT.double(), Et.double()
    v = x @ WT + Et
    return v, (x.shape[1] + 1) * U32 * (x.abs() @ WT.abs() + Et.abs())


# ------------------------------------------------------------------------------------------------ bit for bit: float32 numpy
F = np.float32


def sample_ref(hist, loc, sd, eps, mode, T, A, idx, h, n_begin, n_count, widx=None, index=None, tanh=np.tanh):
    """sample_kernel in float32: cand (n_count, T, A), sample_actions (n_count, h, A) (rows t - idx >= T - idx untouched: NaN here)."""
    cand = np.empty((n_count, T, A), F)
    sa = np.full((n_count, h, A), np.nan, F)
    src = np.asarray(index if index is not None else n_begin + np.arange(n_count), np.int64)
    hist = None if hist is None else hist.reshape(-1, T, A)
    w = np.asarray(widx if widx is not None else np.zeros(n_count), np.int64)
    if idx > 0:
        cand[:, :idx] = hist[w, :idx]
    if idx < T:
        if mode == 2:
            v = eps.reshape(-1, h, A)[src, :T - idx]
        elif mode == 0:
            e = eps.reshape(-1, T, A)[src, idx:]
            v = tanh(((e * sd[None, idx:]).astype(F) + loc[None, idx:]).astype(F)).astype(F)
        else:
            e = eps.reshape(-1, h, A)[src, :T - idx]
            v = (tanh(loc[idx:]).astype(F)[None] + (e * F(0.09)).astype(F)).astype(F)
            v = np.minimum(np.maximum(v, F(-0.99999)), F(0.99999))
        cand[:, idx:] = v
        sa[:, :T - idx] = v
    return cand, sa


def td_lambda_ref(rewards, boot, boot_scale, gamma, lmbda):
    """oracle/mtm_oracle.py::td_lambda (learner.py:300-316) in float32 with every sum taken left to right: for every t the discounted
    rewards are summed again from k = 0 (the O(h^2) loop), disc is the running product gamma^(k + 1) (cumprod), the weights
    (1 - lmbda) and lmbda ** t are Python floats rounded to float32 at the multiplication.  Returns expect_return, scaled boot."""
    n, h = rewards.shape
    g, b = F(gamma), (boot.astype(F) * F(boot_scale)).astype(F)
    er = np.zeros(n, F)
    for t in range(h):
        s, disc = np.zeros(n, F), g
        for k in range(t):
            s = (s + (rewards[:, k] * disc).astype(F)).astype(F)
            disc = F(disc * g)
        s = (s + (b[:, t] * disc).astype(F)).astype(F)
        if t < h - 1:
            s = (s * F(1.0 - lmbda)).astype(F)
        er = (er + (s * F(lmbda ** t)).astype(F)).astype(F)
    return er, b


def gather_ref(Xe, table, rowsrc):
    """Xe (batch, xe_rows, d), table (table_rows, d): out (batch, len(rowsrc), d)."""
    out = np.empty((Xe.shape[0], len(rowsrc), Xe.shape[2]), F)
    for i, s in enumerate(rowsrc):
        out[:, i] = Xe[:, s] if s >= 0 else table[-s - 1][None]
    return out


def tokenize_ref(x, mean, stdv, normalize):
    """float32 or float64 input: (x - mean) / stdv in the input's precision, then float32."""
    if not normalize:
        return x.astype(F)
    if x.dtype == np.float64:
        return ((x - mean.astype(np.float64)) / stdv.astype(np.float64)).astype(F)
    return ((x - mean).astype(F) / stdv).astype(F)


def detokenize_ref(x, mean, stdv, normalize):
    return ((x * stdv).astype(F) + mean).astype(F) if normalize else x.astype(F)


def overlay_rows_mask(T, idx):
    t = np.arange(T)
    return (t <= idx) | ((t >= idx + 2) & (t < T - 1))


def overlay_ref(pred, states_in, T, idx, mean, stdv, normalize):
    """pred, states_in (windows, T, D): the de-tokenised pred and states_out."""
    p = detokenize_ref(pred, mean, stdv, normalize)
    return p, np.where(overlay_rows_mask(T, idx)[None, :, None], p, states_in)


def overlay_rows_ref(pred, states_in, T, idx):
    """pred (windows, nq, D): row q of a window is its q-th overlay row."""
    m = overlay_rows_mask(T, idx)
    out = states_in.copy()
    out[:, m] = pred[:, :int(m.sum())]
    return out
