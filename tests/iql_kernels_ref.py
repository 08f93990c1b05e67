"""References and bounds for the kernels of m3pc_amd/csrc/iql.hip, each alone (the hooks m3pc_debug_iql_* of include/m3pc_hip_debug.h;
tests/test_iql_kernel_edges_gpu.py).  float64 NumPy; the loss kernel's running error analysis reuses the EV class of
tests/mtm_grad_kernels_ref.py (torch float64).  u = 2^-24; gam(n) = n u / (1 - n u).

Products.  Every accumulator is ONE chain of fp32 fmas (v_mfma_f32_32x32x2_f32: an exact product, one rounding per term) in a fixed K
order that starts from the bias (forward) or from 0 (deltas, gradients): gemm_ref's running-sum bound with the kernel's K and no split,
  |acc - ref| <= gam(K) (|b| + sum_k |w_k| |x_k|).
K is what the kernel walks: layer 1 the input width rounded up to 32; layers 2 / 3 hidden; delta<2> 8 (out <= 8) or 32; delta<1>
hidden; dW the padded batch Bp.  (Terms beyond the real extent are exact zeros and round nothing; the bound does not use that.)  ReLU and
the ReLU mask are exact: relu is 1-Lipschitz, and the mask of a delta reads the activation the caller hands in.
  bias gradient: column n of the bias tile sums the rows k with (k / 2) % 32 == n -- two per 64 rows, 2 ceil(Bp / 64) terms -- and five
  butterfly levels add the 32 columns: every term passes at most 2 ceil(Bp / 64) + 5 additions, |db - ref| <= gam(2 ceil(Bp / 64) + 5)
  sum |delta|.
  tanh (the actor's output): E + TANHF_ULPS ulp of the result, an ulp taken as 2 u |tanh| (elementwise_ref.TANHF_ULPS).

Layer-1 features.  (s - mean) / std in float32: the library is built without fast-math and with -ffp-contract=off, so the subtraction
and the division are the correctly rounded IEEE operations np.float32 performs; features32 restates them bit for bit and the product's
reference takes those float32 features as its exact input.

The loss kernel.  A handful of fp32 operations per row, restated operation by operation with EV (value, bound, one rounding u (|v| + e)
per operation); expf and tanhf with EXPF_ULPS / TANHF_ULPS on top of the propagated argument error; fminf(., 100) is 1-Lipschitz, and
where exp(x) (1 - its relative bound) already exceeds 100 -- an expf that overflowed to inf included -- the result is 100 exactly.  The
sign of adv = fl(qt - v) is the sign of qt - v (a correctly rounded difference is 0 only for equal operands), so the weight's branch is
never in doubt: adv == +0 and -0 both take `expectile`.  Block sums (iql_block_sum): six butterfly levels, then the sixteen
wavefront sums in a chain from 0 -- every term passes at most 6 + 16 additions: sum e_i + gam(22) (sum |x_i| + sum e_i).  log_std's
gradient: the same tree per component; a component outside [-20, 2] gets exactly 0.

Adam (csrc/iql.h).  m and v are restated bit for bit in np.float32 in the order iql.h states; p is the stated expression in float64
from those float32 moments, rounded to float32 once -- bit for bit (IEEE double sqrt, division, product, difference on both sides).
The soft update: two fp32 products and one sum, bit for bit.  Where the gradient itself carries an error (every regime but `int`) the
test checks m from zero moments against (1 - beta1) g with the gradient's bound and one rounding, and p from the device's own moments.

Publish: plain transposes and copies, and the operand streams of the host critic_pack (m3pc_debug_critic_pack), bit for bit."""
import math

import numpy as np
import torch

from elementwise_ref import EXPF_ULPS, TANHF_ULPS
from mtm_grad_kernels_ref import EV, TINY, ev_exp, gam

F = np.float32
U32 = 2.0 ** -24
KID = {"fwd1": 1, "fwd2": 2, "fwd3": 3, "loss": 4, "delta2": 5, "delta1": 6, "grad": 7, "eval_out": 8, "copy": 9, "publish": 10}
MAX_BATCH, OUTW = 1024, 32
OMB1, B2, OMB2 = F(1.0 - 0.9), F(0.999), F(1.0 - 0.999)   # the fp32 constants of iql.h
_L = F(math.log(100.0))                                    # the float32 neighbours of ln 100 (test_iql_kernels_ref_cpu.py asserts them)
LN100_LO = _L if float(_L) <= math.log(100.0) else np.nextafter(_L, F(-np.inf))
LN100_HI = np.nextafter(LN100_LO, F(np.inf))
HALF_LOG_2PI = 0.91893853320467274


def pad32(n):
    return (n + 31) & ~31


def train_pass(t):
    return 1 if t == 0 else t + 3


# ------------------------------------------------------------------------------------------------ features and products
def features32(s, om, os_, a, width):
    """Layer 1's input, bit for bit: (s - mean) / std in float32, then the action; the first `width` columns."""
    s, om, os_ = np.asarray(s, F), np.asarray(om, F), np.asarray(os_, F)
    x = (s - om) / os_
    assert x.dtype == F
    if a is not None:
        x = np.concatenate([x, np.asarray(a, F)], 1)
    return np.ascontiguousarray(x[:, :width])


def features64(s, om, os_, a, width):
    x = (np.asarray(s, np.float64) - np.asarray(om, np.float64)) / np.asarray(os_, np.float64)
    if a is not None:
        x = np.concatenate([x, np.asarray(a, np.float64)], 1)
    return x[:, :width]


def layer_ref(x, W, b, K, act="relu"):
    """(rows, in) x (out, in) + (out): the value and the bound of one forward layer; act: relu, none or tanh."""
    x, W, b = np.asarray(x, np.float64), np.asarray(W, np.float64), np.asarray(b, np.float64)
    z = x @ W.T + b
    E = gam(K) * (np.abs(x) @ np.abs(W).T + np.abs(b))
    if act == "relu":
        return np.maximum(z, 0.0), E + TINY
    if act == "tanh":
        t = np.tanh(z)
        return t, E + 2 * TANHF_ULPS * U32 * (np.abs(t) + E) + TINY
    return z, E + TINY


def delta_K(L, out, H):
    return (32 if out > 8 else 8) if L == 2 else H


def delta_ref(d, W, h, K):
    """d (rows, k) deltas of the layer above, W (k, H) its weights, h (rows, H) this layer's activations: (d W) where h > 0, else 0."""
    d, W = np.asarray(d, np.float64), np.asarray(W, np.float64)
    on = np.asarray(h) > 0
    return np.where(on, d @ W, 0.0), np.where(on, gam(K) * (np.abs(d) @ np.abs(W)), 0.0) + TINY


def grad_ref(delta, act, Bp):
    """dW (M, N) = delta^T act over the rows, and db (M): values and bounds."""
    delta, act = np.asarray(delta, np.float64), np.asarray(act, np.float64)
    gW, EW = delta.T @ act, gam(Bp) * (np.abs(delta).T @ np.abs(act))
    gb, Eb = delta.sum(0), gam(2 * ((Bp + 63) // 64) + 5) * np.abs(delta).sum(0)
    return gW, EW + TINY, gb, Eb + TINY


# ------------------------------------------------------------------------------------------------ Adam and the soft update
def adam_moments32(m, v, g):
    """Bit for bit: m + (1 - b1) (g - m);  b2 v + ((1 - b2) g) g."""
    m, v, g = np.asarray(m, F), np.asarray(v, F), np.asarray(g, F)
    with np.errstate(under="ignore"):
        m1 = m + OMB1 * (g - m)
        v1 = B2 * v + (OMB2 * g) * g
    assert m1.dtype == F and v1.dtype == F
    return m1, v1


def adam_param32(p, m1, v1, step_size, sqrt_bc2, eps):
    """The parameter expression in float64 from the float32 moments, rounded once."""
    p, m1, v1 = np.asarray(p, F).astype(np.float64), np.asarray(m1, F).astype(np.float64), np.asarray(v1, F).astype(np.float64)
    return (p - step_size * m1 / (np.sqrt(v1) / sqrt_bc2 + eps)).astype(F)


def soft32(t, p1, omt, tau):
    t, p1 = np.asarray(t, F), np.asarray(p1, F)
    out = F(omt) * t + F(tau) * p1
    assert out.dtype == F
    return out


def adam_scalars(k, lr, t_max=None):
    """(step_size, sqrt_bc2) of 0-based step k as iql_step forms them; t_max: the actor's cosine rate."""
    t = k + 1.0
    bc1, bc2 = 1.0 - math.pow(0.9, t), 1.0 - math.pow(0.999, t)
    if t_max is not None:
        lr = lr * 0.5 * (1.0 + math.cos(3.14159265358979323846 * k / float(t_max)))
    return lr / bc1, math.sqrt(bc2)


def adam64(p, m, v, g, step_size, sqrt_bc2, eps=1e-8):
    """The same three lines in float64 (the chained step of test_iql_kernels_ref_cpu.py); in place."""
    m += (1.0 - 0.9) * (g - m)
    v *= 0.999
    v += (1.0 - 0.999) * g * g
    p -= step_size * m / (np.sqrt(v) / sqrt_bc2 + eps)


# ------------------------------------------------------------------------------------------------ the loss kernel
def _x(v):
    """An input taken as it is (float64 kept: the chained CPU step hands in float64 outputs)."""
    v = torch.as_tensor(np.asarray(v, np.float64))
    return EV(v, torch.zeros_like(v))


def _tree_sum(x, dim=0):
    n = 22  # six butterfly levels and the 16-term chain
    se = x.e.sum(dim)
    return EV(x.v.sum(dim), se + gam(n) * (x.v.abs().sum(dim) + se))


def loss_ref(out7, reward, done, action, log_std, expectile, beta, gamma, A):
    """out7 (7, B, >= max(1, A)): next_v, v, q1t, q2t, q1, q2 in column 0 and the actor's mu in columns [0, A).  expectile, beta, gamma:
    the float32 launch scalars.  Returns a dict of EV: dv, dq1, dq2 (B), dz (B, A), gls (A) -- log_std's gradient, 0 where clamped --
    losses (3), and the per-row adv / ea for the fixture checks."""
    B = np.asarray(reward).shape[0]
    o = [_x(np.asarray(out7[f])[:, 0]) for f in range(6)]
    next_v, v, q1t, q2t, q1, q2 = o
    qt = EV(torch.minimum(q1t.v, q2t.v), torch.zeros_like(v.v))
    inv_b = _x(1.0) / _x(float(B))
    adv = qt - v
    neg = adv.v < 0
    one = _x(1.0)
    wgt = _x(float(expectile)) - _x(neg.double().numpy())          # exact for adv >= 0, one rounding for expectile - 1
    wgt = EV(wgt.v.abs(), wgt.e)
    vl = wgt * adv * adv
    dv = _x(-2.0) * wgt * adv * inv_b
    target = _x(reward) + (one - _x(done)) * _x(float(gamma)) * next_v
    e1, e2 = q1 - target, q2 - target
    q1l, q2l = e1 * e1, e2 * e2
    dq1, dq2 = e1 * inv_b, e2 * inv_b
    arg = _x(float(beta)) * adv
    ex = ev_exp(arg)
    rel = 2 * EXPF_ULPS * U32
    # an argument error can only scale exp: the smallest value the device can hold is exp(arg - e) (1 - rel)
    lo = torch.exp(arg.v - arg.e) * (1.0 - rel)
    ea = EV(ex.v.clamp(max=100.0), torch.where(lo > 100.0, torch.zeros_like(ex.v), ex.e))
    ls = np.asarray(log_std, np.float64)[:A]
    inside = (ls >= -20.0) & (ls <= 2.0)
    lsc = _x(np.clip(ls, -20.0, 2.0))
    sigma = ev_exp(lsc)
    inv_var = one / (sigma * sigma)                                  # (A,)
    mu = _x(np.asarray(out7[6])[:, :A])
    diff = _x(np.asarray(action)[:, :A]) - mu
    wa = ea * inv_b                                                  # (B,)
    wa2 = EV(wa.v[:, None], wa.e[:, None])
    dz = -wa2 * diff * inv_var * (one - mu * mu)
    g_row = wa2 * (one - diff * diff * inv_var)
    ins = torch.as_tensor(inside)
    gls = _tree_sum(g_row, 0)
    gls = EV(torch.where(ins, gls.v, torch.zeros_like(gls.v)), torch.where(ins, gls.e, torch.zeros_like(gls.e)))
    term = _x(0.5) * diff * diff * inv_var + lsc + EV.const(HALF_LOG_2PI)   # (B, A)
    bc = EV(torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64))
    for a in range(A):
        bc = bc + EV(term.v[:, a], term.e[:, a])
    fb = _x(float(B))
    sv, s1, s2, sa = _tree_sum(vl), _tree_sum(q1l), _tree_sum(q2l), _tree_sum(ea * bc)
    losses = [sv / fb, (s1 / fb + s2 / fb) * _x(0.5), sa / fb]
    losses = EV(torch.stack([l.v for l in losses]), torch.stack([l.e for l in losses]))
    return dict(dv=dv, dq1=dq1, dq2=dq2, dz=dz, gls=gls, losses=losses, adv=adv, arg=arg, ea=ea, inside=inside, wgt=wgt)


# ------------------------------------------------------------------------------------------------ eval_out, publish
def eval_out_ref(out, Bp, rows, twin, width):
    """out (passes Bp, 32) float32 -> (rows, width) float32, bit for bit (fminf of two floats is exact)."""
    o = np.asarray(out, F).reshape(-1, OUTW)
    v = o[:rows, :width]
    return np.ascontiguousarray(np.minimum(v, o[Bp:Bp + rows, :width]) if twin else v)


def publish_ref(q):
    """q: a dict W1 (H, SA), b1, W2 (H, H), b2, W3 (1, H), b3 (1) of float32 -> the plain copies the scalar critic reads."""
    return dict(W1T=np.ascontiguousarray(q["W1"].T), b1=q["b1"], W2T=np.ascontiguousarray(q["W2"].T), b2=q["b2"], W3=q["W3"].reshape(-1), b3=q["b3"])


# ------------------------------------------------------------------------------------------------ inputs of the edge cases
REGIMES = ("int", "randn", "offset", "spike")
TINY_POS = np.nextafter(F(0), F(1))     # the smallest positive float32 (a denormal): relu' of it is 1


def product_inputs(regime, rows, K, out, seed, bias=True):
    """x (rows, K), W (out, K), b (out) in float32.  int: integers in [-4, 4] (|b| + sum |w| |x| <= 16 K + 8 < 2^24: every partial sum
    is an integer float32 holds, so the chain is exact in any order); offset: x = 8 + randn (same-signed terms); spike: a term of 1e4 at
    the last k and one of -1e4 mid-chain, between terms of order 1."""
    rng = np.random.RandomState(seed)
    if regime == "int":
        x, W, b = rng.randint(-4, 5, size=(rows, K)), rng.randint(-4, 5, size=(out, K)), rng.randint(-8, 9, size=out)
    else:
        x, W, b = rng.normal(size=(rows, K)), rng.normal(size=(out, K)), rng.normal(size=out)
        if regime == "offset":
            x = x + 8.0
        if regime == "spike":
            x[:, K - 1], W[:, K - 1] = 100.0, 100.0
            x[:, K // 2], W[:, K // 2] = 100.0, -100.0
    if not bias:
        b = b * 0
    return x.astype(F), W.astype(F), b.astype(F)


def int_sum_max(x, W, b=None):
    S = np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(W, np.float64)).T
    return float((S + (0 if b is None else np.abs(np.asarray(b, np.float64)))).max())


def obs_inputs(regime, rows, S, A, seed):
    """state, next_state (rows, S), action (rows, A), obs_mean, obs_std.  int: integer states and means, stds powers of two -- every
    feature is a multiple of 1/2 of magnitude <= 16, exact in float32, and with integer weights so is every partial sum."""
    rng = np.random.RandomState(seed)
    if regime == "int":
        s, s2, a = rng.randint(-4, 5, size=(rows, S)), rng.randint(-4, 5, size=(rows, S)), rng.randint(-4, 5, size=(rows, A))
        om, os_ = rng.randint(-4, 5, size=S), 2.0 ** rng.randint(-1, 2, size=S)
    else:
        s, s2, a = rng.normal(size=(rows, S)) * 2 + 1, rng.normal(size=(rows, S)) * 2 + 1, rng.uniform(-0.9, 0.9, size=(rows, A))
        om, os_ = rng.normal(size=S), rng.uniform(0.5, 2.0, size=S)
        if regime == "offset":
            s, s2 = s + 8.0, s2 + 8.0
        if regime == "spike":
            s[:, S - 1] = s2[:, S - 1] = 1e4
            s[:, S // 2] = s2[:, S // 2] = -1e4
    return [v.astype(F) for v in (s, s2, a, om, os_)]


LOG_STD_EDGES = (-21.0, -20.0, 0.0, 2.0, 2.5)
LOSS_BETA = 2.0      # a power of two: beta adv is exact, so the rows below sit exactly where they say
LOSS_ROWS = ("adv>0", "adv<0", "adv=+0", "adv=-0", "ln100-", "ln100+", "inf", "done1", "done0")


def loss_case(A, B, seed):
    """The loss kernel's inputs with its kinks placed exactly.  out7 (7, B, 32): column 0 of passes 0..5 and columns [0, A) of pass 6
    are read, everything else is NaN.  Rows 0..8 (where the batch has them) are LOSS_ROWS; log_std starts with LOG_STD_EDGES where A
    has room (A = 1: the single component is exactly 2)."""
    rng = np.random.RandomState(seed)
    out7 = np.full((7, B, OUTW), np.nan, F)
    out7[:6, :, 0] = rng.normal(size=(6, B))
    out7[6, :, :A] = np.tanh(rng.normal(size=(B, A)))
    reward, done = rng.normal(size=B).astype(F), (rng.uniform(size=B) < 0.3).astype(F)
    action = rng.uniform(-0.9, 0.9, size=(B, A)).astype(F)

    def put(r, v, q1t, q2t, d=None):
        if r < B:
            out7[1, r, 0], out7[2, r, 0], out7[3, r, 0] = v, q1t, q2t
            if d is not None:
                done[r] = d
    if B > 1:
        put(0, 0.0, 0.5, 0.75)
        put(1, 1.0, 0.25, 2.0)
        put(2, 0.75, 0.75, 3.0)
        put(3, 0.0, 5.0, -0.0)
        put(4, 0.0, LN100_LO / F(LOSS_BETA), 9.0)
        put(5, 0.0, 9.0, LN100_HI / F(LOSS_BETA))
        put(6, 0.0, 60.0, 61.0)
        put(7, 0.5, 0.25, 0.5, 1.0)
        put(8, 0.25, 0.5, 0.5, 0.0)
    ls = rng.uniform(-1.0, 0.5, size=A)
    if A >= len(LOG_STD_EDGES):
        ls[:len(LOG_STD_EDGES)] = LOG_STD_EDGES
    else:
        ls[0] = 2.0
    return dict(out7=out7, reward=reward, done=done, action=action, log_std=ls.astype(F), A=A, B=B, expectile=F(0.7), beta=F(LOSS_BETA), gamma=F(0.99))


def relu_edges(h, seed):
    """Activations with exact +0, -0 and the smallest positive float at known places of every row (in place); returns the three masks."""
    rng = np.random.RandomState(seed)
    kind = rng.randint(0, 6, size=h.shape)
    h[kind == 0] = 0.0
    h[kind == 1] = -0.0
    h[kind == 2] = TINY_POS
    return kind == 0, kind == 1, kind == 2
