"""References, float32 restatements and bounds for the kernels of m3pc_amd/csrc/select.hip, in NumPy only (the hooks and the kernel
ids are in include/m3pc_hip_debug.h, "Selection kernel ids"; tests/test_select_edges_gpu.py runs the kernels, tests/test_select_ref_cpu.py
holds this file to torch and to the oracle).

u = U32 = 2^-24 (one rounding to nearest), ULP = 2^-23 (the largest relative size of one unit in the last place).

Orderings.  topk_order: descending value, ties to the lower index, -0.0 equal to +0.0 -- a stable sort of the negated values; what the
kernels build from 64-bit keys {orderable(value), ~index} or from `better`.  race_keys64 / race_order: the keys tau e - log q of the
multinomial race in float64.

select_body (select_kernel, select_batch_kernel, behind the merge in merge_select_kernel / merge_select_batch_kernel), per element i,
with y_i = tau (e_i - max e) in exact arithmetic (the maximum is found by comparison: exact):
  argument       x_i = fl(fl(e_i - max) tau): two roundings, |x_i - y_i| <= (2 u + u^2) |y_i|, which the exponential turns into the
                 relative error expm1((2 u + u^2) |y_i|) ~ 2 u |y_i|
  expf           EXPF_ULPS = 3 ulp (the OpenCL full-profile bound the project already uses, tests/elementwise_ref.py), as a relative
                 error 3 ULP; r_i = expm1((2 u + u^2) |y_i|) (1 + 3 ULP) + 3 ULP is the relative error of w_i = exp(y_i); a result
                 below the normal range may be flushed: an absolute 2^-126 beside it
  sum            tot adds n non-negative terms in a fixed order: ceil(n / 1024) per thread, 6 butterfly steps, 16 partial sums.  Every
                 term passes through at most D = ceil(n / 1024) + 22 additions: relative g = D u / (1 - D u) on every term.
                 tot is therefore off by at most rT = sum_i p_i ((1 + r_i) (1 + g) - 1), relative (p_i = w_i / sum w: the reference)
  division       p_i = fl(w_i / tot): |p^_i - p_i| <= p_i ((1 + r_i) (1 + u) / (1 - rT) - 1) + 2^-126              (select_p_bound)
  eval_action    e_a = fl(t_a / psum), t_a an fma chain + the same reduction over p^_i a_i, psum the same sum of the p^_i.  The common
                 divisor tot cancels between t_a and psum, so only Q_i = (1 + r_i) (1 + u) - 1 and the two sums matter:
                 F_i = (1 + Q_i) (1 + g) - 1, EN_a = sum p_i |a_i| F_i, ED = sum p_i F_i,
                 |e^_a - e_a| <= (EN_a + |e_a| ED) / (1 - ED), one more rounding u (|e_a| + .), and n 2^-126 max |a| for the flushes.
                 With |e_a| <= S_a = sum p_i |a_i| that is S_a times the accumulated factor                          (select_eval_bound)
  arg-max        by comparison: equal.  The race winner is arg-max_i fl(p^_i / q_i): equal to the float64 arg-max of p_i / q_i when the
                 two best ratios differ by more than their error bounds (race_ratio_margin; the CPU test asserts it for every case)

Float32 restatements, expression for expression (numpy float32 arithmetic rounds every operation once, as the kernels do under
-ffp-contract=off): window_stats_ref, merge_ref, deviation_ref.  Everything they compute by comparison, subtraction or max must be EQUAL
on the GPU: c, the deviation, need, cnt, the margin, n, the merged vector.  Only K*, thr_r and need_race of the race merge pass through
logf: K* = max_i key(f_i, q_i) is held to key_bound, thr_r = fl(K* + fl(tau fl(c - delta))) to key_bound + 2 u |thr_r|, and need_race
is a count that must be equal once no key lies within that distance of thr_r (thr_gap_clear).

Race keys: key32 = fl(fl(tau e) - logf(q)).  |key32 - key64| <= u |tau e| + LOGF_ULPS ULP |log q| + u (|key| + the two before)
(key_bound; LOGF_ULPS = 3, the OpenCL bound of log).  close_pairs names the neighbours of the float64 order that lie closer than the
sum of their bounds: where it is empty the float32 order IS the float64 order."""
import numpy as np

F = np.float32
U32 = 2.0 ** -24
ULP = 2.0 ** -23
EXPF_ULPS = 3
LOGF_ULPS = 3
TINY = 2.0 ** -126

SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 8191, 8192, 8193, 16383, 16384)


# ------------------------------------------------------------------------------------------------ orderings
def topk_order(v, k=None):
    """Indices by descending value, ties to the lower index; -0.0 == +0.0 (numpy compares them equal).  No NaN."""
    v = np.asarray(v)
    assert not np.isnan(v).any()
    o = np.argsort(-(v.astype(np.float64) + 0.0), kind="stable")
    return o if k is None else o[:k]


def race_keys64(tau, e, q):
    return np.float64(F(tau)) * np.asarray(e, np.float64) - np.log(np.asarray(q, np.float64))


def key_bound(tau, e, q):
    te = np.abs(np.float64(F(tau)) * np.asarray(e, np.float64))
    lq = np.abs(np.log(np.asarray(q, np.float64)))
    first = U32 * te + LOGF_ULPS * ULP * lq
    return first + U32 * (np.abs(race_keys64(tau, e, q)) + first)


def race_order(tau, e, q, k=None):
    return topk_order(race_keys64(tau, e, q), k)


def close_pairs(keys, bound, positions):
    """Pairs (a, b) of neighbours in the descending order of `keys`, among the first `positions` + 1 places, whose keys differ by no
    more than bound[a] + bound[b] and are not exactly tied in their inputs' sense (the caller plants exact ties at equal keys AND equal
    bounds: those are excused by equality of the keys)."""
    o = topk_order(keys)
    out = []
    for i in range(min(positions, len(o) - 1)):
        a, b = o[i], o[i + 1]
        if keys[a] == keys[b]:
            continue
        if keys[a] - keys[b] <= bound[a] + bound[b]:
            out.append((int(a), int(b)))
    return out


def thr_gap_clear(values, thr, bound):
    """No value within `bound` of the threshold, except exact hits (which the caller plants and accounts for)."""
    d = np.abs(np.asarray(values, np.float64) - np.float64(thr))
    return not bool(((d <= bound) & (d != 0)).any())


# ------------------------------------------------------------------------------------------------ select
def select_ref(e, a0, tau, q=None):
    """float64: p, eval_action (A,), arg-max, race winner (None without q)."""
    e = np.asarray(e, np.float64)
    tau = np.float64(F(tau))
    mx = e.max()
    w = np.exp(tau * (e - mx))
    p = w / w.sum()
    ev = None if a0 is None else p @ np.asarray(a0, np.float64)
    am = int(np.flatnonzero(e == mx)[0])
    si = None
    if q is not None:
        ratio = p / np.asarray(q, np.float64)
        si = int(np.flatnonzero(ratio == ratio.max())[0])
    return p, ev, am, si


def _select_terms(e, tau):
    e = np.asarray(e, np.float64)
    n = e.size
    y = np.abs(np.float64(F(tau)) * (e - e.max()))
    r = np.expm1((2 * U32 + U32 * U32) * y) * (1 + EXPF_ULPS * ULP) + EXPF_ULPS * ULP
    D = min(max(n - 1, 1), (n + 1023) // 1024 + 22)
    g = D * U32 / (1 - D * U32)
    return r, g


def select_p_bound(e, tau):
    p = select_ref(e, None, tau)[0]
    r, g = _select_terms(e, tau)
    rT = float((p * ((1 + r) * (1 + g) - 1)).sum())
    return p * ((1 + r) * (1 + U32) / (1 - rT) - 1) + TINY


def select_eval_bound(e, a0, tau):
    p, ev, _, _ = select_ref(e, a0, tau)
    a = np.abs(np.asarray(a0, np.float64))
    r, g = _select_terms(e, tau)
    Fi = (1 + (1 + r) * (1 + U32) - 1) * (1 + g) - 1
    EN = (p * Fi) @ a
    ED = float((p * Fi).sum())
    E = (EN + np.abs(ev) * ED) / (1 - ED)
    return E + U32 * (np.abs(ev) + E) + e.size * TINY * a.max()


def race_ratio_margin(e, tau, q):
    """(gap, allowed): the gap between the two best ratios p_i / q_i in float64 and the sum of their error bounds -- select_p_bound
    carried through the division by q, and that division's own rounding.  The winner is decided when gap > allowed, or the two are
    an exact planted tie (gap 0 on bit-equal inputs)."""
    p = select_ref(e, None, tau)[0]
    q = np.asarray(q, np.float64)
    ratio = p / q
    o = topk_order(ratio, 2)
    if len(o) < 2:
        return np.inf, 0.0
    err = select_p_bound(e, tau) / q
    err = err + U32 * (ratio + err)
    return float(ratio[o[0]] - ratio[o[1]]), float(err[o[0]] + err[o[1]])


def thread_sums32(x):
    """What thread t of the 1024 holds after `for (i = t; i < n; i += 1024) s += x[i]` in float32."""
    x = np.asarray(x, F)
    pad = np.zeros(-(-x.size // 1024) * 1024, F)
    pad[:x.size] = x
    acc = np.zeros(1024, F)
    for row in pad.reshape(-1, 1024):
        acc = (acc + row).astype(F)
    return acc


def block_sum32(per_thread):
    """block_sum of select.hip in float32, in its order: the 6-step xor butterfly inside each wave of 64, then the 16 waves' sums
    added to 0 one after the other."""
    v = np.asarray(per_thread, F).reshape(16, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lane ^ o]).astype(F)
    t = F(0)
    for w in range(16):
        t = F(t + v[w, 0])
    return t


def select_underflow32(e, a0):
    """select_body bit for bit where expf returns exactly 1 on the maxima and exactly 0 everywhere else (tau (e - max) < -150): p,
    eval_action and psum in the kernel's own order -- the per-thread fma chains (exact in float64 for these small-integer actions, then
    rounded once) and block_sum32.  Exact for every number m of tied maxima, also where fl(1 / m) m is not 1."""
    e = np.asarray(e, F)
    w = (e == e.max()).astype(F)
    tot = block_sum32(thread_sums32(w))
    p = (w / tot).astype(F)
    psum = block_sum32(thread_sums32(p))
    a0 = np.asarray(a0, F)
    ev = np.zeros(a0.shape[1], F)
    rows = -(-e.size // 1024)
    pp = np.zeros(rows * 1024, F)
    pp[:e.size] = p
    for a in range(a0.shape[1]):
        aa = np.zeros(rows * 1024, F)
        aa[:e.size] = a0[:, a]
        acc = np.zeros(1024, F)
        for s_ in range(rows):
            acc = (aa[s_ * 1024:(s_ + 1) * 1024].astype(np.float64) * pp[s_ * 1024:(s_ + 1) * 1024].astype(np.float64) + acc.astype(np.float64)).astype(F)
        ev[a] = F(block_sum32(acc) / psum)
    return p, ev, psum


def select_ref32(e, a0, tau, q=None):
    """The same operation evaluated in float32 NumPy (not the kernel's summation order): what the bounds are held to on the CPU."""
    e = np.asarray(e, F)
    x = ((e - e.max()) * F(tau)).astype(F)
    w = np.exp(x).astype(F)
    tot = F(0)
    for c in range(0, e.size, 1024):  # a different, but also fixed, order
        tot = F(tot + w[c:c + 1024].sum(dtype=F))
    p = (w / tot).astype(F)
    ev = None
    if a0 is not None:
        ev = ((p[:, None] * np.asarray(a0, F)).astype(F).sum(axis=0, dtype=F) / p.sum(dtype=F)).astype(F)
    return p, ev


# ------------------------------------------------------------------------------------------------ float32 restatements
def window_stats_ref(v, idx, kk, kmin, kmax, window, rr=0, idx_front=None):
    """window_stats_kernel: (n, margin, mx, cnt), top_scores[-rr .. kk)."""
    v = np.asarray(v, F)
    mx = v[idx[0]]
    thr = F(mx - F(window))
    cnt = int((v >= thr).sum())
    n = min(min(max(cnt, kmin), kmax), kk)
    margin = F(mx - v[idx[n]]) if n < kk else F(np.inf)
    full = np.concatenate([np.asarray(idx_front, np.int64)[len(idx_front) - rr:] if rr else np.zeros(0, np.int64), np.asarray(idx[:kk], np.int64)])
    return (n, margin, mx, cnt), v[full]


def lower_median(d):
    """The element of rank (m - 1) // 2 of the ascending order (value, then position)."""
    d = np.asarray(d)
    return d[np.argsort(d, kind="stable")[(d.size - 1) // 2]]


def race_key32(tau, e, q):
    """float32 evaluation with numpy's log (NOT bit-equal to logf: for the CPU checks of key_bound only)."""
    return (F(tau) * np.asarray(e, F)).astype(F) - np.log(np.asarray(q, F)).astype(F)


def merge_ref(b, lst, r, n, list_scores, f, delta, expo=None, tau=0.0):
    """rescore_merge_body.  Returns a dict: c, dev, need, margin, thr (float32, exact on the GPU), merged (float32, exact), and for a
    race merge kbest / thr_r (float64) with kbound / thr_r_bound, and need_race (the float64 count)."""
    b = np.asarray(b, F)
    lst = np.asarray(lst, np.int64)[: r + n]
    ls = np.asarray(list_scores, F)[: r + n]
    f = np.asarray(f, F)[: r + n]
    m = r + n
    d = (ls - f).astype(F)
    c = F(lower_median(d))
    dev = F(np.abs((d - c).astype(F)).max())
    fbest = F(f.max())
    thr = F(F(fbest + c) - F(delta))
    need = int((b > thr).sum())
    b_last = ls[m - 1]
    un = b[b < b_last]
    bout = F(un.max()) if un.size else F(-np.inf)
    margin = F(np.inf) if n >= b.size else F(thr - bout)
    merged = (b - c).astype(F)
    merged[lst[r:]] = f[r:]
    merged[lst[:r]] = f[:r]
    out = dict(c=c, dev=dev, need=need, margin=margin, thr=thr, merged=merged)
    if expo is not None:
        q = np.asarray(expo, F)
        kf = race_keys64(tau, f, q[lst])
        kb = key_bound(tau, f, q[lst])
        j = int(np.argmax(kf))
        kbest, kbound = float(kf[j]), float(kb.max())  # (the float32 maximum may be another entry's key: the largest bound covers it)
        shift = np.float64(F(F(tau) * F(c - F(delta))))
        thr_r = kbest + shift
        thr_r_bound = kbound + 2 * U32 * (abs(thr_r) + kbound)
        keys = race_keys64(tau, b, q)
        out.update(kbest=kbest, kbound=kbound, thr_r=thr_r, thr_r_bound=thr_r_bound, keys=keys, keys_bound=key_bound(tau, b, q),
                   need_race=int((keys >= thr_r).sum()))
    return out


def deviation_ref(b, f):
    """deviation_stats_kernel: (c, max |d - c|, max |f|), all float32 and exact on the GPU."""
    b, f = np.asarray(b, F), np.asarray(f, F)
    d = (b - f).astype(F)
    c = F(lower_median(d))
    return c, F(np.abs((d - c).astype(F)).max()), F(np.abs(f).max())


def scatter_ref(dst, src, index):
    out = np.array(dst, copy=True)
    out[np.asarray(index, np.int64)] = src
    return out


# ------------------------------------------------------------------------------------------------ inputs, shared by the CPU and GPU files
def rng(seed):
    return np.random.default_rng(seed)


def topk_values(regime, n, seed):
    """The value regimes of the top-k cases (float32)."""
    g = rng(seed)
    if regime == "randn":
        return g.standard_normal(n).astype(F)
    if regime == "few":  # a handful of distinct values: the index decides
        return (np.round(g.standard_normal(n) * 2.0) / 2.0).astype(F)
    if regime == "equal":
        return np.full(n, 1.25, F)
    if regime == "zeros":  # +0.0 mixed with -0.0 (and a few ones)
        v = np.where(g.random(n) < 0.5, F(0.0), F(-0.0)).astype(F)
        v[g.random(n) < 0.1] = 1.0
        return v
    if regime == "inf":  # +inf and -inf entries, more -inf than finite: k can exceed the count of finite scores
        v = g.standard_normal(n).astype(F)
        c = g.random(n)
        v[c < 0.6] = -np.inf
        v[c > 0.95] = np.inf
        return v
    if regime == "denormal":
        return (g.integers(-40, 41, n).astype(np.float64) * 2.0 ** -149).astype(F)
    raise ValueError(regime)


TOPK_REGIMES = ("randn", "few", "equal", "zeros", "inf", "denormal")


def select_inputs(regime, n, A, seed):
    """(e, a0, tau, q) of a select case.  underflow_m: m tied maxima, everything else 400 below at tau = 1 (expf gives exactly 0),
    small-integer actions; tie: two candidates with identical e and q that win the race."""
    g = rng(seed)
    q = np.maximum(g.exponential(1.0, n), 2.0 ** -25).astype(F)
    a0 = g.standard_normal((n, A)).astype(F)
    if regime.startswith("underflow"):
        m = min(int(regime[len("underflow"):]), n)
        e = (g.standard_normal(n) * 2.0).astype(F) - F(400.0)
        top = np.sort(g.choice(n, m, replace=False))
        e[top] = F(7.0)
        a0 = g.integers(-8, 9, (n, A)).astype(F)
        a0[top] = (g.integers(-2, 3, (m, A)) * 4).astype(F)  # multiples of 4: the mean over m in {1, 2, 4} is exact
        return e, a0, 1.0, q
    if regime == "tau0.01":
        e, tau = (g.standard_normal(n) * 15.0 + 400.0).astype(F), 0.01
    elif regime in ("tau1", "tie"):
        e, tau = (g.standard_normal(n) * 0.5).astype(F), 1.0
    else:
        raise ValueError(regime)
    if regime == "tie" and n >= 4:
        i, j = sorted(g.choice(n, 2, replace=False))
        e[i] = e[j] = F(e.max() + F(1.0))
        q[i] = q[j] = F(2.0 ** -22)  # p / q of the pair is far above everyone else's: they tie for the race, i < j wins
    return e, a0, tau, q
