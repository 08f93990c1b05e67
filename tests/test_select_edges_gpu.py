"""Every kernel of m3pc_amd/csrc/select.hip alone, at its edges, against the references of tests/select_ref.py: through the lab hooks
m3pc_debug_topk_ex, _topk_race_batch, _window_stats, _scatter, _select_batch, _merge_select_batch, _calibrate_stats, _eval_bound_batch,
_gather_listed, _variates_batch and, for the one-window merge / select / eval-bound kernels, through the public entry points of a small
handle (m3pc_select, m3pc_rescore_merge, m3pc_rescore_merge_race, m3pc_merge_race_select, m3pc_eval_bound, m3pc_draw_variates).

Every launch asserts the kernel id its launcher recorded ("Selection kernel ids" in include/m3pc_hip_debug.h);
test_every_selection_kernel_was_reached checks that the file reached exactly the ids of that list.  Lists, counts, medians, margins and
merged vectors are compared for EQUALITY: tests/test_select_ref_cpu.py asserts, on the references alone, that no case of this file leaves
a decision inside a rounding bound (no two race keys among the listed positions closer than their key bounds, no key within its bound of
a race threshold), except the exact ties and exact threshold hits the cases plant.  p and eval_action are held to the element-wise
bounds select_ref derives; two regimes (everything but m tied maxima underflows; a planted exact tie in the race) are exact there too.
NaN sits in everything a kernel may not read (entries past n, padding columns of a0, list slots outside the slice); every output has
sentinels around it that are compared bit for bit with their state before the call.  The case builders are NumPy only: importing this
file needs no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import select_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F = np.float32
vp, ci, cf, ll = C.c_void_p, C.c_int, C.c_float, C.c_longlong
pi = C.POINTER(ci)
G = 8            # guard elements in front of and behind every output
ISENT = -77      # sentinel of int outputs
FSENT = -31744.0  # sentinel of float outputs
WINDOWS = (1, 3, 65)
REACHED = set()
WORST = {}  # (kernel id, output) -> largest err / bound


class TopkArgs(C.Structure):
    """m3pc_debug_topk_args."""
    _fields_ = [("v", vp), ("expo", vp), ("tau", cf), ("n_windows", ci), ("n", ci), ("k", ci), ("out", vp), ("out_stride", ci),
                ("scores_out", vp), ("kk", ci), ("variant", ci), ("picked", pi), ("stream", vp)]


class TailArgs(C.Structure):
    """m3pc_debug_tail_args."""
    _fields_ = [("scores", vp), ("expo", vp), ("race", ci), ("select", ci), ("temperature", cf), ("n_windows", ci), ("n_total", ci),
                ("list", vp), ("list_scores", vp), ("list_rescored", vp), ("rmax", ci), ("list_stride", ci), ("f_stride", ci), ("f_lo", ci),
                ("r", pi), ("n", pi), ("delta", C.POINTER(cf)), ("merged", vp), ("stats", vp), ("host_stats", vp), ("seq", cf), ("a0", vp),
                ("a0_window_stride", ll), ("a0_stride", ll), ("A", ci), ("p", vp), ("eval_action", vp), ("argmax", vp), ("sample_idx", vp),
                ("sample_action", vp), ("stream", vp)]


class EvalBatchArgs(C.Structure):
    """m3pc_debug_eval_batch_args."""
    _fields_ = [("merged", vp), ("n_windows", ci), ("n_total", ci), ("list", vp), ("rmax", ci), ("list_stride", ci), ("n_listed", ci),
                ("r", pi), ("n", pi), ("delta", C.POINTER(cf)), ("a0", vp), ("a0_window_stride", ll), ("a0_stride", ll), ("A", ci),
                ("temperature", cf), ("eval_tol", cf), ("stats", vp), ("host_stats", vp), ("seq", cf), ("stream", vp)]


def declare(lib):
    """Prototypes of the hooks this file and tests/test_select_ref_cpu.py call."""
    lib.m3pc_debug_topk.restype, lib.m3pc_debug_topk.argtypes = ci, [vp, ci, ci, vp, vp]
    lib.m3pc_debug_topk_ex.restype, lib.m3pc_debug_topk_ex.argtypes = ci, [C.POINTER(TopkArgs)]
    lib.m3pc_debug_select_picked.restype, lib.m3pc_debug_select_picked.argtypes = ci, []
    lib.m3pc_debug_select_picked_set.restype, lib.m3pc_debug_select_picked_set.argtypes = C.c_uint, [ci]
    lib.m3pc_debug_window_stats.restype, lib.m3pc_debug_window_stats.argtypes = ci, [vp, ci, vp, ci, ci, ci, cf, vp, vp, cf, vp, ci, vp]
    lib.m3pc_debug_scatter.restype, lib.m3pc_debug_scatter.argtypes = ci, [vp, vp, ci, vp, vp, vp]
    lib.m3pc_debug_variates_batch.restype = ci
    lib.m3pc_debug_variates_batch.argtypes = [C.c_ulonglong, C.POINTER(C.c_ulonglong), ci, ll, ll, vp, vp]
    lib.m3pc_debug_topk_race_batch.restype, lib.m3pc_debug_topk_race_batch.argtypes = ci, [vp, vp, cf, ci, ci, ci, ci, ci, vp, vp, vp]
    lib.m3pc_debug_gather_listed.restype, lib.m3pc_debug_gather_listed.argtypes = ci, [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp]
    lib.m3pc_debug_merge_select_batch.restype, lib.m3pc_debug_merge_select_batch.argtypes = ci, [C.POINTER(TailArgs)]
    lib.m3pc_debug_eval_bound_batch.restype, lib.m3pc_debug_eval_bound_batch.argtypes = ci, [C.POINTER(EvalBatchArgs)]
    lib.m3pc_debug_select_batch.restype = ci
    lib.m3pc_debug_select_batch.argtypes = [vp, vp, ll, ll, ci, ci, ci, cf, vp, vp, vp, vp, vp, vp, vp]
    lib.m3pc_debug_calibrate_stats.restype, lib.m3pc_debug_calibrate_stats.argtypes = ci, [vp, vp, ci, cf, vp, C.POINTER(cf), vp]
    return lib


def header_ids():
    src = open(os.path.join(ROOT, "include", "m3pc_hip_debug.h")).read()
    block = src[src.index("Selection kernel ids:"):src.index("(end of the selection kernel ids)")]
    return {int(n): k for n, k in re.findall(r"(?:^|;|\*)\s*(\d+) ([a-z0-9_]+_kernel)", block, re.M)}


# ================================================================================================ the case tables (NumPy only)
def topk_ks(n):
    return sorted({k for k in (1, 63, 64, 65, 129, 1024, n) if k <= n})


def topk_variants(n, k):
    """(variant, kernel id) of every form of m3pc_debug_topk_ex that is legal for one window of n values and k ranks."""
    out = [(0, 7 if n <= 2048 else 5 if k <= 64 else 3)]
    if n <= 2048:
        out += [(1, 12), (2, 7)]
    if k <= 64:
        out.append((3, 5))
    out.append((4, 3))
    return out


def topk_batch_kid(n, k):
    return 8 if n <= 2048 else 6 if k <= 64 else 4


def topk_batch_ks(n):
    return sorted({k for k in (1, 64, 65, 129, n if n <= 2048 else 1024) if k <= n})


RACE_FLAVOURS = (("tau0.01", 0.01), ("tau1", 1.0), ("tie", 1.0))


def race_case(n, flavour, seed=0):
    """(e, q, tau, rr, kk): scores, Exp(1) variates, the number of racers and of score entries listed.  tie: two candidates with
    identical e and q whose key is the best of all -- the lower index ranks first."""
    tau = dict(RACE_FLAVOURS)[flavour]
    for attempt in range(16):  # the first draw whose listed race keys lie further apart than their bounds (the CPU file asserts it)
        g = R.rng(7000 + 13 * n + seed + 100003 * attempt)
        e = (g.standard_normal(n) * (15.0 if tau < 0.1 else 0.5) + (400.0 if tau < 0.1 else 0.0)).astype(F)
        q = np.maximum(g.exponential(1.0, n), 2.0 ** -25).astype(F)
        if flavour == "tie" and n >= 2:
            i, j = sorted(g.choice(n, 2, replace=False))
            e[i] = e[j] = F(e.max() + F(0.5))
            q[i] = q[j] = F(2.0 ** -22)
        if flavour == "tau0.01" and n >= 4:  # the last two candidates rank first and second by score: the last key pair of the last
            e[n - 1] = F(e.max() + F(30.0))  # quarter of a ranking kernel's loop decides every other rank
            e[n - 2] = F(e[n - 1] - F(15.0))
        if not R.close_pairs(R.race_keys64(tau, e, q), R.key_bound(tau, e, q), min(64, n)):
            break
    return e, q, tau, min(64, n), min(129, n)


def race_cases():
    return [(n, fl) for n in R.SIZES for fl, _ in RACE_FLAVOURS]


SELECT_SIZES = R.SIZES + (16385,)
# underflow25: fl(1 / 25) does not sum to 1 -- the one regime in which the division by psum shows in the bits
SELECT_REGIMES = ("tau0.01", "tau1", "underflow1", "underflow2", "underflow4", "underflow25", "tie")
SELECT_SHAPES = ((1, 1), (3, 1), (3, 4), (17, 1), (17, 4))  # (A, a0_stride / A)


def select_case(n, regime, A, seed=0):
    return R.select_inputs(regime, n, A, 9000 + 17 * n + 3 * A + seed)


def select_cases():
    """(n, regime, A, mult) of every single-window select the GPU file holds to the reference."""
    out = []
    for n in SELECT_SIZES:
        for regime in SELECT_REGIMES:
            for A, mult in (SELECT_SHAPES if n <= 16384 else ((3, 1), (3, 4))):
                out.append((n, regime, A, mult))
    return out


MERGE_PAIRS = ((0, 1), (0, 1024), (64, 960), (2, 8), (32, 128))
MERGE_CASES = [(r, n, nt, flavour) for (r, n) in MERGE_PAIRS for nt in sorted({max(r + n, n, 2) if r + n < 1024 else 1024, 1024, 4097})
               for flavour in ("randn", "tied", "delta0", "planted") if n <= nt]


def merge_case(r, n, n_total, flavour, seed=0):
    """A synthetic certified merge: b = f + 3.25 + noise over n_total candidates, the n best by b listed behind the r best by race key
    (best racer last, as m3pc_topk_race_window lays them out), the best scorer planted among the racers too (a candidate in both
    parts).  tied: the noise is a small multiple of 1/8 and f a multiple of 2^-6, so that d = b - f is exact and ties at the lower
    median.  planted: delta is chosen so that the threshold lies below every listed score; two un-listed candidates are then planted
    AT thr (not counted) and one ulp above it (counted), and one un-listed candidate behind the last listed one gets its score
    (b_last); the three get a large q, which keeps them out of the race list."""
    g = R.rng(5000 + 131 * r + 7 * n + n_total + seed)
    tau = 1.0 if (r + n) % 3 else 0.01
    scale = 0.5 if tau == 1.0 else 15.0
    delta = 0.0 if flavour == "delta0" else 0.05 if tau == 1.0 else 5.0
    if flavour == "tied":
        f_all = (np.round(g.standard_normal(n_total) * scale * 64) / 64 + 100.0).astype(F)
        b = (f_all + F(3.25) + (g.integers(-3, 4, n_total) * 0.125).astype(F)).astype(F)
    else:
        f_all = (g.standard_normal(n_total) * scale + 100.0).astype(F)
        b = (f_all + F(3.25) + ((g.random(n_total) - 0.5) * 1.6 * max(delta, 0.01)).astype(F)).astype(F)
    q = np.maximum(g.exponential(1.0, n_total), 2.0 ** -25).astype(F)
    planted = {}

    def lists():
        score = R.topk_order(b, n)
        race = R.race_order(tau, b, q, r)[::-1].copy()
        if r and score[0] not in race:
            race[0] = score[0]
        return np.concatenate([race, score]).astype(np.int32)

    lst = lists()
    ls, f = b[lst], f_all[lst]
    un = np.setdiff1d(np.arange(n_total), lst)
    if flavour == "planted" and un.size >= 3:
        ref = R.merge_ref(b, lst, r, n, ls, f, 0.0)
        delta = float(F(ref["thr"] - ls[-1] + F(0.25 * scale)))  # thr(delta = 0) = fbest + c: the new thr lies scale / 4 below b_last
        thr = R.merge_ref(b, lst, r, n, ls, f, delta)["thr"]
        assert thr < ls[-1]
        lo = un[np.argsort(b[un], kind="stable")[:2]]  # the two lowest un-listed scores: far below the list
        hi = np.setdiff1d(un[un > lst[-1]], lo)
        q[lo] = F(1000.0)
        b[lo[0]], b[lo[1]] = thr, np.nextafter(thr, F(np.inf))
        planted = dict(at_thr=int(lo[0]), above_thr=int(lo[1]))
        if hi.size:
            q[hi[-1]], b[hi[-1]] = F(1000.0), ls[-1]
            planted["at_b_last"] = int(hi[-1])
        assert np.array_equal(lists(), lst), "planting moved a listed entry"
    return dict(b=b, q=q, tau=tau, delta=delta, lst=lst, ls=ls, f=f, r=r, n=n, planted=planted)


WINDOW_CASES = [  # (n_total, kk, kmin, kmax, window flavour, rr)
    (1, 1, 1, 1, "zero", 0), (2, 2, 1, 1, "edge", 1), (255, 65, 8, 64, "edge", 0), (256, 129, 8, 128, "zero", 64),
    (257, 129, 8, 128, "below_kmin", 1), (1025, 129, 8, 128, "above_kmax", 64), (1025, 100, 8, 128, "above_kk", 0),
    (1024, 1024, 1, 1023, "edge", 64), (16384, 1024, 8, 1023, "edge", 64), (16384, 129, 8, 128, "above_kmax", 1)]


def window_case(n_total, kk, kmin, kmax, flavour, rr, seed=0):
    """(v, front, idx, window): idx = the kk best of v, front = rr arbitrary candidates in front of it.  edge: three candidates are
    planted exactly AT fl(mx - window) (inside) and three one ulp below it (outside); zero: window = 0 with the maximum held by
    three candidates; below_kmin / above_kmax / above_kk: a window that holds 2 / kmax + 7 / kk + 5 candidates."""
    g = R.rng(3000 + n_total + 7 * kk + rr + seed)
    v = (g.standard_normal(n_total) * 15.0 + 400.0).astype(F)
    srt = np.sort(v)[::-1]
    window = 0.0
    if flavour == "zero":
        v[g.choice(n_total, min(3, n_total), replace=False)] = F(srt[0] + F(1.0))
    elif flavour == "edge" and n_total >= 8:
        window = float(F(10.0))
        mx = v.max()
        thr = F(mx - F(window))
        spots = g.choice(np.flatnonzero(v < thr - F(1.0)), 6, replace=False) if (v < thr - F(1.0)).sum() >= 6 else []
        for j, s in enumerate(spots):
            v[s] = thr if j < 3 else np.nextafter(thr, F(-np.inf))
    elif flavour in ("below_kmin", "above_kmax", "above_kk"):
        want = {"below_kmin": 2, "above_kmax": kmax + 7, "above_kk": kk + 5}[flavour]
        window = float(F(F(srt[0] - srt[want - 1]) + F(srt[want - 1] - srt[want]) * F(0.5)))
    idx = R.topk_order(v, kk).astype(np.int32)
    front = g.integers(0, n_total, rr).astype(np.int32)
    return v, front, idx, window


CALIB_SIZES = (1023, 1025, 2047, 2049, 8193, 16383)


def calib_case(n, seed=0):
    """The planted-tie recipe of tests/test_certified_step_gpu.py: b = f + 3.25 + noise, two exact ties in d = b - f, one AT the
    lower median, so that the (value, index) order decides the rank there."""
    g = R.rng(100 + n + seed)
    f = (g.standard_normal(n) * 15.0 + 100.0).astype(F)
    b = (f + (3.25 + (g.random(n) - 0.5) * 2.0).astype(F)).astype(F)
    order = np.argsort((b - f).astype(F), kind="stable")
    for src, dst in ((order[(n - 1) // 2], order[(n - 1) // 2 + 1]), (order[n // 4], order[n // 4 + 1])):
        f[dst], b[dst] = f[src], b[src]
    return b, f


SCATTER_SIZES = (1, 255, 256, 257, 1024)

# the kernel ids each family of cases names (tests/test_select_ref_cpu.py holds the union to the header's list)
CASE_IDS = {"topk": {3, 5, 7, 12}, "topk_batch": {4, 6, 8}, "topk_race": {5, 9, 10}, "topk_race_batch": {11}, "select": {1, 2},
            "window": {13}, "merge": {14, 15, 16}, "calibration": {17}, "eval_bound": {18, 19}, "scatter": {20}, "gather": {21},
            "variates": {22, 23}}


# ================================================================================================ GPU plumbing
@pytest.fixture(scope="module")
def lib():
    from hip_util import lab_library
    return declare(lab_library())


@pytest.fixture(scope="module")
def handle(lib):
    """A small handle of the lab library (action_dim 3): the public entry points read its device and its A only."""
    from m3pc_amd import capi
    dims = capi.Dims(11, 3, 8, 64, 2, 1, 1, 8, 1, 0, 64, 0)
    h = vp()
    assert lib.m3pc_create(C.byref(dims), 0, C.byref(h)) == 0, lib.m3pc_last_error()
    yield h
    lib.m3pc_destroy(h)


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def nan_tail(a, pad=G):
    """a (float32, any shape, flattened) followed by `pad` NaN: what lies past n may not be read."""
    a = np.asarray(a, F).reshape(-1)
    return dev(np.concatenate([a, np.full(pad, np.nan, F)]))


def guarded(count, dtype):
    """A sentinel buffer of G + count + G elements; returns (buffer, pointer to element G, copy before the call)."""
    sent = ISENT if dtype == torch.int32 else FSENT
    buf = torch.full((G + max(count, 0) + G,), sent, device=DEV, dtype=dtype)
    return buf, buf.data_ptr() + G * buf.element_size(), buf.clone()


def bits(t):
    return t.contiguous().view(torch.int32)


def owned(buf, before, lo, hi, what):
    """buf[G + lo, G + hi) belongs to the call; everything else keeps its bits.  Returns the owned part (numpy)."""
    after = buf.clone()
    after[G + lo:G + hi] = before[G + lo:G + hi]
    assert torch.equal(bits(after), bits(before)), f"{what}: a guard element was written"
    return buf[G + lo:G + hi].cpu().numpy()


def picked_is(lib, want, what):
    got = lib.m3pc_debug_select_picked()
    assert got == want, f"{what}: the launcher recorded kernel {got}, the case is for {want}"
    REACHED.add(want)


def record(kid, key, err, bound, what):
    ratio = float(np.max(err / bound)) if np.size(err) else 0.0
    print(f"{what}: {key} err / bound {ratio:.3g}")
    assert ratio <= 1.0, f"{what}: {key} misses its bound, err / bound = {ratio:.4g}"
    WORST[(kid, key)] = max(WORST.get((kid, key), 0.0), ratio)


def topk_ex(lib, v_dev, n, k, variant, want, what, expo=None, tau=0.0, windows=1, out_stride=1, kk=0, scores=False, want_first=0):
    """One m3pc_debug_topk_ex call on a guarded list.  Plain source: returns the (windows, k) ranks.  Race pair (expo with variant 0 or
    5): returns (racers best first, score entries, racers' scores, score entries' scores)."""
    pair = expo is not None and variant in (0, 5)
    front = k if (pair or out_stride == -1) else 0
    count = front + (kk if pair else 0 if out_stride == -1 else windows * k)
    buf, ptr, before = guarded(count, torch.int32)
    sbuf, sptr, sbefore = guarded(count, torch.float32)
    a = TopkArgs()
    a.v, a.expo, a.tau = v_dev.data_ptr(), None if expo is None else expo.data_ptr(), tau
    a.n_windows, a.n, a.k, a.out_stride, a.kk, a.variant = windows, n, k, out_stride, kk, variant
    a.out = ptr + 4 * (front if pair else (front - 1) if out_stride == -1 else 0)
    a.scores_out = (sptr + 4 * front) if scores else None
    pk = (ci * 2)(-1, -1)
    a.picked, a.stream = C.cast(pk, pi), stream()
    assert lib.m3pc_debug_topk_ex(C.byref(a)) == 0, (what, lib.m3pc_last_error())
    torch.cuda.synchronize()
    assert pk[0] == want and pk[0] == lib.m3pc_debug_select_picked(), f"{what}: the launcher recorded kernel {pk[0]}, the case is for {want}"
    assert pk[1] == want_first, f"{what}: the score list was ranked by kernel {pk[1]}, the case is for {want_first}"
    REACHED.update({want} | ({want_first} if want_first else set()))
    got = owned(buf, before, 0, count, what)
    assert not (got == ISENT).any(), f"{what}: a rank was not written"
    sgot = owned(sbuf, sbefore, 0, count if scores else 0, what + " scores")
    if pair:
        return got[:front][::-1], got[front:], (sgot[:front][::-1], sgot[front:]) if scores else None
    if out_stride == -1:
        return got[::-1].reshape(1, k)
    return got.reshape(windows, k)


# ================================================================================================ top-k
@pytest.mark.parametrize("n", R.SIZES)
def test_topk_every_variant_equals_the_stable_order(lib, n):
    """The dispatch and every forced kernel that is legal for (n, k), on six value regimes: each list EQUALS the stable order, hence
    every variant equals every other."""
    for regime in R.TOPK_REGIMES:
        v = R.topk_values(regime, n, 11 * n + len(regime))
        vd = nan_tail(v)
        order = R.topk_order(v)
        for k in topk_ks(n):
            for variant, kid in topk_variants(n, k):
                what = f"topk n {n} k {k} {regime} variant {variant}"
                got = topk_ex(lib, vd, n, k, variant, kid, what)[0]
                assert np.array_equal(got, order[:k]), f"{what}: differs from the stable order at rank {int(np.flatnonzero(got != order[:k])[0])}"


@pytest.mark.parametrize("n", [2049, 4096, 16384])
def test_topk_selection_lists_minus_inf_entries_once(lib, n):
    """-inf scores with k above the number of finite ones: the selection kernel (variant 3, and the dispatch at k <= 64) must list
    distinct elements -- the finite ones, then the -inf ones in index order -- as the bitonic kernel does.  Before winners were
    removed by index, the lowest -inf element came back in every remaining round."""
    g = R.rng(n)
    v = np.full(n, -np.inf, F)
    fin = g.choice(n, 10, replace=False)
    v[fin] = g.standard_normal(10).astype(F)
    vd = nan_tail(v)
    for k in (11, 64):
        ref = R.topk_order(v, k)
        assert len(set(ref.tolist())) == k and not np.isfinite(v[ref[10:]]).any()
        lists = {variant: topk_ex(lib, vd, n, k, variant, kid, f"-inf n {n} k {k} variant {variant}")[0] for variant, kid in topk_variants(n, k)}
        for variant, got in lists.items():
            assert len(set(got.tolist())) == k, f"n {n} k {k} variant {variant}: an element is listed twice"
            assert np.array_equal(got, ref), f"n {n} k {k} variant {variant}"


# launch_topk's dispatch through m3pc_debug_topk on torch's own stable sort, at the (n, k) of the fp32 re-score and its neighbours
@pytest.mark.parametrize("n", [5, 64, 1000, 1024, 1025, 2048, 2049, 8192, 16384])
@pytest.mark.parametrize("k", [1, 16, 64])
def test_topk_order_matches_stable_sort(lib, n, k):
    if k > n:
        pytest.skip("k <= n by contract")
    g = torch.Generator(device=DEV).manual_seed(n * 131 + k)
    for ties in (False, True):
        v = torch.randn(n, device=DEV, generator=g)
        if ties:
            v = torch.round(v * 2.0) / 2.0  # a handful of distinct values: the order is decided by the index
        out = torch.full((k,), -1, device=DEV, dtype=torch.int32)
        assert lib.m3pc_debug_topk(v.data_ptr(), n, k, out.data_ptr(), stream()) == 0, lib.m3pc_last_error()
        torch.cuda.synchronize()
        picked_is(lib, 7 if n <= 2048 else 5, f"topk n {n} k {k}")
        ref = torch.sort(-v, stable=True).indices[:k].to(torch.int32)
        assert torch.equal(out, ref), (n, k, ties)


@pytest.mark.parametrize("n", R.SIZES)
def test_topk_batch_rows_are_the_one_window_lists(lib, n):
    """launch_topk_batch (variant 6) at 1, 3 and 65 windows: row w is bit for bit the one-window list of row w, which is the stable order."""
    for regime in ("randn", "inf"):
        rows = np.stack([R.topk_values(regime, n, 500 * w + n) for w in range(max(WINDOWS))])
        for E in WINDOWS:
            vd = nan_tail(rows[:E])
            for k in topk_batch_ks(n):
                what = f"topk batch n {n} k {k} windows {E} {regime}"
                got = topk_ex(lib, vd, n, k, 6, topk_batch_kid(n, k), what, windows=E)
                for w in range(E):
                    assert np.array_equal(got[w], R.topk_order(rows[w], k)), f"{what}: window {w}"
                    if w in (0, E - 1):
                        one = topk_ex(lib, nan_tail(rows[w]), n, k, 0, topk_variants(n, k)[0][1], what + " one window")[0]
                        assert np.array_equal(got[w], one), f"{what}: window {w} differs from the one-window call"


@pytest.mark.parametrize("n,flavour", race_cases())
def test_topk_race_sources(lib, n, flavour):
    """launch_topk_race (topk_rank_blocks2_kernel / topk_rank_blocks2_dyn_kernel), its refused-opt-in branch (launch_topk +
    topk_select_kernel on the race keys) and the forced selection kernel on a race source, out_stride 1 and -1: the race list EQUALS
    the float64 key order, the score list the stable order, scores_out is v[winner] bit for bit."""
    e, q, tau, rr, kk = race_case(n, flavour)
    ed, qd = nan_tail(e), nan_tail(q)
    racers, scorers = R.race_order(tau, e, q, rr), R.topk_order(e, kk)
    one = 9 if n <= 2048 else 10
    what = f"race n {n} {flavour}"
    r0, s0, sc = topk_ex(lib, ed, n, rr, 0, one, what + " variant 0", expo=qd, tau=tau, out_stride=-1, kk=kk, scores=True, want_first=one)
    assert np.array_equal(r0, racers), f"{what}: the race list differs from the float64 key order"
    assert np.array_equal(s0, scorers), f"{what}: the score list differs from the stable order"
    assert np.array_equal(sc[0].view(np.uint32), e[racers].view(np.uint32)) and np.array_equal(sc[1].view(np.uint32), e[scorers].view(np.uint32))
    r5, s5, _ = topk_ex(lib, ed, n, rr, 5, 5, what + " variant 5", expo=qd, tau=tau, out_stride=-1, kk=kk, want_first=topk_variants(n, kk)[0][1])
    assert np.array_equal(r5, racers) and np.array_equal(s5, scorers), f"{what}: the refused-opt-in branch differs"
    for stride in (1, -1):
        r3 = topk_ex(lib, ed, n, rr, 3, 5, what + f" variant 3 stride {stride}", expo=qd, tau=tau, out_stride=stride)[0]
        assert np.array_equal(r3, racers), f"{what}: the selection kernel on the race keys differs (out_stride {stride})"


@pytest.mark.parametrize("n", R.SIZES)
def test_topk_race_batch_rows_are_the_one_window_lists(lib, n):
    """topk_rank_batch_kernel at 1, 3 and 65 windows: list and scores of window w are launch_topk_race's on row w, bit for bit."""
    rmax, kmax = min(64, n), min(128, max(n - 1, 1))
    kk, LS = min(kmax + 1, n), rmax + kmax + 1
    rows = [race_case(n, "tau0.01", seed=w) for w in range(max(WINDOWS))]
    tau = rows[0][2]
    for E in WINDOWS:
        ed, qd = nan_tail(np.stack([r[0] for r in rows[:E]])), nan_tail(np.stack([r[1] for r in rows[:E]]))
        lst, lptr, lbefore = guarded(E * LS, torch.int32)
        sc, sptr, sbefore = guarded(E * LS, torch.float32)
        assert lib.m3pc_debug_topk_race_batch(ed.data_ptr(), qd.data_ptr(), tau, E, n, kmax, 1, rmax, lptr, sptr, stream()) == 0, lib.m3pc_last_error()
        torch.cuda.synchronize()
        picked_is(lib, 11, f"race batch n {n} windows {E}")
        L = owned(lst, lbefore, 0, E * LS, "race batch list").reshape(E, LS)
        S = owned(sc, sbefore, 0, E * LS, "race batch scores").reshape(E, LS)
        assert (L[:, rmax + kk:] == ISENT).all() and (S[:, rmax + kk:] == F(FSENT)).all(), "a slot behind the kk score entries was written"
        for w in range(E):
            e, q = rows[w][0], rows[w][1]
            assert np.array_equal(L[w, :rmax][::-1], R.race_order(tau, e, q, rmax)) and np.array_equal(L[w, rmax:rmax + kk], R.topk_order(e, kk)), (n, E, w)
            assert np.array_equal(S[w, :rmax + kk].view(np.uint32), e[L[w, :rmax + kk]].view(np.uint32)), (n, E, w)
            if w in (0, E - 1):
                r0, s0, _ = topk_ex(lib, nan_tail(e), n, rmax, 0, 9 if n <= 2048 else 10, "race one window", expo=nan_tail(q), tau=tau,
                                    out_stride=-1, kk=kk, scores=True, want_first=9 if n <= 2048 else 10)
                assert np.array_equal(L[w, :rmax][::-1], r0) and np.array_equal(L[w, rmax:rmax + kk], s0), (n, E, w)


# ================================================================================================ select
def run_select(lib, handle, e, a0, mult, tau, q, windows=1, public=False, null=None):
    """select_batch_kernel through m3pc_debug_select_batch (any A), or select_kernel through m3pc_select (the handle's A = 3), on NaN-
    padded inputs and guarded outputs.  e (E, n), a0 (E, n, A), q (E, n) or None.  null: the name of one optional output to leave out.
    Returns dict name -> numpy (E, ...)."""
    E, n = e.shape
    A = a0.shape[2]
    ed = nan_tail(e)
    a0p = np.full((E, n, mult * A), np.nan, F)
    a0p[:, :, :A] = a0
    ad = nan_tail(a0p)
    qd = None if q is None else nan_tail(q)
    names = {"p": (E * n, torch.float32), "eval_action": (E * A, torch.float32), "argmax": (E, torch.int32),
             "sample_idx": (E, torch.int32), "sample_action": (E * A, torch.float32)}
    if q is None:
        names.pop("sample_idx"), names.pop("sample_action")
    if null:
        names.pop(null)
    bufs = {k: guarded(c, t) for k, (c, t) in names.items()}
    ptr = lambda k: bufs[k][1] if k in bufs else None
    if public:
        assert E == 1 and A == 3
        rc = lib.m3pc_select(handle, ed.data_ptr(), ad.data_ptr(), mult * A, n, tau, None if qd is None else qd.data_ptr(), ptr("p"),
                             ptr("eval_action"), ptr("argmax"), ptr("sample_idx"), ptr("sample_action"), stream())
    else:
        rc = lib.m3pc_debug_select_batch(ed.data_ptr(), ad.data_ptr(), n * mult * A, mult * A, E, n, A, tau, None if qd is None else qd.data_ptr(),
                                         ptr("p"), ptr("eval_action"), ptr("argmax"), ptr("sample_idx"), ptr("sample_action"), stream())
    assert rc == 0, lib.m3pc_last_error()
    torch.cuda.synchronize()
    picked_is(lib, 1 if public else 2, f"select n {n} A {A}")
    out = {}
    for k, (c, t) in names.items():
        out[k] = owned(bufs[k][0], bufs[k][2], 0, c, f"select {k}").reshape(E, -1)
        assert not (out[k] == (ISENT if t == torch.int32 else F(FSENT))).any(), f"select n {n}: {k} was not written"
    return out


def hold_select(out, e, a0, tau, q, regime, kid, what):
    """One window's outputs against select_ref: p and eval_action within their bounds (EQUAL in the underflow regime), the arg-max and
    the race winner equal, sample_action the winner's row bit for bit."""
    p64, ev64, am, si = R.select_ref(e, a0, tau, q)
    assert int(out["argmax"][0]) == am, f"{what}: arg-max {int(out['argmax'][0])}, reference {am}"
    assert int(out["sample_idx"][0]) == si, f"{what}: race winner {int(out['sample_idx'][0])}, reference {si}"
    assert np.array_equal(out["sample_action"].view(np.uint32), a0[si].view(np.uint32)), f"{what}: sample_action is not the winner's row"
    if regime.startswith("underflow"):
        m = int((e == e.max()).sum())
        assert m == min(int(regime[len("underflow"):]), e.size)
        p32, ev32, _ = R.select_underflow32(e, a0)
        assert np.array_equal(out["p"], p64.astype(F)) and set(np.unique(out["p"]).tolist()) <= {0.0, float(F(1.0 / m))}, f"{what}: p is not exactly 1 / {m} on the maxima"
        assert np.array_equal(out["p"].view(np.uint32), p32.view(np.uint32))
        assert np.array_equal(out["eval_action"].view(np.uint32), ev32.view(np.uint32)), f"{what}: eval_action {out['eval_action'].tolist()} is not the kernel's order in float32 {ev32.tolist()}"
        if m in (1, 2, 4):
            assert np.array_equal(out["eval_action"], a0[e == e.max()].astype(np.float64).mean(axis=0).astype(F)), f"{what}: eval_action is not the exact mean"
        return
    assert np.isfinite(out["p"]).all() and np.isfinite(out["eval_action"]).all()
    record(kid, "p", np.abs(out["p"].astype(np.float64) - p64), R.select_p_bound(e, tau), what)
    record(kid, "eval_action", np.abs(out["eval_action"].astype(np.float64) - ev64), R.select_eval_bound(e, a0, tau), what)


@pytest.mark.parametrize("n", SELECT_SIZES)
def test_select_against_fp64(lib, handle, n):
    """select_batch_kernel (one window, A in {1, 3, 17}, a0_stride A and 4 A) and select_kernel (m3pc_select, A = 3; the only one that
    takes n = 16385) in every regime; the two kernels are the same device function: bit-equal where both run."""
    for (n_, regime, A, mult) in [c for c in select_cases() if c[0] == n]:
        e, a0, tau, q = select_case(n, regime, A)
        what = f"select n {n} A {A} stride {mult}A {regime}"
        outs = []
        if n <= 16384:
            outs.append((2, run_select(lib, handle, e[None], a0[None], mult, tau, q[None])))
        if A == 3:
            outs.append((1, run_select(lib, handle, e[None], a0[None], mult, tau, q[None], public=True)))
        for kid, out in outs:
            hold_select({k: v[0] for k, v in out.items()}, e, a0, tau, q, regime, kid, what + f" kernel {kid}")
        if len(outs) == 2:
            for k in outs[0][1]:
                assert np.array_equal(outs[0][1][k].view(np.uint32), outs[1][1][k].view(np.uint32)), f"{what}: {k} of the two kernels differs"


@pytest.mark.parametrize("n", [1, 65, 1025, 16384])
def test_select_optional_outputs(lib, handle, n):
    """Each optional output null in turn, and no expo: the other outputs keep their bits."""
    e, a0, tau, q = select_case(n, "tau1", 3)
    for public in (False, True):
        full = run_select(lib, handle, e[None], a0[None], 4, tau, q[None], public=public)
        for null in ("p", "eval_action", "argmax", "sample_idx", "sample_action"):
            part = run_select(lib, handle, e[None], a0[None], 4, tau, q[None], public=public, null=null)
            for k, v in part.items():
                assert np.array_equal(v.view(np.uint32), full[k].view(np.uint32)), f"n {n}: {k} changed when {null} was left out"
        part = run_select(lib, handle, e[None], a0[None], 4, tau, None, public=public)
        for k, v in part.items():
            assert np.array_equal(v.view(np.uint32), full[k].view(np.uint32)), f"n {n}: {k} changed without expo"


@pytest.mark.parametrize("n", R.SIZES)
def test_select_batch_rows_are_the_one_window_results(lib, handle, n):
    """select_batch_kernel at 3 and 65 windows (A = 3 and 17, a0_stride 4 A): window w's outputs are the one-window call's on row w."""
    for A in (3, 17):
        rows = [select_case(n, ("tau1", "tau0.01", "tie", "underflow2")[w % 4], A, seed=w) for w in range(max(WINDOWS))]
        for E in WINDOWS[1:]:
            e, a0, q = (np.stack([r[i] for r in rows[:E]]) for i in (0, 1, 3))
            for tau in (1.0, 0.01):
                got = run_select(lib, handle, e, a0, 4, tau, q, windows=E)
                for w in sorted({0, 1, E - 1}):
                    one = run_select(lib, handle, e[w:w + 1], a0[w:w + 1], 4, tau, q[w:w + 1])
                    for k, v in one.items():
                        assert np.array_equal(got[k][w].view(np.uint32), v[0].view(np.uint32)), f"n {n} A {A} windows {E}: {k} of window {w}"


# ================================================================================================ window statistics
@pytest.mark.parametrize("case", WINDOW_CASES, ids=lambda c: "-".join(map(str, c)))
def test_window_stats_equal_the_restatement(lib, case):
    n_total, kk, kmin, kmax, flavour, rr = case
    v, front, idx, window = window_case(*case)
    (n, margin, mx, cnt), top = R.window_stats_ref(v, idx, kk, kmin, kmax, window, rr, front)
    vd = nan_tail(v)
    lst = dev(np.concatenate([np.full(G, 2 ** 30, np.int32), front, idx, np.full(G, 2 ** 30, np.int32)]))  # (ids no candidate has)
    hs = torch.zeros(8, dtype=torch.float32).pin_memory()
    for with_top in (True, False):
        st, sptr, sbefore = guarded(4, torch.float32)
        ts, tptr, tbefore = guarded(rr + kk, torch.float32)
        rc = lib.m3pc_debug_window_stats(vd.data_ptr(), n_total, lst.data_ptr() + 4 * (G + rr), kk, kmin, kmax, window, sptr, hs.data_ptr(), 5.0,
                                         tptr + 4 * rr if with_top else None, rr, stream())
        assert rc == 0, lib.m3pc_last_error()
        torch.cuda.synchronize()
        picked_is(lib, 13, f"window stats {case}")
        got = owned(st, sbefore, 0, 4, "window stats")
        want = np.array([n, margin, mx, cnt], F)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{case}: stats {got.tolist()}, restatement {want.tolist()}"
        assert np.array_equal(hs.numpy()[:4].view(np.uint32), want.view(np.uint32)) and hs.numpy()[4] == 5.0
        t = owned(ts, tbefore, 0, rr + kk if with_top else 0, "top_scores")
        if with_top:
            assert np.array_equal(t.view(np.uint32), top.view(np.uint32)), f"{case}: top_scores"
    if flavour == "edge" and n_total >= 8:
        thr = F(mx - F(window))
        assert cnt == int((v > thr).sum()) + 3 and int((v == np.nextafter(thr, F(-np.inf))).sum()) == 3


# ================================================================================================ merge
def run_merge(lib, handle, c, kind, hs=None, seq=0.0, nstats=8):
    """kind: 'merge' m3pc_rescore_merge (r = 0), 'race' m3pc_rescore_merge_race, 'select' m3pc_merge_race_select.  List slots outside
    the slice hold NaN / ids no candidate has."""
    b, q, lst, ls, f, r, n = c["b"], c["q"], c["lst"], c["ls"], c["f"], c["r"], c["n"]
    nt, m = b.size, r + n
    bd, qd = nan_tail(b), nan_tail(q)
    ld = dev(np.concatenate([np.full(G, 2 ** 30, np.int32), lst, np.full(G, 2 ** 30, np.int32)]))
    lsd = dev(np.concatenate([np.full(G, np.nan, F), ls, np.full(G, np.nan, F)]))
    fd = dev(np.concatenate([np.full(G, np.nan, F), f, np.full(G, np.nan, F)]))
    mg, mptr, mbefore = guarded(nt, torch.float32)
    st, sptr, sbefore = guarded(nstats, torch.float32)
    hp = None if hs is None else hs.data_ptr()
    lp, lsp, fp = ld.data_ptr() + 4 * G, lsd.data_ptr() + 4 * G, fd.data_ptr() + 4 * G
    sel = None
    if kind == "merge":
        assert r == 0
        rc = lib.m3pc_rescore_merge(handle, bd.data_ptr(), nt, lp, n, lsp, fp, c["delta"], mptr, sptr, hp, seq, stream())
    elif kind == "race":
        rc = lib.m3pc_rescore_merge_race(handle, bd.data_ptr(), qd.data_ptr(), c["tau"], nt, lp, r, n, lsp, fp, c["delta"], mptr, sptr, hp, seq, stream())
    else:
        a0 = R.rng(nt).standard_normal((nt, 3)).astype(F)
        ad = nan_tail(a0)
        sel = {k: guarded(cnt, t) for k, (cnt, t) in {"p": (nt, torch.float32), "eval_action": (3, torch.float32), "argmax": (1, torch.int32),
                                                        "sample_idx": (1, torch.int32), "sample_action": (3, torch.float32)}.items()}
        rc = lib.m3pc_merge_race_select(handle, bd.data_ptr(), qd.data_ptr(), c["tau"], nt, lp, r, n, lsp, fp, c["delta"], mptr, sptr, hp, seq,
                                        ad.data_ptr(), 3, sel["p"][1], sel["eval_action"][1], sel["argmax"][1], sel["sample_idx"][1],
                                        sel["sample_action"][1], stream())
    assert rc == 0, lib.m3pc_last_error()
    torch.cuda.synchronize()
    picked_is(lib, 15 if kind == "select" else 14, f"merge {kind} r {r} n {n} n_total {nt}")
    merged = owned(mg, mbefore, 0, nt, "merged")
    stats = owned(st, sbefore, 0, nstats, "merge stats")
    if sel is not None:
        sel = {k: owned(bf, before, 0, bf.numel() - 2 * G, f"merge select {k}") for k, (bf, _, before) in sel.items()}
        sel["a0"] = a0
    return merged, stats, sel


def hold_merge(c, merged, stats, race, what):
    ref = R.merge_ref(c["b"], c["lst"], c["r"], c["n"], c["ls"], c["f"], c["delta"], c["q"] if race else None, c["tau"])
    assert np.array_equal(merged.view(np.uint32), ref["merged"].view(np.uint32)), f"{what}: the merged vector differs at {int((merged != ref['merged']).sum())} entries"
    want = np.array([ref["c"], ref["dev"], ref["need"], ref["margin"]], F)
    assert np.array_equal(stats[:4].view(np.uint32), want.view(np.uint32)), f"{what}: stats {stats[:4].tolist()}, restatement {want.tolist()}"
    if race:
        assert stats[4] == 0.0 and int(stats[5]) == ref["need_race"], f"{what}: need_race {stats[5]}, float64 count {ref['need_race']}"
        record(14, "K*", abs(float(stats[6]) - ref["kbest"]), ref["kbound"], what)
        record(14, "thr_r", abs(float(stats[7]) - ref["thr_r"]), ref["thr_r_bound"], what)
    p = c["planted"]
    if p:
        assert c["b"][p["at_thr"]] == ref["thr"] and c["b"][p["above_thr"]] > ref["thr"] and ref["need"] >= 1


@pytest.mark.parametrize("case", MERGE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_merge_equals_the_restatement(lib, handle, case):
    """rescore_merge_kernel with and without a race list, then merge_select_kernel: the bits of the merge followed by m3pc_select."""
    r, n, nt, flavour = case
    c = merge_case(*case)
    merged, stats, _ = run_merge(lib, handle, c, "race")
    hold_merge(c, merged, stats, True, f"race merge {case}")
    if r == 0:
        m4, s4, _ = run_merge(lib, handle, c, "merge", nstats=4)
        hold_merge(c, m4, s4, False, f"merge {case}")
        assert np.array_equal(m4.view(np.uint32), merged.view(np.uint32)) and np.array_equal(s4.view(np.uint32), stats[:4].view(np.uint32))
    m2, s2, sel = run_merge(lib, handle, c, "select")
    assert np.array_equal(m2.view(np.uint32), merged.view(np.uint32)) and np.array_equal(s2.view(np.uint32), stats.view(np.uint32)), f"{case}: merge_select's merge differs"
    one = run_select(lib, handle, merged[None], sel["a0"][None], 1, c["tau"], c["q"][None], public=True)
    for k, v in one.items():
        assert np.array_equal(v[0].view(np.uint32), sel[k].view(np.uint32)), f"{case}: {k} of merge_select is not the select's on the merged vector"


def test_four_statistics_merge_clears_the_race_slots(lib, handle):
    """A four-statistics merge on a host block a race merge has just filled: slots 5..7 read 0, slot 4 the new sequence number."""
    hs = torch.zeros(8, dtype=torch.float32).pin_memory()
    c = merge_case(2, 8, 1024, "randn")
    _, st, _ = run_merge(lib, handle, c, "race", hs=hs, seq=3.0)
    h = hs.numpy()
    assert h[4] == 3.0 and h[5] == st[5] and h[6] == st[6] and h[7] == st[7] and h[6] != 0.0
    c0 = merge_case(0, 8, 1024, "randn")
    _, s4, _ = run_merge(lib, handle, c0, "merge", hs=hs, seq=4.0, nstats=4)
    assert h[4] == 4.0 and np.array_equal(h[:4].view(np.uint32), s4.view(np.uint32)) and (h[5:] == 0.0).all(), h.tolist()


@pytest.mark.parametrize("E", WINDOWS)
def test_merge_select_batch_rows_are_the_one_window_results(lib, handle, E):
    """merge_select_batch_kernel, the five (r, n) pairs cycling over the windows of n_total = 1024: window w's merged row, statistics and
    select outputs are the one-window kernels' bit for bit; race and four-statistics forms."""
    nt, rmax, LS, A = 1024, 64, 64 + 1024, 3
    for race in (1, 0):
        cs = [merge_case(0 if not race else MERGE_PAIRS[w % 5][0], MERGE_PAIRS[w % 5][1] if race or MERGE_PAIRS[w % 5][0] == 0 else 8, nt,
                         ("randn", "tied", "delta0")[w % 3], seed=w) for w in range(E)]
        tau = 1.0
        for c in cs:
            c["tau"] = tau
        L = np.full((E, LS), 2 ** 30, np.int32)
        S, Fr = np.full((E, LS), np.nan, F), np.full((E, LS), np.nan, F)
        for w, c in enumerate(cs):
            lo, hi = rmax - c["r"], rmax + c["n"]
            L[w, lo:hi], S[w, lo:hi], Fr[w, lo:hi] = c["lst"], c["ls"], c["f"]
        a0 = R.rng(nt).standard_normal((nt, A)).astype(F)
        a = TailArgs()
        keep = [nan_tail(np.stack([c["b"] for c in cs])), nan_tail(np.stack([c["q"] for c in cs])), dev(L), dev(S), dev(Fr), nan_tail(np.tile(a0, (E, 1, 1)))]
        a.scores, a.expo, a.list, a.list_scores, a.list_rescored, a.a0 = (t.data_ptr() for t in keep)
        a.race, a.select, a.temperature, a.n_windows, a.n_total = race, 1, tau, E, nt
        a.rmax, a.list_stride, a.f_stride, a.f_lo = rmax, LS, LS, 0
        rr, nn, dd = (ci * E)(*[c["r"] for c in cs]), (ci * E)(*[c["n"] for c in cs]), (cf * E)(*[c["delta"] for c in cs])
        a.r, a.n, a.delta = C.cast(rr, pi), C.cast(nn, pi), C.cast(dd, C.POINTER(cf))
        a.a0_window_stride, a.a0_stride, a.A = nt * A, A, A
        outs = {k: guarded(cnt, t) for k, (cnt, t) in {"merged": (E * nt, torch.float32), "stats": (E * 8, torch.float32), "p": (E * nt, torch.float32),
                                                         "eval_action": (E * A, torch.float32), "argmax": (E, torch.int32), "sample_idx": (E, torch.int32),
                                                         "sample_action": (E * A, torch.float32)}.items()}
        for k, (bf, ptr, _) in outs.items():
            setattr(a, k, ptr)
        a.stream = stream()
        assert lib.m3pc_debug_merge_select_batch(C.byref(a)) == 0, lib.m3pc_last_error()
        torch.cuda.synchronize()
        picked_is(lib, 16, f"merge select batch windows {E} race {race}")
        got = {k: owned(bf, before, 0, bf.numel() - 2 * G, f"batch {k}").reshape(E, -1) for k, (bf, _, before) in outs.items()}
        for w in sorted({0, 1, 2, 3, 4, E - 1} & set(range(E))):
            c = cs[w]
            merged, stats, _ = run_merge(lib, handle, c, "race" if race else "merge", nstats=8 if race else 4)
            assert np.array_equal(got["merged"][w].view(np.uint32), merged.view(np.uint32)), (E, race, w)
            assert np.array_equal(got["stats"][w][:stats.size].view(np.uint32), stats.view(np.uint32)), (E, race, w)
            one = run_select(lib, handle, merged[None], a0[None], 1, tau, c["q"][None], public=True)
            for k, v in one.items():
                assert np.array_equal(got[k][w].view(np.uint32), v[0].view(np.uint32)), f"windows {E} race {race}: {k} of window {w}"


# ================================================================================================ calibration statistics
@pytest.mark.parametrize("n", CALIB_SIZES)
def test_deviation_stats_across_tiles(lib, n):
    """deviation_stats_kernel across its 2048-entry tile and across a change of the per-thread element count, with ties at the median."""
    b, f = calib_case(n)
    c, devi, fmx = R.deviation_ref(b, f)
    d = (b - f).astype(F)
    assert int((d == c).sum()) >= 2
    st, sptr, sbefore = guarded(8, torch.float32)
    delta = cf()
    bd, fd = nan_tail(b), nan_tail(f)
    rc = lib.m3pc_debug_calibrate_stats(bd.data_ptr(), fd.data_ptr(), n, 1.6, sptr, C.byref(delta), stream())
    assert rc == 0, lib.m3pc_last_error()
    torch.cuda.synchronize()
    picked_is(lib, 17, f"deviation stats n {n}")
    got = owned(st, sbefore, 0, 8, "deviation stats")
    want = np.array([c, devi, fmx, 0, 0, 0, 0, 0], F)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, got.tolist(), want.tolist())
    assert F(delta.value) == F(max(float(F(1.6)) * float(devi), 1e-6 * float(fmx), 1e-30))


# ================================================================================================ scatter, gather
@pytest.mark.parametrize("n", SCATTER_SIZES)
def test_scatter(lib, n):
    g = R.rng(n)
    nt = 2 * n + 3
    index = g.permutation(nt)[:n].astype(np.int32)
    src, dst0 = g.standard_normal(n).astype(F), g.standard_normal(nt).astype(F)
    for with_copy in (True, False):
        dst, dptr, _ = guarded(nt, torch.float32)
        dst[G:G + nt] = dev(dst0)
        dbefore = dst.clone()
        cp, cptr, cbefore = guarded(n, torch.int32)
        sd, ixd = nan_tail(src), dev(np.concatenate([index, np.full(G, 2 ** 30, np.int32)]))
        rc = lib.m3pc_debug_scatter(sd.data_ptr(), ixd.data_ptr(), n, dptr, cptr if with_copy else None, stream())
        assert rc == 0, lib.m3pc_last_error()
        torch.cuda.synchronize()
        picked_is(lib, 20, f"scatter n {n}")
        got = owned(dst, dbefore, 0, nt, "scatter dst")
        assert np.array_equal(got.view(np.uint32), R.scatter_ref(dst0, src, index).view(np.uint32))
        cgot = owned(cp, cbefore, 0, n if with_copy else 0, "index_copy")
        assert not with_copy or np.array_equal(cgot, index)


@pytest.mark.parametrize("E", WINDOWS)
def test_gather_listed(lib, E):
    """gather_listed_kernel: rows of 7 and 65 floats (more than a wave), an entry that names no candidate leaves its row untouched."""
    g = R.rng(E)
    nt, LS, lo, hi = 37, 12, 2, 9
    for row in (7, 65):
        sa = g.standard_normal((E, nt, row)).astype(F)
        lst = g.integers(0, nt, (E, LS)).astype(np.int32)
        lst[:, :lo], lst[:, hi:] = 2 ** 30, 2 ** 30
        lst[0, lo + 1] = -1
        m = hi - lo
        cand, cptr, cbefore = guarded(E * m * row, torch.float32)
        wi, wptr, wbefore = guarded(E * m, torch.int32)
        sad, ld = nan_tail(sa), dev(lst)
        rc = lib.m3pc_debug_gather_listed(sad.data_ptr(), ld.data_ptr(), E, nt, row, LS, lo, hi, cptr, wptr, stream())
        assert rc == 0, lib.m3pc_last_error()
        torch.cuda.synchronize()
        picked_is(lib, 21, f"gather listed windows {E}")
        got = owned(cand, cbefore, 0, E * m * row, "cand").reshape(E, m, row)
        want = np.stack([sa[w][np.clip(lst[w, lo:hi], 0, nt - 1)] for w in range(E)])
        want[0, 1] = F(FSENT)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(owned(wi, wbefore, 0, E * m, "window_index"), np.repeat(np.arange(E), m))


# ================================================================================================ eval bound, variates: the batched forms
@pytest.mark.parametrize("E", WINDOWS)
def test_eval_bound_batch_rows_are_the_one_window_results(lib, handle, E):
    """eval_bound_kernel (m3pc_eval_bound; held to its float64 reference at its edge sizes by tests/test_eval_bound_gpu.py) and
    eval_bound_batch_kernel: window w's eight floats are the one-window call's bit for bit, and within 1e-3 of tests/eval_bound_ref.py."""
    import eval_bound_ref as EB
    nt, A, rmax, n_listed, tau, tol = 1025, 3, 4, 129, F(1.0), F(np.inf)
    LS = rmax + n_listed
    g = R.rng(40 + E)
    m = (-np.minimum(60.0, 0.05 * g.permuted(np.tile(np.arange(nt), (E, 1)), axis=1)) + 37.0).astype(F)
    a0 = np.tanh(g.standard_normal((E, nt, A))).astype(F)
    rs, ns = [w % (rmax + 1) for w in range(E)], [(5 * w) % n_listed for w in range(E)]
    ds = [float(F(0.012 * (1 + w % 3))) for w in range(E)]
    L = np.full((E, LS), 2 ** 30, np.int32)
    for w in range(E):
        L[w, rmax - rs[w]:rmax] = g.choice(nt, rs[w], replace=False)
        L[w, rmax:] = R.topk_order(m[w], n_listed)
    md, ad, ld = nan_tail(m), nan_tail(a0), dev(L)
    a = EvalBatchArgs()
    a.merged, a.list, a.a0 = md.data_ptr(), ld.data_ptr(), ad.data_ptr()
    a.n_windows, a.n_total, a.rmax, a.list_stride, a.n_listed = E, nt, rmax, LS, n_listed
    rr, nn, dd = (ci * E)(*rs), (ci * E)(*ns), (cf * E)(*ds)
    a.r, a.n, a.delta = C.cast(rr, pi), C.cast(nn, pi), C.cast(dd, C.POINTER(cf))
    a.a0_window_stride, a.a0_stride, a.A, a.temperature, a.eval_tol = nt * A, A, A, tau, tol
    st, sptr, sbefore = guarded(8 * E, torch.float32)
    a.stats, a.stream = sptr, stream()
    assert lib.m3pc_debug_eval_bound_batch(C.byref(a)) == 0, lib.m3pc_last_error()
    torch.cuda.synchronize()
    picked_is(lib, 19, f"eval bound batch windows {E}")
    got = owned(st, sbefore, 0, 8 * E, "eval bound stats").reshape(E, 8)
    for w in sorted({0, 1, E - 1} & set(range(E))):
        s1, p1, b1 = guarded(8, torch.float32)
        rc = lib.m3pc_eval_bound(handle, md.data_ptr() + 4 * w * nt, nt, ld.data_ptr() + 4 * (w * LS + rmax - rs[w]), rs[w], ns[w], n_listed,
                                 ad.data_ptr() + 4 * w * nt * A, A, A, tau, ds[w], tol, p1, None, 0.0, stream())
        assert rc == 0, lib.m3pc_last_error()
        torch.cuda.synchronize()
        picked_is(lib, 18, "eval bound")
        one = owned(s1, b1, 0, 8, "eval bound one window")
        assert np.array_equal(one.view(np.uint32), got[w].view(np.uint32)), (E, w, one.tolist(), got[w].tolist())
        ref = EB.eval_bound_fast(m[w], a0[w], L[w, rmax - rs[w]:], rs[w], ns[w], n_listed, float(tau), ds[w])
        for name, gv, wv in (("eval_bound", one[0], ref["eval_bound"]), ("P_U", one[2], ref["P_U"]), ("bound(n_listed)", one[6], ref["bound_listed"])):
            assert abs(float(gv) - wv) <= 1e-3 * wv, (E, w, name, float(gv), wv)
        assert int(one[1]) == ns[w] and int(one[7]) == ref["n_U"]


@pytest.mark.parametrize("E", WINDOWS)
def test_variates_batch_rows_are_the_one_step_normals(lib, handle, E):
    """variates_kernel (m3pc_draw_variates) against tests/variates_ref.py, and variates_batch_kernel: window w's normals are
    m3pc_draw_variates' for step steps[w], bit for bit -- aligned and unaligned slices, more than one block of 256 threads."""
    import variates_ref as V
    seed, n_total, row = 0x1234567 + E, 301, 7
    steps = [3 + 5 * w for w in range(E)]
    flat = n_total * row
    for g0, g1 in ((0, flat), (5, flat - 2), (4, 1032)):
        out, optr, obefore = guarded(E * (g1 - g0), torch.float32)
        rc = lib.m3pc_debug_variates_batch(seed, (C.c_ulonglong * E)(*steps), E, g0, g1, optr, stream())
        assert rc == 0, lib.m3pc_last_error()
        torch.cuda.synchronize()
        picked_is(lib, 23, f"variates batch windows {E}")
        got = owned(out, obefore, 0, E * (g1 - g0), "variates batch").reshape(E, g1 - g0)
        for w in sorted({0, E // 2, E - 1}):
            eps, eptr, ebefore = guarded(flat, torch.float32)
            ex, xptr, xbefore = guarded(n_total, torch.float32)
            assert lib.m3pc_draw_variates(handle, seed, steps[w], 0, n_total, row, eptr, xptr, stream()) == 0, lib.m3pc_last_error()
            torch.cuda.synchronize()
            picked_is(lib, 22, "draw variates")
            one = owned(eps, ebefore, 0, flat, "eps")
            assert np.array_equal(got[w].view(np.uint32), one[g0:g1].view(np.uint32)), (E, w, g0, g1)
            if g0 == 0:
                ref = np.asarray(V.eps(seed, steps[w], n_total, row), np.float64).reshape(-1)
                assert np.abs(one.astype(np.float64) - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
                qref = np.asarray(V.expo(seed, steps[w], n_total), np.float64).reshape(-1)
                assert np.abs(owned(ex, xbefore, 0, n_total, "expo").astype(np.float64) - qref).max() <= 1e-5 * max(1.0, qref.max())


# ================================================================================================ the table
def test_every_selection_kernel_was_reached(lib):
    """Runs last in the file: the ids the launches above reported are exactly the header's list."""
    ids = header_ids()
    assert len(ids) == 23 and sorted(ids) == list(range(1, 24))
    assert REACHED == set(ids), f"not reached: {sorted(set(ids) - REACHED)}; not in the header: {sorted(REACHED - set(ids))}"
    for (kid, key), ratio in sorted(WORST.items()):
        print(f"kernel {kid} {ids[kid]} {key}: largest err / bound {ratio:.3g}")
