"""The three kernels of a lock-step batch's tail (csrc/select.hip: topk_rank_batch_kernel, gather_listed_kernel,
merge_select_batch_kernel) through their lab hooks (include/m3pc_hip_debug.h), on synthetic vectors and without a model.

Every batched kernel takes its window from the grid and runs the device functions of the one-window kernels, so window w of a
batched launch must give what the one-window entry points give on row w -- m3pc_topk_race_window / m3pc_topk_window for the lists,
m3pc_merge_race_select / m3pc_rescore_merge (+ m3pc_select) for the merge -- BIT FOR BIT: every comparison below is torch.equal on
whole buffers, sentinels included.  The one-window results are computed once per (n_total, rmax, kmax) for max_batch windows; the
batched launches at E = 1, 2, 5, max_batch are compared with their first E rows.

Inputs hold one row more than max_batch; for a launch of E windows every input row >= E is NaN (the launch may not read it) and
every output row >= E, the extra row included, must keep its sentinel (the launch may not write it)."""
import ctypes as C

import numpy as np
import pytest
import torch

from m3pc_amd import capi

pytestmark = pytest.mark.gpu

MAX_BATCH = 8
ES = (1, 2, 5, MAX_BATCH)
H, A = 2, 3          # sample_actions rows of H * A floats; the select reads the first A of them
TAU = 0.05
ISENT = -7           # sentinel of the int32 outputs (no candidate id)
FSENT = -12345.5     # sentinel of the float outputs (no score of the synthetic vectors)
EINVAL = -1          # M3PC_EINVAL
vp, ci, cf, ll = C.c_void_p, C.c_int, C.c_float, C.c_longlong


class TailArgs(C.Structure):  # m3pc_debug_tail_args
    _fields_ = [("scores", vp), ("expo", vp), ("race", ci), ("select", ci), ("temperature", cf), ("n_windows", ci), ("n_total", ci),
                ("list", vp), ("list_scores", vp), ("list_rescored", vp), ("rmax", ci), ("list_stride", ci), ("f_stride", ci),
                ("f_lo", ci), ("r", C.POINTER(ci)), ("n", C.POINTER(ci)), ("delta", C.POINTER(cf)), ("merged", vp), ("stats", vp),
                ("host_stats", vp), ("seq", cf), ("a0", vp), ("a0_window_stride", ll), ("a0_stride", ll), ("A", ci), ("p", vp),
                ("eval_action", vp), ("argmax", vp), ("sample_idx", vp), ("sample_action", vp), ("stream", vp)]


@pytest.fixture(scope="module")
def lab():
    from hip_util import lab_library
    lib = lab_library()
    lib.m3pc_debug_topk_race_batch.restype = ci
    lib.m3pc_debug_topk_race_batch.argtypes = [vp, vp, cf, ci, ci, ci, ci, ci, vp, vp, vp]
    lib.m3pc_debug_gather_listed.restype = ci
    lib.m3pc_debug_gather_listed.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp]
    lib.m3pc_debug_merge_select_batch.restype = ci
    lib.m3pc_debug_merge_select_batch.argtypes = [C.POINTER(TailArgs)]
    return lib


@pytest.fixture(scope="module")
def handle():
    h = capi.Handle(11, A, 16, max_candidates=64, max_batch=MAX_BATCH)
    yield h
    h.close()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


_VEC = {}


def _place(v, q, pair, rank, others):
    """Give both candidates of `pair` (equal scores) ONE variate that puts their -- then bit-equal -- race keys at ranks rank | rank + 1
    among `others` (ids whose keys stay as they are)."""
    key = (TAU * v[others].double() - q[others].double().log()).sort(descending=True).values
    k = float(key[rank - 1] + key[rank]) / 2 if rank < key.numel() else float(key[-1]) - 1.0
    q[pair[0]] = q[pair[1]] = float(torch.exp(TAU * v[pair[0]].double() - k))


def _vectors(n):
    """scores / expo (MAX_BATCH + 1, n) and sample_actions (MAX_BATCH + 1, n, H, A), the same for every case of one n, with exact
    ties built in per row (and asserted here, so that none of them is lost unnoticed):
      scores    ranks 0 | 1 | 2 (the edge of the kmax = 1 list and the very top), 128 | 129 and 991 | 992 (the edges of the other
                two lists) hold equal values; where n allows, the tied pairs sit at the indices 63 | 64, 1023 | 1024 and 2047 | 2048,
                one on each side of a boundary -- 2048 is where the one-window launcher changes kernels -- so the lower index
                is the one a list keeps;
      race keys a tied pair of scores with ONE variate has bit-equal keys: the pair of ranks 0 | 1 wins the race (the edge of the
                rmax = 1 list), the pair of ranks 128 | 129 sits at race ranks 31 | 32 (the edge of the rmax = 32 list), the pair at
                2047 | 2048 at race ranks 5 | 6."""
    if n in _VEC:
        return _VEC[n]
    g = torch.Generator().manual_seed(1000 + n)
    v = torch.empty(MAX_BATCH + 1, n)
    q = torch.empty(MAX_BATCH + 1, n).exponential_(1, generator=g).clamp_(min=1e-4)
    for w in range(MAX_BATCH + 1):
        s = torch.sort(torch.randn(n, generator=g) * 15.0 + 100.0, descending=True).values
        ties = [t for t in ((0, 1), (1, 2), (128, 129), (991, 992)) if t[1] < n]
        for a, b in ties:
            s[b] = s[a]
        # rank -> index: a random permutation, with the boundary indices swapped onto the tied ranks
        perm = torch.randperm(n, generator=g)
        for (a, b), lo in zip(((0, 1), (128, 129), (991, 992)), (63, 1023, 2047)):
            if b < n and lo + 1 < n:
                for rank, idx in ((a, lo), (b, lo + 1)):
                    at = int((perm == idx).nonzero())
                    perm[at], perm[rank] = int(perm[rank]), idx
        v[w, perm] = s
        pairs = [(int(perm[a]), int(perm[b])) for a, b in ((0, 1), (128, 129), (991, 992)) if b < n]
        pairs = [(min(p), max(p)) for p in pairs]
        rest = torch.tensor([i for i in range(n) if all(i not in p for p in pairs)], dtype=torch.long)
        if pairs:
            q[w, pairs[0][0]] = q[w, pairs[0][1]] = 1e-12  # (-log q = 27.6: beyond every other key)
        placed = list(pairs[0]) if pairs else []
        if len(pairs) > 2:
            _place(v[w], q[w], pairs[2], 5, torch.cat([rest, torch.tensor(placed)]))
            placed += list(pairs[2])
        if len(pairs) > 1:
            _place(v[w], q[w], pairs[1], 31, torch.cat([rest, torch.tensor(placed)]))
        # -- what was built
        sv = torch.sort(v[w], descending=True, stable=True).values
        for kk in (2, 129, 992):
            assert kk >= n or sv[kk - 1] == sv[kk]
        for b, lo in ((1, 63), (129, 1023), (992, 2047)):
            assert b >= n or lo + 1 >= n or (v[w, lo] == v[w, lo + 1] and q[w, lo] == q[w, lo + 1])
        ko = torch.argsort(TAU * v[w].double() - q[w].double().log(), descending=True, stable=True)
        for rank, need in ((0, 2), (31, 130), (5, 993)):
            if n >= need:
                a, b = int(ko[rank]), int(ko[rank + 1])
                assert v[w, a] == v[w, b] and q[w, a] == q[w, b], (n, w, rank)
    sa = torch.rand(MAX_BATCH + 1, n, H, A, generator=g) * 2.0 - 1.0
    _VEC[n] = (v.cuda().contiguous(), q.cuda().contiguous(), sa.cuda().contiguous())
    return _VEC[n]


def _nan_rows(t, e):
    """A copy of t whose rows >= e are NaN: what a launch of e windows may not read."""
    c = t.clone()
    c[e:] = float("nan")
    return c


def _refused(n, kmax, rmax):
    """What the one-window calls refuse: more race entries than candidates."""
    return rmax > n


def _single_lists(handle, v, q, n, kmax, rmax):
    ls = rmax + kmax + 1
    lst = torch.full((MAX_BATCH + 1, ls), ISENT, dtype=torch.int32, device="cuda")
    lsc = torch.full((MAX_BATCH + 1, ls), FSENT, dtype=torch.float32, device="cuda")
    for w in range(MAX_BATCH):
        if rmax > 0:
            handle.topk_race_window(v[w], q[w], TAU, kmax, 1, rmax, lst=lst[w], list_scores=lsc[w])
        else:
            handle.topk_window(v[w], kmax, 1, 0.0, top=lst[w], top_scores=lsc[w])
    return lst, lsc


def _rn(n, kmax, rmax):
    """Per-window r / n / delta that differ within one launch; window 0 lists everything the ranking wrote."""
    kk = min(kmax + 1, n)
    r = [max(rmax - 3 * w, 0) for w in range(MAX_BATCH)]
    m = [max(1, kk - 7 * w - (1 if w else 0)) for w in range(MAX_BATCH)]
    d = [float(np.float32(0.015625 * (w + 1) + 0.001 * w)) for w in range(MAX_BATCH)]
    return r, m, d


def _rescored(lsc, n, seed):
    """fp32 re-scores in the list's layout: the listed score less a shift of 3.25 plus noise on a grid of 1/4 (ties among the
    deviations, the lower median decided by position)."""
    g = torch.Generator().manual_seed(seed)
    noise = (torch.randint(-2, 3, lsc.shape, generator=g).float() * 0.25).cuda()
    return torch.where(lsc == FSENT, torch.full_like(lsc, FSENT), lsc - 3.25 + noise).contiguous()


def _out_buffers(n):
    f32 = dict(dtype=torch.float32, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    E1 = MAX_BATCH + 1
    return dict(merged=torch.full((E1, n), FSENT, **f32), stats=torch.full((E1, 8), FSENT, **f32), p=torch.full((E1, n), FSENT, **f32),
                eval_action=torch.full((E1, A), FSENT, **f32), argmax=torch.full((E1,), ISENT, **i32),
                sample_idx=torch.full((E1,), ISENT, **i32), sample_action=torch.full((E1, A), FSENT, **f32))


def _single_merge(handle, v, q, sa, lst, lsc, f, n, rmax, r, m, d):
    o = _out_buffers(n)
    for w in range(MAX_BATCH):
        sel = (o["p"][w], o["eval_action"][w], o["argmax"][w : w + 1], o["sample_idx"][w : w + 1], o["sample_action"][w : w + 1])
        if rmax > 0:
            lo = rmax - r[w]
            handle.merge_race_select(v[w], q[w], TAU, lst[w, lo:], r[w], m[w], lsc[w, lo:], f[w, lo:], sa[w, :, 0], delta=d[w],
                                     merged=o["merged"][w], stats=o["stats"][w], out=sel)
        else:
            handle.rescore_merge(v[w], lst[w], m[w], lsc[w], f[w], delta=d[w], merged=o["merged"][w], stats=o["stats"][w])
            handle.select(o["merged"][w], sa[w, :, 0], TAU, q[w], out=sel)
    return o


def _check_rows(name, got, want, e):
    assert torch.equal(got[:e], want[:e]), f"{name}: windows < {e} differ from the one-window results"
    sent = torch.full_like(got[e:], ISENT if got.dtype == torch.int32 else FSENT)
    assert torch.equal(got[e:], sent), f"{name}: rows >= {e} were written"


@pytest.mark.parametrize("rmax", [0, 1, 32])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 625, 1024, 2047, 2048, 2049, 4096, 16384])
def test_batched_tail_equals_one_window_calls(lab, handle, n, rmax):
    v, q, sa = _vectors(n)
    ran = 0
    for kmax in (1, 128, 991):
        if _refused(n, kmax, rmax):
            continue
        ran += 1
        ls = rmax + kmax + 1
        kk = min(kmax + 1, n)
        lst1, lsc1 = _single_lists(handle, v, q, n, kmax, rmax)
        # the order itself, against a stable sort (descending, ties to the lower index), so that both sides cannot be wrong alike
        for w in (0, MAX_BATCH - 1):
            want = torch.sort(v[w], descending=True, stable=True).indices[:kk].to(torch.int32)
            assert torch.equal(lst1[w, rmax : rmax + kk], want)
        r, m, d = _rn(n, kmax, rmax)
        f = _rescored(lsc1, n, 7 * n + kmax + rmax)
        ref = _single_merge(handle, v, q, sa, lst1, lsc1, f, n, rmax, r, m, d)
        ri, mi, di = (ci * MAX_BATCH)(*r), (ci * MAX_BATCH)(*m), (cf * MAX_BATCH)(*d)
        for e in ES:
            ve, qe, sae = _nan_rows(v, e), _nan_rows(q, e), _nan_rows(sa, e)
            lst = torch.full_like(lst1, ISENT)
            lsc = torch.full_like(lsc1, FSENT)
            rc = lab.m3pc_debug_topk_race_batch(_ptr(ve), _ptr(qe), TAU, e, n, kmax, 1, rmax, _ptr(lst), _ptr(lsc), _stream())
            assert rc == 0, lab.m3pc_last_error()
            _check_rows("list", lst, lst1, e)
            _check_rows("list_scores", lsc, lsc1, e)
            # merge + certificates + select on the lists and re-scores of the one-window side (rows >= e: NaN / no candidate)
            o = _out_buffers(n)
            host = torch.full((MAX_BATCH + 1, 8), FSENT, dtype=torch.float32).pin_memory()
            le, lse, fe = lst1.clone(), _nan_rows(lsc1, e), _nan_rows(f, e)
            le[e:] = ISENT
            seq = float(100 * e + ran)
            a = TailArgs(_ptr(ve), _ptr(qe), int(rmax > 0), 1, TAU, e, n, _ptr(le), _ptr(lse), _ptr(fe), rmax, ls, ls, 0, ri, mi, di,
                         _ptr(o["merged"]), _ptr(o["stats"]), host.data_ptr(), seq, _ptr(sae), n * H * A, H * A, A,
                         _ptr(o["p"]), _ptr(o["eval_action"]), _ptr(o["argmax"]), _ptr(o["sample_idx"]), _ptr(o["sample_action"]),
                         _stream())
            rc = lab.m3pc_debug_merge_select_batch(C.byref(a))
            assert rc == 0, lab.m3pc_last_error()
            torch.cuda.synchronize()
            for k in o:
                _check_rows(k, o[k], ref[k], e)
            # the host copy: the statistics (zeros behind a four-statistics merge), closed by the sequence number
            st = ref["stats"][:e].cpu()
            want_h = torch.where(st == FSENT, torch.zeros_like(st), st)
            want_h[:, 4] = seq
            assert torch.equal(host[:e], want_h)
            assert torch.equal(host[e:], torch.full_like(host[e:], FSENT))
    assert ran or n < 32


def test_compact_rescores_equal_list_layout(lab, handle):
    """The re-scores as ONE m3pc_score_actions call leaves them -- (E m,) window-major for the slice [rmax - rfirst, rmax + kmin) of
    every list (f_stride = m, f_lo = rmax - rfirst) -- give the merge of the same values in the list's layout."""
    n, rmax, kmax, rfirst, kmin, e = 625, 32, 128, 8, 24, 5
    v, q, sa = _vectors(n)
    ls, m0, lo = rmax + kmax + 1, rfirst + kmin, rmax - rfirst
    lst1, lsc1 = _single_lists(handle, v, q, n, kmax, rmax)
    f = _rescored(lsc1, n, 99)
    r, m, d = [rfirst] * MAX_BATCH, [kmin] * MAX_BATCH, [0.03125] * MAX_BATCH
    ref = _single_merge(handle, v, q, sa, lst1, lsc1, f, n, rmax, r, m, d)
    compact = torch.cat([f[:e, lo : lo + m0].reshape(-1), torch.full((3,), float("nan"), device="cuda")]).contiguous()
    o = _out_buffers(n)
    a = TailArgs(_ptr(v), _ptr(q), 1, 1, TAU, e, n, _ptr(lst1), _ptr(lsc1), _ptr(compact), rmax, ls, m0, lo, (ci * MAX_BATCH)(*r),
                 (ci * MAX_BATCH)(*m), (cf * MAX_BATCH)(*d), _ptr(o["merged"]), _ptr(o["stats"]), None, 0.0, _ptr(sa), n * H * A, H * A, A,
                 _ptr(o["p"]), _ptr(o["eval_action"]), _ptr(o["argmax"]), _ptr(o["sample_idx"]), _ptr(o["sample_action"]), _stream())
    assert lab.m3pc_debug_merge_select_batch(C.byref(a)) == 0, lab.m3pc_last_error()
    torch.cuda.synchronize()
    for k in o:
        _check_rows(k, o[k], ref[k], e)


def test_merge_alone_and_refusals(lab, handle):
    """select == 0 is m3pc_rescore_merge per window and writes no select output; bad per-window sizes are refused before a launch."""
    n, rmax, kmax, e = 65, 0, 16, 2
    v, q, sa = _vectors(n)
    ls = rmax + kmax + 1
    lst1, lsc1 = _single_lists(handle, v, q, n, kmax, rmax)
    f = _rescored(lsc1, n, 5)
    r, m, d = [0] * MAX_BATCH, [9, 4] + [1] * (MAX_BATCH - 2), [0.25] * MAX_BATCH
    ref = _single_merge(handle, v, q, sa, lst1, lsc1, f, n, rmax, r, m, d)
    o = _out_buffers(n)

    def call(rr, mm, dd, select=0):
        a = TailArgs(_ptr(v), None, 0, select, TAU, e, n, _ptr(lst1), _ptr(lsc1), _ptr(f), rmax, ls, ls, 0, (ci * MAX_BATCH)(*rr),
                     (ci * MAX_BATCH)(*mm), (cf * MAX_BATCH)(*dd), _ptr(o["merged"]), _ptr(o["stats"]), None, 0.0, None, 0, 0, A,
                     _ptr(o["p"]), None, _ptr(o["argmax"]), None, None, _stream())
        return lab.m3pc_debug_merge_select_batch(C.byref(a))

    for bad in (dict(mm=[0] + m[1:]), dict(mm=[ls + 1] + m[1:]), dict(rr=[1] + r[1:]), dict(dd=[-1.0] + d[1:]),
                dict(dd=[float("nan")] + d[1:]), dict(mm=[n + 1] + m[1:])):
        kw = dict(rr=r, mm=m, dd=d)
        kw.update(bad)
        assert call(**kw) == EINVAL, bad
    torch.cuda.synchronize()
    for k in o:
        _check_rows(k, o[k], ref[k], 0)  # nothing was launched
    assert call(r, m, d) == 0, lab.m3pc_last_error()
    torch.cuda.synchronize()
    _check_rows("merged", o["merged"], ref["merged"], e)
    _check_rows("stats", o["stats"], ref["stats"], e)
    for k in ("p", "argmax"):
        _check_rows(k, o[k], ref[k], 0)


def test_gather_of_listed_candidates(lab, handle):
    """cand / window_index of the slices [lo, hi) of every window's list: lengths 0, 1 and max_rescore, a slice that starts among the
    race entries and ends among the score entries, and one that runs over list slots no ranking wrote (n_total below the list's
    length): those rows stay untouched."""
    for n, rmax, kmax, slices in ((625, 32, 128, ((40, 40), (0, 1), (31, 32), (32, 33), (20, 20 + handle.max_rescore), (29, 37))),
                                  (3, 1, 128, ((0, 6),))):
        v, q, sa = _vectors(n)
        ls, kk = rmax + kmax + 1, min(kmax + 1, n)
        lst1, _ = _single_lists(handle, v, q, n, kmax, rmax)
        for e in (1, 5, MAX_BATCH):
            le = lst1.clone()
            le[e:] = 1 << 30  # (rows the launch may not read: ids that would index far outside sample_actions)
            sae = _nan_rows(sa, e)
            for lo, hi in slices:
                m = hi - lo
                cand = torch.full((e * m + 1, H, A), FSENT, dtype=torch.float32, device="cuda")
                widx = torch.full((e * m + 1,), ISENT, dtype=torch.int32, device="cuda")
                rc = lab.m3pc_debug_gather_listed(_ptr(sae), _ptr(le), e, n, H * A, ls, lo, hi, _ptr(cand), _ptr(widx), _stream())
                assert rc == 0, lab.m3pc_last_error()
                want = torch.full_like(cand, FSENT)
                for w in range(e):
                    ids = lst1[w, lo:hi].long()
                    ok = ids >= 0
                    assert bool(ok[: max(0, min(hi, rmax + kk) - lo)].all())
                    want[w * m : (w + 1) * m][ok] = sa[w, ids[ok]]
                assert torch.equal(cand, want), (n, e, lo, hi)
                ww = torch.arange(e, dtype=torch.int32, device="cuda").repeat_interleave(m)
                assert torch.equal(widx[: e * m], ww) and int(widx[-1]) == ISENT
        assert lab.m3pc_debug_gather_listed(_ptr(sa), _ptr(lst1), 1, n, H * A, ls, 5, ls + 1, _ptr(sa), None, _stream()) == EINVAL


def test_more_windows_than_one_launch_carries(lab, handle):
    """The per-window r / n / delta travel in the kernel arguments, 64 windows per launch: 70 windows take two launches, and window
    64 + i must get entry 64 + i of the host arrays and row 64 + i of every device array."""
    e, n, rmax, kmax = 70, 65, 4, 16
    ls, kk = rmax + kmax + 1, kmax + 1
    g = torch.Generator().manual_seed(70)
    v = (torch.randn(e, n, generator=g) * 15.0 + 100.0).cuda()
    q = torch.empty(e, n).exponential_(1, generator=g).clamp_(min=1e-4).cuda()
    sa = (torch.rand(e, n, H, A, generator=g) * 2.0 - 1.0).cuda()
    lst = torch.full((e, ls), ISENT, dtype=torch.int32, device="cuda")
    lsc = torch.full((e, ls), FSENT, dtype=torch.float32, device="cuda")
    rc = lab.m3pc_debug_topk_race_batch(_ptr(v), _ptr(q), TAU, e, n, kmax, 1, rmax, _ptr(lst), _ptr(lsc), _stream())
    assert rc == 0, lab.m3pc_last_error()
    f = _rescored(lsc, n, 70)
    r = [w % (rmax + 1) for w in range(e)]
    m = [1 + w % kk for w in range(e)]
    d = [float(np.float32(0.0078125 * (w + 1))) for w in range(e)]
    f32 = dict(dtype=torch.float32, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    o = dict(merged=torch.full((e, n), FSENT, **f32), stats=torch.full((e, 8), FSENT, **f32), p=torch.full((e, n), FSENT, **f32),
             eval_action=torch.full((e, A), FSENT, **f32), argmax=torch.full((e,), ISENT, **i32),
             sample_idx=torch.full((e,), ISENT, **i32), sample_action=torch.full((e, A), FSENT, **f32))
    a = TailArgs(_ptr(v), _ptr(q), 1, 1, TAU, e, n, _ptr(lst), _ptr(lsc), _ptr(f), rmax, ls, ls, 0, (ci * e)(*r), (ci * e)(*m), (cf * e)(*d),
                 _ptr(o["merged"]), _ptr(o["stats"]), None, 0.0, _ptr(sa), n * H * A, H * A, A, _ptr(o["p"]), _ptr(o["eval_action"]),
                 _ptr(o["argmax"]), _ptr(o["sample_idx"]), _ptr(o["sample_action"]), _stream())
    assert lab.m3pc_debug_merge_select_batch(C.byref(a)) == 0, lab.m3pc_last_error()
    for w in (0, 1, 63, 64, 65, 69):
        lst1, _ = handle.topk_race_window(v[w], q[w], TAU, kmax, 1, rmax, list_scores=torch.empty(ls, **f32))
        assert torch.equal(lst1[: rmax + kk], lst[w, : rmax + kk])
        lo = rmax - r[w]
        mg, st, sel = handle.merge_race_select(v[w], q[w], TAU, lst[w, lo:], r[w], m[w], lsc[w, lo:], f[w, lo:], sa[w, :, 0], delta=d[w])
        assert torch.equal(mg, o["merged"][w]) and torch.equal(st, o["stats"][w]), w
        for got, want in zip((o["p"][w], o["eval_action"][w], o["argmax"][w : w + 1], o["sample_idx"][w : w + 1], o["sample_action"][w : w + 1]),
                             sel):
            assert torch.equal(got, want), w
