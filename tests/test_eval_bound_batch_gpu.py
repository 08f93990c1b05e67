"""eval_bound_batch_kernel (csrc/select.hip: the eval_action certificate of every window of a lock-step batch in one launch) through
its lab hook m3pc_debug_eval_bound_batch (include/m3pc_hip_debug.h), on synthetic vectors and without a model.

The batched kernel takes its window from the grid and runs the device function of the one-window kernel, so window w's eight
statistics must be m3pc_eval_bound's on that window's rows BIT FOR BIT; they are also held against the fp64 reference of
tests/eval_bound_ref.py to that file's 1e-3 relative.  The windows of one launch differ in (r, n, delta): window 0 has a candidate
in both list parts, window 1 has n == n_listed, window 2 has delta = 0 (exactly 0 out), windows 3 and 4 have other counts.  Rows the
launch does not own keep their sentinels, every host block closes with the sequence number, and two launches give the same bits."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import eval_bound_ref as R
from m3pc_amd import capi

pytestmark = pytest.mark.gpu
f32 = lambda x: float(np.float32(x))
INF = float("inf")
EINVAL = -1
MAXE = 5
FSENT = -12345.5
vp, ci, cf, ll = C.c_void_p, C.c_int, C.c_float, C.c_longlong
# per window: (r, n, delta); n is clipped to n_listed, r to n_total
WINDOWS = ((2, 8, 0.012), (0, 10 ** 6, 4.87), (1, 1, 0.0), (2, 40, 0.012), (3, 0, 1.0))
LISTS = {1: (4, 129), 4: (64, 960)}  # a0 stride multiple -> (rmax, score entries listed)


class EvalBatchArgs(C.Structure):  # m3pc_debug_eval_batch_args
    _fields_ = [("merged", vp), ("n_windows", ci), ("n_total", ci), ("list", vp), ("rmax", ci), ("list_stride", ci), ("n_listed", ci),
                ("r", C.POINTER(ci)), ("n", C.POINTER(ci)), ("delta", C.POINTER(cf)), ("a0", vp), ("a0_window_stride", ll),
                ("a0_stride", ll), ("A", ci), ("temperature", cf), ("eval_tol", cf), ("stats", vp), ("host_stats", vp), ("seq", cf),
                ("stream", vp)]


@pytest.fixture(scope="module")
def lab():
    from hip_util import lab_library
    lib = lab_library()
    lib.m3pc_debug_eval_bound_batch.restype = ci
    lib.m3pc_debug_eval_bound_batch.argtypes = [C.POINTER(EvalBatchArgs)]
    return lib


@pytest.fixture(scope="module")
def handle():
    h = capi.Handle(11, 3, 8, n_embd=64, n_head=2, max_candidates=8)  # (m3pc_eval_bound reads the handle's device only)
    yield h
    h.close()


def _window(n_total, A, mult, rmax, L, rw, nw, tau, seed):
    """One window: scores whose softmax weights fall by ~5 % per rank, a0 = tanh of normals in rows of mult * A floats, a list row
    of rmax + L + 3 entries -- the r race entries END at rmax, the score entries (descending, ties to the lower index) start there,
    everything else is -1 -- with race entry 0 also a listed, not re-scored score entry and, from r = 2 on, race entry 1 the best
    score entry."""
    g = np.random.default_rng(seed)
    n_listed = min(L, n_total)
    n, r = min(nw, n_listed), min(rw, n_total)
    z = -np.minimum(60.0, 0.05 * np.arange(n_total) + g.uniform(0.0, 0.02, n_total))
    m = np.empty(n_total, dtype=np.float32)
    m[g.permutation(n_total)] = (z / tau + 37.0).astype(np.float32)
    buf = np.zeros((n_total, mult * A), dtype=np.float32)
    buf[:, :A] = np.tanh(g.normal(size=(n_total, A))).astype(np.float32)
    score = np.argsort(-m.astype(np.float64), kind="stable")[:n_listed]
    race = g.choice(n_total, size=r, replace=False) if r else np.zeros(0, dtype=np.int64)
    if r >= 1:
        race[0] = score[min(n + 1, n_listed - 1)]
    if r >= 2 and score[0] != race[0]:
        race[1] = score[0]
    row = np.full(rmax + L + 3, -1, dtype=np.int32)
    row[rmax - r : rmax] = race
    row[rmax : rmax + n_listed] = score
    return m, buf, row, r, n, n_listed


@pytest.mark.parametrize("n_total", [1, 2, 63, 64, 65, 1023, 1024, 1025, 16384])
def test_batched_kernel_equals_the_one_window_call_and_the_reference(lab, handle, n_total):
    dev = handle.device
    worst = 0.0
    host = torch.zeros((MAXE + 1) * 8, dtype=torch.float32).pin_memory()
    hnp = host.numpy()
    seq = 0.0
    for A in (1, 3, 17):
        for mult in (1, 4):
            rmax, L = LISTS[mult]
            tau32 = f32(1.0 if A == 3 else 0.01)
            wins = [_window(n_total, A, mult, rmax, L, rw, nw, tau32, 7919 * n_total + 100 * A + 10 * mult + w)
                    for w, (rw, nw, _) in enumerate(WINDOWS)]
            deltas = [f32(d) for _, _, d in WINDOWS]
            n_listed, LS = wins[0][5], rmax + L + 3
            assert all(w[5] == n_listed for w in wins)
            if n_total > 8:  # (the planted entry sits in both parts, and is counted once)
                assert wins[0][2][rmax - wins[0][3]] in wins[0][2][rmax + wins[0][4] : rmax + n_listed]
            assert wins[1][4] == n_listed and deltas[2] == 0.0
            # one row more than the largest launch, NaN / -1: no launch may read it
            md = torch.full((MAXE + 1, n_total), float("nan"), device=dev)
            ad = torch.full((MAXE + 1, n_total, mult * A), float("nan"), device=dev)
            ld = torch.full((MAXE + 1, LS), -1, dtype=torch.int32, device=dev)
            for w, (m, buf, row, _, _, _) in enumerate(wins):
                md[w], ad[w], ld[w] = torch.from_numpy(m).to(dev), torch.from_numpy(buf).to(dev), torch.from_numpy(row).to(dev)
            refs = [R.eval_bound_fast(m, buf[:, :A], row[rmax - r : rmax + n_listed], r, n, n_listed, tau32, deltas[w])
                    for w, (m, buf, row, r, n, _) in enumerate(wins)]
            # a finite tolerance shared by the windows: between two of window 0's bounds where they lie >= 5 % apart
            b = refs[0]["bounds"]
            ts = [t for t in range(1, len(b)) if b[t - 1] > 0 and b[t - 1] >= 1.05 * b[t]]
            tols = [INF]
            if ts:
                t = min(ts, key=lambda t: abs(t - len(b) // 2))
                tols.append(f32(math.sqrt(b[t - 1] * b[t]) if b[t] > 0 else 0.5 * b[t - 1]))
            for tol in tols:
                # the one-window call on every window's rows, once
                one = torch.full((MAXE, 8), float("nan"), device=dev)
                for w, (_, _, _, r, n, _) in enumerate(wins):
                    handle.eval_bound(md[w], ld[w, rmax - r :], r, n, n_listed, ad[w, :, :A], tau32, deltas[w], tol, stats=one[w])
                torch.cuda.synchronize()
                one = one.cpu().numpy()
                for E in (1, 3, 5):
                    what = (n_total, A, mult, E, tol)
                    ra, na = (ci * E)(*[w[3] for w in wins[:E]]), (ci * E)(*[w[4] for w in wins[:E]])
                    da = (cf * E)(*deltas[:E])
                    outs = []
                    for rep in range(2):
                        st = torch.full((MAXE + 1, 8), FSENT, device=dev)
                        hnp[:] = FSENT
                        seq = seq % 1000000 + 1
                        a = EvalBatchArgs(md.data_ptr(), E, n_total, ld.data_ptr(), rmax, LS, n_listed, ra, na, da, ad.data_ptr(),
                                          n_total * mult * A, mult * A, A, tau32, tol, st.data_ptr(), host.data_ptr(), seq,
                                          torch.cuda.current_stream().cuda_stream)
                        assert lab.m3pc_debug_eval_bound_batch(C.byref(a)) == 0, lab.m3pc_last_error()
                        torch.cuda.synchronize()
                        got = st.cpu().numpy()
                        outs.append(got.copy())
                        # every host block of the launch closes with the sequence number, payload as on the device; the rest untouched
                        hb = hnp.reshape(MAXE + 1, 8)
                        assert np.all(hb[:E, 4] == seq), what
                        assert np.array_equal(hb[:E][:, [0, 1, 2, 3, 5, 6, 7]].view(np.uint32), got[:E][:, [0, 1, 2, 3, 5, 6, 7]].view(np.uint32)), what
                        assert np.all(hb[E:] == FSENT) and np.all(got[E:] == FSENT), what
                    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), what
                    got = outs[0]
                    # bit for bit the one-window call, all eight floats (slot 4 is not written on the device: the sentinel / NaN)
                    keep = [0, 1, 2, 3, 5, 6, 7]
                    assert np.array_equal(got[:E][:, keep].view(np.uint32), one[:E][:, keep].view(np.uint32)), (what, got[:E], one[:E])
                    for w in range(E):
                        ref = refs[w]
                        for name, g_, want in (("eval_bound", got[w, 0], ref["eval_bound"]), ("P_U", got[w, 2], ref["P_U"]),
                                               ("bound(n_listed)", got[w, 6], ref["bound_listed"])):
                            if want == 0.0:
                                assert g_ == 0.0, (what, w, name, g_)
                            else:
                                worst = max(worst, abs(float(g_) - want) / want)
                                assert abs(float(g_) - want) <= 1e-3 * want, (what, w, name, float(g_), want)
                        assert int(got[w, 7]) == ref["n_U"], (what, w)
                        if tol == INF:
                            assert int(got[w, 1]) == wins[w][4], (what, w)
                    if E >= 3:
                        assert got[2, 0] == 0.0 and got[2, 6] == 0.0, what  # delta = 0: exactly 0
    print(f"n_total {n_total}: largest relative deviation from the fp64 reference {worst:.3e}")


def test_hook_refuses_bad_arguments(lab, handle):
    dev = handle.device
    n_total, A, rmax, L = 64, 3, 4, 32
    md, ad = torch.zeros((2, n_total), device=dev), torch.zeros((2, n_total, A), device=dev)
    ld = torch.zeros((2, rmax + L), dtype=torch.int32, device=dev)
    st = torch.zeros((2, 8), device=dev)

    def call(**kw):
        v = dict(merged=md.data_ptr(), n_windows=2, n_total=n_total, list=ld.data_ptr(), rmax=rmax, list_stride=rmax + L, n_listed=L,
                 r=(ci * 2)(2, 0), n=(ci * 2)(8, L), delta=(cf * 2)(0.5, 0.0), a0=ad.data_ptr(), a0_window_stride=n_total * A, a0_stride=A,
                 A=A, temperature=1.0, eval_tol=1e-3, stats=st.data_ptr(), host_stats=None, seq=0.0,
                 stream=torch.cuda.current_stream().cuda_stream)
        v.update(kw)
        return lab.m3pc_debug_eval_bound_batch(C.byref(EvalBatchArgs(**v)))

    assert call() == 0, lab.m3pc_last_error()
    torch.cuda.synchronize()
    for bad in (dict(merged=None), dict(list=None), dict(a0=None), dict(stats=None), dict(eval_tol=0.0), dict(eval_tol=float("nan")),
                dict(n_windows=0), dict(n_total=0), dict(n_total=16385), dict(A=0), dict(A=1025), dict(rmax=65), dict(n_listed=L + 1),
                dict(list_stride=rmax + L - 1), dict(r=(ci * 2)(5, 0)), dict(r=(ci * 2)(-1, 0)), dict(n=(ci * 2)(8, L + 1)),
                dict(n=(ci * 2)(-1, 0)), dict(delta=(cf * 2)(-1.0, 0.0)), dict(delta=(cf * 2)(float("nan"), 0.0))):
        assert call(**bad) == EINVAL, bad
    assert lab.m3pc_debug_eval_bound_batch(None) == EINVAL
