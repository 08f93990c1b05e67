"""mo_adamw_kernel (m3pc_amd/csrc/mtm_opt.hip) alone, through its lab hook m3pc_debug_mtm_adamw (include/m3pc_hip_debug.h), against the
float64 restatement tests/mtm_opt_ref.py within the per-element bound derived there (u = 2^-24; nothing is read from the device).

One launch over tensors of 1, 3, 63, 64, 65, 257, 4 * 64 + 3 elements and, because a workgroup owns MO_CHUNK = 2048 elements of one
tensor, 2048 + 5 and 3 * 2048 elements (more than one workgroup per tensor, a ragged last one), laid out back to back (bases off 16
bytes: the element-by-element path, every tensor boundary inside what would be one block of a flat grid) and 64-float aligned (the
16-byte path with its scalar tail), with mixed flags: decay on / off, active / inactive (an inactive tensor between two active ones),
per-tensor step counts 0, 1, 999 and 10^6 - 1 (t = 1, 2, 1000, 10^6)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mtm_opt_ref as OR

pytestmark = pytest.mark.gpu
vp, ci, ll, dbl = C.c_void_p, C.c_int, C.c_longlong, C.c_double
NUMELS = [1, 3, 63, 64, 65, 257, 4 * 64 + 3, 2048 + 5, 3 * 2048]
DECAY = [1, 0, 1, 0, 1, 1, 0, 1, 0]
ACTIVE = [1, 1, 0, 1, 1, 0, 1, 1, 1]
STEPS = [0, 1, 5, 999, 10 ** 6 - 1, 7, 0, 1, 999]
HAS_B = [1, 0, 1, 1, 0, 1, 1, 1, 1]
LR, WD, B1, B2, EPS = 9.7553e-4, 5e-3, 0.9, 0.999, 1e-8


class Args(C.Structure):
    _fields_ = [("n", ci), ("p", C.POINTER(vp)), ("b", C.POINTER(vp)), ("g_off", C.POINTER(ll)), ("s_off", C.POINTER(ll)), ("numel", C.POINTER(ll)),
                ("decay", C.POINTER(ci)), ("active", C.POINTER(ci)), ("grad", vp), ("grad_floats", ll), ("exp_avg", vp), ("exp_avg_sq", vp),
                ("state_floats", ll), ("steps_in", vp), ("steps_out", vp), ("write_bf16", ci), ("lr_t", dbl), ("weight_decay", dbl), ("beta1", dbl),
                ("beta2", dbl), ("eps", dbl), ("stream", vp), ("n_blocks", C.POINTER(ci))]


@pytest.fixture(scope="module")
def lib():
    from hip_util import lab_library
    lab = lab_library()
    lab.m3pc_debug_mtm_adamw.restype, lab.m3pc_debug_mtm_adamw.argtypes = ci, [C.POINTER(Args)]
    return lab


def _offsets(aligned, lead):
    offs, at = [], lead
    for n in NUMELS:
        offs.append(at)
        at += (n + 63) // 64 * 64 if aligned else n
    return offs, at


def _inputs(case, seed):
    """{p, g, m, v}: flat float32 host arrays, one segment after another (no padding: the layout adds it)."""
    rng = np.random.RandomState(seed)
    out = {k: [] for k in "pgmv"}
    for n in NUMELS:
        p = rng.normal(size=n).astype(np.float32)
        g = (rng.normal(size=n) * 10.0 ** rng.randint(-8, 2, size=n)).astype(np.float32)
        m = (rng.normal(size=n) * 1e-2).astype(np.float32)
        v = (rng.normal(size=n) ** 2 * 1e-4).astype(np.float32)
        if case == "zero":      # g = 0 with m = v = 0: p only decays, exactly
            g[:], m[:], v[:] = 0.0, 0.0, 0.0
        elif case == "specials":  # -0, denormals (alone and beside zero moments), +-1e18, an exact zero among ordinary values
            sp = np.array([-0.0, 1e-42, -3e-45, 1e18, -1e18, 0.0], np.float32)
            idx = np.arange(n) % 9
            for j, s in enumerate(sp):
                g[idx == j] = s
            zero_mv = (np.arange(n) // 9) % 2 == 1
            m[zero_mv], v[zero_mv] = 0.0, 0.0
        for k, a in zip("pgmv", (p, g, m, v)):
            out[k].append(a)
    return out


def _run(lib, inp, aligned, write_bf16, lead=0):
    """-> dict of host results.  lead: floats in front of the first segment (1 with the back-to-back layout: every base off 16 bytes)."""
    n = len(NUMELS)
    offs, total = _offsets(aligned, lead)
    flat = {}
    for k in "pgmv":
        a = np.full(total + 64, np.float32(777.0) if k == "p" else np.float32(0.5))  # (guard values between and behind the segments)
        for o, seg in zip(offs, inp[k]):
            a[o:o + seg.size] = seg
        flat[k] = torch.from_numpy(a.astype(np.float32)).cuda()
    bsz = [2 * x for x in NUMELS]
    bbuf = [torch.full((s + 8,), 0x1234, dtype=torch.int16, device="cuda") for s in bsz]
    steps_in = torch.tensor(STEPS, dtype=torch.int64, device="cuda")
    steps_out = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    a = Args()
    a.n = n
    a.p = (vp * n)(*[flat["p"].data_ptr() + 4 * o for o in offs])
    a.b = (vp * n)(*[(bbuf[i].data_ptr() if HAS_B[i] else None) for i in range(n)])
    a.g_off, a.s_off, a.numel = (ll * n)(*offs), (ll * n)(*offs), (ll * n)(*NUMELS)
    a.decay, a.active = (ci * n)(*DECAY), (ci * n)(*ACTIVE)
    a.grad, a.grad_floats = flat["g"].data_ptr(), total
    a.exp_avg, a.exp_avg_sq, a.state_floats = flat["m"].data_ptr(), flat["v"].data_ptr(), total
    a.steps_in, a.steps_out = steps_in.data_ptr(), steps_out.data_ptr()
    a.write_bf16 = write_bf16
    a.lr_t, a.weight_decay, a.beta1, a.beta2, a.eps = LR, WD, B1, B2, EPS
    a.stream = torch.cuda.current_stream().cuda_stream
    nb = ci(0)
    a.n_blocks = C.pointer(nb)
    torch.cuda.synchronize()
    rc = lib.m3pc_debug_mtm_adamw(C.byref(a))
    assert rc == 0, lib.m3pc_last_error()
    torch.cuda.synchronize()
    assert nb.value == sum((x + 2047) // 2048 for x in NUMELS)
    res = {k: flat[k].cpu().numpy() for k in "pgmv"}
    res["offs"], res["total"] = offs, total
    res["b"] = [b.cpu().numpy() for b in bbuf]
    res["steps"] = steps_out.cpu().numpy()
    return res


@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("case", ["random", "zero", "specials"])
def test_adamw_kernel_against_the_restatement(lib, case, aligned):
    inp = _inputs(case, 11)
    lead = 0 if aligned else 1
    res = _run(lib, inp, aligned, 1, lead)
    again = _run(lib, inp, aligned, 1, lead)
    for k in "pmv":
        assert res[k].tobytes() == again[k].tobytes(), "run to run: " + k
    assert all(x.tobytes() == y.tobytes() for x, y in zip(res["b"], again["b"]))
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    covered = np.zeros(res["total"] + 64, bool)
    for i, (n, o) in enumerate(zip(NUMELS, res["offs"])):
        sl = slice(o, o + n)
        covered[sl] = True
        p0, g0, m0, v0 = (inp[k][i] for k in "pgmv")
        pr, mr, vr, st, bp, bm, bv = OR.adamw_tensor(p0, g0, m0, v0, STEPS[i], LR, WD, DECAY[i], ACTIVE[i], B1, B2, EPS)
        assert res["steps"][i] == st, (i, res["steps"][i], st)
        if not ACTIVE[i]:  # every bit stays, the bf16 copies included
            assert res["p"][sl].tobytes() == p0.tobytes() and res["m"][sl].tobytes() == m0.tobytes() and res["v"][sl].tobytes() == v0.tobytes(), i
            assert (res["b"][i] == 0x1234).all(), i
            continue
        assert np.isfinite(res["p"][sl]).all() and np.isfinite(res["m"][sl]).all() and np.isfinite(res["v"][sl]).all(), i
        for k, got, ref, bound in (("p", res["p"][sl], pr, bp), ("m", res["m"][sl], mr, bm), ("v", res["v"][sl], vr, bv)):
            w = OR.worst(got, ref, bound)
            worst[k] = max(worst[k], w)
            assert w <= 1.0, (case, aligned, i, n, k, w)
        if case == "zero":
            keep = (1.0 - LR * WD) if DECAY[i] else 1.0
            assert res["p"][sl].tobytes() == (p0.astype(np.float64) * keep).astype(np.float32).tobytes(), i
            assert not res["m"][sl].any() and not res["v"][sl].any()
        if HAS_B[i]:  # hi | lo, exact; nothing behind them
            hi, lo = OR.bf16_split(res["p"][sl])
            assert res["b"][i][:n].tobytes() == hi.tobytes() and res["b"][i][n:2 * n].tobytes() == lo.tobytes(), i
            assert (res["b"][i][2 * n:] == 0x1234).all(), i
    # nothing outside the segments moved (guard values), and the gradient is read-only
    assert (res["p"][~covered] == np.float32(777.0)).all() and (res["m"][~covered] == 0.5).all() and (res["v"][~covered] == 0.5).all()
    g_in = np.full(res["total"] + 64, np.float32(0.5))
    for o, seg in zip(res["offs"], inp["g"]):
        g_in[o:o + seg.size] = seg
    assert res["g"].tobytes() == g_in.tobytes()
    print(f"mo_adamw_kernel {case} {'aligned' if aligned else 'back to back'}: worst err / bound  p {worst['p']:.3f}  m {worst['m']:.3f}  v {worst['v']:.3f}")


def test_write_bf16_off_leaves_the_copies(lib):
    inp = _inputs("random", 12)
    on, off = _run(lib, inp, True, 1), _run(lib, inp, True, 0)
    for k in "pmv":
        assert on[k].tobytes() == off[k].tobytes(), k
    assert all((b == 0x1234).all() for b in off["b"])


def test_refusals(lib):
    a = Args()
    assert lib.m3pc_debug_mtm_adamw(None) == -1
    a.n = 0
    assert lib.m3pc_debug_mtm_adamw(C.byref(a)) == -1 and b"n 0" in lib.m3pc_last_error()
    a.n = 1
    assert lib.m3pc_debug_mtm_adamw(C.byref(a)) == -1 and b"null" in lib.m3pc_last_error()
