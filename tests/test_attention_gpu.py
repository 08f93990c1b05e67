"""Every attention kernel of the library (attn.hip, attn_bf16.hip), in every head width it is built for, element by element against
the float64 reference of tests/attn_ref.py and its rounding-derived bound, through the lab hook m3pc_debug_attention.

Each case names the kernel id the dispatch must pick (the list is in include/m3pc_hip_debug.h); test_every_kernel_id_has_a_case
checks that the cases reach every id of that list.  Every case runs in four score regimes (attn_ref.make_inputs: N(0, 1), peaked
with the dominant key on a tile seam / the last key / the first shared key / inside the pre-reduced block, a large common offset,
identical keys), on inputs whose unread memory (columns past n_head hd, rows past L1 / Lq inside the batch strides) is NaN and
with an output buffer whose guard rows and columns hold a sentinel."""
import ctypes as C
import os
import re

import pytest
import torch

import attn_ref as R
from hip_util import lab_library

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -31744.0  # exact in bf16 and fp32; no attention output comes near it
PRESTATS = 50

# (name, dtype, hd, n_head, batch, Lq, L1, L2, Lq2, Lp, orow1, orow2, expected kernel id)
#  Lp > 0: a pre-reduced block (batch-shared queries).  Pads keep every row and stride on 16 bytes.
CASES = [
    # fp32: attn_pair_kernel<4> (batch * heads * ceil(Lq / 128) <= 64, Lk <= 64)
    ("f32_pair_b1", 0, 128, 8, 1, 33, 17, 32, 0, 0, 0, 0, 1),
    ("f32_pair_b16", 0, 128, 4, 16, 1, 2, 0, 0, 0, 0, 0, 1),
    # fp32: attn_split_kernel
    ("f32_split32", 0, 32, 2, 16, 65, 97, 32, 0, 0, 0, 0, 2),
    ("f32_split32_l1", 0, 32, 2, 8, 31, 1, 0, 0, 0, 0, 0, 2),
    ("f32_split64", 0, 64, 2, 1, 129, 200, 56, 0, 0, 0, 0, 3),
    ("f32_split64_h8", 0, 64, 8, 8, 32, 16, 16, 0, 0, 0, 0, 3),
    ("f32_split128", 0, 128, 8, 8, 31, 65, 0, 0, 0, 0, 0, 4),
    ("f32_split128_255", 0, 128, 4, 12, 1, 127, 128, 0, 0, 0, 0, 4),
    # fp32: attn_kernel<HDT, NCH>
    ("f32_nch1_32", 0, 32, 2, 257, 32, 64, 0, 0, 0, 0, 0, 5),
    ("f32_nch2_32", 0, 32, 2, 300, 97, 96, 31, 0, 0, 0, 0, 6),
    ("f32_nch4_32", 0, 32, 2, 256, 256, 192, 0, 0, 0, 0, 0, 7),
    ("f32_nch1_64", 0, 64, 2, 300, 33, 48, 15, 0, 0, 0, 0, 8),
    ("f32_nch2_64", 0, 64, 8, 257, 64, 65, 0, 0, 0, 0, 0, 9),
    ("f32_nch4_64", 0, 64, 2, 512, 1, 129, 127, 0, 0, 0, 0, 10),
    ("f32_nch1_128", 0, 128, 8, 256, 129, 31, 2, 0, 0, 0, 0, 11),
    ("f32_nch2_128", 0, 128, 4, 2048, 17, 97, 0, 0, 0, 0, 0, 12),
    ("f32_nch4_128", 0, 128, 8, 16, 128, 63, 130, 0, 0, 0, 0, 13),
    # bf16: the pipelined kernels at their exact shapes (4 heads of 128, batch * 4 >= 1024)
    ("pipe49", 1, 128, 4, 512, 49, 49, 0, 0, 0, 1, 0, 20),
    ("pipe49_b2048", 1, 128, 4, 2048, 49, 49, 0, 0, 0, 0, 0, 20),
    ("pipe17_32", 1, 128, 4, 257, 17, 17, 32, 32, 0, 32, 0, 21),
    ("pipe_dec49", 1, 128, 4, 300, 32, 49, 0, 0, 47, 0, 0, 22),
    ("pipe_mix", 1, 128, 4, 2048, 1, 49, 79, 31, 0, 0, 1, 23),
    ("pipe_mix_q4", 1, 128, 4, 257, 4, 49, 79, 28, 0, 0, 4, 23),
    ("pipe_wide97", 1, 128, 4, 256, 97, 97, 0, 0, 0, 0, 0, 24),
    ("pipe_wide33_64", 1, 128, 4, 300, 33, 33, 64, 64, 0, 64, 0, 25),
    ("pipe_wide_dec", 1, 128, 4, 257, 64, 97, 0, 0, 95, 0, 0, 26),
    # bf16: two windows per tile
    ("pack2_32", 1, 32, 2, 64, 16, 15, 0, 0, 0, 0, 0, 27),
    ("pack2_64", 1, 64, 2, 65, 1, 9, 0, 0, 0, 0, 0, 28),
    ("pack2_128", 1, 128, 8, 257, 15, 16, 0, 0, 0, 0, 0, 29),
    # bf16: attn_bf16_direct_kernel<HDT, 1, 2> / <HDT, 2, 2> / <HDT, 2, 4>
    ("direct12_32", 1, 32, 2, 1, 1, 2, 0, 0, 0, 0, 0, 30),
    ("direct22_32", 1, 32, 2, 16, 33, 31, 2, 0, 0, 0, 0, 31),
    ("direct24_32_q2", 1, 32, 2, 8, 31, 48, 48, 33, 0, 33, 0, 32),
    ("direct12_64", 1, 64, 2, 300, 31, 31, 0, 0, 0, 2, 0, 33),
    ("direct22_64", 1, 64, 8, 12, 64, 64, 0, 0, 0, 0, 0, 34),
    ("direct24_64", 1, 64, 2, 256, 65, 63, 65, 0, 0, 0, 0, 35),
    ("direct12_128_pre", 1, 128, 8, 1, 32, 1, 0, 0, 63, 0, 0, 36),
    ("direct22_128", 1, 128, 4, 16, 48, 48, 0, 0, 0, 0, 0, 37),
    ("direct24_128", 1, 128, 4, 300, 97, 96, 0, 0, 0, 0, 0, 38),
    ("direct24_128_pre", 1, 128, 4, 257, 31, 49, 31, 0, 129, 0, 0, 38),
    # bf16: attn_bf16_kernel<HDT, 4> (Lk > 128)
    ("nch4_32", 1, 32, 2, 16, 129, 128, 128, 0, 0, 0, 0, 39),
    ("nch4_64_q2", 1, 64, 8, 256, 1, 129, 0, 30, 0, 30, 0, 40),
    ("nch4_64_q256", 1, 64, 2, 8, 256, 255, 0, 0, 0, 0, 0, 40),
    ("nch4_128", 1, 128, 8, 12, 65, 63, 129, 0, 0, 0, 0, 41),
    ("nch4_128_pre", 1, 128, 4, 8, 32, 130, 0, 0, 50, 0, 0, 41),
]
PIPELINED = range(20, 27)
WORST = {}  # (kernel id, regime) -> largest err / bound


def header_ids():
    """The ids the header's list names, without the A/B-only ones (42..47)."""
    src = open(os.path.join(ROOT, "include", "m3pc_hip_debug.h")).read()
    block = src[src.index("Kernel ids"):src.index("int m3pc_debug_attention(")]
    ids = set()
    for line in block.splitlines():
        if "A/B-only" in line:
            continue
        for a, b in re.findall(r"\((\d+)\.\.(\d+)\)", line):
            ids |= set(range(int(a), int(b) + 1))
        line = re.sub(r"\(\d+\.\.\d+\)", "", line)
        line = re.sub(r"<[^>]*>|hd [\d / ]+|NCH [\d / ]+|for [^;]*", "", line)
        ids |= {int(x) for x in re.findall(r"(?<![\w+])(\d+)(?= )", line) if int(x) >= 1}
    return ids


def _hook(lib):
    fn = lib.m3pc_debug_attention
    fn.restype = C.c_int
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    fn.argtypes = [i, vp, ll, i, i, i, vp, i, i, i, vp, vp, ll, i, i, vp, vp, i, i, vp, vp, i, i, vp, vp, ll, i, i, i, i, C.c_float, i,
                   C.POINTER(C.c_int), vp]
    return fn


def _poisoned(x, rows, ld, et, batch=None):
    """x (.., n, W) into a NaN buffer of `rows` rows of `ld` elements (per batch element when batch is given)."""
    shape = (batch, rows, ld) if batch is not None else (rows, ld)
    buf = torch.full(shape, float("nan"), device="cuda", dtype=et)
    buf[..., :x.shape[-2], :x.shape[-1]] = x.to(et)
    return buf


def _dom(case, regime, ci):
    """The dominant key of the peaked regime: inside the pre block, else the first shared key, else a tile seam, else the last key."""
    name, dt, hd, nh, B, Lq, L1, L2, Lq2, Lp, o1, o2, kid = case
    if Lp:
        return L1 + L2 + Lp // 2
    if L2:
        return L1
    seams = [j for j in (31, 32, 63, 64, 127, 128) if j < L1 + L2]
    return seams[ci % len(seams)] if seams else L1 + L2 - 1


def run_case(lib, case, regime, t, kernel=0):
    """One call of the hook on poisoned buffers; returns (O buffer, picked, layout)."""
    name, dt, hd, nh, B, Lq, L1, L2, Lq2, Lp, o1, o2, kid = case
    et = torch.bfloat16 if dt else torch.float32
    W = nh * hd
    ldq, ldkv, ld2, ldp, ldo = W + 8, W + 16, W + 24, W + 8, W + 8
    shared_q = Lp > 0
    # (4 poisoned rows behind every segment: the pipelined kernels fetch rows in pieces of 4 and mask what lies past the segment)
    Q = _poisoned(t["q"][0], Lq + 4, ldq, et) if shared_q else _poisoned(t["q"], Lq + 4, ldq, et, B)
    K1, V1 = _poisoned(t["k1"], L1 + 4, ldkv, et, B), _poisoned(t["v1"], L1 + 4, ldkv, et, B)
    Q2 = _poisoned(t["q2"], Lq2 + 4, ld2, et) if Lq2 else None
    K2 = _poisoned(t["k2"], L2 + 4, ld2, et) if L2 else None
    V2 = _poisoned(t["v2"], L2 + 4, ld2, et) if L2 else None
    Kp = _poisoned(t["kp"], Lp + 4, ldp, et) if Lp else None
    Vp = _poisoned(t["vp"], Lp + 4, ldp, et) if Lp else None
    pre = torch.full((nh * Lq * (2 + hd),), float("nan"), device="cuda") if Lp else None
    R_out = max(o1 + Lq, o2 + Lq2) + 2  # (two guard rows after the last segment)
    Ob = torch.full((B + 1, R_out, ldo), SENT, device="cuda", dtype=et)  # (one whole guard element behind the batch)
    O = Ob[:B]
    picked = (C.c_int * 2)()
    ptr = lambda x: x.data_ptr() if x is not None else None
    rc = _hook(lib)(dt, Q.data_ptr(), 0 if shared_q else Q.stride(0), ldq, Lq, o1, ptr(Q2), ld2, Lq2, o2, K1.data_ptr(), V1.data_ptr(),
                    K1.stride(0), ldkv, L1, ptr(K2), ptr(V2), ld2, L2, ptr(Kp), ptr(Vp), ldp, Lp, ptr(pre), O.data_ptr(), O.stride(0),
                    ldo, B, nh, hd, hd ** -0.5, kernel, picked, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.m3pc_last_error()
    torch.cuda.synchronize()
    assert (Ob[B] == SENT).all(), "a store went past the last batch element"
    return O, (picked[0], picked[1])


def check_case(case, regime, t, O, chunk_elems=1 << 26):
    """Every batch element against the float64 reference (on the GPU, chunked over the batch), the guards against the sentinel.
    Returns the largest err / bound."""
    name, dt, hd, nh, B, Lq, L1, L2, Lq2, Lp, o1, o2, kid = case
    W = nh * hd
    Lk = L1 + L2 + Lp
    nq = Lq + Lq2
    cb = max(1, min(B, chunk_elems // max(1, nh * nq * Lk * 4)))
    worst = 0.0
    rows = None
    for b0 in range(0, B, cb):
        b1 = min(B, b0 + cb)
        q = t["q"] if Lp else t["q"][b0:b1]
        ref = R.attention_ref(q, t["k1"][b0:b1], t["v1"][b0:b1], nh, hd ** -0.5, q2=t["q2"], k2=t["k2"], v2=t["v2"], kp=t["kp"],
                              vp=t["vp"], orow1=o1, orow2=o2, n_rows=O.shape[1])
        if regime == "peaked":
            assert float(ref["p"].amax(-1).min()) >= 0.9, "peaked regime: no key carries 0.9 of the weight"
        rows = ref["rows"]
        got = O[b0:b1].double()
        out = got[:, rows, :W]
        assert torch.isfinite(out).all(), f"{name}/{regime}: non-finite output (a poisoned element was read)"
        assert not (out == SENT).any(), f"{name}/{regime}: an output element was not written"
        bnd = R.bound(ref, dt)[:, rows]
        err = (out - ref["O"][:, rows]).abs()
        ratio = float((err / bnd).max())
        if ratio > 1:
            i = int((err - bnd).flatten().argmax())
            raise AssertionError(f"{name}/{regime}: err / bound {ratio:.3g} (worst flat index {i}, err {float(err.flatten()[i]):.3g}, "
                                 f"bound {float(bnd.flatten()[i]):.3g})")
        worst = max(worst, ratio)
        assert (got[:, ~rows] == SENT).all(), f"{name}/{regime}: a guard row was written"
        assert (got[:, :, W:] == SENT).all(), f"{name}/{regime}: a guard column was written"
    return worst


@pytest.fixture(scope="module")
def lib():
    return lab_library()


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c[0] for c in CASES])
def test_attention_kernel_against_float64(lib, ci, regime):
    case = CASES[ci]
    name, dt, hd, nh, B, Lq, L1, L2, Lq2, Lp, o1, o2, kid = case
    t = R.make_inputs(regime, B, Lq, L1, nh, hd, Lq2=Lq2, L2=L2, Lp=Lp, shared_q=Lp > 0, dom=_dom(case, regime, ci), dtype=dt,
                      device="cuda", seed=1000 * ci + R.REGIMES.index(regime))
    O, picked = run_case(lib, case, regime, t)
    assert picked == (kid, PRESTATS if Lp else 0), f"{name}: dispatch picked {picked}, the case is for kernel {kid}"
    worst = check_case(case, regime, t, O)
    WORST[(kid, regime)] = max(WORST.get((kid, regime), 0.0), worst)
    if kid in PIPELINED:  # the pipelined kernels stay the direct kernel bit for bit, in every regime
        O1, picked1 = run_case(lib, case, regime, t, kernel=1)
        assert picked1[0] not in PIPELINED
        assert torch.equal(O.view(torch.int16), O1.view(torch.int16)), f"{name}/{regime}: pipelined != direct kernel {picked1[0]}"
    print(f"{name:18s} {regime:7s} kernel {kid:2d}  max err/bound {worst:.3g}")


@pytest.mark.parametrize("name", ["pipe49", "pipe_mix", "direct24_64", "f32_nch1_32", "f32_nch2_128", "pack2_64"])
def test_a_batch_element_does_not_depend_on_its_position(lib, name):
    """Rotating the batch rotates the output bit for bit (same kernel picked): no persistent-workgroup iteration, item split or
    tile pairing leaks into the arithmetic of an element."""
    ci = [c[0] for c in CASES].index(name)
    case = CASES[ci]
    _, dt, hd, nh, B, Lq, L1, L2, Lq2, Lp, o1, o2, kid = case
    t = R.make_inputs("randn", B, Lq, L1, nh, hd, Lq2=Lq2, L2=L2, Lp=Lp, shared_q=Lp > 0, dtype=dt, device="cuda", seed=7 + ci)
    O, picked = run_case(lib, case, "randn", t)
    r = 37 % B
    tr = dict(t)
    for k in ("k1", "v1") + (() if Lp else ("q",)):
        tr[k] = torch.roll(t[k], r, 0)
    Or, pickedr = run_case(lib, case, "randn", tr)
    assert picked == pickedr == (kid, PRESTATS if Lp else 0)
    assert torch.equal(torch.roll(O, r, 0).view(torch.int16 if dt else torch.int32), Or.view(torch.int16 if dt else torch.int32))


def test_every_kernel_id_has_a_case():
    """The cases above name every kernel id of include/m3pc_hip_debug.h (and each case asserts that the dispatch picked it): a kernel
    added to the dispatch and the list without a case fails here.  Prints the largest err / bound per (kernel, regime) seen."""
    want = header_ids()
    assert len([i for i in want if i < 20]) == 13 and len([i for i in want if 20 <= i < 50]) == 22 and PRESTATS in want, sorted(want)
    have = {c[-1] for c in CASES} | ({PRESTATS} if any(c[9] for c in CASES) else set())
    assert have == want, (sorted(want - have), sorted(have - want))
    if WORST:
        print("\nlargest err / bound per (kernel, regime):")
        for kid in sorted({k for k, _ in WORST}):
            print(f"  kernel {kid:2d}: " + "  ".join(f"{rg} {WORST[(kid, rg)]:.3g}" for rg in R.REGIMES if (kid, rg) in WORST))
