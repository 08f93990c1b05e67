"""Every kernel of m3pc_amd/csrc/mtm_grad.hip at its edges, each alone through its lab hook (include/m3pc_hip_debug.h: m3pc_debug_mg_gemm,
_layernorm, _colsum, _attention, _tokens, _std, _loss_bwd -- the launchers m3pc_mtm_grad itself goes through) against the references
of tests/mtm_grad_kernels_ref.py.

Each case names the kernel id its launch must report (the header's "MTM-gradient kernel ids"); test_every_mtm_grad_kernel_has_a_case
checks that the cases reach exactly the 15 ids.  The product runs in four regimes: `int` must EQUAL the reference, `randn`, `offset`
and `spike` (a large term at k = K - 1 and one at k = 63) are held to the derived element-wise bound; the copies, the embedding and the
column sums are held bit for bit to a restatement in the kernel's order; everything else to its derived bound.  Everything a kernel may
not read holds NaN (padding of a padded ld, rows a row map skips, rows >= M or >= K, token rows of hidden timesteps, the floats behind
P); every output holds a sentinel in its padding and in a guard row and is compared bit for bit with its state before the call
outside the elements the call owns."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_ref as AR
import gemm_ref as GM
import mtm_grad_kernels_ref as R
import mtm_grad_lab as ML
import mtm_loss_ref as LR
from elementwise_ref import ln_inputs
from mtm_grad_kernels_ref import F, KID

pytestmark = pytest.mark.gpu

SENT = -31744.0
DEV = "cuda"
ci = C.c_int
WORST = {}   # (kernel id, output) -> largest err / bound
EXACT = {}   # kernel id -> comparisons that were exact
REACHED = set()
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    return ML.lab()


def P(t):
    return None if t is None else t.data_ptr()


def call(lib, fn, a, want, what, *args):
    """Runs a hook, checks its return code and the kernel id(s) it reports; want: an id or a tuple of ids (all launched, the last last)."""
    picked = (ci * 2)(-1, -1)
    want = want if isinstance(want, tuple) else (want,)
    st = torch.cuda.current_stream().cuda_stream
    if a is None:
        rc = getattr(lib, fn)(*args, st, C.cast(picked, ML.pi))
    else:
        a.picked = C.cast(picked, ML.pi)
        a.stream = st
        rc = getattr(lib, fn)(C.byref(a))
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a device error: nothing more is started on that device
        pytest.exit(f"{what}: {e}", returncode=3)
    if rc != 0:
        msg = lib.m3pc_last_error()
        if b"HIP" in msg or b"hip" in msg:
            pytest.exit(f"{what}: {msg}", returncode=3)
        raise AssertionError((what, msg))
    assert picked[0] == want[-1] and picked[1] == sum(1 << i for i in want), f"{what}: the launcher reports kernel {picked[0]} (set {picked[1]:#x}), the case is for {want}"
    REACHED.update(want)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def nan_rows(x, ld, prow=None, tail=1):
    """x's rows at physical rows prow (default: in order) of a NaN buffer with leading dimension ld and `tail` NaN rows behind."""
    prow = torch.arange(x.shape[0], device=DEV) if prow is None else prow
    buf = torch.full((int(prow.max()) + 1 + tail, ld), NAN, device=DEV)
    buf[prow, :x.shape[1]] = x.float()
    return buf


def sent(rows, ld, dtype=torch.float32):
    return torch.full((rows + 1, ld), SENT, device=DEV, dtype=dtype)


def owned(buf, before, rows, cols, what):
    """The elements the call owns (rows x cols: index tensors or slices), all written; outside them the buffer kept its bits."""
    after = buf.clone()
    after[rows, cols] = before[rows, cols]
    assert torch.equal(_bits(after), _bits(before)), f"{what}: a padding column, a guard row or a row of no owner was written"
    o = buf[rows, cols]
    assert not bool((o == SENT).any()), f"{what}: an element was not written"
    return o


def same(t, before, what):
    assert torch.equal(_bits(t), _bits(before)), f"{what}: an input was written"


def hold(kid, key, out, ref, bound, what, exact_regime=False):
    """exact_regime: equality; else err <= bound wherever the reference is finite, specials at the same places; the ratio is recorded."""
    out, ref = out.double(), ref.double()
    if exact_regime:
        assert torch.equal(out, ref), f"{what}: {key} differs from the exact result at {int((out != ref).sum())} elements, largest {float((out - ref).abs().max())}"
        EXACT[kid] = EXACT.get(kid, 0) + 1
        return
    assert LR.same_specials(out.cpu().numpy(), ref.cpu().numpy()), f"{what}: {key} has NaN / inf where the reference has none (or the reverse)"
    ok = torch.isfinite(ref)
    if not bool(ok.any()):
        return
    ratio = float(((out - ref).abs()[ok] / bound.expand_as(ref)[ok]).max())
    WORST[(kid, key)] = max(WORST.get((kid, key), 0.0), ratio)
    print(f"{what}: {key} err / bound {ratio:.3g}")
    assert ratio <= 1, f"{what}: {key} err / bound {ratio:.3g}"


def exact(kid, got, want, what):
    """Bit for bit against a numpy restatement."""
    got = got.detach().cpu().numpy()
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = got.view(np.int32) != want.view(np.int32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ from the restatement in the kernel's order"
    EXACT[kid] = EXACT.get(kid, 0) + 1


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ------------------------------------------------------------------------------------------------ the product
SIZES = (1, 31, 32, 33, 65)
K_PLAIN = (1, 3, 4, 8, 12, 15, 16, 17, 20, 31, 32, 33, 256)
K_SPLIT = (1, 5, 15, 16, 17, 32, 33, 48, 49, 64, 65, 80, 200)
EPI = ("bias", "bias2", "pos_T", "res", "gelu_aux", "gelu_out", "acc", "cmap")


def _gemm_cases():
    cs = []
    add = lambda form, M, N, K, **kw: cs.append(dict(form=form, M=M, N=N, K=K, **kw))
    # every K edge in each layout of its form; M and N walk through the tile edges
    for i, K in enumerate(K_PLAIN):
        add("fwd", SIZES[i % 5], SIZES[(i + 2) % 5], K, rpg=(1, 5)[i % 2], bias=True)
        add("dx", SIZES[(i + 1) % 5], SIZES[(i + 3) % 5], K, acc=bool(i % 2), cmap=bool((i // 2) % 2))
    for i, K in enumerate(K_SPLIT):
        for j, kmap in enumerate(("none", "dec", "enc")):
            add("dw", SIZES[(i + j) % 5], SIZES[(i + 2 * j + 1) % 5], K, kmap=kmap)
    # every (M, N) tile shape in both forms: 65 x 65 is nine tiles (the last workgroup of the plain form keeps one wavefront), 1 x 1 one
    for M in SIZES:
        for N in SIZES:
            add("fwd" if (M + N) % 2 else "dx", M, N, 20, rpg=5)
            add("dw", M, N, 33, kmap="none")
    # the epilogues, each alone and as the model combines them (M crosses multiples of pos_T)
    e = dict(M=33, N=33, K=20)
    for kw in (dict(bias=True), dict(bias=True, bias2=True), dict(bias=True, bias2=True, pos_T=1), dict(bias=True, bias2=True, pos_T=5),
               dict(pos_T=5), dict(res=True), dict(gelu_out=True), dict(acc=True), dict(bias=True, res=True), dict(bias=True, gelu_out=True),
               dict(bias=True, bias2=True, pos_T=5, cmap=True, rpg=5)):
        add("fwd", **e, **kw)
    for kw in (dict(gelu_aux=True), dict(gelu_aux=True, acc=True, cmap=True), dict(acc=True, cmap=True)):
        add("dx", **e, **kw)
    add("dw", 33, 31, 49, kmap="dec", bias=True, acc=True)
    add("dw", 6, 64, 3, kmap="enc")
    # a k-contiguous operand 4 bytes off 16-byte alignment: the scalar path, the same bits
    add("fwd", 33, 31, 20, bias=True, unaligned=True)
    add("dx", 31, 33, 32, unaligned=True)
    for c in cs:
        c["split"] = c["form"] == "dw"
        c["kid"] = KID["gemm_split"] if c["split"] else KID["gemm"]
        c["name"] = f"{c['form']}_M{c['M']}_N{c['N']}_K{c['K']}" + "".join(f"_{k}{'' if v is True else v}" for k, v in c.items() if k in EPI + ("rpg", "kmap", "unaligned") and v)
    return list({c["name"]: c for c in cs}.values())


GEMM_CASES = _gemm_cases()


def gemm_launch(lib, c, t, off=0):
    """Lays the logical tensors out as the form reads them and runs the hook.  off: floats the k-contiguous operand's base is moved by."""
    M, N, K, form = c["M"], c["N"], c["K"], c["form"]
    A, W = t["A"], t["W"]
    a = ML.GemmArgs()
    keep = []

    def op(buf, s_o, s_k, rmap, map_k, shift=0):
        if shift:
            big = torch.full((buf.numel() + 4,), NAN, device=DEV)
            big[shift:shift + buf.numel()] = buf.reshape(-1)
            buf = big[shift:shift + buf.numel()]
            keep.append(big)
        keep.append(buf)
        return ML.Op(buf.data_ptr(), s_o, s_k, (ci * 3)(*rmap), map_k, buf.numel()), buf

    none = (0, 0, 0)
    if form == "fwd":
        rpg = c.get("rpg", 1)
        amap = (rpg, 4 * rpg, 2 * rpg)
        lda = (K + 3) // 4 * 4 + 4
        a.A, Ab = op(nan_rows(A, lda, GM.map_rows(amap, M, DEV)), lda, 1, amap, 0, off)
        ldb = (K + 3) // 4 * 4
        a.B, Bb = op(nan_rows(W, ldb), ldb, 1, none, 0)
        want_vec = (off == 0, True)
    elif form == "dx":
        a.A, Ab = op(nan_rows(A, K), K, 1, none, 0, off)
        a.B, Bb = op(nan_rows(W.T, N + 1), 1, N + 1, none, 0)
        want_vec = (K % 4 == 0 and off == 0, False)
    else:
        T = 7
        kmap = {"none": none, "dec": (T, 4 * T, 2 * T), "enc": (1, 9, 3)}[c["kmap"]]
        prow = GM.map_rows(kmap, K, DEV)
        a.A, Ab = op(nan_rows(A.T, M + 1, prow), 1, M + 1, kmap, 1)
        a.B, Bb = op(nan_rows(W.T, N + 2, prow), 1, N + 2, kmap, 1)
        want_vec = (False, False)
    # the launcher's own `vec` rule, restated: the case is on the path it is meant for
    for o, w in zip((a.A, a.B), want_vec):
        assert bool(o.s_k == 1 and not o.map_k and o.s_o % 4 == 0 and o.p % 16 == 0) == w, (c["name"], "vec")
    cmap = (3, 5, 2) if c.get("cmap") else none
    crow = GM.map_rows(cmap, M, DEV)
    ldc = N + 3
    rows = int(crow.max()) + 1
    Cb = sent(rows, ldc)
    if c.get("acc"):
        Cb[crow, :N] = t["c0"]
    aux = lambda x: None if x is None else nan_rows(x, ldc, crow)
    res, gaux = aux(t.get("res")), aux(t.get("gelu_aux"))
    Gb = sent(rows, ldc) if c.get("gelu_out") else None
    a.C, a.ldc, a.c_len, a.cmap, a.M, a.N, a.K = P(Cb), ldc, Cb.numel(), (ci * 3)(*cmap), M, N, K
    bias, bias2, pos = t.get("bias"), t.get("bias2"), t.get("pos")
    a.bias, a.bias2, a.pos, a.pos_T = P(bias), P(bias2), P(pos), c.get("pos_T") or 0
    a.res, a.gelu_aux, a.gelu_out, a.accumulate, a.splitk = P(res), P(gaux), P(Gb), int(bool(c.get("acc"))), int(c["split"])
    before, gbefore = Cb.clone(), (None if Gb is None else Gb.clone())
    ins = [(x, x.clone()) for x in (Ab, Bb, res, gaux) if x is not None]
    call(lib, "m3pc_debug_mg_gemm", a, c["kid"], c["name"])
    for x, b in ins:
        same(x, b, c["name"])
    cols = slice(0, N)
    out = owned(Cb, before, crow, cols, c["name"] + " C")
    g = None if Gb is None else owned(Gb, gbefore, crow, cols, c["name"] + " gelu_out")
    return out, g


def gemm_tensors(c, regime, seed):
    return R.gemm_inputs(regime, c["M"], c["N"], c["K"], DEV, seed, bias=bool(c.get("bias")), bias2=bool(c.get("bias2")), pos_T=c.get("pos_T") or 0,
                         res=bool(c.get("res")), gelu_aux=bool(c.get("gelu_aux")), c0=bool(c.get("acc")))


@pytest.mark.parametrize("c", GEMM_CASES, ids=[c["name"] for c in GEMM_CASES])
def test_gemm_against_float64(lib, c):
    for ri, regime in enumerate(R.GEMM_REGIMES):
        what = f"{c['name']}/{regime}"
        t = gemm_tensors(c, regime, 1000 * c["K"] + 10 * c["M"] + c["N"] + ri)
        out, g = gemm_launch(lib, c, t)
        ref = R.mg_gemm_ref(t, pos_T=c.get("pos_T") or 1, splitk=c["split"], gelu_out=bool(c.get("gelu_out")))
        hold(c["kid"], "C", out, ref["C"], ref["E"], what, regime == "int")
        if g is not None:
            hold(c["kid"], "gelu_out", g, ref["G"], ref["EG"], what)
        if c.get("unaligned"):
            out1, g1 = gemm_launch(lib, c, t, off=1)
            assert torch.equal(_bits(out1), _bits(out)), f"{what}: the scalar path of the unaligned operand gives other bits"
            EXACT[c["kid"]] = EXACT.get(c["kid"], 0) + 1


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_CASES = [dict(rows=rows, d=d, mapped=mapped, name=f"ln_r{rows}_d{d}" + ("_map" if mapped else ""))
            for rows in (1, 3, 4, 5, 9) for d in (64, 192, 1024) for mapped in (False, True)]
LN_MAP = (5, 20, 10)


@pytest.mark.parametrize("c", LN_CASES, ids=[c["name"] for c in LN_CASES])
def test_layernorm_forward_and_backward_against_float64(lib, c):
    rows, d = c["rows"], c["d"]
    xmap = LN_MAP if c["mapped"] else (0, 0, 0)
    prow = GM.map_rows(xmap, rows, DEV)
    r = torch.arange(rows, device=DEV)
    for ri, regime in enumerate(("randn", "offset")):
        what = f"{c['name']}/{regime}"
        x, g, b, _, _ = ln_inputs(regime, rows, d, False, DEV, 100 * d + rows + ri)
        X = nan_rows(x, d, prow)
        # forward: Y and st
        a = ML.LnArgs()
        Y, st = sent(rows, d), sent(rows, 2)
        yb, sb, xb = Y.clone(), st.clone(), X.clone()
        a.X, a.xmap, a.x_rows, a.g, a.b, a.Y, a.st, a.rows, a.d = P(X), (ci * 3)(*xmap), X.shape[0], P(g), P(b), P(Y), P(st), rows, d
        call(lib, "m3pc_debug_mg_layernorm", a, KID["ln_fwd"], what)
        same(X, xb, what)
        y = owned(Y, yb, r, slice(0, d), what + " Y")
        s = owned(st, sb, r, slice(0, 2), what + " st")
        hold(KID["ln_fwd"], "Y", y, GM.layernorm64(x, g, b), GM.ln_bound(x, g, b), what)
        m64, r64 = R.ln_stats64(x)
        dm, dr = R.ln_stat_bound(x)
        hold(KID["ln_fwd"], "mean", s[:, 0], m64, dm, what)
        hold(KID["ln_fwd"], "rstd", s[:, 1], r64, dr, what)
        # backward, alone: the statistics are the float64 ones rounded to float32
        stin = torch.stack([m64.float(), r64.float()], 1).contiguous()
        dy = torch.randn(rows, d, device=DEV, generator=torch.Generator(device=DEV).manual_seed(d + rows + ri))
        dY = nan_rows(dy, d)
        for accumulate in (0, 1):
            dX = sent(X.shape[0] - 1, d)
            dx0 = torch.randn(rows, d, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7 + ri)) if accumulate else torch.full((rows, d), 7.5, device=DEV)
            dX[prow] = dx0                                    # accumulate 0: garbage the call must overwrite
            a = ML.LnArgs()
            a.backward, a.X, a.xmap, a.x_rows, a.g, a.st, a.dY, a.dX = 1, P(X), (ci * 3)(*xmap), X.shape[0], P(g), P(stin), P(dY), P(dX)
            a.rows, a.d, a.accumulate = rows, d, accumulate
            before, ins = dX.clone(), [(t, t.clone()) for t in (X, stin, dY)]
            call(lib, "m3pc_debug_mg_layernorm", a, KID["ln_bwd"], what)
            for t, tb in ins:
                same(t, tb, what)
            out = owned(dX, before, prow, slice(0, d), what + " dX")
            ev = R.ln_bwd_ref(x, dy, g, stin[:, 0], stin[:, 1], dx0 if accumulate else None)
            hold(KID["ln_bwd"], "dX+=" if accumulate else "dX", out, ev.v, ev.bound(), what)


# ------------------------------------------------------------------------------------------------ column sums
ALL = (1 << 64) - 1


def _colsum_cases():
    cs = []
    shapes = [(1, 1), (63, 1), (1, 64), (64, 1), (13, 5), (65, 1), (43, 3), (129, 1), (3, 43)]  # (nseq, n): 1, 63, 64, 64, 65, 65, 129, 129, 129 rows
    Cs = (1, 6, 255, 256, 257, 768)
    for i, (nseq, n) in enumerate(shapes):
        for j in range(2):
            k = 2 * i + j
            sel = {0: ALL, 1: ALL & ~0b100 & ~(1 << (n // 2)), 2: 1, 3: ALL}[k % 4] if n > 1 else ALL
            cs.append(dict(nseq=nseq, n=n, C=Cs[k % 6], compact=k % 2, withx=bool((k // 2) % 2), sel=sel, j0=(0, 2)[(k // 3) % 2], out1=bool(k % 3)))
    cs.append(dict(nseq=2, n=64, C=6, compact=0, withx=True, sel=1 << 63, j0=0, out1=True))   # only bit 63 at n = 64
    cs.append(dict(nseq=2, n=64, C=257, compact=1, withx=False, sel=1, j0=3, out1=False))     # only bit 0
    cs.append(dict(nseq=3, n=43, C=768, compact=1, withx=True, sel=ALL & ~(1 << 7), j0=1, out1=True))
    for C_ in Cs:
        cs.append(dict(nseq=65, n=1, C=C_, compact=0, withx=True, sel=ALL, j0=0, out1=True))
    for c in cs:
        c["out1"] = c["out1"] and c["withx"]
        c["name"] = f"cs_{c['nseq']}x{c['n']}_C{c['C']}" + ("_compact" if c["compact"] else "") + ("_X" if c["withx"] else "") + f"_sel{c['sel'] & ((1 << c['n']) - 1):x}_j{c['j0']}" + ("" if c["out1"] or not c["withx"] else "_no1")
    return list({c["name"]: c for c in cs}.values())


COLSUM_CASES = _colsum_cases()


def colsum_run(lib, c, seed, part=None):
    nseq, n, C_, j0, sel = c["nseq"], c["n"], c["C"], c["j0"], c["sel"]
    L = j0 + n + 1
    total, buf_rows = nseq * n, (nseq - 1) * L + j0 + n
    rng = np.random.RandomState(seed)
    rowsel = R.colsum_rows(nseq, L, j0, n, sel)
    ldy = C_ + 3
    dYn = np.full((total if c["compact"] else buf_rows, ldy), np.nan, F)
    Xn = np.full((buf_rows, C_), np.nan, F)
    stn = np.full((total, 2), np.nan, F)
    for q, br in rowsel:                                   # only the selected rows hold numbers
        dYn[q if c["compact"] else br, :C_] = rng.normal(size=C_)
        Xn[br] = rng.normal(size=C_) * 3 + 1
        stn[q] = (rng.normal(), np.exp(rng.normal()))
    dY, X, st = dev(dYn), (dev(Xn) if c["withx"] else None), (dev(stn) if c["withx"] else None)
    chunks = (total + 63) // 64
    need = chunks * 2 * C_
    if part is None:
        part = torch.full((need + 8,), SENT, device=DEV, dtype=torch.float64)
    o0 = sent(0, C_ + 1)
    o1 = sent(0, C_ + 1) if c["out1"] else None
    a = ML.ColsumArgs()
    a.dY, a.dy_compact, a.ldy, a.X, a.st, a.nseq, a.L, a.j0, a.n, a.sel, a.C = P(dY), c["compact"], ldy, P(X), P(st), nseq, L, j0, n, sel, C_
    a.part, a.part_doubles, a.buf_rows, a.out0, a.out1 = P(part), need, buf_rows, P(o0), P(o1)
    pb, b0, b1 = part.clone(), o0.clone(), (None if o1 is None else o1.clone())
    ins = [(t, t.clone()) for t in (dY, X, st) if t is not None]
    call(lib, "m3pc_debug_mg_colsum", a, (KID["colsum"], KID["colsum_fin"]), c["name"])
    for t, tb in ins:
        same(t, tb, c["name"])
    assert torch.equal(_bits(part[need:]), _bits(pb[need:])), f"{c['name']}: the scratch was written beyond chunks * 2 * C doubles"
    z = torch.zeros(1, dtype=torch.long, device=DEV)
    got0 = owned(o0, b0, z, slice(0, C_), c["name"] + " out0")[0]
    got1 = None if o1 is None else owned(o1, b1, z, slice(0, C_), c["name"] + " out1")[0]
    w0, w1 = R.colsum_ref(dYn, c["compact"], Xn if c["withx"] else None, stn, nseq, L, j0, n, sel, C_)
    exact(KID["colsum_fin"], got0, w0, c["name"] + " out0")
    if got1 is not None:
        exact(KID["colsum_fin"], got1, w1, c["name"] + " out1")
    EXACT[KID["colsum"]] = EXACT.get(KID["colsum"], 0) + 1
    return part


@pytest.mark.parametrize("c", COLSUM_CASES, ids=[c["name"] for c in COLSUM_CASES])
def test_column_sums_bit_for_bit(lib, c):
    colsum_run(lib, c, 17 + c["C"] + c["nseq"])


def test_a_column_sum_of_fewer_chunks_ignores_the_scratch_of_the_one_before(lib):
    big = dict(nseq=129, n=1, C=257, compact=0, withx=True, sel=ALL, j0=0, out1=True, name="cs_scratch_three_chunks")
    small = dict(nseq=1, n=1, C=257, compact=0, withx=True, sel=ALL, j0=0, out1=True, name="cs_scratch_one_chunk")
    part = colsum_run(lib, big, 5)
    colsum_run(lib, small, 6, part=part)   # (exact against its own restatement: nothing of the first call's partials is added)


# ------------------------------------------------------------------------------------------------ attention
ATT_L = (1, 4, 63, 64, 65, 128, 129, 256)
ATT_HEADS = ((64, 2, 32), (64, 1, 64), (128, 1, 128))


def _attn_cases():
    cs = []
    for li, L in enumerate(ATT_L):
        for hi, (d, nh, hd) in enumerate(ATT_HEADS):
            regimes = AR.REGIMES if hi == 0 else (AR.REGIMES[(li + hi) % 4],)
            for regime in regimes:
                B = 1 if (L == 1 and nh == 1) or L > 65 else (3 if L <= 4 else 2 if nh == 2 else 1)
                cs.append(dict(L=L, d=d, nh=nh, hd=hd, regime=regime, B=B, name=f"att_L{L}_d{d}_h{nh}x{hd}_B{B}_{regime}"))
    assert any(c["B"] * c["nh"] * c["L"] == 1 for c in cs) and any(c["B"] * c["nh"] * c["L"] % 4 for c in cs)
    return cs


ATT_CASES = _attn_cases()


def attn_args(which, c, QKV=None, Pb=None, O=None, dO=None, dQKV=None):
    a = ML.AttnArgs()
    a.which, a.QKV, a.P, a.O, a.dO, a.dQKV = which, P(QKV), P(Pb), P(O), P(dO), P(dQKV)
    a.B, a.L, a.d, a.nh, a.hd, a.scale = c["B"], c["L"], c["d"], c["nh"], c["hd"], c["hd"] ** -0.5
    return a


def p_buffer(p, fill=NAN):
    """P (B, nh, L, L) with 64 floats behind it that no kernel may touch."""
    n = p.numel()
    buf = torch.full((n + 64,), fill, device=DEV)
    buf[:n] = p.reshape(-1).float()
    return buf, n


def attn_inputs(c, seed):
    t = AR.make_inputs(c["regime"], c["B"], c["L"], c["L"], c["nh"], c["hd"], dtype=0, device=DEV, seed=seed)
    QKV = torch.cat([t["q"], t["k1"], t["v1"]], -1).contiguous()
    dO = torch.randn(c["B"], c["L"], c["d"], device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed + 1))
    return QKV, dO


def third(d, i):
    return slice(i * d, (i + 1) * d)


@pytest.mark.parametrize("c", ATT_CASES, ids=[c["name"] for c in ATT_CASES])
def test_attention_kernels_alone_against_float64(lib, c):
    B, L, d, nh = c["B"], c["L"], c["d"], c["nh"]
    what, scale = c["name"], c["hd"] ** -0.5
    QKV, dO = attn_inputs(c, 31 * L + d + nh)
    rows = torch.arange(B * L, device=DEV)
    qkv2, do2 = nan_rows(QKV.reshape(B * L, 3 * d), 3 * d), nan_rows(dO.reshape(B * L, d), d)
    # forward
    Pref, EP, Oref, EO = R.attn_fwd_ref(QKV, nh, scale)
    Pb, n = p_buffer(torch.full_like(Pref, SENT), SENT)
    O = sent(B * L, d)
    pb, ob, qb = Pb.clone(), O.clone(), qkv2.clone()
    call(lib, "m3pc_debug_mg_attention", attn_args(0, c, qkv2, Pb, O), KID["attn_fwd"], what + " fwd")
    same(qkv2, qb, what)
    assert torch.equal(_bits(Pb[n:]), _bits(pb[n:])) and not bool((Pb[:n] == SENT).any()), f"{what}: P written beyond (B, nh, L, L) or not everywhere"
    hold(KID["attn_fwd"], "P", Pb[:n].reshape(Pref.shape), Pref, EP, what)
    hold(KID["attn_fwd"], "O", owned(O, ob, rows, slice(0, d), what + " O").reshape(B, L, d), Oref, EO, what)
    # dV = P^T dO on the float64 softmax rounded to float32
    Pin = Pref.float()
    Pb, n = p_buffer(Pin)
    dQKV = sent(B * L, 3 * d)
    pb, db, dob = Pb.clone(), dQKV.clone(), do2.clone()
    call(lib, "m3pc_debug_mg_attention", attn_args(1, c, None, Pb, None, do2, dQKV), KID["attn_col"], what + " dV")
    same(Pb, pb, what)
    same(do2, dob, what)
    ev = R.attn_col_ref(Pin, dO, nh, 1.0)
    hold(KID["attn_col"], "dV", owned(dQKV, db, rows, third(d, 2), what + " dV").reshape(B, L, d), ev.v, ev.bound(), what)
    # dS over P and dQ
    dQKV = sent(B * L, 3 * d)
    db = dQKV.clone()
    call(lib, "m3pc_debug_mg_attention", attn_args(2, c, qkv2, Pb, None, do2, dQKV), KID["attn_row"], what + " row")
    same(qkv2, qb, what)
    same(do2, dob, what)
    assert torch.equal(_bits(Pb[n:]), _bits(pb[n:])), f"{what}: dS written beyond (B, nh, L, L)"
    ds, dq = R.attn_row_ref(Pin, dO, QKV, nh, scale)
    hold(KID["attn_row"], "dS", Pb[:n].reshape(Pref.shape), ds.v, ds.bound(), what)
    hold(KID["attn_row"], "dQ", owned(dQKV, db, rows, third(d, 0), what + " dQ").reshape(B, L, d), dq.v, dq.bound(), what)
    # dK = dS^T Q scale on the float64 dS rounded to float32
    dsin = ds.v.float()
    Sb, n = p_buffer(dsin)
    dQKV = sent(B * L, 3 * d)
    sb, db = Sb.clone(), dQKV.clone()
    call(lib, "m3pc_debug_mg_attention", attn_args(3, c, qkv2, Sb, None, None, dQKV), KID["attn_col"], what + " dK")
    same(Sb, sb, what)
    ev = R.attn_col_ref(dsin, QKV[..., :d], nh, scale)
    hold(KID["attn_col"], "dK", owned(dQKV, db, rows, third(d, 1), what + " dK").reshape(B, L, d), ev.v, ev.bound(), what)


@pytest.mark.parametrize("L,heads", [(65, ATT_HEADS[0]), (129, ATT_HEADS[1]), (4, ATT_HEADS[2])])
def test_the_chain_reuses_p_in_place(lib, L, heads):
    """fwd -> col(dV) -> row -> col(dK) on ONE P buffer and one dQKV, as block_bwd runs them, gives the bits of the four kernels run
    alone on copies: the row kernel's dS lands where the last kernel reads it, and no kernel touches another's third of dQKV."""
    d, nh, hd = heads
    c = dict(L=L, d=d, nh=nh, hd=hd, B=2, regime="randn")
    B = 2
    QKV, dO = attn_inputs(c, 99 + L)
    qkv2, do2 = QKV.reshape(B * L, 3 * d).contiguous(), dO.reshape(B * L, d).contiguous()
    n = B * nh * L * L
    run = lambda which, Pb, O, dQKV, k: call(lib, "m3pc_debug_mg_attention", attn_args(which, c, qkv2, Pb, O, do2, dQKV), k, f"chain L{L} {which}")
    Pc, Oc, Dc = torch.full((n + 64,), SENT, device=DEV), sent(B * L, d), sent(B * L, 3 * d)
    guard = Dc[B * L:].clone()
    for which, k in ((0, KID["attn_fwd"]), (1, KID["attn_col"]), (2, KID["attn_row"]), (3, KID["attn_col"])):
        run(which, Pc, Oc, Dc, k)
    assert torch.equal(_bits(Dc[B * L:]), _bits(guard)) and not bool((Dc[:B * L] == SENT).any()) and bool((Pc[n:] == SENT).all())
    # staged: every kernel on its own copies
    P1, O1 = torch.full((n + 64,), SENT, device=DEV), sent(B * L, d)
    run(0, P1, O1, None, KID["attn_fwd"])
    D1, D2, D3 = sent(B * L, 3 * d), sent(B * L, 3 * d), sent(B * L, 3 * d)
    run(1, P1.clone(), None, D1, KID["attn_col"])
    P2 = P1.clone()
    run(2, P2, None, D2, KID["attn_row"])
    run(3, P2.clone(), None, D3, KID["attn_col"])
    staged = torch.cat([D2[:B * L, third(d, 0)], D3[:B * L, third(d, 1)], D1[:B * L, third(d, 2)]], 1)
    assert torch.equal(_bits(Dc[:B * L]), _bits(staged)) and torch.equal(_bits(Pc), _bits(P2)) and torch.equal(_bits(Oc), _bits(O1))
    for k in (KID["attn_fwd"], KID["attn_col"], KID["attn_row"]):
        EXACT[k] = EXACT.get(k, 0) + 1


# ------------------------------------------------------------------------------------------------ token layout
def mask_sets(T):
    al, last = list(range(T)), [T - 1]
    sets = {"all_visible": [al, al, al, al], "alternating": [al[0::2], al[1::2], al[0::2], al[1::2]],
            "middle_key_hidden": [al, [], al, last], "two_middle_keys_hidden": [[0], [], [], al]}
    for k in range(4):
        sets[f"one_token_key{k}"] = [last if j == k else [] for j in range(4)]
    return sets


def _token_cases():
    cs, i = [], 0
    for T in (1, 5, 64):
        for name in mask_sets(T):
            cs.append(dict(T=T, B=(1, 3)[i % 2], SA=((1, 1), (17, 6), (12, 8))[i % 3], mask=name, name=f"tok_T{T}_{name}"))
            i += 1
    for c in cs:
        c["name"] += f"_B{c['B']}_S{c['SA'][0]}A{c['SA'][1]}"
    return cs


TOKEN_CASES = _token_cases()


@pytest.mark.parametrize("c", TOKEN_CASES, ids=[c["name"] for c in TOKEN_CASES])
def test_token_kernels_bit_for_bit(lib, c):
    T, B, d, what = c["T"], c["B"], 64, c["name"]
    feat = (c["SA"][0], c["SA"][1], 1, 1)
    bits, kept, eoff, Le = R.mask_bits(mask_sets(T)[c["mask"]], T)
    rng = np.random.RandomState(T + B + feat[0])
    f = lambda *s: rng.normal(size=s).astype(F)
    tok = [f(B, T, feat[k]) for k in range(4)]
    for k in range(4):
        for t in range(T):
            if not (bits[k] >> t) & 1:
                tok[k][:, t] = np.nan                       # the rows of hidden timesteps are never read
    W, bias, pdim, mtok, pos = [f(d, feat[k]) for k in range(4)], [f(d) for _ in range(4)], [f(d) for _ in range(4)], [f(d) for _ in range(4)], f(T, d)
    keep = [[dev(x) for x in xs] for xs in (tok, W, bias, pdim, mtok)]
    posd = dev(pos)

    def args(which, **kw):
        a = ML.TokensArgs()
        for k in range(4):
            a.tok[k], a.W[k], a.bias[k], a.pdim[k], a.mtok[k] = (P(keep[i][k]) for i in range(5))
            a.bits[k], a.kept[k], a.eoff[k], a.feat[k] = bits[k], kept[k], eoff[k], feat[k]
        a.which, a.pos, a.B, a.T, a.d, a.Le = which, P(posd), B, T, d, Le
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    enc = torch.arange(B * Le, device=DEV)
    # embed
    X = sent(B * Le, d)
    xb = X.clone()
    call(lib, "m3pc_debug_mg_tokens", args(0, X=P(X)), KID["embed"], what + " embed")
    exact(KID["embed"], owned(X, xb, enc, slice(0, d), what + " X"), R.embed_ref(tok, W, bias, pdim, pos, bits, B, T, d).reshape(B * Le, d), what + " embed")
    # gather: the visible rows from src, the mask token of every hidden token
    srcn = f(B, Le, d)
    src, Z = nan_rows(dev(srcn.reshape(B * Le, d)), d), sent(B * 4 * T, d)
    zb, sb = Z.clone(), src.clone()
    call(lib, "m3pc_debug_mg_tokens", args(1, src=P(src), dst=P(Z)), KID["gather"], what + " gather")
    same(src, sb, what)
    z = owned(Z, zb, torch.arange(B * 4 * T, device=DEV), slice(0, d), what + " Zin")
    zref = R.gather_ref(srcn, mtok, bits, B, T, d)
    exact(KID["gather"], z, zref.reshape(B * 4 * T, d), what + " gather")
    # scatter of rows whose hidden tokens hold NaN; scatter o gather is the identity on the visible rows
    for name, zin in (("scatter", f(B, 4 * T, d)), ("scatter o gather", zref.copy())):
        for k in range(4):
            for t in range(T):
                if not (bits[k] >> t) & 1:
                    zin[:, k * T + t] = np.nan
        zsrc, E = nan_rows(dev(zin.reshape(B * 4 * T, d)), d), sent(B * Le, d)
        eb, zsb = E.clone(), zsrc.clone()
        call(lib, "m3pc_debug_mg_tokens", args(2, src=P(zsrc), dst=P(E)), KID["scatter"], what + " " + name)
        same(zsrc, zsb, what)
        got = owned(E, eb, enc, slice(0, d), what + " dEncN")
        exact(KID["scatter"], got, (srcn if name != "scatter" else R.scatter_ref(zin, bits, B, T, d)).reshape(B * Le, d), what + " " + name)
    # tokv of every key that keeps a token
    for k in range(4):
        if kept[k]:
            out = sent(B * kept[k], feat[k])
            ob = out.clone()
            call(lib, "m3pc_debug_mg_tokens", args(3, key=k, out=P(out)), KID["tokv"], what + f" tokv {k}")
            got = owned(out, ob, torch.arange(B * kept[k], device=DEV), slice(0, feat[k]), what + " tokv")
            exact(KID["tokv"], got, R.tokv_ref(tok[k], bits[k], T), what + f" tokv {k}")


# ------------------------------------------------------------------------------------------------ std, the loss backward
LOSS_SHAPES = [(1, 11, 3), (3, 17, 6), (5, 1, 1)]
LOSS_SETTINGS = [(R.CLIP_ACTIONS, 1), (R.NORM_L2, 15), (R.CLIP_ACTIONS, 6), (R.NORM_L2, 0)]
LOSS_CASES = [dict(B=B, T=T, S=S, A=A, flags=fl, keys=lk, special=None, name=f"loss_B{B}_T{T}_S{S}_A{A}_f{fl}_k{lk}")
              for (B, S, A) in LOSS_SHAPES for T in (1, 8, 64) for fl, lk in LOSS_SETTINGS]
LOSS_CASES += [dict(B=5, T=8, S=1, A=1, flags=R.NORM_L2, keys=15, special="zero_target", name="loss_norm_l2_of_a_zero_target"),
               dict(B=3, T=8, S=17, A=6, flags=R.CLIP_ACTIONS, keys=15, special="all_visible", name="loss_every_action_visible"),
               dict(B=1, T=1, S=11, A=3, flags=R.NORM_L2, keys=15, special="all_visible", name="loss_every_action_visible_T1")]


@pytest.mark.parametrize("c", LOSS_CASES, ids=[c["name"] for c in LOSS_CASES])
def test_std_and_loss_backward_against_float64(lib, c):
    B, T, S, A, flags, keys, what = c["B"], c["T"], c["S"], c["A"], c["flags"], c["keys"], c["name"]
    pred, mu, ls, tgt, eps = R.loss_inputs(B, T, S, A, 1, bool(flags & R.CLIP_ACTIONS))
    if c["special"] == "zero_target":
        tgt[0][3, 0] = 0.0
    mask = R.loss_masks(T, 3, all_visible=c["special"] == "all_visible")
    assert c["special"] == "all_visible" or not (mask[1] >> (T - 1)) & 1      # the last action timestep (bit 63 at T = 64) is hidden
    rows = B * T
    r = torch.arange(rows, device=DEV)
    pred, tgt = [x.to(DEV) for x in pred], [x.to(DEV) for x in tgt]
    mu, ls, eps = mu.to(DEV), ls.to(DEV), eps.to(DEV)
    # std
    sdb = sent(rows, A)
    sb, lb = sdb.clone(), ls.clone()
    call(lib, "m3pc_debug_mg_std", None, KID["std"], what + " std", P(ls), P(sdb), rows * A)
    same(ls, lb, what)
    got = owned(sdb.reshape(-1), sb.reshape(-1), torch.arange(rows * A, device=DEV), Ellipsis, what + " sd")
    ev = R.std_ref(ls)
    hold(KID["std"], "sd", got.reshape(rows, A), ev.v, ev.bound(), what)
    # the loss backward, alone: sd is the float64 value rounded to float32
    sd = ev.v.float().contiguous()
    hidden = T - bin(mask[1]).count("1")
    with np.errstate(divide="ignore"):
        inv_cnt = float(F(np.float64(1.0) / np.float64(B * hidden * A)))      # as mg_run computes it: inf when every action is visible
    a = ML.LossBwdArgs()
    widths = (S, 1, 1)
    # (the kernel writes compact rows: the outputs are flat, a guard row of sentinels behind)
    dpf = [torch.full((rows * widths[j] + 8,), SENT, device=DEV) for j in range(3)]
    dmu, dls = torch.full((rows * A + 8,), SENT, device=DEV), torch.full((rows * A + 8,), SENT, device=DEV)
    for j in range(3):
        a.pred[j], a.dpred[j] = P(pred[j]), P(dpf[j])
    for k in range(4):
        a.tgt[k], a.mask[k] = P(tgt[k]), mask[k]
    a.mu, a.sd, a.ls, a.eps, a.dmu, a.dls = P(mu), P(sd), P(ls), P(eps), P(dmu), P(dls)
    a.batch, a.T, a.S, a.A, a.flags, a.loss_keys, a.entropy_reg, a.inv_cnt = B, T, S, A, flags, keys, 0.1, inv_cnt
    ins = [(t, t.clone()) for t in pred + tgt + [mu, sd, ls, eps]]
    call(lib, "m3pc_debug_mg_loss_bwd", a, KID["loss_bwd"], what)
    for t, tb in ins:
        same(t, tb, what)
    rp, rmu, rls = R.loss_bwd_ref(pred, mu, sd, ls, tgt, eps, mask, B, T, S, A, flags, keys, 0.1, inv_cnt)
    outs = [(dpf[j], rows * widths[j], rp[j], ("dstates", "drewards", "dreturns")[j]) for j in range(3)] + [(dmu, rows * A, rmu, "dmu"), (dls, rows * A, rls, "dls")]
    for buf, n, ev, key in outs:
        assert bool((buf[n:] == SENT).all()) and not bool((buf[:n] == SENT).any()), f"{what}: {key} written beyond its rows or not everywhere"
        hold(KID["loss_bwd"], key, buf[:n].reshape(ev.v.shape), ev.v, ev.bound(), what)
    if c["special"] == "zero_target":
        assert bool(torch.isnan(dpf[0][3])) and int(torch.isnan(dpf[0][:rows]).sum()) == 1
    if c["special"] == "all_visible":
        assert not np.isfinite(inv_cnt) and not bool(dls[:rows * A].any()) and bool(torch.isfinite(dmu[:rows * A]).all())
        assert all(bool(torch.isfinite(dpf[j][:rows * widths[j]]).all()) for j in range(3))


# ------------------------------------------------------------------------------------------------ closing
def test_every_mtm_grad_kernel_has_a_case():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "m3pc_hip_debug.h")).read()
    block = hdr[hdr.index("MTM-gradient kernel ids"):hdr.index("(end of the MTM-gradient kernel ids)")]
    ids = {int(n): k for n, k in re.findall(r"(\d+) (mg_[a-z0-9_]+_kernel(?:<[a-z]+>)?)", block)}
    assert len(ids) == 15
    print("\nlargest err / bound per kernel and output:")
    for (kid, key), v in sorted(WORST.items()):
        print(f"  {kid:2d} {ids[kid]:24s} {key:10s} {v:.3g}")
    print("exact comparisons per kernel:", {ids[k]: v for k, v in sorted(EXACT.items())})
    if REACHED:  # (run alone, this test has nothing to say)
        assert REACHED == set(ids), f"the cases reach {sorted(REACHED)}, the header lists {sorted(ids)}"
        bitwise = {KID[k] for k in ("gemm", "gemm_split", "colsum", "colsum_fin", "embed", "gather", "scatter", "tokv")}
        assert bitwise <= set(EXACT), f"no exact comparison ran for {sorted(bitwise - set(EXACT))}"
