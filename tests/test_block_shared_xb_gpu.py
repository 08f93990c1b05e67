"""The bf16-residual fused layer tail (block_fused_kernel<0, 0|1, 1>) reading shared leading rows: with x_bf16 and res_L > 0 the
residual comes from a compact block -- the res_nshared shared rows stored once, then every sequence's res_L - res_nshared own rows
(block_res_row_xb in csrc/kernels.h; the embedding kernel writes that block for the first encoder layer of a candidate pass).

The reference is the plain x_bf16 launch of the same kernel instance on the EXPANDED rows (the shared block repeated in front of each
sequence's own rows): the compact launch must give the same bits in every output -- X'', the LayerNorm rows (TAIL 0) or the next
layer's Q|K|V rows (TAIL 1) -- and leave the rows past M, the padding columns and its inputs untouched.  Nothing here is a
tolerance: both launches add the same residual values to the same products in the same order.

The shapes put the three boundaries a residual piece of 8 rows can cross (shared -> own, own -> the next sequence's shared rows, the
end of M) inside pieces, on piece edges, and many times per piece.

Xout is a buffer of its own in this form: the residual block has another shape than X'' (full rows r), so the in-place launch of the
plain form does not exist here and block_fused_accepts refuses Xout == res.  One case stores no X'' at all; one writes X'' into the
same allocation the compact block lives in, directly in front of it (the layout of run_encoder), while the block is being read."""
import ctypes as C

import pytest
import torch

import block_ref as R
import test_block_edges_gpu as E

pytestmark = pytest.mark.gpu

D, DEV, SENT = R.D, E.DEV, E.SENT
BF = torch.bfloat16
# (res_L, res_nshared, sequences, extra rows of a last, partial sequence, padded leading dimensions)
SHAPES = [
    (49, 33, 1, 0, False),   # one partial tile
    (49, 33, 3, 0, True),    # a partial second tile; every boundary inside an 8-row piece
    (49, 33, 6, 0, False),   # 294 rows: a sequence straddling a tile edge
    (48, 32, 3, 0, False),   # boundaries on piece edges
    (5, 2, 27, 0, False),    # 135 rows: many boundaries per piece
    (49, 48, 3, 0, False),   # one own row per sequence
    (49, 1, 3, 0, False),    # one shared row
    (49, 33, 2, 40, False),  # M ends inside a sequence's own rows (138 rows)
    (49, 33, 2, 7, False),   # M ends inside a sequence's shared rows (105 rows)
]
IDS = [f"L{L}_ns{ns}_n{n}" + (f"_plus{x}" if x else "") + ("_pad" if p else "") for L, ns, n, x, p in SHAPES]


@pytest.fixture(scope="module")
def lib():
    return E.lab()


def _rows(L, ns, nseq, extra, seed):
    """The compact block (shared rows, then own rows sequence by sequence) and the M expanded rows it stands for."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    nfull = nseq + (1 if extra else 0)
    shared = torch.randn(ns, D, device=DEV, generator=g).to(BF)
    own = torch.randn(nfull, L - ns, D, device=DEV, generator=g).to(BF)
    M = nseq * L + extra
    expanded = torch.cat([torch.cat([shared, own[b]]) for b in range(nfull)])[:M]
    n_own = sum(max(0, min(L, M - b * L) - ns) for b in range(nfull))  # own rows that a token row < M names
    compact = torch.cat([shared, own.reshape(-1, D)[:n_own]])
    O = torch.randn(M, D, device=DEV, generator=g).to(BF)
    return M, O, compact, expanded


def _padded(rows, ld, fill=float("nan")):
    """rows + one guard row, leading dimension ld: NaN wherever the kernel may not read."""
    buf = torch.full((rows.shape[0] + 1, ld), fill, device=DEV, dtype=BF)
    buf[:-1, :D] = rows
    return buf


def _launch(lib, dev, M, O, res, ldr, res_L, ns, tail, X, ldx, out, ldo):
    a = E.BArgs()
    picked = (E.ci * 1)(-1)
    a.O, a.ldo, a.M = O.data_ptr(), O.shape[1], M
    a.res, a.ldr, a.res_L, a.res_nshared = res.data_ptr(), ldr, res_L, ns
    a.Wo, a.W1, a.W2, a.stream_buf = dev["Wo"].data_ptr(), dev["W1"].data_ptr(), dev["W2"].data_ptr(), E.stream_buf(lib)["b"].data_ptr()
    a.bo, a.b1, a.b2 = dev["bo"].data_ptr(), dev["b1"].data_ptr(), dev["b2"].data_ptr()
    a.ln2_g, a.ln2_b, a.lnA_g, a.lnA_b = dev["g2"].data_ptr(), dev["be2"].data_ptr(), dev["gA"].data_ptr(), dev["bA"].data_ptr()
    a.x_bf16 = 1
    if X is not None:
        a.Xout, a.ldx = X.data_ptr(), ldx
    if tail == 1:
        a.QKVout, a.ldq, a.qkv_bytes, a.bqkv, a.Wqkv = out.data_ptr(), ldo, M * ldo * 2, dev["bqkv"].data_ptr(), dev["Wqkv"].data_ptr()
    else:
        a.Hout, a.ldh = out.data_ptr(), ldo
    a.picked = C.cast(picked, C.POINTER(E.ci))
    a.stream = torch.cuda.current_stream().cuda_stream
    rc = lib.m3pc_debug_block_ex(C.byref(a))
    assert rc == 0, lib.m3pc_last_error()
    torch.cuda.synchronize()
    assert picked[0] == 16 + tail, picked[0]


def _same(a, b, what):
    assert torch.equal(E._bits(a), E._bits(b)), what


@pytest.mark.parametrize("tail", [0, 1], ids=["plain", "qkv"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_compact_rows_give_the_bits_of_expanded_rows(lib, shape, tail):
    L, ns, nseq, extra, pad = shape
    _, dev = E.params("random")
    M, O, compact, expanded = _rows(L, ns, nseq, extra, 100 * L + ns + nseq)
    ldr = 520 if pad else 512
    ldo = (1544 if pad else 1536) if tail else (520 if pad else 512)
    wid = 3 * D if tail else D
    Ob = _padded(O, 520 if pad else 512)
    outs = []
    for res, rl, rn in ((_padded(expanded, ldr), 0, 0), (_padded(compact, ldr), L, ns)):
        X = torch.full((M + 1, ldr), SENT, device=DEV, dtype=BF)
        out = torch.full((M + 1, ldo), SENT, device=DEV, dtype=BF)
        res0 = res.clone()
        _launch(lib, dev, M, Ob, res, ldr, rl, rn, tail, X, ldr, out, ldo)
        _same(res, res0, "the residual rows were written")
        outs.append((X, out))
    (Xr, outr), (Xc, outc) = outs
    # the reference launch wrote every element it owns and nothing else (so the comparison below also says: rows past M, padding
    # columns and the guard row are untouched by the compact launch)
    assert not bool((Xr[:M, :D] == SENT).any()) and not bool((outr[:M, :wid] == SENT).any())
    assert bool(torch.isfinite(Xr[:M, :D].float()).all()) and bool(torch.isfinite(outr[:M, :wid].float()).all())
    assert bool((Xr[M] == SENT).all()) and bool((outr[M] == SENT).all()) and bool((Xr[:, D:] == SENT).all()) and bool((outr[:, wid:] == SENT).all())
    _same(Xc, Xr, "X'' differs from the launch on expanded rows")
    _same(outc, outr, ("Q|K|V" if tail else "LayerNorm rows") + " differ from the launch on expanded rows")


@pytest.mark.parametrize("tail", [0, 1], ids=["plain", "qkv"])
def test_without_xout_and_with_xout_in_front_of_the_block(lib, tail):
    """X'' dead (nothing stored: Xout aliases nothing), and X'' written into the allocation that holds the compact block, directly in
    front of it, while the block is read: the same LayerNorm / Q|K|V bits as the launch on expanded rows, X'' the same bits, and the
    block unchanged.  In place (Xout == res) is not a form of this layout."""
    L, ns, nseq = 49, 33, 6
    _, dev = E.params("random")
    M, O, compact, expanded = _rows(L, ns, nseq, 0, 7)
    ldo, wid = (1536, 3 * D) if tail else (D, D)
    Ob = _padded(O, D)
    Xr = torch.full((M + 1, D), SENT, device=DEV, dtype=BF)
    outr = torch.full((M + 1, ldo), SENT, device=DEV, dtype=BF)
    _launch(lib, dev, M, Ob, _padded(expanded, D), D, 0, 0, tail, Xr, D, outr, ldo)
    # no Xout
    out = torch.full((M + 1, ldo), SENT, device=DEV, dtype=BF)
    _launch(lib, dev, M, Ob, _padded(compact, D), D, L, ns, tail, None, 0, out, ldo)
    _same(out, outr, "no Xout: the rows behind X'' differ")
    # Xout = rows [0, M) of one allocation, the compact block = the rows behind them
    nc = compact.shape[0]
    both = torch.full((M + nc + 1, D), SENT, device=DEV, dtype=BF)
    both[M:M + nc] = compact
    out = torch.full((M + 1, ldo), SENT, device=DEV, dtype=BF)
    _launch(lib, dev, M, Ob, both[M:], D, L, ns, tail, both, D, out, ldo)
    _same(both[:M], Xr[:M], "X'' in front of the block differs")
    _same(both[M:M + nc], compact, "the compact block was written")
    assert bool((both[M + nc] == SENT).all())
    _same(out, outr, "Xout in front of the block: the rows behind X'' differ")
    # in place, or any overlap of X'' with the block, is refused before anything is launched; the same arguments with X'' directly in
    # front of the block (the control: nothing else about them is at fault) or in a buffer of its own are accepted
    a = E.BArgs()
    a.O, a.ldo, a.M = Ob.data_ptr(), D, M
    a.res, a.ldr, a.res_L, a.res_nshared = both.data_ptr(), D, L, ns
    a.Wo, a.W1, a.W2, a.stream_buf = dev["Wo"].data_ptr(), dev["W1"].data_ptr(), dev["W2"].data_ptr(), E.stream_buf(lib)["b"].data_ptr()
    a.bo, a.b1, a.b2 = dev["bo"].data_ptr(), dev["b1"].data_ptr(), dev["b2"].data_ptr()
    a.ln2_g, a.ln2_b, a.lnA_g, a.lnA_b = dev["g2"].data_ptr(), dev["be2"].data_ptr(), dev["gA"].data_ptr(), dev["bA"].data_ptr()
    a.x_bf16, a.ldx, a.Hout, a.ldh = 1, D, out.data_ptr(), ldo
    row = D * 2  # bytes
    blk = both.data_ptr() + M * row
    for res, xout, ok in ((both.data_ptr(), both.data_ptr(), False),  # in place
                          (blk, both.data_ptr(), True),               # X'' ends where the block begins
                          (blk, both.data_ptr() + row, False),        # its last row on the block's first
                          (blk, blk + (nc - 1) * row, False),         # its first row on the block's last
                          (both.data_ptr(), both.data_ptr() + nc * row, True),  # X'' begins where the block ends
                          (blk, Xr.data_ptr(), True)):                # a buffer of its own
        a.res, a.Xout = res, xout
        assert (lib.m3pc_debug_block_accepts(C.byref(a)) == 0) == ok, (res - both.data_ptr(), xout - both.data_ptr(), ok, lib.m3pc_last_error())
