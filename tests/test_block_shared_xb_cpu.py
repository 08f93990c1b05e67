"""The row mapping of the compact bf16 residual block (block_res_row_xb, csrc/kernels.h: the one function both the embedding kernel
and the fused layer tail address it with), through the lab library's host-only entry m3pc_debug_block_res_row -- no GPU.  Token row
r = b res_L + w reads row w of the shared block when w < res_nshared, else own row b (res_L - res_nshared) + w - res_nshared behind
it.  The shapes are those of tests/test_block_shared_xb_gpu.py."""
import ctypes as C

import pytest

from hip_util import lab_library

CASES = [(49, 33, 1), (49, 33, 3), (49, 33, 6), (48, 32, 3), (5, 2, 27), (49, 48, 3), (49, 1, 3), (49, 0, 2), (49, 49, 2)]


@pytest.fixture(scope="module")
def row():
    lib = lab_library()
    lib.m3pc_debug_block_res_row.restype, lib.m3pc_debug_block_res_row.argtypes = C.c_int, [C.c_int] * 3
    return lib.m3pc_debug_block_res_row


@pytest.mark.parametrize("L,ns,nseq", CASES)
def test_mapping(row, L, ns, nseq):
    got = [row(r, L, ns) for r in range(L * nseq)]
    want = [w if w < ns else ns + b * (L - ns) + (w - ns) for b in range(nseq) for w in range(L)]
    assert got == want
    # every own row is named exactly once, the shared rows once per sequence, and the block has no holes
    own = [g for g in got if g >= ns]
    assert sorted(own) == list(range(ns, ns + nseq * (L - ns)))
    assert all(got.count(w) == nseq for w in range(ns))


def test_out_of_range_arguments(row):
    assert row(-1, 49, 33) == -1 and row(0, 0, 0) == -1 and row(0, 5, 6) == -1 and row(0, 5, -1) == -1
