"""Every GEMM kernel of the library's dispatch (gemm.hip, gemm_f32_direct.hip, gemm_glds.hip, gemm_big.hip, gemm_line.hip,
gemm_x3.hip) with every epilogue its launcher accepts, element by element against the float64 reference of tests/gemm_ref.py and
its rounding-derived bound, through the lab hook m3pc_debug_gemm_ex.

Each case names its shape, its epilogue and the kernel id, split count, peel row and flags the dispatch must report (the id list
is in include/m3pc_hip_debug.h); test_every_gemm_kernel_id_has_a_case checks that the cases reach exactly the ids of that list, and
tests/test_gemm_ref_cpu.py::test_case_table_names_what_the_dispatch_picks holds the table to the dispatch without a GPU.  Every case
runs in the regimes of gemm_ref.make_inputs: `int` (exact: the kernel must EQUAL the reference), N(0, 1), one k on a k-tile seam
carrying most of every sum, and a large common offset with cancelling weights.  Everything a kernel may not read holds NaN (the
padding columns of A, W, res and the row table, the gap rows of a row-mapped A, the rows behind A, the split-K workspace); the
output buffer holds a sentinel in its padding columns, in the gap rows of a row-mapped C, in guard rows and in one whole guard
block behind it, and is compared bit for bit with its state before the call outside the elements the call owns."""
import ctypes as C
import os
import re

import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -31744.0  # exact in bf16 and fp32; no case comes near it (int regime: |C| <= 9 K + 192)
WS_BYTES = 64 << 20
DIRECT = (5, 6)  # the few-row kernels sum 16 K slices
DEV = "cuda"


class Args(C.Structure):
    """m3pc_debug_gemm_args (include/m3pc_hip_debug.h)."""
    _fields_ = [("dtype", C.c_int), ("A", C.c_void_p), ("lda", C.c_int), ("amap", C.c_int * 3), ("W", C.c_void_p), ("ldw", C.c_int),
                ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("bias", C.c_void_p), ("rowtab", C.c_void_p), ("rt_mod", C.c_int),
                ("rt_ld", C.c_int), ("gelu", C.c_int), ("res", C.c_void_p), ("ldr", C.c_int), ("C", C.c_void_p), ("f32out", C.c_int),
                ("ldc", C.c_int), ("cmap", C.c_int * 3), ("ws", C.c_void_p), ("ws_bytes", C.c_longlong), ("a_padded", C.c_int),
                ("ln_g", C.c_void_p), ("ln_b", C.c_void_p), ("ln_out", C.c_void_p), ("a_ln_g", C.c_void_p), ("a_ln_b", C.c_void_p),
                ("variant", C.c_int), ("stream", C.c_void_p), ("picked", C.POINTER(C.c_int))]


def case(name, dt, M, N, K, epi, expect, f32out=None, T=0, k=1, ws="big", a_padded=0, ln=False, a_ln=False, variant=0, pad=True,
         amap_only=False, regimes=None, rmap=None):
    """epi: letters b bias, g GELU, r residual in a tensor of its own, R residual aliasing C, t row table (rt_mod = T or 8).
    expect: (kernel id, S, peel, flags).  T > 0: the decoder-embed pattern RowMap{T, 4 T, k T} on A and C (amap_only: on A alone) with
    rt_mod = T; rmap: an explicit {rpg, gstride, off} on A and C with rt_mod = rpg instead (the pruned decoder's {kept, Le, offset}).
    ws: "big" (64 MiB), None, or a byte count.  pad False: leading dimensions equal to the row lengths."""
    f32out = (dt != 1) if f32out is None else f32out
    if regimes is None:
        regimes = ("randn", "spike", "offset") if a_ln else R.REGIMES
    return dict(name=name, dt=dt, M=M, N=N, K=K, epi=epi, expect=tuple(expect), f32out=f32out, T=T, k=k, ws=ws, a_padded=a_padded, ln=ln,
                a_ln=a_ln, variant=variant, pad=pad, amap_only=amap_only, regimes=regimes, rmap=rmap)


F, B, X = 0, 1, 2
CASES = [
    # ---- gemm_kernel<float, 64, 64> (id 1), no workspace: M around one and two 64-row tiles, N = 64 / 192 / 128, one, two, three and
    #      five k-tiles (the prologue's nloc > 1 / nloc > 2 branches, an odd count in the two-step loop), every epilogue of launch_t
    case("f32_m1_k32", F, 1, 64, 32, "b", (1, 1, 0, 0), ws=None),
    case("f32_m63_k64_gelu", F, 63, 192, 64, "bg", (1, 1, 0, 0), ws=None),
    case("f32_m64_k96_res", F, 64, 128, 96, "br", (1, 1, 0, 0), ws=None),
    case("f32_m65_k512_tab", F, 65, 64, 512, "bt", (1, 1, 0, 0), ws=None),
    case("f32_m127_alias", F, 127, 192, 96, "R", (1, 1, 0, 0), ws=None),
    case("f32_m128_nopad", F, 128, 128, 64, "", (1, 1, 0, 0), ws=None, pad=False),
    case("f32_m129_k160", F, 129, 128, 160, "b", (1, 1, 0, 0), ws=None),
    case("f32_embed_T8", F, 40, 512, 512, "t", (1, 1, 0, 0), ws=None, T=8, k=2),
    case("f32_embed_T32_var2", F, 96, 512, 512, "t", (1, 4, 0, 0), T=32, k=3, variant=2),  # (split-K + reduce with both row maps)
    # ---- gemm_kernel<float, 128, 128> (id 2): N % 128 == 0 and >= 512 tiles of 128 x 128
    case("f32_128_m8065", F, 8065, 1024, 64, "bg", (2, 1, 0, 0), ws=None),
    case("f32_128_m8191_res", F, 8191, 1024, 96, "br", (2, 1, 0, 0), ws=None),
    case("f32_128_m8192_tab", F, 8192, 1024, 32, "bt", (2, 1, 0, 0)),  # (a workspace, and still no split: >= 768 tiles)
    case("f32_128_plain", F, 8193, 1024, 160, "b", (2, 1, 0, 0), ws=None),
    case("f32_128_embed_T32", F, 16384, 512, 512, "t", (2, 1, 0, 0), T=32, k=3),  # (dec_embed of an fp32 candidate pass)
    case("f32_128_embed_T8", F, 16392, 512, 64, "t", (2, 1, 0, 0), ws=None, T=8, k=2),
    # ---- split-K (id 1, S > 1) and its reduce kernels
    case("f32_split16", F, 65, 128, 2048, "b", (1, 16, 0, 0)),
    case("f32_split16_gelu", F, 40, 192, 2048, "bg", (1, 16, 0, 0)),
    case("f32_split_nkt4", F, 33, 64, 512, "br", (1, 4, 0, 0), variant=2),  # S capped by nkt / 4
    case("f32_split_smallws", F, 65, 128, 2048, "bR", (1, 5, 0, 0), ws=5 * 65 * 128 * 4 + 64),  # S cut by ws_bytes
    case("f32_nosplit_200tiles", F, 1600, 512, 512, "b", (1, 1, 0, 0)),  # S = 1: 200 tiles at K = 512
    case("f32_split_ln256", F, 33, 256, 2048, "bR", (1, 16, 0, 2), ln=True),
    case("f32_split_ln512", F, 65, 512, 2048, "br", (1, 16, 0, 2), ln=True),
    case("f32_split_ln1024", F, 7, 1024, 2048, "bg", (1, 16, 0, 2), ln=True),
    case("f32_split_ln2048_unfused", F, 33, 2048, 2048, "b", (1, 16, 0, 0), ln=True),
    case("f32_split_ln_cmap_unfused", F, 64, 512, 2048, "t", (1, 16, 0, 0), ln=True, T=32, k=1),
    # ---- gemm_f32_direct_kernel (id 5): a workspace, M <= 1024, K = 512, fewer than 200 tiles of 64 x 64; N = 32 (mod 64) allowed
    case("dir_m1", F, 1, 64, 512, "b", (5, 1, 0, 0)),
    case("dir_m33_n96_gelu", F, 33, 96, 512, "bg", (5, 1, 0, 0)),
    case("dir_m1024_alias", F, 1024, 512, 512, "bR", (5, 1, 0, 0)),
    case("dir_m95_res", F, 95, 1536, 512, "br", (5, 1, 0, 0)),
    case("dir_embed_T8", F, 40, 512, 512, "t", (5, 1, 0, 0), T=8, k=1),
    case("dir_embed_T32", F, 96, 512, 512, "t", (5, 1, 0, 0), T=32, k=3),
    case("dir_a_ln", F, 50, 512, 512, "b", (5, 1, 0, 0), a_ln=True),
    case("dir_a_ln_m1", F, 1, 1536, 512, "b", (5, 1, 0, 0), a_ln=True),
    # ---- gemm_kernel<bf16, 64, 64> (id 3): few rows, or N not a multiple of 128; k-tiles of 64
    case("bf_m1_k64", B, 1, 64, 64, "b", (3, 1, 0, 0)),
    case("bf_m63_k128_f32", B, 63, 192, 128, "b", (3, 1, 0, 0), f32out=True),
    case("bf_m64_k192_gelu", B, 64, 128, 192, "bg", (3, 1, 0, 0)),
    case("bf_m65_gelu_f32", B, 65, 1536, 512, "bg", (3, 1, 0, 0), f32out=True),
    case("bf_m127_res", B, 127, 192, 2048, "br", (3, 1, 0, 0)),
    case("bf_m129_alias_f32", B, 129, 512, 2048, "bR", (3, 1, 0, 0), f32out=True),
    case("bf_m128_tab", B, 128, 64, 320, "bt", (3, 1, 0, 0)),
    case("bf_embed_T8", B, 40, 512, 512, "t", (3, 1, 0, 0), f32out=True, T=8, k=0),
    case("bf_embed_T32", B, 96, 512, 512, "t", (3, 1, 0, 0), f32out=True, T=32, k=2),
    case("bf_n192_manyrows", B, 20001, 192, 64, "b", (3, 1, 0, 0)),
    # ---- gemm_kernel<bf16, 128, 128> (id 4): many rows with an epilogue the LDS-DMA kernels do not instantiate
    case("bf_128_res_bf16out", B, 8065, 1024, 64, "br", (4, 1, 0, 0)),
    case("bf_128_tab_bf16out", B, 8192, 1024, 128, "bt", (4, 1, 0, 0)),
    # ---- gemm_glds_ring3_kernel (id 7): many rows; K < 192, a residual, a row table or K >= 1024 below gemm_big's row count
    case("ring_k64", B, 8192, 1024, 64, "b", (7, 1, 0, 0)),
    case("ring_k128_m1_f32", B, 8193, 1024, 128, "b", (7, 1, 0, 0), f32out=True),
    case("ring_k192_m127_gelu", B, 8319, 1024, 192, "bg", (7, 1, 0, 0), variant=26),
    case("ring_peel_res", B, 24876, 512, 128, "br", (7, 1, 24576, 0), f32out=True),
    case("ring_peel_forced_off", B, 24876, 512, 128, "bR", (7, 1, 0, 0), f32out=True, variant=26),
    case("ring_k512_alias", B, 16385, 512, 512, "bR", (7, 1, 0, 0), f32out=True),
    case("ring_k1024_gelu_f32", B, 8200, 1024, 1024, "bg", (7, 1, 0, 0), f32out=True),
    case("ring_k2048", B, 16511, 512, 2048, "b", (7, 1, 0, 0)),
    case("ring_embed_T32", B, 16384, 512, 512, "t", (7, 1, 0, 0), f32out=True, T=32, k=1),
    case("ring_embed_T8", B, 16392, 512, 512, "t", (7, 1, 0, 0), f32out=True, T=8, k=3),
    # ---- gemm_glds_kernel through launch_tile<128, 128, 2, 2, 64> (id 8, variant 2)
    case("tile_m1_gelu_f32", B, 8193, 1024, 64, "bg", (8, 1, 0, 0), f32out=True, variant=2),
    case("tile_m127_res", B, 8319, 1024, 192, "br", (8, 1, 0, 0), f32out=True, variant=2),
    case("tile_tab", B, 8192, 1024, 128, "bt", (8, 1, 0, 0), f32out=True, variant=2),
    case("tile_bf16out", B, 8192, 1024, 512, "b", (8, 1, 0, 0), variant=2),
    case("tile_f32", B, 8255, 1024, 64, "b", (8, 1, 0, 0), f32out=True, variant=2),
    case("tile_gelu_bf16out", B, 8193, 1024, 128, "bg", (8, 1, 0, 0), variant=2),
    case("tile_embed_T32", B, 16384, 512, 512, "t", (8, 1, 0, 0), f32out=True, T=32, k=0, variant=2),
    case("tile_embed_T8", B, 16392, 512, 128, "t", (8, 1, 0, 0), f32out=True, T=8, k=1, variant=2),
    # ---- gemm_big_kernel (id 9): K >= 1024, N % 256 == 0, >= 224 tiles of 256 x 256
    case("big_k1024_ragged_alias", B, 28749, 512, 1024, "bR", (9, 1, 0, 0), f32out=True),
    case("big_k2048", B, 28672, 512, 2048, "b", (9, 1, 0, 0)),
    case("big_gelu_m1", B, 28673, 512, 1024, "bg", (9, 1, 0, 0)),
    case("big_gelu_f32_m255", B, 28927, 512, 1024, "bg", (9, 1, 0, 0), f32out=True),
    case("big_f32_res", B, 28700, 512, 1024, "br", (9, 1, 0, 0), f32out=True, variant=37),
    case("big_f32_plain", B, 28801, 512, 1024, "b", (9, 1, 0, 0), f32out=True),
    # ---- gemm_line_kernel<128> (id 10): 192 <= K < 1024, no residual, >= 256 tiles; flag 1: the persistent form
    case("line_k192", B, 8192, 512, 192, "b", (10, 1, 0, 1)),
    case("line_persistent_gelu", B, 16384, 1024, 512, "bg", (10, 1, 0, 1)),
    case("line_ragged_clamped", B, 16424, 1024, 512, "b", (10, 1, 0, 0), f32out=True),
    case("line_ragged_padded", B, 16424, 1024, 512, "bg", (10, 1, 0, 1), f32out=True, a_padded=1),
    case("line_m1_padded", B, 16385, 512, 256, "b", (10, 1, 0, 1), a_padded=1),
    case("line_m127_clamped", B, 16511, 512, 960, "bg", (10, 1, 0, 0)),
    case("line_rowmapped_A", B, 16384, 512, 512, "b", (10, 1, 0, 0), f32out=True, T=32, k=2, amap_only=True),
    case("line_res_forced", B, 8192, 512, 256, "br", (10, 1, 0, 1), f32out=True, variant=43),
    case("line_res_ragged_forced", B, 8200, 512, 256, "bR", (10, 1, 0, 0), f32out=True, variant=43),
    # ---- gemm_line_kernel<256> (id 11, variant 44)
    case("line256", B, 8192, 512, 192, "b", (11, 1, 0, 1), variant=44),
    case("line256_ragged_padded", B, 8321, 512, 512, "bg", (11, 1, 0, 1), f32out=True, variant=44, a_padded=1),
    case("line256_res_clamped", B, 8447, 256, 512, "br", (11, 1, 0, 0), f32out=True, variant=44),
    case("line256_f32", B, 8193, 512, 256, "b", (11, 1, 0, 0), f32out=True, variant=44),
    case("line256_gelu_bf16out", B, 8448, 256, 512, "bg", (11, 1, 0, 1), variant=44),
    # ---- gemm_x3_kernel<64, 64> (id 12): k-tiles of 32
    case("x3_m1_k32", X, 1, 64, 32, "b", (12, 1, 0, 0), ws=None),
    case("x3_m63_k64_gelu", X, 63, 192, 64, "bg", (12, 1, 0, 0), ws=None),
    case("x3_m65_k96_res", X, 65, 128, 96, "br", (12, 1, 0, 0), ws=None),
    case("x3_m129_tab", X, 129, 64, 512, "bt", (12, 1, 0, 0), ws=None),
    case("x3_m127_bf16out", X, 127, 192, 160, "b", (12, 1, 0, 0), ws=None, f32out=False),
    case("x3_gelu_bf16out", X, 64, 128, 512, "bg", (12, 1, 0, 0), ws=None, f32out=False),
    case("x3_embed_T8", X, 40, 512, 512, "t", (12, 1, 0, 0), ws=None, T=8, k=1),
    case("x3_embed_T32", X, 96, 512, 512, "t", (12, 4, 0, 0), T=32, k=2),
    case("x3_split16", X, 65, 128, 2048, "bR", (12, 16, 0, 0)),
    case("x3_split_nkt4", X, 33, 64, 512, "bg", (12, 4, 0, 0)),
    case("x3_split_smallws", X, 65, 128, 2048, "b", (12, 5, 0, 0), ws=5 * 65 * 128 * 4 + 64),
    case("x3_nosplit_200tiles", X, 1600, 512, 512, "br", (12, 1, 0, 0)),
    case("x3_split_ln512", X, 33, 512, 2048, "bR", (12, 16, 0, 2), ln=True),
    # ---- gemm_x3_kernel<128, 128> (id 13)
    case("x3_128_m8065", X, 8065, 1024, 64, "b", (13, 1, 0, 0)),
    case("x3_128_m8191_gelu", X, 8191, 1024, 96, "bg", (13, 1, 0, 0), ws=None),
    case("x3_128_alias", X, 8192, 1024, 32, "bR", (13, 1, 0, 0), ws=None),
    case("x3_128_bf16out", X, 8193, 1024, 64, "b", (13, 1, 0, 0), ws=None, f32out=False),
    case("x3_128_gelu_bf16out", X, 8319, 1024, 96, "bg", (13, 1, 0, 0), f32out=False),
    case("x3_128_tab", X, 8192, 1024, 160, "bt", (13, 1, 0, 0), ws=None),
    case("x3_128_embed_T32", X, 16384, 512, 512, "t", (13, 1, 0, 0), T=32, k=1),  # (dec_embed of an x3 candidate pass)
    case("x3_128_embed_T8", X, 16392, 512, 64, "t", (13, 1, 0, 0), ws=None, T=8, k=3),
]
# gemm_f32_direct_group_kernel (id 6, flags 4), problems (row map on A and C, rows) of one launch; rt_mod = rpg.  The four
# decoder-embedding GEMMs of run_decoder_full, RowMap{T, 4 T, k T}; and the pruned decoder's two or three kept keys, RowMap{kept, Le,
# offset} with n kept rows (the launcher pads the unused problems of the kernel's argument).  The problems differ in their row
# counts: a workgroup past a problem's own tiles returns early
GROUPS = [("group_T8", [((8, 32, 8 * k), 8 * b) for k, b in enumerate((5, 3, 5, 1))]),
          ("group_T32", [((32, 128, 32 * k), 32 * b) for k, b in enumerate((3, 3, 2, 3))]),
          ("group_kept3", [((4, 11, 0), 4 * 7), ((1, 11, 4), 1 * 7), ((6, 11, 5), 6 * 7)]),
          ("group_kept2", [((17, 49, 0), 17 * 16), ((32, 49, 17), 32 * 16)])]
WORST = {}  # (kernel id, regime) -> largest err / bound
EXACT = [0]  # int-regime runs that matched exactly


def header_ids():
    """The GEMM kernel ids the header's list names."""
    src = open(os.path.join(ROOT, "include", "m3pc_hip_debug.h")).read()
    block = src[src.index("GEMM kernel ids"):src.index("not listed, not reachable")]
    ids = set()
    for line in block.splitlines()[1:]:
        line = re.sub(r"^\s*\*\s*", "", line)
        line = re.sub(r"\(S > 1.*", "", line)
        line = re.sub(r"<[^>]*>", "", line)
        line = re.sub(r"^\w+\.hip:", "", line)
        ids |= {int(x) for x in re.findall(r"(?:^|;)\s*(\d+) ", line)}
    return ids


def lab():
    from hip_util import lab_library
    lib = lab_library()
    for fn in (lib.m3pc_debug_gemm_ex, lib.m3pc_debug_gemm_plan):
        fn.restype = C.c_int
        fn.argtypes = [C.POINTER(Args)]
    lib.m3pc_debug_gemm_group.restype = C.c_int
    lib.m3pc_debug_gemm_group.argtypes = [C.POINTER(Args), C.c_int]
    return lib


def layout(c):
    """Leading dimensions and row maps of a case."""
    dt, M, N, K, T = c["dt"], c["M"], c["N"], c["K"], c["T"]
    p = c["pad"]
    L = dict(lda=K + (8 if p else 0), ldw=K + (16 if p else 0), ldc=N + (8 if p else 0), ldr=N + (4 if p else 0), rt_ld=N + (4 if p else 0),
             rt_mod=(T or 8) if "t" in c["epi"] else 0, amap=None, cmap=None)
    if T:
        L["amap"] = (T, 4 * T, c["k"] * T)
        L["cmap"] = None if c["amap_only"] else L["amap"]
    if c.get("rmap"):
        L["amap"] = L["cmap"] = tuple(c["rmap"])
        L["rt_mod"] = c["rmap"][0] if "t" in c["epi"] else 0
    if "R" in c["epi"]:
        L["ldr"] = L["ldc"]
    rows = lambda m: M if m is None else ((M + m[0] - 1) // m[0]) * m[1] + m[2] + m[0]  # (what the kernels' buffer ranges assume)
    L["rows_a"], L["rows_c"] = rows(L["amap"]), rows(L["cmap"])
    return L


def fill_args(c, L, ptr, picked=None):
    """The hook's argument structure; ptr maps a buffer name to its address (the plan-only entry never follows them)."""
    a = Args()
    a.dtype, a.A, a.lda, a.W, a.ldw, a.M, a.N, a.K = c["dt"], ptr("A"), L["lda"], ptr("W"), L["ldw"], c["M"], c["N"], c["K"]
    a.amap = (C.c_int * 3)(*(L["amap"] or (0, 0, 0)))
    a.cmap = (C.c_int * 3)(*(L["cmap"] or (0, 0, 0)))
    a.bias = ptr("bias") if "b" in c["epi"] else None
    if L["rt_mod"]:
        a.rowtab, a.rt_mod, a.rt_ld = ptr("rowtab"), L["rt_mod"], L["rt_ld"]
    a.gelu = int("g" in c["epi"])
    if "r" in c["epi"]:
        a.res = ptr("res")
    elif "R" in c["epi"]:
        a.res = ptr("C")
    a.ldr, a.C, a.f32out, a.ldc = L["ldr"], ptr("C"), int(c["f32out"]), L["ldc"]
    if c["ws"] is not None:
        a.ws, a.ws_bytes = ptr("ws"), WS_BYTES if c["ws"] == "big" else c["ws"]
    a.a_padded = c["a_padded"]
    if c["ln"]:
        a.ln_g, a.ln_b, a.ln_out = ptr("ln_g"), ptr("ln_b"), ptr("ln_out")
    if c["a_ln"]:
        a.a_ln_g, a.a_ln_b = ptr("a_ln_g"), ptr("a_ln_b")
    a.variant = c["variant"]
    if picked is not None:
        a.picked = C.cast(picked, C.POINTER(C.c_int))
    return a


def plan_of(lib, c):
    """What the dispatch would launch for a case, from the plan-only entry (no GPU): (rc, picked)."""
    picked = (C.c_int * 4)()
    a = fill_args(c, layout(c), lambda name: 0x10000000, picked)
    rc = lib.m3pc_debug_gemm_plan(C.byref(a))
    return rc, tuple(picked)


def _nan(rows, ld, et):
    return torch.full((rows, ld), float("nan"), device=DEV, dtype=et)


_WS = {}


def build(c, regime, seed, spike_k=None):
    """Logical tensors and poisoned device buffers of one run."""
    dt, M, N, K = c["dt"], c["M"], c["N"], c["K"]
    L = layout(c)
    et = torch.bfloat16 if dt == 1 else torch.float32
    ot = torch.float32 if c["f32out"] else torch.bfloat16
    t = R.make_inputs(regime, M, N, K, dtype=dt, bias="b" in c["epi"], rt_mod=L["rt_mod"], res=c["epi"].count("r") + c["epi"].count("R") > 0,
                      spike_k=spike_k, device=DEV, seed=seed)
    if not c["f32out"] and t["res"] is not None and "R" in c["epi"]:
        t["res"] = t["res"].to(ot).float()  # (a residual that lives in a bf16 C)
    arow, crow = R.map_rows(L["amap"], M, DEV), R.map_rows(L["cmap"], M, DEV)
    bufs = {}
    bufs["A"] = _nan(L["rows_a"] + (127 if c["a_padded"] else 0) + 2, L["lda"], et)  # (gap rows, the rows behind A, the padding: NaN)
    bufs["A"][arow, :K] = t["A"].to(et)
    bufs["W"] = _nan(N + 2, L["ldw"], et)
    bufs["W"][:N, :K] = t["W"].to(et)
    if t["bias"] is not None:
        bufs["bias"] = t["bias"].clone()
    if L["rt_mod"]:
        bufs["rowtab"] = _nan(L["rt_mod"] + 1, L["rt_ld"], torch.float32)
        bufs["rowtab"][:L["rt_mod"], :N] = t["rowtab"]
    rc = L["rows_c"]
    bufs["C"] = torch.full((2 * rc + 4, L["ldc"]), SENT, device=DEV, dtype=ot)  # (guard rows and one whole guard block behind)
    if "r" in c["epi"]:
        bufs["res"] = _nan(rc + 2, L["ldr"], torch.float32)
        bufs["res"][crow, :N] = t["res"]
    elif "R" in c["epi"]:
        bufs["C"][crow, :N] = t["res"].to(ot)
    if c["ws"] is not None:
        if "ws" not in _WS:
            _WS["ws"] = torch.empty(WS_BYTES // 4, device=DEV)
        _WS["ws"].fill_(float("nan"))
        bufs["ws"] = _WS["ws"]
    g = torch.Generator(device=DEV).manual_seed(seed + 77)
    for key, d, on in (("ln", N, c["ln"]), ("a_ln", K, c["a_ln"])):
        if on:
            bufs[key + "_g"] = 1 + 0.1 * torch.randn(d, device=DEV, generator=g)
            bufs[key + "_b"] = 0.1 * torch.randn(d, device=DEV, generator=g)
    if c["ln"]:
        bufs["ln_out"] = torch.full((M + 4, N), SENT, device=DEV)
    return t, L, bufs, arow, crow


def check(c, regime, t, L, bufs, before, crow, picked, chunk_elems=1 << 25):
    """Every element of every row against the float64 reference (on the GPU, chunked over rows); returns the largest err / bound."""
    name, dt, M, N, K = c["name"], c["dt"], c["M"], c["N"], c["K"]
    Cb = bufs["C"]
    got_all = Cb[crow, :N]
    assert torch.isfinite(got_all).all(), f"{name}/{regime}: non-finite output (a poisoned element was read)"
    if "R" not in c["epi"]:
        assert not (got_all == SENT).any(), f"{name}/{regime}: an output element was not written"
    after = Cb.clone()
    after[crow, :N] = before[crow, :N]
    assert torch.equal(after.view(torch.int32 if c["f32out"] else torch.int16), before.view(torch.int32 if c["f32out"] else torch.int16)), \
        f"{name}/{regime}: a guard (padding column, gap row, guard row or the block behind C) was written"
    del after
    S_split = 16 if picked[0] in DIRECT else picked[1]
    a_ln = (bufs["a_ln_g"], bufs["a_ln_b"]) if c["a_ln"] else None
    exact = regime == "int" and "g" not in c["epi"] and not c["a_ln"]
    worst = 0.0
    step = max(64, chunk_elems // max(K, N))
    for r0 in range(0, M, step):
        r1 = min(M, r0 + step)
        ref = R.gemm_ref(t["A"][r0:r1], t["W"], bias=t["bias"], rowtab=t["rowtab"], rt_mod=max(L["rt_mod"], 1), gelu="g" in c["epi"],
                         res=None if t["res"] is None else t["res"][r0:r1], a_ln=a_ln, row0=r0)
        got = got_all[r0:r1].double()
        if exact:
            want = ref["C"] if c["f32out"] else ref["C"].float().to(torch.bfloat16).double()
            bad = got != want
            assert not bad.any(), (f"{name}/int: {int(bad.sum())} elements differ from the exact result, first at row "
                                   f"{r0 + int(bad.any(1).nonzero()[0])}, max |diff| {float((got - want).abs().max())}")
        else:
            bnd = R.bound(ref, dt, K, S_split, c["f32out"])
            err = (got - ref["C"]).abs()
            ratio = float((err / bnd).max())
            if ratio > 1:
                i = int((err / bnd).flatten().argmax())
                raise AssertionError(f"{name}/{regime}: err / bound {ratio:.3g} at row {r0 + i // N} column {i % N} (err "
                                     f"{float(err.flatten()[i]):.3g}, bound {float(bnd.flatten()[i]):.3g})")
            worst = max(worst, ratio)
    if c["ln"]:
        y = bufs["ln_out"]
        if picked[3] & 2:  # against the float64 LayerNorm of the kernel's own fp32 C: the bound is the LayerNorm's own rounding
            assert torch.isfinite(y[:M]).all() and not (y[:M] == SENT).any(), f"{name}/{regime}: ln_out"
            Cown = got_all.double()
            ln = R.layernorm64(Cown, bufs["ln_g"], bufs["ln_b"])
            r = float(((y[:M].double() - ln).abs() / R.ln_bound(Cown, bufs["ln_g"], bufs["ln_b"])).max())
            assert r <= 1, f"{name}/{regime}: fused LayerNorm err / bound {r:.3g}"
            assert (y[M:] == SENT).all(), f"{name}/{regime}: a guard row of ln_out was written"
        else:
            assert (y == SENT).all(), f"{name}/{regime}: ln_out written although the launch reports no fused LayerNorm"
    return worst, exact


@pytest.fixture(scope="module")
def lib():
    return lab()


def _spike_k(c, ri):
    seams = [k for k in (15, 16, 31, 32, 63, 64, 127, 128) if k < c["K"]] + [c["K"] - 1]
    return seams[(ri + len(c["name"])) % len(seams)]


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_gemm_kernel_against_float64(lib, ci):
    c = CASES[ci]
    rc, planned = plan_of(lib, c)
    assert rc == 0, lib.m3pc_last_error()
    assert planned == c["expect"], f"{c['name']}: the dispatch would launch {planned}, the case is for {c['expect']}"
    for ri, regime in enumerate(c["regimes"]):
        sk = _spike_k(c, ci)
        t, L, bufs, arow, crow = build(c, regime, 1000 * ci + ri, spike_k=sk)
        before = bufs["C"].clone()
        picked = (C.c_int * 4)()
        a = fill_args(c, L, lambda n: bufs[n].data_ptr(), picked)
        a.stream = torch.cuda.current_stream().cuda_stream
        rc = lib.m3pc_debug_gemm_ex(C.byref(a))
        assert rc == 0, lib.m3pc_last_error()
        torch.cuda.synchronize()
        assert tuple(picked) == c["expect"], f"{c['name']}: dispatch reports {tuple(picked)}, the case is for {c['expect']}"
        worst, exact = check(c, regime, t, L, bufs, before, crow, tuple(picked))
        EXACT[0] += int(exact)
        WORST[(picked[0], regime)] = max(WORST.get((picked[0], regime), 0.0), worst)
        print(f"{c['name']:28s} {regime:6s} kernel {picked[0]:2d} S {picked[1]:2d} peel {picked[2]:5d} flags {picked[3]}  "
              + ("exact" if exact else f"max err/bound {worst:.3g}") + (f"  (spike at k = {sk})" if regime == "spike" else ""))
        del t, bufs, before


@pytest.mark.parametrize("name,problems", GROUPS, ids=[g[0] for g in GROUPS])
def test_grouped_decoder_embedding(lib, name, problems):
    """Two to four row-mapped, row-tabled fp32 problems in one launch of gemm_f32_direct_group_kernel, each checked as a case of its own."""
    n = len(problems)
    for ri, regime in enumerate(R.REGIMES):
        cs = [case(f"{name}_{k}", F, M, 512, 512, "t", (6, 1, 0, 4), rmap=m) for k, (m, M) in enumerate(problems)]
        built = [build(c, regime, 5000 + 10 * ri + k, spike_k=(31, 32, 255, 511)[k]) for k, c in enumerate(cs)]
        befores = [b[2]["C"].clone() for b in built]
        picked = (C.c_int * 4)()
        arr = (Args * n)()
        for k, (c, b) in enumerate(zip(cs, built)):
            arr[k] = fill_args(c, b[1], lambda n, b=b: b[2][n].data_ptr(), picked)
            arr[k].stream = torch.cuda.current_stream().cuda_stream
        assert lib.m3pc_debug_gemm_group(arr, n) == 0, lib.m3pc_last_error()
        torch.cuda.synchronize()
        assert tuple(picked) == (6, 1, 0, 4), tuple(picked)
        for c, (t, L, bufs, arow, crow), before in zip(cs, built, befores):
            worst, exact = check(c, regime, t, L, bufs, before, crow, tuple(picked))
            EXACT[0] += int(exact)
            WORST[(6, regime)] = max(WORST.get((6, regime), 0.0), worst)
        print(f"{name:28s} {regime:6s} kernel  6 flags 4  " + ("exact" if regime == "int" else f"max err/bound {WORST[(6, regime)]:.3g}"))


# (dtype, N, K, epilogue, fp32 output, full row count): many-row problems whose prefixes a shard split produces
PREFIX = [(B, 512, 512, "b", False, 40000), (B, 2048, 512, "bg", False, 20000), (B, 512, 1024, "bR", True, 30000),
          (B, 512, 2048, "br", True, 30011), (X, 512, 512, "b", True, 20077), (X, 2048, 512, "bg", True, 20077), (F, 1024, 64, "br", True, 8192)]


@pytest.mark.parametrize("dt,N,K,epi,f32out,M", PREFIX, ids=[f"dt{p[0]}_N{p[1]}_K{p[2]}_{p[3]}" for p in PREFIX])
def test_a_row_does_not_depend_on_the_row_count(lib, dt, N, K, epi, f32out, M):
    """The first M' rows of a many-row problem, run alone through the default dispatch (no workspace: no split-K), have the bits they
    have in the full run, whatever kernel either run picks: what tests/test_hip_parity.py::test_sharding_is_exact rests on."""
    full = case("full", dt, M, N, K, epi, (0, 0, 0, 0), f32out=f32out, ws=None, pad=False)
    t, L, bufs, arow, crow = build(full, "randn", 31 * N + K)
    outs = {}
    for Mp in (M, 305, 4096, M // 2):
        c = dict(full, M=Mp)
        Cb = torch.full((Mp + 2, L["ldc"]), SENT, device=DEV, dtype=bufs["C"].dtype)
        if "R" in epi:
            Cb[:Mp, :N] = t["res"][:Mp].to(Cb.dtype)
        b2 = dict(bufs, C=Cb)
        picked = (C.c_int * 4)()
        a = fill_args(c, layout(c), lambda n: b2[n].data_ptr(), picked)
        a.stream = torch.cuda.current_stream().cuda_stream
        assert lib.m3pc_debug_gemm_ex(C.byref(a)) == 0, lib.m3pc_last_error()
        torch.cuda.synchronize()
        outs[Mp] = (Cb, tuple(picked))
        assert (Cb[Mp:] == SENT).all()
    view = torch.int32 if f32out else torch.int16
    print(f"dtype {dt} N {N} K {K} {epi}: " + "  ".join(f"M' {m}: kernel {p[0]}" for m, (_, p) in outs.items()))
    for Mp in (305, 4096, M // 2):
        same = torch.equal(outs[Mp][0][:Mp, :N].contiguous().view(view), outs[M][0][:Mp, :N].contiguous().view(view))
        assert same, f"rows [0, {Mp}) differ between M = {Mp} (kernel {outs[Mp][1][0]}) and M = {M} (kernel {outs[M][1][0]})"


def refusal_cases():
    """(what, case, edits of the argument structure): calls the hook must refuse."""
    ok = case("ok", F, 65, 128, 64, "b", (1, 1, 0, 0), ws=None)
    okb = case("okb", B, 8192, 1024, 64, "b", (7, 1, 0, 0))
    return [
        ("N not a multiple of 64", dict(ok, N=96), {}),
        ("K not a whole k-tile (fp32)", dict(ok, K=48), {}),
        ("K not a whole k-tile (bf16)", dict(okb, K=96), {}),
        ("misaligned A", ok, {"A": 4}),
        ("lda rows off 16 bytes", ok, {"lda": 66}),
        ("ldc below N", ok, {"ldc": 64}),
        ("rowtab with rt_mod 0", dict(ok, epi="bt"), {"rt_mod": 0}),
        ("row map with gstride < rpg", dict(ok, T=8), {"cmap": (8, 4, 0)}),
        ("GELU and residual together", dict(ok, epi="bgr"), {}),
        ("ln_out with bf16 C", dict(okb, ln=True), {}),
        ("a_ln on a problem the few-row kernel rejects", dict(ok, K=1024, ws="big", a_ln=True), {}),
        ("a_ln without a workspace", dict(ok, K=512, a_ln=True), {}),
        ("forced line kernel with a row table", dict(okb, K=512, epi="bt", f32out=True, variant=43), {}),
        ("forced gemm_big below K = 1024", dict(okb, variant=37), {}),
        ("a variant of the experimental tilings", dict(okb, variant=9), {}),
    ]


def edit_args(a, edit):
    for key, v in edit.items():
        if key == "A":
            a.A = a.A + v
        elif key == "cmap":
            a.cmap = (C.c_int * 3)(*v)
        else:
            setattr(a, key, v)
    return a


@pytest.mark.parametrize("ri", range(15), ids=[r[0].replace(" ", "_") for r in refusal_cases()])
def test_uncovered_shapes_are_refused_before_launch(lib, ri):
    """M3PC_EINVAL with a message, nothing reported as launched, and the poisoned output buffer is untouched."""
    what, c, edit = refusal_cases()[ri]
    t, L, bufs, arow, crow = build(dict(c, a_ln=False, ln=False), "randn", 9)
    for key, d in (("ln", c["N"]), ("a_ln", c["K"])):
        bufs[key + "_g"], bufs[key + "_b"] = torch.ones(d, device=DEV), torch.zeros(d, device=DEV)
    bufs["ln_out"] = torch.full((c["M"], c["N"]), SENT, device=DEV)
    before = bufs["C"].clone()
    picked = (C.c_int * 4)()
    a = edit_args(fill_args(c, L, lambda n: bufs[n].data_ptr(), picked), edit)
    a.stream = torch.cuda.current_stream().cuda_stream
    rc = lib.m3pc_debug_gemm_ex(C.byref(a))
    torch.cuda.synchronize()
    assert rc != 0, f"{what}: accepted"
    assert lib.m3pc_last_error(), what
    assert tuple(picked) == (0, 0, 0, 0)
    assert torch.equal(bufs["C"], before) and (bufs["ln_out"] == SENT).all(), f"{what}: refused, but the output was written"
    print(f"{what}: {lib.m3pc_last_error().decode()}")


def test_every_gemm_kernel_id_has_a_case():
    """The cases name exactly the kernel ids of include/m3pc_hip_debug.h (each case asserts that the dispatch picked its id): a kernel
    added to the dispatch and the list without a case fails here.  Prints the largest err / bound per (kernel, regime) seen."""
    want = header_ids()
    assert want == set(range(1, 14)), sorted(want)
    have = {c["expect"][0] for c in CASES} | {6}
    assert have == want, (sorted(want - have), sorted(have - want))
    if WORST:
        print(f"\nint-regime runs that equal the reference exactly: {EXACT[0]}")
        print("largest err / bound per (kernel, regime):")
        for kid in sorted({k for k, _ in WORST}):
            print(f"  kernel {kid:2d}: " + "  ".join(f"{rg} {WORST[(kid, rg)]:.3g}" for rg in R.REGIMES if (kid, rg) in WORST))
