"""ctypes mirrors of the m3pc_debug_mg_* argument structures (include/m3pc_hip_debug.h) and the lab library with them bound; shared by
tests/test_mtm_grad_kernel_edges_gpu.py and the refusal test of tests/test_mtm_grad_kernels_ref_cpu.py."""
import ctypes as C

vp, ci, ll, u64 = C.c_void_p, C.c_int, C.c_longlong, C.c_ulonglong
pi = C.POINTER(ci)


class Op(C.Structure):
    _fields_ = [("p", vp), ("s_o", ll), ("s_k", ll), ("map", ci * 3), ("map_k", ci), ("len", ll)]


class GemmArgs(C.Structure):
    _fields_ = [("A", Op), ("B", Op), ("C", vp), ("ldc", ll), ("c_len", ll), ("cmap", ci * 3), ("M", ci), ("N", ci), ("K", ci), ("bias", vp),
                ("bias2", vp), ("pos", vp), ("pos_T", ci), ("res", vp), ("gelu_aux", vp), ("gelu_out", vp), ("accumulate", ci), ("splitk", ci),
                ("stream", vp), ("picked", pi)]


class LnArgs(C.Structure):
    _fields_ = [("backward", ci), ("X", vp), ("xmap", ci * 3), ("x_rows", ll), ("g", vp), ("b", vp), ("Y", vp), ("st", vp), ("dY", vp),
                ("dX", vp), ("rows", ci), ("d", ci), ("accumulate", ci), ("stream", vp), ("picked", pi)]


class ColsumArgs(C.Structure):
    _fields_ = [("dY", vp), ("dy_compact", ci), ("ldy", ll), ("X", vp), ("st", vp), ("nseq", ci), ("L", ci), ("j0", ci), ("n", ci), ("sel", u64),
                ("C", ci), ("part", vp), ("part_doubles", ll), ("buf_rows", ll), ("out0", vp), ("out1", vp), ("stream", vp), ("picked", pi)]


class AttnArgs(C.Structure):
    _fields_ = [("which", ci), ("QKV", vp), ("P", vp), ("O", vp), ("dO", vp), ("dQKV", vp), ("B", ci), ("L", ci), ("d", ci), ("nh", ci),
                ("hd", ci), ("scale", C.c_float), ("stream", vp), ("picked", pi)]


class TokensArgs(C.Structure):
    _fields_ = [("which", ci), ("tok", vp * 4), ("W", vp * 4), ("bias", vp * 4), ("pdim", vp * 4), ("pos", vp), ("mtok", vp * 4),
                ("bits", u64 * 4), ("kept", ci * 4), ("eoff", ci * 4), ("feat", ci * 4), ("B", ci), ("T", ci), ("d", ci), ("Le", ci),
                ("X", vp), ("src", vp), ("dst", vp), ("key", ci), ("out", vp), ("stream", vp), ("picked", pi)]


class LossBwdArgs(C.Structure):
    _fields_ = [("pred", vp * 3), ("mu", vp), ("sd", vp), ("ls", vp), ("tgt", vp * 4), ("eps", vp), ("dpred", vp * 3), ("dmu", vp),
                ("dls", vp), ("mask", u64 * 4), ("batch", ci), ("T", ci), ("S", ci), ("A", ci), ("flags", ci), ("loss_keys", ci),
                ("entropy_reg", C.c_float), ("inv_cnt", C.c_float), ("stream", vp), ("picked", pi)]


HOOKS = {"m3pc_debug_mg_gemm": GemmArgs, "m3pc_debug_mg_layernorm": LnArgs, "m3pc_debug_mg_colsum": ColsumArgs,
         "m3pc_debug_mg_attention": AttnArgs, "m3pc_debug_mg_tokens": TokensArgs, "m3pc_debug_mg_loss_bwd": LossBwdArgs}


def bind(lib):
    for name, st in HOOKS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ci, [C.POINTER(st)]
    lib.m3pc_debug_mg_std.restype, lib.m3pc_debug_mg_std.argtypes = ci, [vp, vp, ll, vp, pi]
    return lib


def lab():
    from hip_util import lab_library
    return bind(lab_library())
