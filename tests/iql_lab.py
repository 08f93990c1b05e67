"""ctypes mirrors of the m3pc_debug_iql_* argument structures (include/m3pc_hip_debug.h) and the lab library with them bound; shared by
tests/test_iql_kernel_edges_gpu.py and the refusal test of tests/test_iql_kernels_ref_cpu.py."""
import ctypes as C

vp, ci, ll, cf, cd = C.c_void_p, C.c_int, C.c_longlong, C.c_float, C.c_double
pi = C.POINTER(ci)
NET_FIELDS = ("W1", "b1", "W2", "b2", "W3", "b3")


class Net(C.Structure):
    _fields_ = [(n, vp) for n in NET_FIELDS] + [("in_", ci), ("out", ci)]


class IqlArgs(C.Structure):
    _fields_ = [("net", Net * 6), ("am", Net * 4), ("av", Net * 4), ("log_std", vp), ("ls_m", vp), ("ls_v", vp), ("om", vp), ("os", vp),
                ("state", vp), ("action", vp), ("reward", vp), ("next_state", vp), ("done", vp), ("h1", vp), ("h2", vp), ("out", vp), ("d3", vp),
                ("d2", vp), ("d1", vp), ("losses", vp), ("B", ci), ("H", ci), ("S", ci), ("A", ci), ("npass", ci), ("pass_net", ci * 7),
                ("pass_next", ci * 7), ("expectile", cf), ("beta", cf), ("gamma", cf), ("omt", cf), ("tau", cf), ("omb1", cf), ("b2", cf),
                ("omb2", cf), ("step_size", cd * 4), ("sqrt_bc2", cd), ("eps", cd), ("which", ci), ("stream", vp), ("picked", pi)]


class PublishArgs(C.Structure):
    _fields_ = [("q", Net * 2)] + [(n, vp * 2) for n in ("W1T", "b1", "W2T", "b2", "W3", "b3", "W1F", "W2F")] + \
               [("om", vp), ("os", vp), ("c_om", vp), ("c_os", vp), ("S", ci), ("SA", ci), ("H", ci), ("streams", ci), ("stream", vp), ("picked", pi)]


HOOKS = {"m3pc_debug_iql_forward": IqlArgs, "m3pc_debug_iql_loss": IqlArgs, "m3pc_debug_iql_delta": IqlArgs, "m3pc_debug_iql_grad": IqlArgs,
         "m3pc_debug_iql_publish": PublishArgs}


def bind(lib):
    for name, st in HOOKS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ci, [C.POINTER(st)]
    lib.m3pc_debug_iql_eval_out.restype, lib.m3pc_debug_iql_eval_out.argtypes = ci, [vp, ci, ci, ci, ci, vp, vp, pi]
    lib.m3pc_debug_iql_copy.restype, lib.m3pc_debug_iql_copy.argtypes = ci, [vp, vp, ll, vp, pi]
    lib.m3pc_debug_critic_pack.restype, lib.m3pc_debug_critic_pack.argtypes = ci, [vp, vp, ci, ci, vp, vp, C.POINTER(ll), C.POINTER(ll)]
    lib.m3pc_last_error.restype = C.c_char_p
    return lib


def lab():
    from hip_util import lab_library
    return bind(lab_library())
