"""The IQL trainer without a GPU: m3pc_iql_* are declared in include/m3pc_hip.h, exported by the library and bound by
m3pc_amd/capi.py; every refusal comes before any HIP call (m3pc_iql_create makes none, so a trainer exists on a machine without a
device); the NumPy restatement the GPU tests compare against (tests/iql_ref.py) reproduces the float64 run of the real reference
ImplicitQLearning captured in tests/golden/g7_iql.npz; the recipes meet the fixture conditions; examples/critic_loop.c compiles."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import iql_ref as R
from m3pc_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m3pc_iql_create", "m3pc_iql_destroy", "m3pc_iql_load", "m3pc_iql_export", "m3pc_iql_set_step", "m3pc_iql_get_step", "m3pc_iql_train_step",
       "m3pc_iql_train", "m3pc_iql_publish_critic", "m3pc_iql_evaluate")
S, A, H = 11, 3, 64


@pytest.fixture(scope="module")
def lib():
    return capi.load_library(build.build_library())


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "g7_iql.npz"))


@pytest.fixture(scope="module")
def runs():
    """The float64 restatement of every case, run once."""
    return {case: R.run(case) for case in R.CASES}


def _header():
    return open(os.path.join(ROOT, "include", "m3pc_hip.h")).read()


def test_every_entry_point_is_declared_exported_and_bound(lib):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/m3pc_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in capi.EXPORTS
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    parts = ("QF", "Q_TARGET", "VF", "ACTOR", "QF_ADAM_M", "QF_ADAM_V", "VF_ADAM_M", "VF_ADAM_V", "ACTOR_ADAM_M", "ACTOR_ADAM_V")
    for j, name in enumerate(parts):
        assert int(re.search(r"#define M3PC_IQL_%s (\d+)" % name, code).group(1)) == j == getattr(capi, "IQL_" + name)
    for j, name in enumerate(("Q_MIN", "Q_TARGET_MIN", "V", "ACTOR_MEAN")):
        assert int(re.search(r"#define M3PC_IQL_%s (\d+)" % name, code).group(1)) == j == getattr(capi, "IQL_" + name)
    # m3pc_iql_args as the binding lays it out
    body = re.search(r"typedef struct m3pc_iql_args \{(.*?)\} m3pc_iql_args;", code, flags=re.S).group(1)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(" ", 1)[1].replace("long ", "").split(",")]
    assert fields == [n for n, _ in capi.IqlArgs._fields_]
    assert lib.m3pc_abi_version() == 7 == capi.ABI_VERSION and "#define M3PC_ABI_VERSION 7" in code
    assert "m3pc_iql_create" in re.search(r"/\* ABI history\..*?\*/", _header(), flags=re.S).group(0)
    assert "iql.hip" in build.SOURCES


def _fake_handle(s=S, a=A, hidden=0):
    """Stands in for a handle: m3pc_iql_create reads the m3pc_dims a handle starts with, and its device index behind them."""
    buf = C.create_string_buffer(256)
    C.memmove(buf, C.byref(capi.Dims(s, a, 8, 64, 2, 2, 1, 64, 1, hidden, 64, 0)), C.sizeof(capi.Dims))
    return buf, C.c_void_p(C.addressof(buf))


def _args(**over):
    a = dict(v_lr=3e-4, q_lr=3e-4, actor_lr=3e-4, expectile=0.7, beta=3.0, discount=0.99, tau=0.005, actor_t_max=1000, flags=0)
    a.update(over)
    return capi.IqlArgs(**a)


def _named(part, s=S, a=A, h=H, drop=None, resize=None):
    names = [n for n in R.part_names(part)]
    shapes = R.part_shapes(part, s, a, h)
    keep, arr = [], (capi.NamedTensor * len(names))()
    for j, (n, sh) in enumerate(zip(names, shapes)):
        x = np.zeros(sh, np.float32) if n != resize else np.zeros(int(np.prod(sh)) + 1, np.float32)
        nb = (n if n != drop else n + ".gone").encode()
        keep.append((x, nb))
        arr[j] = capi.NamedTensor(nb, x.ctypes.data, x.size, 0)
    return keep, arr, len(names)


def test_every_bad_argument_is_refused_without_a_gpu(lib):
    keep, h = _fake_handle()
    err = lib.m3pc_last_error
    q = C.c_void_p()

    # m3pc_iql_create(h, hidden, out)
    assert lib.m3pc_iql_create(None, H, C.byref(q)) == -1 and b"null" in err()
    assert lib.m3pc_iql_create(h, H, None) == -1 and b"null" in err()
    for hidden in (0, 32, 96, 512, -64):
        assert lib.m3pc_iql_create(h, hidden, C.byref(q)) == -1 and b"hidden" in err(), hidden
    for s, a in ((0, 3), (11, 0), (11, 33), (33, 32), (64, 1), (60, 5)):
        k2, h2 = _fake_handle(s, a)
        assert lib.m3pc_iql_create(h2, H, C.byref(q)) == -1 and b"covered sizes" in err(), (s, a)
    assert not q.value
    for hidden in (64, 128, 256):  # (the covered widths; S + A = 64 is the widest input, S alone may pass 32)
        for s, a in ((32, 32), (33, 3), (40, 6), (63, 1), (1, 1)):
            k2, h2 = _fake_handle(s, a)
            assert lib.m3pc_iql_create(h2, hidden, C.byref(q)) == 0 and q.value, (s, a)
            assert lib.m3pc_iql_destroy(q) == 0
    assert lib.m3pc_iql_destroy(None) == 0
    q = C.c_void_p()
    assert lib.m3pc_iql_create(h, H, C.byref(q)) == 0 and q.value

    # m3pc_iql_load(iql, part, tensors, n, obs_mean, obs_std, stream): everything below is refused before the storage is made
    kq, aq, nq = _named("qf")
    fp = C.POINTER(C.c_float)
    om = (C.c_float * S)()
    assert lib.m3pc_iql_load(None, capi.IQL_QF, aq, nq, None, None, None) == -1 and b"null" in err()
    assert lib.m3pc_iql_load(q, capi.IQL_QF, None, nq, None, None, None) == -1 and b"null" in err()
    for part in (-1, 10):
        assert lib.m3pc_iql_load(q, part, aq, nq, None, None, None) == -1 and b"part" in err(), part
    assert lib.m3pc_iql_load(q, capi.IQL_QF, aq, nq, C.cast(om, fp), None, None) == -1 and b"come together" in err()
    assert lib.m3pc_iql_load(q, capi.IQL_QF, aq, nq, None, C.cast(om, fp), None) == -1 and b"come together" in err()
    for part, code in (("qf", capi.IQL_QF), ("qf", capi.IQL_Q_TARGET), ("vf", capi.IQL_VF), ("actor", capi.IQL_ACTOR), ("qf", capi.IQL_QF_ADAM_M),
                       ("vf", capi.IQL_VF_ADAM_V), ("actor", capi.IQL_ACTOR_ADAM_M)):
        last = R.part_names(part)[-1]
        k1, a1, n1 = _named(part, drop=last)
        assert lib.m3pc_iql_load(q, code, a1, n1, None, None, None) == -1 and b"missing '%s'" % last.encode() in err(), (part, code)
        k1, a1, n1 = _named(part, resize=last)
        assert lib.m3pc_iql_load(q, code, a1, n1, None, None, None) == -1 and b"elements, expected" in err(), (part, code)
    assert lib.m3pc_iql_load(q, capi.IQL_VF, aq, nq, None, None, None) == -1 and b"missing 'v.net.0.weight'" in err()  # (another part's names)
    k1, a1, n1 = _named("qf", s=S + 1)
    assert lib.m3pc_iql_load(q, capi.IQL_QF, a1, n1, None, None, None) == -1 and b"'q1.net.0.weight' has" in err()   # (another state_dim)

    # m3pc_iql_export(iql, part, tensors, n, stream)
    assert lib.m3pc_iql_export(None, capi.IQL_QF, aq, nq, None) == -1 and b"null" in err()
    assert lib.m3pc_iql_export(q, capi.IQL_QF, None, nq, None) == -1 and b"null" in err()
    assert lib.m3pc_iql_export(q, 10, aq, nq, None) == -1 and b"part" in err()
    k1, a1, n1 = _named("qf", drop="q2.net.4.bias")
    assert lib.m3pc_iql_export(q, capi.IQL_QF, a1, n1, None) == -1 and b"no room" in err()
    assert lib.m3pc_iql_export(q, capi.IQL_QF, aq, nq, None) == -2 and b"not loaded" in err()

    # m3pc_iql_set_step / _get_step: the host's mirror
    t = C.c_longlong(-1)
    assert lib.m3pc_iql_set_step(None, 0) == -1 and lib.m3pc_iql_set_step(q, -1) == -1 and b"total_it" in err()
    assert lib.m3pc_iql_get_step(q, None) == -1 and lib.m3pc_iql_get_step(None, C.byref(t)) == -1
    assert lib.m3pc_iql_get_step(q, C.byref(t)) == 0 and t.value == 0
    assert lib.m3pc_iql_set_step(q, 12345) == 0 and lib.m3pc_iql_get_step(q, C.byref(t)) == 0 and t.value == 12345
    assert lib.m3pc_iql_set_step(q, 0) == 0

    # m3pc_iql_train_step(iql, args, batch, state, action, reward, next_state, done, losses, stream)
    buf = C.create_string_buffer(1 << 12)
    p = C.c_void_p(C.addressof(buf))

    def step(r=q, a=_args(), batch=8, s=p, ac=p, w=p, s2=p, d=p):
        return lib.m3pc_iql_train_step(r, None if a is None else C.byref(a), batch, s, ac, w, s2, d, None, None)

    assert step(r=None) == -1 and b"null" in err()
    assert step(a=None) == -1 and b"null" in err()
    for k in ("s", "ac", "w", "s2", "d"):
        assert step(**{k: None}) == -1 and b"null" in err(), k
    for batch in (0, -1, 1025):
        assert step(batch=batch) == -1 and b"batch" in err(), batch
    bad = (dict(v_lr=-1e-3), dict(q_lr=math.nan), dict(actor_lr=math.inf), dict(expectile=0.0), dict(expectile=1.0), dict(expectile=math.nan),
           dict(beta=math.inf), dict(beta=math.nan), dict(discount=-0.1), dict(discount=math.nan), dict(tau=-0.1), dict(tau=1.5), dict(tau=math.nan),
           dict(actor_t_max=0), dict(flags=1))
    for over in bad:
        assert step(a=_args(**over)) == -1, over
        assert lib.m3pc_last_error(), over
    assert step() == -2 and b"qf is not loaded" in err()   # nothing is loaded

    # m3pc_iql_train(iql, args, rb, n_steps, batch, n_online, seed, step, losses, stream)
    rb, other = C.c_void_p(), C.c_void_p()
    k3, h3 = _fake_handle(S + 1, A)
    assert lib.m3pc_replay_create(h, 0, 8, 8, 37, 64, C.byref(rb)) == 0 and lib.m3pc_replay_create(h3, 0, 8, 8, 37, 64, C.byref(other)) == 0

    def train(r=q, a=_args(), b=rb, n=2, batch=8):
        return lib.m3pc_iql_train(r, None if a is None else C.byref(a), b, n, batch, 0, 1, 0, None, None)

    assert train(r=None) == -1 and train(a=None) == -1 and train(b=None) == -1 and b"null" in err()
    for n in (0, -1):
        assert train(n=n) == -1 and b"n_steps" in err()
    for batch in (0, 1025):
        assert train(batch=batch) == -1 and b"batch" in err()
    assert train(a=_args(flags=2)) == -1 and b"flags" in err()
    assert train(b=other) == -1 and b"does not fit" in err()
    assert train() == -2 and b"not loaded" in err()

    # m3pc_iql_publish_critic(iql, h, stream)
    assert lib.m3pc_iql_publish_critic(None, h, None) == -1 and lib.m3pc_iql_publish_critic(q, None, None) == -1 and b"null" in err()
    assert lib.m3pc_iql_publish_critic(q, h, None) == -1 and b"does not fit" in err()        # a handle without a critic
    k4, h4 = _fake_handle(hidden=128)
    assert lib.m3pc_iql_publish_critic(q, h4, None) == -1 and b"does not fit" in err()       # a critic of another width
    k5, h5 = _fake_handle(hidden=H)
    assert lib.m3pc_iql_publish_critic(q, h5, None) == -2 and b"qf is not loaded" in err()

    # m3pc_iql_evaluate(iql, which, states, actions, rows, out, stream)
    assert lib.m3pc_iql_evaluate(None, capi.IQL_V, p, p, 4, p, None) == -1 and b"null" in err()
    assert lib.m3pc_iql_evaluate(q, capi.IQL_V, None, p, 4, p, None) == -1 and lib.m3pc_iql_evaluate(q, capi.IQL_V, p, p, 4, None, None) == -1
    assert lib.m3pc_iql_evaluate(q, capi.IQL_Q_MIN, p, None, 4, p, None) == -1 and b"null" in err()   # the twin needs actions
    for which in (-1, 4):
        assert lib.m3pc_iql_evaluate(q, which, p, p, 4, p, None) == -1 and b"which" in err()
    assert lib.m3pc_iql_evaluate(q, capi.IQL_V, p, None, 0, p, None) == -1 and b"rows" in err()
    for which in (capi.IQL_Q_MIN, capi.IQL_Q_TARGET_MIN, capi.IQL_V, capi.IQL_ACTOR_MEAN):
        assert lib.m3pc_iql_evaluate(q, which, p, p, 4, p, None) == -2 and b"not loaded" in err(), which

    assert lib.m3pc_iql_destroy(q) == 0 and lib.m3pc_replay_destroy(rb) == 0 and lib.m3pc_replay_destroy(other) == 0
    del keep, kq, k1, k2, k3, k4, k5


@pytest.mark.parametrize("case", list(R.CASES))
def test_the_restatement_is_the_reference_in_float64(golden, runs, case):
    """tests/iql_ref.py against the .double() run of the real ImplicitQLearning: the 20 losses of every case, and for the case
    h64 the first step's exp_avg and the final parameters, at 1e-10."""
    ref, losses, g1 = runs[case]
    want = golden[case + "/losses64"]
    assert losses.shape == want.shape == (R.N_STEPS, 3)
    assert np.abs(losses - want).max() <= 1e-10 * np.abs(want).max(), np.abs(losses / want - 1).max()
    if case != "h64":
        return
    for j, key in enumerate(("state", "action", "reward", "next_state", "done")):   # the recipe is the captured one
        assert np.array_equal(R.make_batches(case, 1)[0][j], golden[case + "/batch0/" + key]), key
    for n in golden[case + "/grad_names"]:
        part, name = str(n).split("/")
        m64 = golden[case + "/exp_avg64/" + str(n)]
        got = (1 - R.BETA1) * g1[part][name].reshape(m64.shape)
        assert np.abs(got - m64).max() <= 1e-10 * max(np.abs(m64).max(), 1e-300), n
    for n in golden[case + "/param_names"]:
        part, name = str(n).split("/")
        p64 = golden[case + "/final64/" + str(n)]
        assert np.abs(ref.p[part][name].reshape(p64.shape) - p64).max() <= 1e-10 * np.abs(p64).max(), n
        p32 = golden[case + "/final32/" + str(n)]
        assert p32.dtype == np.float32 and np.abs(p32 - p64).max() <= golden[case + "/ref32_param_dev"][list(golden[case + "/param_names"]).index(n)]


@pytest.mark.parametrize("case", list(R.CASES))
def test_the_recipes_meet_the_fixture_conditions(golden, runs, case):
    """A ReLU, expectile or clamp kink inside rounding distance would make the gradient itself discontinuous: the float64 run stays
    away from all of them, and still reaches every branch."""
    ref = runs[case][0]
    assert ref.min_preact > 1e-4, ref.min_preact                 # every hidden pre-activation of all seven forward passes, over all 20 steps
    assert ref.min_adv > 1e-4, ref.min_adv                       # over all 20 steps
    assert ref.min_clamp_gap > 1e-3, ref.min_clamp_gap           # |beta adv - ln 100|, over all 20 steps
    assert ref.n_clamped >= 1 and ref.n_done >= 1
    ls = R.make_state(case)[0]["actor"]["log_std"]
    assert (ls > R.LOG_STD_MAX).any() and ((ls > R.LOG_STD_MIN) & (ls < R.LOG_STD_MAX)).any()
    assert min(np.abs(ls - R.LOG_STD_MAX).min(), np.abs(ls - R.LOG_STD_MIN).min()) > 1e-3
    got = np.array([ref.min_preact, ref.min_adv, ref.min_clamp_gap, ref.n_clamped, ref.n_done])
    assert np.allclose(got, golden[case + "/conditions"], rtol=1e-6), (got, golden[case + "/conditions"])
    # what the GPU tests scale their tolerances from is there, and is what float32 loses: small, not zero
    for key, n in (("ref32_grad_dev", 25), ("ref32_loss_dev", 3), ("ref32_param_dev", 37)):
        dev = golden[case + "/" + key]
        assert dev.shape == (n,) and (dev >= 0).all() and dev.max() < 1e-3, (key, dev.max())
    assert float(golden[case + "/ref32_traj_dev"]) == golden[case + "/ref32_param_dev"].max()
    assert (golden[case + "/ref32_grad_dev"] > 0).sum() >= 24     # (log_std's clamped component aside, every tensor has a gradient)
    # 16 x the deviation of a single-number tensor is at least the spacing of float32 at it (iql_ref.SEEDS)
    for n, dev in zip(golden[case + "/grad_names"], golden[case + "/ref32_grad_dev"]):
        assert not str(n).endswith("net.4.bias") or str(n).startswith("actor/") or dev >= 2.0 ** -27, (n, dev)


def test_the_cosine_rate_is_the_schedulers():
    """The closed form against torch's recursive CosineAnnealingLR over a whole period."""
    import torch
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=3e-4)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 50)
    for k in range(50):
        assert abs(opt.param_groups[0]["lr"] - R.actor_lr(3e-4, k, 50)) <= 1e-12 * 3e-4, k
        opt.step()
        sched.step()


def test_example_compiles_and_links(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    libpath = build.build_library()
    libdir = os.path.dirname(libpath)
    exe = tmp_path / "critic_loop"
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "examples", "critic_loop.c"), "-o", str(exe), "-L", libdir, "-l:" + os.path.basename(libpath),
                           "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.join(rocm, "lib")])
    out = subprocess.check_output(["nm", "-u", str(exe)], text=True)
    for name in ("m3pc_iql_create", "m3pc_iql_load", "m3pc_iql_train", "m3pc_iql_publish_critic", "m3pc_iql_evaluate", "m3pc_replay_push_episodes"):
        assert name in out, name
