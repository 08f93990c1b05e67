"""The episode store without a GPU: m3pc_episodes_* are declared in include/m3pc_hip.h, exported by the library and bound by
m3pc_amd/capi.py; every M3PC_EINVAL refusal comes before any HIP call (m3pc_episodes_create makes none at all, so a store exists
on a machine without a device); and the NumPy restatement the GPU tests compare against (tests/episodes_ref.py) is itself pinned:
on hand-worked windows at every branch of the two rules, on HipPlanner._window_host / _goal_window_host, and on the reference's
value loop written out."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import episodes_ref as R
from m3pc_amd import build, capi
from m3pc_amd.planner import HipPlanner
from m3pc_amd.rollout import new_trajectory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m3pc_episodes_create", "m3pc_episodes_destroy", "m3pc_episodes_reset", "m3pc_episodes_observe", "m3pc_episodes_record",
       "m3pc_episodes_windows", "m3pc_episodes_values", "m3pc_episodes_export")
T, H, S, A = 8, 4, 11, 3


@pytest.fixture(scope="module")
def lib():
    return capi.load_library(build.build_library())


def _header():
    return open(os.path.join(ROOT, "include", "m3pc_hip.h")).read()


def test_every_entry_point_is_declared_exported_and_bound(lib):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/m3pc_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in capi.EXPORTS
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    for macro, value in (("M3PC_WINDOW_PLAN", capi.WINDOW_PLAN), ("M3PC_WINDOW_GOAL", capi.WINDOW_GOAL)):
        assert int(re.search(r"#define %s (\d+)" % macro, code).group(1)) == value
    assert "m3pc_episodes_create" in re.search(r"/\* ABI history\..*?\*/", _header(), flags=re.S).group(0)
    exports = open(os.path.join(ROOT, "m3pc_amd", "csrc", "exports.map")).read()
    assert "m3pc_*" in exports  # (the version script exports the m3pc_ prefix: nm -D agrees with capi.EXPORTS in test_abi_cpu.py)
    assert "episodes.hip" in build.SOURCES


def _fake_handle(traj_length=T):
    """Stands in for a handle: m3pc_episodes_create reads the m3pc_dims a handle starts with, and its device index behind them."""
    buf = C.create_string_buffer(256)
    C.memmove(buf, C.byref(capi.Dims(S, A, traj_length, 64, 2, 2, 1, 64, 1, 0, 64, 0)), C.sizeof(capi.Dims))
    return buf, C.c_void_p(C.addressof(buf))


def test_every_bad_argument_is_refused_without_a_gpu(lib):
    keep, h = _fake_handle()
    ep = C.c_void_p()
    err = lib.m3pc_last_error

    # m3pc_episodes_create(h, n_envs, max_steps, out)
    assert lib.m3pc_episodes_create(None, 5, 40, C.byref(ep)) == -1 and b"null" in err()
    assert lib.m3pc_episodes_create(h, 5, 40, None) == -1 and b"null" in err()
    assert lib.m3pc_episodes_create(h, 0, 40, C.byref(ep)) == -1 and b"n_envs" in err()
    assert lib.m3pc_episodes_create(h, -3, 40, C.byref(ep)) == -1 and b"n_envs" in err()
    assert lib.m3pc_episodes_create(h, 5, T - 1, C.byref(ep)) == -1 and b"max_steps" in err()
    assert not ep.value
    assert lib.m3pc_episodes_create(h, 5, T, C.byref(ep)) == 0 and ep.value  # (max_steps == T is the smallest store)
    assert lib.m3pc_episodes_destroy(ep) == 0
    assert lib.m3pc_episodes_destroy(None) == 0
    ep = C.c_void_p()
    assert lib.m3pc_episodes_create(h, 5, 40, C.byref(ep)) == 0 and ep.value

    buf = C.create_string_buffer(4096)
    p = C.c_void_p(C.addressof(buf))
    I = C.c_int

    def ids(*v):
        return (I * len(v))(*v)

    calls = {
        "reset": lambda e=ep, i=None, n=5: lib.m3pc_episodes_reset(e, i, n, None, 0, 0, None),
        "observe": lambda e=ep, i=None, n=5, obs=p: lib.m3pc_episodes_observe(e, i, n, obs, 0, 0, None),
        "record": lambda e=ep, i=None, n=5, a=p, r=p, lo=-1.0, hi=1.0: lib.m3pc_episodes_record(e, i, n, a, r, lo, hi, 0, None),
        "windows": lambda e=ep, i=None, n=5, mode=capi.WINDOW_PLAN, hor=H, s=p, a=p, r=p: lib.m3pc_episodes_windows(e, i, n, mode, hor, s, a, r, None, None),
        "values": lambda e=ep, i=None, n=5, g=0.99, v=p: lib.m3pc_episodes_values(e, i, n, g, 0, v, None),
    }
    for name, call in calls.items():
        assert call(e=None) == -1 and b"null" in err(), name
        for n in (0, -1, 6):  # n outside [1, n_envs]
            assert call(n=n) == -1 and b"outside [1, n_envs=5]" in err(), (name, n)
        assert call(i=ids(0, 5), n=2) == -1 and b"outside [0, n_envs=5)" in err(), name
        assert call(i=ids(-1), n=1) == -1 and b"outside [0, n_envs=5)" in err(), name
        assert call(i=ids(3, 1, 3), n=3) == -1 and b"repeated" in err(), name
        assert call(i=ids(4, 4), n=2) == -1 and b"repeated" in err(), name
    # (a repeated id in one call says nothing about the next one: the same id is fine again -- checked on the GPU)
    assert calls["observe"](obs=None) == -1 and b"null" in err()
    assert calls["record"](a=None) == -1 and b"null" in err()
    assert calls["record"](r=None) == -1 and b"null" in err()
    assert calls["record"](lo=1.0, hi=-1.0) == -1 and b"clip_min" in err()
    assert calls["record"](lo=float("nan")) == -1 and b"clip_min" in err()
    for k in ("s", "a", "r"):
        assert calls["windows"](**{k: None}) == -1 and b"null" in err(), k
    for hor in (0, -1, T + 1):
        assert calls["windows"](hor=hor) == -1 and b"horizon" in err(), hor
    assert calls["windows"](mode=2) == -1 and b"mode" in err()
    assert calls["values"](v=None) == -1 and b"null" in err()
    for g in (-0.5, float("nan"), float("inf")):
        assert calls["values"](g=g) == -1 and b"discount" in err(), g
    # m3pc_episodes_export(ep, env, obs, act, rew, path_length, on_device, stream)
    assert lib.m3pc_episodes_export(None, 0, None, None, None, None, 0, None) == -1 and b"null" in err()
    for env in (-1, 5):
        assert lib.m3pc_episodes_export(ep, env, None, None, None, None, 0, None) == -1 and b"env" in err()
    pl = I(-7)
    assert lib.m3pc_episodes_export(ep, 2, None, None, None, C.byref(pl), 0, None) == 0 and pl.value == 0  # (the mirror: no HIP call)
    assert lib.m3pc_episodes_destroy(ep) == 0
    del keep


def _traj(end, M=40, f64=False, seed=0):
    """An episode of `end` steps with the observation of step `end` written: row i of obs is i + 1 everywhere, act 100 + i, rew 200 + i."""
    tr = new_trajectory(S, A, M)
    if f64:
        tr["observations"] = np.zeros((M, S), dtype=np.float64)
    for i in range(end + 1):
        tr["observations"][i] = i + 1
    for i in range(end):
        tr["actions"][i] = 100 + i
        tr["rewards"][i] = 200 + i
    tr["path_length"] = end
    return tr


def _rows(x):
    return [int(v) for v in x[:, 0]]


@pytest.mark.parametrize("end,h,obs,act", [
    (0, 8, [1, 0, 0, 0, 0, 0, 0, 0], [0] * 8),                                          # the first step: one history row, h = T
    (T - H - 1, 5, [1, 2, 3, 4, 0, 0, 0, 0], [100, 101, 102, 0, 0, 0, 0, 0]),           # end + H < T: the horizon still shrinks
    (T - H, 4, [1, 2, 3, 4, 5, 0, 0, 0], [100, 101, 102, 103, 0, 0, 0, 0]),             # end + H == T: the first full horizon
    (T - H + 1, 4, [2, 3, 4, 5, 6, 0, 0, 0], [101, 102, 103, 104, 0, 0, 0, 0]),         # the window starts to slide
    (39, 4, [36, 37, 38, 39, 40, 0, 0, 0], [135, 136, 137, 138, 0, 0, 0, 0]),           # path_length = max_steps - 1
])
def test_plan_window_by_hand(end, h, obs, act):
    s, a, r, hh = R.window_plan(_traj(end), T, H)
    assert hh == h and R.horizon_of(end, T, H) == h
    assert s.dtype == a.dtype == r.dtype == np.float32 and s.shape == (T, S) and a.shape == (T, A) and r.shape == (T, 1)
    assert _rows(s) == obs and _rows(a) == act
    assert _rows(r) == [v + 100 if v else 0 for v in act]
    assert np.all(s == s[:, :1]) and np.all(a == a[:, :1])


def test_goal_window_by_hand():
    # way-points everywhere: row i of the observation block is i + 1 for ALL i, the history rows included
    def goal(end):
        tr = _traj(end, f64=True)
        tr["observations"][:] = np.arange(1, 41, dtype=np.float64)[:, None]
        return R.window_goal(tr, T, H)

    s, a, r, h = goal(0)
    assert h == 8 and _rows(s) == [1, 2, 3, 4, 5, 6, 7, 8] and _rows(a) == [0] * 8  # future rows are way-points
    s, a, r, h = goal(T - H + 1)
    assert h == 4 and _rows(s) == [2, 3, 4, 5, 6, 7, 8, 9] and _rows(a) == [101, 102, 103, 104, 0, 0, 0, 0] and _rows(r) == [201, 202, 203, 204, 0, 0, 0, 0]
    s, a, r, h = goal(36)  # end + h == max_steps: the last full window, smart == T
    assert _rows(s) == [33, 34, 35, 36, 37, 38, 39, 40]
    s, a, r, h = goal(37)  # smart = 7 < T: the buffer ends inside the window
    assert h == 4 and _rows(s) == [34, 35, 36, 37, 38, 39, 40, 0] and _rows(a) == [133, 134, 135, 136, 0, 0, 0, 0]
    s, a, r, h = goal(39)  # path_length = max_steps - 1: smart = 5 = hl
    assert _rows(s) == [36, 37, 38, 39, 40, 0, 0, 0] and _rows(a) == [135, 136, 137, 138, 0, 0, 0, 0]
    assert s.dtype == np.float32
    with pytest.raises(AssertionError):
        R.window_plan(_traj(39) | {"path_length": 40}, T, H)


def _planner_stub():
    """What HipPlanner._window_host / _goal_window_host read of a planner, without a device."""
    st = types.SimpleNamespace(T=T, S=S, A=A, cfg=types.SimpleNamespace(horizon=H))
    st._blocks = lambda flat: HipPlanner._blocks(st, flat)
    st._rtg_value = lambda rtg, percentage: float(rtg)
    return st


def test_restatement_agrees_with_the_planner_host_windows():
    rng = np.random.RandomState(3)
    st = _planner_stub()
    flat = np.empty((T * (S + A + 1),), dtype=np.float32)
    for end in list(range(0, 12)) + [500, 990, 991, 992, 993, 995, 998, 999]:
        tr = new_trajectory(S, A, 1000)  # (the host goal window carries the reference's literal 1000)
        tr["observations"][: end + 1] = rng.normal(size=(end + 1, S))
        tr["actions"][:end] = rng.uniform(-1, 1, size=(end, A))
        tr["rewards"][:end] = rng.normal(size=(end, 1))
        tr["path_length"] = end
        h, _ = HipPlanner._window_host(st, tr, 1.0, 1.0, flat)
        want = [b.copy() for b in st._blocks(flat)]
        s, a, r, hh = R.window_plan(tr, T, H)
        assert hh == h and all(np.array_equal(x, y) for x, y in zip((s, a, r), want)), end
        # the zero-shot buffer: float64 way-points in every observation row
        wp = dict(tr, observations=rng.normal(size=(1000, S)))
        h, _ = HipPlanner._goal_window_host(st, wp, 1.0, 1.0, flat)
        want = [b.copy() for b in st._blocks(flat)]
        s, a, r, hh = R.window_goal(wp, T, H)
        assert hh == h and all(np.array_equal(x, y) for x, y in zip((s, a, r), want)), end


@pytest.mark.parametrize("discount,use_avg", [(0.99, False), (1.0, True), (0.0, False)])
def test_values_restatement_is_the_reference_loop(discount, use_avg):
    rng = np.random.RandomState(5)
    M = 40
    rew = np.zeros((M, 1), dtype=np.float32)
    rew[:29] = rng.normal(size=(29, 1))
    # replay_buffer.py:70, 234-243, written out
    discounts = (discount ** np.arange(M))[:, None]
    vals = np.zeros((M, 1), dtype=np.float32)
    for t in range(M):
        vals[t] = (rew[t + 1:] * discounts[: -t - 1]).sum(axis=0)
    if use_avg:
        vals = (vals / np.arange(1, M + 1)[::-1][:, None]).astype(np.float32)
    got = R.values(rew, discount, use_avg)
    assert got.dtype == np.float32 and np.array_equal(got, vals[:, 0])
    assert got[M - 1] == 0 and np.all(got[29:] == 0)
    if discount == 0.0:
        assert np.array_equal(got[:-1], rew[1:, 0])
    # by hand: three rewards, discount 1/2
    assert np.array_equal(R.values(np.float32([7, 1, 2, 4]), 0.5), np.float32([1 + 1 + 1, 2 + 2, 4, 0]))
    assert np.array_equal(R.values(np.float32([7, 1, 2, 4]), 1.0, True), np.float32([7 / 4, 6 / 3, 4 / 2, 0]))


def test_clip_restatement():
    a = np.float32([-2.0, -1.0, -0.0, 0.0, 0.25, 1.0, 1.5, np.nan])
    c = R.clip(a, -1, 1)
    assert np.array_equal(c[:-1], np.float32([-1, -1, -0.0, 0, 0.25, 1, 1])) and np.isnan(c[-1]) and np.signbit(c[2]) and not np.signbit(c[3])
