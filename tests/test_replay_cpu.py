"""The replay buffer without a GPU: m3pc_replay_* are declared in include/m3pc_hip.h, exported by the library and bound by
m3pc_amd/capi.py; every refusal that needs no stored entry comes before any HIP call (m3pc_replay_create makes none, so a buffer
exists on a machine without a device); the host half of DeviceReplayBuffer.from_arrays and the NumPy restatement the GPU tests
compare against (tests/replay_ref.py) reproduce tests/golden/g6_replay.npz -- captured from the real reference ReplayBuffer -- bit for
bit; and the restated index draws are exact, bijective where they must be, and distributed as the header says."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import replay_ref as R
from m3pc_amd import build, capi, replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m3pc_replay_create", "m3pc_replay_destroy", "m3pc_replay_append", "m3pc_replay_append_transitions", "m3pc_replay_push_episodes",
       "m3pc_replay_sample_segments", "m3pc_replay_sample_transitions", "m3pc_replay_values_up_bound", "m3pc_replay_counts",
       "m3pc_replay_path_lengths")
S, A, M, L = 11, 3, 40, 8
KEYS5 = ("state", "action", "reward", "next_state", "done")


@pytest.fixture(scope="module")
def lib():
    return capi.load_library(build.build_library())


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "g6_replay.npz"))


def _header():
    return open(os.path.join(ROOT, "include", "m3pc_hip.h")).read()


def test_every_entry_point_is_declared_exported_and_bound(lib):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/m3pc_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in capi.EXPORTS
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    for macro, value in (("M3PC_REPLAY_UNIFORM", capi.REPLAY_UNIFORM), ("M3PC_REPLAY_LENGTH", capi.REPLAY_LENGTH),
                         ("M3PC_REPLAY_OFFLINE", capi.REPLAY_OFFLINE), ("M3PC_REPLAY_ONLINE", capi.REPLAY_ONLINE)):
        assert int(re.search(r"#define %s (\d+)" % macro, code).group(1)) == value
    assert (R.UNIFORM, R.LENGTH) == (capi.REPLAY_UNIFORM, capi.REPLAY_LENGTH)
    assert "m3pc_replay_create" in re.search(r"/\* ABI history\..*?\*/", _header(), flags=re.S).group(0)
    assert "replay.hip" in build.SOURCES
    # the generator is shared, not copied: one definition, in the header both users include
    csrc = os.path.join(ROOT, "m3pc_amd", "csrc")
    defs = [f for f in sorted(os.listdir(csrc)) if os.path.isfile(os.path.join(csrc, f)) and re.search(r"void philox4x32_10\(", open(os.path.join(csrc, f)).read())]
    assert defs == ["philox.h"]
    for f in ("select.hip", "replay.hip"):
        assert '#include "philox.h"' in open(os.path.join(csrc, f)).read()
    for f in ("episodes.hip", "replay.hip"):  # (the staging blocks likewise: episodes.h includes stage.h)
        assert '#include "episodes.h"' in open(os.path.join(csrc, f)).read()


def _fake_handle():
    """Stands in for a handle: m3pc_replay_create reads the m3pc_dims a handle starts with, and its device index behind them."""
    buf = C.create_string_buffer(256)
    C.memmove(buf, C.byref(capi.Dims(S, A, 8, 64, 2, 2, 1, 64, 1, 0, 64, 0)), C.sizeof(capi.Dims))
    return buf, C.c_void_p(C.addressof(buf))


def test_every_bad_argument_is_refused_without_a_gpu(lib):
    keep, h = _fake_handle()
    err = lib.m3pc_last_error
    rb = C.c_void_p()
    I = C.c_int

    # m3pc_replay_create(h, traj_capacity, max_steps, segment_length, offline_capacity, online_capacity, out)
    assert lib.m3pc_replay_create(None, 5, M, L, 37, 64, C.byref(rb)) == -1 and b"null" in err()
    assert lib.m3pc_replay_create(h, 5, M, L, 37, 64, None) == -1 and b"null" in err()
    for caps in ((-1, 37, 64), (5, -1, 64), (5, 37, -2)):
        assert lib.m3pc_replay_create(h, caps[0], M, L, caps[1], caps[2], C.byref(rb)) == -1 and b"capacity" in err(), caps
    assert lib.m3pc_replay_create(h, 5, 0, 1, 37, 64, C.byref(rb)) == -1 and b"max_steps" in err()
    for seg in (0, -1, M + 1):
        assert lib.m3pc_replay_create(h, 5, M, seg, 37, 64, C.byref(rb)) == -1 and b"segment_length" in err(), seg
    assert not rb.value
    assert lib.m3pc_replay_create(h, 0, M, M, 0, 0, C.byref(rb)) == 0 and rb.value  # (every part disabled; L == M is the longest segment)
    assert lib.m3pc_replay_destroy(rb) == 0 and lib.m3pc_replay_destroy(None) == 0
    rb = C.c_void_p()
    assert lib.m3pc_replay_create(h, 5, M, L, 37, 64, C.byref(rb)) == 0 and rb.value

    buf = C.create_string_buffer(1 << 16)
    p = C.c_void_p(C.addressof(buf))

    def ints(*v):
        return (I * len(v))(*v)

    # m3pc_replay_append(rb, n, obs, act, rew, val, lens, on_device, stream)
    def append(r=rb, n=2, o=p, a=p, w=p, v=p, lens=ints(L, M)):
        return lib.m3pc_replay_append(r, n, o, a, w, v, lens, 0, None)

    assert append(r=None) == -1 and b"null" in err()
    for k in ("o", "a", "w", "v", "lens"):
        assert append(**{k: None}) == -1 and b"null" in err(), k
    for n in (0, -1, 6):
        assert append(n=n, lens=ints(*[L] * 6)) == -1 and b"outside [1, traj_capacity=5]" in err(), n
    assert append(lens=ints(L, L - 1)) == -1 and b"lens[1] = 7" in err()    # shorter than a segment
    assert append(lens=ints(M + 1, L)) == -1 and b"lens[0] = 41" in err()   # longer than the storage
    assert append(lens=ints(0, L)) == -1 and b"lens[0]" in err()

    # m3pc_replay_append_transitions(rb, which, n, state, action, reward, next_state, done, on_device, stream)
    def trans(r=rb, which=capi.REPLAY_OFFLINE, n=3, s=p, a=p, w=p, s2=p, d=p):
        return lib.m3pc_replay_append_transitions(r, which, n, s, a, w, s2, d, 0, None)

    assert trans(r=None) == -1 and b"null" in err()
    for k in ("s", "a", "w", "s2", "d"):
        assert trans(**{k: None}) == -1 and b"null" in err(), k
    for which in (-1, 2):
        assert trans(which=which) == -1 and b"ring" in err(), which
    for which, cap in ((capi.REPLAY_OFFLINE, 37), (capi.REPLAY_ONLINE, 64)):
        for n in (0, -1, cap + 1):
            assert trans(which=which, n=n) == -1 and b"outside [1, capacity=%d]" % cap in err(), (which, n)

    # m3pc_replay_push_episodes(rb, ep, env_ids, n, discount, use_avg, final_obs, final_on_device, taken, stream)
    ep, other = C.c_void_p(), C.c_void_p()
    assert lib.m3pc_episodes_create(h, 5, M, C.byref(ep)) == 0 and lib.m3pc_episodes_create(h, 5, M + 1, C.byref(other)) == 0

    def push(r=rb, e=ep, ids=None, n=5, g=0.99):
        return lib.m3pc_replay_push_episodes(r, e, ids, n, g, 0, None, 0, None, None)

    assert push(r=None) == -1 and b"null" in err()
    assert push(e=None) == -1 and b"null" in err()
    assert push(e=other) == -1 and b"does not fit" in err()
    for n in (0, -1, 6):
        assert push(n=n) == -1 and b"outside [1, n_envs=5]" in err(), n
    assert push(ids=ints(0, 5), n=2) == -1 and b"outside [0, n_envs=5)" in err()
    assert push(ids=ints(-1), n=1) == -1 and b"outside [0, n_envs=5)" in err()
    assert push(ids=ints(3, 1, 3), n=3) == -1 and b"repeated" in err()
    for g in (-0.5, float("nan"), float("inf")):
        assert push(g=g) == -1 and b"discount" in err(), g
    taken = I(-7)
    assert lib.m3pc_replay_push_episodes(rb, ep, None, 5, 0.99, 0, None, 0, C.byref(taken), None) == 0 and taken.value == 0  # (empty episodes: nothing to do, no HIP call)

    # m3pc_replay_sample_segments(rb, batch, mode, traj_index, start_index, index_on_device, seed, step, states, actions, rewards, returns, returns_f32, out_traj, out_start, stream)
    def seg(r=rb, b=4, mode=capi.REPLAY_UNIFORM, ti=None, si=None, s=p, a=p, w=p, v=p):
        return lib.m3pc_replay_sample_segments(r, b, mode, ti, si, 0, 1, 0, s, a, w, v, 0, None, None, None)

    assert seg(r=None) == -1 and b"null" in err()
    for k in ("s", "a", "w", "v"):
        assert seg(**{k: None}) == -1 and b"null" in err(), k
    for b in (0, -1):
        assert seg(b=b) == -1 and b"batch" in err(), b
    for mode in (-1, 2):
        assert seg(mode=mode) == -1 and b"mode" in err(), mode
    assert seg(ti=p) == -1 and b"come together" in err()
    assert seg(si=p) == -1 and b"come together" in err()
    assert seg() == -2 and b"holds no trajectory" in err()  # M3PC_ESTATE: an empty buffer
    assert seg(mode=capi.REPLAY_LENGTH) == -2

    # m3pc_replay_sample_transitions(rb, batch, n_online, index, index_on_device, seed, step, state, action, reward, next_state, done, out_index, stream)
    def tr(r=rb, b=4, n_on=2, s=p, a=p, w=p, s2=p, d=p):
        return lib.m3pc_replay_sample_transitions(r, b, n_on, None, 0, 1, 0, s, a, w, s2, d, None, None)

    assert tr(r=None) == -1 and b"null" in err()
    for k in ("s", "a", "w", "s2", "d"):
        assert tr(**{k: None}) == -1 and b"null" in err(), k
    for b in (0, -1):
        assert tr(b=b) == -1 and b"batch" in err(), b
    for n_on in (-1, 5):
        assert tr(n_on=n_on) == -1 and b"n_online" in err(), n_on
    assert tr() == -2 and b"online ring is empty" in err()
    assert tr(n_on=0) == -2 and b"offline ring is empty" in err()
    # (more rows than a NON-EMPTY ring holds is M3PC_EINVAL: that needs a stored entry, tests/test_replay_gpu.py)

    assert lib.m3pc_replay_values_up_bound(None, p, None) == -1 and b"null" in err()
    assert lib.m3pc_replay_values_up_bound(rb, None, None) == -1 and b"null" in err()
    assert lib.m3pc_replay_values_up_bound(rb, p, None) == -2 and b"holds no trajectory" in err()
    c = [I(-1), I(-1), I(-1)]
    assert lib.m3pc_replay_counts(None, None, None, None) == -1
    assert lib.m3pc_replay_counts(rb, *[C.byref(x) for x in c]) == 0 and [x.value for x in c] == [0, 0, 0]
    assert lib.m3pc_replay_path_lengths(rb, None, 5) == -1 and b"null" in err()
    assert lib.m3pc_replay_path_lengths(rb, ints(0), 1) == 0
    assert lib.m3pc_replay_destroy(rb) == 0 and lib.m3pc_episodes_destroy(ep) == 0 and lib.m3pc_episodes_destroy(other) == 0
    del keep


# ------------------------------------------------------------------------------------------------ the golden
def _host_buffer(golden, mode):
    seed = int(golden["seed"])
    np.random.seed(seed)
    random.seed(seed)
    d = R.golden_dataset(seed)
    return replay.host_buffer(R.golden_config(mode), d["observations"], d["actions"], d["rewards"], d["dones_float"], d["terminals_float"],
                              d["next_observations"], discount=float(golden[f"{mode}.discount"]), max_path_length=R.GOLDEN_M)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _model(golden, mode, hb):
    cfg = R.golden_config(mode)
    m = R.HostReplay(R.GOLDEN_S, R.GOLDEN_A, len(hb.path_lengths), R.GOLDEN_M, cfg.traj_length, cfg.trans_buffer_size, cfg.trans_buffer_size)
    for i in range(len(hb.path_lengths)):
        m.append(hb.observations[i], hb.actions[i], hb.rewards[i], hb.values[i], hb.path_lengths[i])
    for row in zip(*hb.trans):
        m.append_transition(False, row[0], row[1], row[2][0], row[3], row[4])
    return m


def _check_batches(golden, mode, tag, m):
    g = lambda k: golden[f"{mode}.{tag}.{k}"]
    s, a, r, v = m.segments(g("traj.index"), g("traj.start"))
    assert _same(s, g("traj.states")) and _same(a, g("traj.actions")) and _same(r, g("traj.rewards")) and _same(v, g("traj.returns"))
    assert v.dtype == np.float64 and s.dtype == np.float32
    got = m.transitions(g("trans.index"), int(g("trans.n_online")))
    for k, x in zip(KEYS5, got):
        assert _same(x, g(f"trans.{k}")), k


@pytest.mark.parametrize("mode", ["uniform", "prob"])
def test_the_restatement_is_the_reference_buffer(golden, mode):
    hb = _host_buffer(golden, mode)
    g = lambda k: golden[f"{mode}.{k}"]
    # from_arrays' host half under the capture's seeds: the reference's buffer after __init__
    assert hb.values.dtype == np.float64 and hb.observations.dtype == np.float32
    for k in ("observations", "actions", "rewards", "values", "path_lengths", "p", "values_up_bound"):
        assert _same(getattr(hb, k), g(f"init.{k}")), k
    assert hb.use_avg == (mode == "prob") and (hb.path_lengths >= 4).all() and len(hb.path_lengths) == 5
    for k, x in zip(KEYS5, hb.trans):
        assert np.array_equal(np.float32(x).reshape(len(x), -1), g(f"init.offline.{k}")), k
    assert not g("init.offline.done").any()  # (terminals * 0)
    m = _model(golden, mode, hb)
    assert _same(m.values_up_bound()[:, None], g("init.values_up_bound"))
    _check_batches(golden, mode, "first", m)
    assert int(g("first.trans.n_online")) == 0  # (below using_online_threshold: all offline)
    # two online episodes: FIFO update, online transitions, the online value rounding (with use_avg: the float64 quotient)
    seed = int(golden["seed"])
    for k in range(2):
        tr = R.golden_trajectory(seed, k, hb.discount, hb.use_avg)
        obs = R.golden_rollout(seed, k)[0]
        assert tr["values"].dtype == np.float64
        assert m.push_episode(np.vstack([tr["observations"][:tr["path_length"]], np.zeros((R.GOLDEN_M - tr["path_length"], R.GOLDEN_S), np.float32)]),
                              tr["actions"], tr["rewards"], tr["path_length"], hb.discount, hb.use_avg, final_obs=obs[tr["path_length"]]) == 1
    assert _same(np.stack([t[0] for t in m.traj]), g("updated.observations")) and _same(np.stack([t[1] for t in m.traj]), g("updated.actions"))
    assert _same(np.stack([t[2] for t in m.traj])[..., None], g("updated.rewards"))
    assert _same(np.stack([t[3] for t in m.traj])[..., None], g("updated.values"))
    assert _same(np.asarray(m.lens), g("updated.path_lengths")) and _same(m.values_up_bound()[:, None], g("updated.values_up_bound"))
    if hb.use_avg:  # the quotient is NOT a float32: rounding it, as m3pc_episodes_values does, would miss the reference
        v = g("updated.values")[-2:]
        assert not np.array_equal(v, v.astype(np.float32).astype(np.float64))
    else:
        v = g("updated.values")[-2:]
        assert np.array_equal(v, v.astype(np.float32).astype(np.float64))
    got = m.transitions(np.arange(len(m.trans[True])), len(m.trans[True]))
    for k, x in zip(KEYS5, got):
        assert np.array_equal(x.reshape(len(x), -1), g(f"updated.online.{k}")), k
    assert int(g("updated.total_step")) == sum(R.GOLDEN_ROLLOUTS)
    _check_batches(golden, mode, "second", m)
    assert int(g("second.trans.n_online")) == 4  # (B // 2 once the online ring has reached the threshold)


# ------------------------------------------------------------------------------------------------ the draws
def test_draws_by_hand():
    assert R.pick_trajectory(0xFFFFFFFF, R.UNIFORM, [9]) == 0 and R.pick_trajectory(0x12345678, R.LENGTH, [9]) == 0      # count 1 -> 0
    assert R.pick_start(0xFFFFFFFF, 8, 8) == 0 and R.pick_start(0, 8, 8) == 0                                              # len == L -> start 0
    assert R.pick_trajectory(0xFFFFFFFF, R.UNIFORM, [8] * 7) == 6 and R.pick_trajectory(0, R.UNIFORM, [8] * 7) == 0        # the last / first index
    assert R.pick_trajectory(0xFFFFFFFF, R.LENGTH, [8, 9, 40, 23, 8]) == 4 and R.pick_trajectory(0, R.LENGTH, [8, 9, 40, 23, 8]) == 0
    assert R.pick_start(0xFFFFFFFF, 40, 8) == 32 and R.pick_start(0x80000000, 40, 8) == 16
    # cum = [0, 8, 17, 57, 80, 88]: r = (w * 88) >> 32
    for r, want in ((7, 0), (8, 1), (16, 1), (17, 2), (56, 2), (57, 3), (79, 3), (80, 4), (87, 4)):
        w = -(-(r << 32) // 88)  # the smallest word whose r is this one
        assert R.mulshift(w, 88) == r and R.pick_trajectory(w, R.LENGTH, [8, 9, 40, 23, 8]) == want, r
    ti, si = R.draw_segments(7, 3, 50, R.LENGTH, [8, 9, 40, 23, 8], 8)
    assert ti.dtype == si.dtype == np.int32 and ((0 <= ti) & (ti < 5)).all() and (si >= 0).all()
    assert (si <= np.array([8, 9, 40, 23, 8])[ti] - 8).all() and (si[(ti == 0) | (ti == 4)] == 0).all()
    a = R.draw_segments(7, 3, 50, R.UNIFORM, [8, 9, 40, 23, 8], 8)
    b = R.draw_segments(7, 4, 50, R.UNIFORM, [8, 9, 40, 23, 8], 8)
    assert not np.array_equal(a[0], b[0]) and np.array_equal(a[0][:20], R.draw_segments(7, 3, 20, R.UNIFORM, [8, 9, 40, 23, 8], 8)[0])


@pytest.mark.parametrize("n", [1, 2, 3, 37, 64, 65, 1000])
def test_pi_is_a_bijection(n):
    for seed, step, online in ((1, 0, True), (1, 0, False), (0xDEADBEEFCAFE, 1 << 40, True)):
        keys = R.round_keys(seed, step, online)
        assert len(keys) == 4 and all(0 <= k <= R.MASK for k in keys)
        assert sorted(R.pi(j, n, keys) for j in range(n)) == list(range(n)), (n, seed)
    assert R.round_keys(1, 0, True) != R.round_keys(1, 0, False) and R.round_keys(1, 0, True) != R.round_keys(1, 1, True)
    idx = R.draw_transitions(5, 9, min(n, 16), min(n, 8), n, n)
    assert len(set(idx[: min(n, 16)])) == min(n, 16) and len(set(idx[min(n, 16):])) == min(n, 8)


CHI2_SEED, CHI2_STEP = 20240611, 5  # (fixed; the draws are deterministic, and this pair passes: checked before it was committed)


def test_draws_are_distributed_as_stated():
    lens, Lseg, n = [8, 9, 40, 23, 8], 8, 20000
    ti, si = R.draw_segments(CHI2_SEED, CHI2_STEP, n, R.LENGTH, lens, Lseg)
    expect = n * np.array(lens) / sum(lens)
    chi2 = float((((np.bincount(ti, minlength=5) - expect) ** 2) / expect).sum())
    print("proportional chi2 (4 dof):", chi2)
    assert chi2 < 18.47  # the 0.999 quantile of chi-square with 4 degrees of freedom
    tu, _ = R.draw_segments(CHI2_SEED, CHI2_STEP, n, R.UNIFORM, lens, Lseg)
    chi2 = float((((np.bincount(tu, minlength=5) - n / 5) ** 2) / (n / 5)).sum())
    print("uniform chi2 (4 dof):", chi2)
    assert chi2 < 18.47
    # starts of the rows that drew trajectory 3 (len 23): uniform over 16 values; 0.999 quantile for 15 degrees of freedom: 37.70
    st = si[ti == 3]
    chi2 = float((((np.bincount(st, minlength=16) - len(st) / 16) ** 2) / (len(st) / 16)).sum())
    print("start chi2 (15 dof):", chi2, "over", len(st))
    assert st.max() == 15 and chi2 < 37.70
    # trajectory 2 (len 40): 33 starts; 0.999 quantile for 32 degrees of freedom: 62.49
    st = si[ti == 2]
    chi2 = float((((np.bincount(st, minlength=33) - len(st) / 33) ** 2) / (len(st) / 33)).sum())
    print("start chi2 (32 dof):", chi2, "over", len(st))
    assert st.max() == 32 and chi2 < 62.49
