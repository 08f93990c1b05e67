"""The replay buffer on the device (m3pc_replay_*, m3pc_amd/replay.py) against its NumPy restatement (tests/replay_ref.py) and the
golden captured from the reference ReplayBuffer (tests/golden/g6_replay.npz): segments and transitions bit for bit at caller indices
and at the library's own draws, the FIFO rings through two wrap-arounds, episodes pushed straight from an episode store, the column
maximum, and the reference's batches end to end.

Shapes: (S, A) = (11, 3) and (17, 6), max_steps 40, L = 8, trajectory capacity 5, transition capacities 37 (offline) and 64 (online)
-- the smallest that reach ring wrap-around, a non-power-of-two domain of the transition permutation, rows that are not 16-byte
aligned, path_length == L and path_length == max_steps; one case with capacity 300 and batch 700 for more than one block per launch
and the staging boundaries."""
import os
import random
import subprocess
import types

import numpy as np
import pytest
import torch

import episodes_ref
import replay_ref as R
from m3pc_amd import capi, synth
from m3pc_amd.episodes import EpisodeStore
from m3pc_amd.planner import HipPlanner
from m3pc_amd.replay import DeviceReplayBuffer
from m3pc_amd.rollout import evaluate_plan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, L = 40, 8
SHAPES = [(11, 3), (17, 6)]
KEYS5 = ("state", "action", "reward", "next_state", "done")


def _handle(S, A):
    return capi.Handle(S, A, 8, n_embd=64, n_head=2, max_candidates=64)


def _cfg(mode="uniform", B=6, TB=8, threshold=4):
    return types.SimpleNamespace(traj_length=L, traj_batch_size=B, traj_buffer_size=5, trans_batch_size=TB, trans_buffer_size=64,
                                 select_mode=mode, mtm_iter_per_rollout=3, using_online_threshold=threshold)


def _np(t):
    return t.cpu().numpy()


def _same(got, want):
    """Bit for bit, dtype and shape included."""
    got, want = np.ascontiguousarray(_np(got) if isinstance(got, torch.Tensor) else got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def _traj(rng, S, A, length):
    """A random trajectory with nothing behind its path length but values (which the reference holds for all max_steps rows)."""
    obs, act, rew = np.zeros((M, S), np.float32), np.zeros((M, A), np.float32), np.zeros((M,), np.float32)
    obs[:length], act[:length], rew[:length] = rng.normal(size=(length, S)), rng.uniform(-1, 1, size=(length, A)), rng.normal(size=(length,))
    return obs, act, rew, rng.normal(size=(M,)) * 10.0, length


def _pairs(lens):
    """Every (trajectory, start) of a buffer."""
    ti = np.concatenate([np.full((n - L + 1,), i) for i, n in enumerate(lens)]).astype(np.int32)
    si = np.concatenate([np.arange(n - L + 1) for n in lens]).astype(np.int32)
    return ti, si


def _check_segments(buf, model, ti, si, **kw):
    got = buf.traj_sample(indices=(ti, si), **kw)
    want = model.segments(ti, si, returns_f32=kw.get("returns_f32", False))
    for k, w in zip(("states", "actions", "rewards", "returns"), want):
        assert _same(got[k], w), k
    return got


# ---------------------------------------------------------------------------------------------- 5, 9: caller indices, the ring, the maximum
@pytest.mark.parametrize("S,A", SHAPES)
def test_segments_at_caller_indices_through_two_wraps(S, A):
    rng = np.random.RandomState(S)
    hd = _handle(S, A)
    buf = DeviceReplayBuffer(hd, _cfg(), 5, M, offline_capacity=37, online_capacity=64)
    model = R.HostReplay(S, A, 5, M, L, 37, 64)
    lengths = [L, M, 23, 9, 40, 8, 31, 17, 8, 40, 12]  # path_length == L and == max_steps among them
    done = 0
    for k, upto in enumerate((3, 5, 7, 11)):  # 3, then 2, 2 and 4 more: capacity 5 is passed twice
        new = [_traj(rng, S, A, n) for n in lengths[done:upto]]
        done = upto
        cols = [np.stack([t[j] for t in new]) for j in range(4)]
        if k % 2:  # device arrays, then host arrays (staged by the library)
            buf.append(*[torch.from_numpy(c).cuda() for c in cols], [t[4] for t in new])
        else:
            buf.append(*cols, [t[4] for t in new])
        for t in new:
            model.append(*t)
        assert len(buf) == min(upto, 5) == len(model.traj) and buf.path_lengths.tolist() == model.lens
        assert np.array_equal(buf.p, np.array(model.lens) / sum(model.lens))
        ti, si = _pairs(model.lens)  # exhaustive, start = len - L included
        assert (si == np.array(model.lens)[ti] - L).sum() == len(model.lens)
        got = _check_segments(buf, model, ti, si)
        assert got["returns"].dtype == torch.float64 and got["rewards"].shape == (len(ti), L, 1)
        dev = _check_segments(buf, model, torch.from_numpy(ti).cuda(), torch.from_numpy(si).cuda())  # the same indices on the device
        assert all(torch.equal(got[key], dev[key]) for key in got)
        _check_segments(buf, model, ti[::3], si[::3], returns_f32=True)
        # values_up_bound: numpy.max over the held trajectories, every one of the max_steps rows
        ub = buf.values_up_bound
        assert ub.shape == (M, 1) and _same(ub, model.values_up_bound()[:, None])
    # a host index out of range is refused; a device index the host cannot see is clamped into range
    with pytest.raises(capi.M3pcError, match="m3pc error -1.*traj_index"):
        buf.traj_sample(indices=([5], [0]))
    with pytest.raises(capi.M3pcError, match="m3pc error -1.*start_index"):
        buf.traj_sample(indices=([0], [model.lens[0] - L + 1]))
    got = buf.traj_sample(indices=(torch.tensor([99, -3], dtype=torch.int32).cuda(), torch.tensor([99, -3], dtype=torch.int32).cuda()))
    want = model.segments([4, 0], [model.lens[4] - L, 0])
    assert _same(got["states"], want[0]) and _same(got["returns"], want[3])
    with pytest.raises(capi.M3pcError, match="m3pc error -1.*lens"):
        buf.append(*[np.stack([t]) for t in _traj(rng, S, A, L)[:4]], [L - 1])
    assert buf.path_lengths.tolist() == model.lens
    torch.cuda.synchronize()
    buf.close()
    hd.close()


# ---------------------------------------------------------------------------------------------- 6: the library's draws
@pytest.mark.parametrize("capacity,B", [(5, 6), (300, 700)])
def test_drawn_segments_are_the_restatement(capacity, B):
    S, A = 11, 3
    rng = np.random.RandomState(capacity)
    hd = _handle(S, A)
    lens = [int(v) for v in rng.randint(L, M + 1, size=capacity)]
    lens[0], lens[-1] = L, M
    new = [_traj(rng, S, A, n) for n in lens]
    model = R.HostReplay(S, A, capacity, M, L, 0, 0)
    for t in new:
        model.append(*t)
    seen = {}
    for mode, code in (("uniform", R.UNIFORM), ("prob", R.LENGTH)):
        buf = DeviceReplayBuffer(hd, _cfg(mode, B), capacity, M, seed=0x1234_5678_9ABC, offline_capacity=0, online_capacity=0)
        buf.append(*[np.stack([t[j] for t in new]) for j in range(4)], lens)  # (capacity 300: host arrays of up to 1.6 MB through the staging blocks)
        for step in (0, 1, (1 << 40) + 7):
            buf.step = step
            got, (ti, si) = buf.traj_sample(return_indices=True)
            assert buf.step == step + 1
            wt, ws = R.draw_segments(buf.seed, step, B, code, lens, L)
            assert _same(ti, wt) and _same(si, ws), (mode, step)
            for k, w in zip(("states", "actions", "rewards", "returns"), model.segments(wt, ws)):
                assert _same(got[k], w), (mode, step, k)
            seen[(mode, step)] = (wt, got)
        buf.step = 1  # the same (seed, step) again: bit for bit; the fp32-returns flag: the float64 value rounded
        again = buf.traj_sample()
        assert all(torch.equal(again[k], seen[(mode, 1)][1][k]) for k in again)
        buf.step = 1
        f32 = buf.traj_sample(returns_f32=True)
        assert f32["returns"].dtype == torch.float32 and torch.equal(f32["returns"], again["returns"].to(torch.float32))
        assert torch.equal(f32["states"], again["states"])
        assert not np.array_equal(seen[(mode, 0)][0], seen[(mode, 1)][0])  # two steps differ
        buf.step = 0
        assert [b["states"].shape for b in buf] == [(B, L, S)] * 3 and buf.step == 3  # __iter__: mtm_iter_per_rollout batches
        torch.cuda.synchronize()
        buf.close()
    assert not np.array_equal(seen[("uniform", 0)][0], seen[("prob", 0)][0])
    hd.close()


# ---------------------------------------------------------------------------------------------- 7: episodes of a store
def _ulps(a, b):
    a, b = np.float32(a).view(np.int32).astype(np.int64), np.float32(b).view(np.int32).astype(np.int64)
    a, b = np.where(a < 0, -(a & 0x7FFFFFFF), a), np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


def _rows(buf, lens, i):
    """Trajectory i back from the device, rows [0, len): its segments at every start, laid side by side."""
    n = lens[i]
    starts = np.arange(n - L + 1, dtype=np.int32)
    b = buf.traj_sample(indices=(np.full_like(starts, i), starts))
    return {k: np.concatenate([_np(v)[:-1, 0], _np(v)[-1]]) for k, v in b.items()}


@pytest.mark.parametrize("S,A", SHAPES)
@pytest.mark.parametrize("use_avg", [False, True])
def test_push_from_a_store(S, A, use_avg):
    rng = np.random.RandomState(S + use_avg)
    E, lengths = 5, [5, M, L, 23, 13]  # one shorter than L (skipped as a trajectory), one full, one of exactly L steps
    hd = _handle(S, A)
    store = EpisodeStore(hd, E, M)
    store.reset()
    for step in range(M):
        ids = [e for e in range(E) if lengths[e] > step]
        store.observe(rng.normal(size=(len(ids), S)).astype(np.float32), ids)
        store.record(rng.uniform(-1.5, 1.5, size=(len(ids), A)).astype(np.float32), rng.normal(size=(len(ids),)).astype(np.float32), ids)
    eps = [{k: (_np(v) if isinstance(v, torch.Tensor) else v) for k, v in store.export(e).items()} for e in range(E)]
    assert [t["path_length"] for t in eps] == lengths
    discount = 1.5 if use_avg else 0.99  # (> 1: the reference's use_avg switch, with discount 1)
    final = rng.normal(size=(E, S)).astype(np.float32)
    buf = DeviceReplayBuffer(hd, _cfg(), 5, M, discount=discount, offline_capacity=37, online_capacity=37)
    model = R.HostReplay(S, A, 5, M, L, 37, 37)
    assert buf.use_avg == use_avg and buf.discount == (1.0 if use_avg else 0.99)

    # (trans_sample splits B // 2 : B - B // 2; to read the online ring alone, row for row in logical order, the test talks to the library)
    def online_rows():
        n = len(model.trans[True])
        out = [torch.empty((n, w), device="cuda") for w in (S, A, 1, S, 1)]
        idx = np.arange(n, dtype=np.int32)
        capi.check(hd.lib.m3pc_replay_sample_transitions(buf._rb, n, n, idx.ctypes.data, 0, 0, 0, *[capi._ptr(t) for t in out], None,
                                                         capi._stream(hd.device)))
        for k, g, w in zip(KEYS5, out, model.transitions(idx, n)):
            assert _same(g, w), k

    def pushed(ids, fin):
        taken = buf.update_from_store(store, ids, fin)
        want = 0
        for i, e in enumerate(range(E) if ids is None else ids):
            want += model.push_episode(eps[e]["observations"], eps[e]["actions"], eps[e]["rewards"], lengths[e], buf.discount, use_avg,
                                       None if fin is None else np.asarray(_np(fin) if isinstance(fin, torch.Tensor) else fin)[i])
        assert taken == want
        assert buf.counts() == (len(model.traj), 0, len(model.trans[True])) and buf.path_lengths.tolist() == model.lens
        online_rows()

    pushed([3, 0], None)                            # without final_obs: len - 1 transitions each; 26 of 37 slots
    assert buf.counts() == (1, 0, 22 + 4)
    pushed(None, final)                             # all five, 89 transitions into 37 slots: the ring wraps inside one call
    assert buf.counts() == (5, 0, 37) and buf.total_step == 28 + sum(lengths)
    pushed([4, 2], torch.from_numpy(final[:2]).cuda())  # final_obs on the device; the trajectory ring wraps
    assert buf.path_lengths.tolist() == [L, 23, 13, 13, L]
    # the trajectory blocks are export's; the values: one fp32 ulp of the restatement's, exactly widened; use_avg: the exact fp64 quotient
    for i, e in enumerate([2, 3, 4, 4, 2]):
        got = _rows(buf, model.lens, i)
        n = lengths[e]
        assert _same(got["states"], eps[e]["observations"][:n]) and _same(got["actions"], eps[e]["actions"][:n])
        assert _same(got["rewards"], eps[e]["rewards"][:n])
        v = got["returns"][:, 0]
        assert v.dtype == np.float64
        f = v * np.arange(M, M - n, -1) if use_avg else v  # (not exact with use_avg: only to find the fp32 value next to it)
        f32 = np.float32(f)
        want = episodes_ref.values(eps[e]["rewards"], buf.discount, False)[:n]
        assert int(_ulps(f32, want).max()) <= 1, (e, _ulps(f32, want).max())
        if use_avg:  # given that fp32 value (either neighbour of the restatement's): the unrounded float64 quotient
            cands = [np.float64(np.nextafter(want, s)) / np.arange(M, M - n, -1) for s in (np.float32(-np.inf), np.float32(np.inf))]
            cands.append(np.float64(want) / np.arange(M, M - n, -1))
            assert all(any(v[t] == c[t] for c in cands) for t in range(n)), e
        else:
            assert np.array_equal(v, f32.astype(np.float64))  # exactly widened
    # the store is unchanged
    assert [int(v) for v in store.path_length] == lengths
    for e in range(E):
        t = store.export(e)
        assert t["path_length"] == lengths[e] and all(_same(t[k], eps[e][k]) for k in ("observations", "actions", "rewards"))
    torch.cuda.synchronize()
    buf.close()
    store.close()
    hd.close()


# ---------------------------------------------------------------------------------------------- 8: transition batches
@pytest.mark.parametrize("S,A", SHAPES)
def test_transition_batches(S, A):
    rng = np.random.RandomState(7 * S)
    hd = _handle(S, A)
    buf = DeviceReplayBuffer(hd, _cfg(TB=12, threshold=41), 5, M, seed=99, offline_capacity=37, online_capacity=64)
    model = R.HostReplay(S, A, 5, M, L, 37, 64)

    def fill(online, n, device):
        rows = [rng.normal(size=(n, S)).astype(np.float32), rng.uniform(-1, 1, size=(n, A)).astype(np.float32),
                rng.normal(size=(n,)).astype(np.float32), rng.normal(size=(n, S)).astype(np.float32), (rng.uniform(size=(n,)) < 0.3).astype(np.float32)]
        buf.append_transitions(*([torch.from_numpy(r).cuda() for r in rows] if device else rows), online=online)
        for i in range(n):
            model.append_transition(online, *[r[i] for r in rows])

    def check(indices, n_on, got):
        for k, g, w in zip(KEYS5, got, model.transitions(indices, n_on)):
            assert g.dtype == torch.float32 and _same(g, w), k

    fill(False, 30, False)
    fill(True, 40, True)
    assert buf.counts() == (0, 30, 40) and buf.split() == (0, 12)  # below using_online_threshold = 41: all offline
    idx = rng.randint(0, 30, size=12).astype(np.int32)
    check(idx, 0, buf.trans_sample(indices=idx))
    got, drawn = buf.trans_sample(return_indices=True)  # drawn: distinct, the restatement's
    want = R.draw_transitions(99, 0, 0, 12, 40, 30)
    assert _same(drawn, want) and len(set(want.tolist())) == 12 and buf.step == 1
    check(want, 0, got)
    with pytest.raises(capi.M3pcError, match="m3pc error -1.*offline ring, which holds 30"):
        buf.trans_sample(batch_size=31)
    fill(False, 20, True)   # 50 into 37: the offline ring wraps
    fill(True, 30, False)   # 70 into 64: the online ring wraps
    assert buf.counts() == (0, 37, 64) and buf.split() == (6, 6) and buf.split(9) == (4, 5)  # B // 2 online rows FIRST, the rest offline
    idx = np.concatenate([rng.randint(0, 64, size=6), rng.randint(0, 37, size=6)]).astype(np.int32)
    idx[0], idx[5], idx[6], idx[11] = 0, 63, 0, 36
    check(idx, 6, buf.trans_sample(indices=idx))
    check(idx, 6, buf.trans_sample(indices=torch.from_numpy(idx).cuda()))
    for B in (12, 9, 74):  # 74 = 37 online + 37 offline: every offline entry exactly once
        step = buf.step
        got, drawn = buf.trans_sample(batch_size=B, return_indices=True)
        want = R.draw_transitions(99, step, B // 2, B - B // 2, 64, 37)
        assert _same(drawn, want) and len(set(want[: B // 2].tolist())) == B // 2 and len(set(want[B // 2:].tolist())) == B - B // 2
        check(want, B // 2, got)
    assert sorted(want[37:].tolist()) == list(range(37))
    with pytest.raises(capi.M3pcError, match="m3pc error -1.*offline ring, which holds 37"):
        buf.trans_sample(batch_size=76)
    with pytest.raises(capi.M3pcError, match="m3pc error -1.*index\\[6\\] = 37"):
        buf.trans_sample(indices=np.int32([0] * 6 + [37] + [0] * 5))
    torch.cuda.synchronize()
    buf.close()
    hd.close()


# ---------------------------------------------------------------------------------------------- 10: the reference's batches, end to end
@pytest.mark.parametrize("mode", ["uniform", "prob"])
def test_from_arrays_reproduces_the_reference(mode, golden_dir):
    g = np.load(os.path.join(golden_dir, "g6_replay.npz"))
    seed = int(g["seed"])
    d = R.golden_dataset(seed)
    hd = capi.Handle(R.GOLDEN_S, R.GOLDEN_A, 4, n_embd=64, n_head=2, max_candidates=64)
    np.random.seed(seed)
    random.seed(seed)
    buf = DeviceReplayBuffer.from_arrays(hd, R.golden_config(mode), d["observations"], d["actions"], d["rewards"], d["dones_float"],
                                         d["terminals_float"], d["next_observations"], discount=float(g[f"{mode}.discount"]),
                                         max_path_length=R.GOLDEN_M)
    key = lambda k: g[f"{mode}.{k}"]

    def check(tag):
        b = buf.traj_sample(indices=(key(f"{tag}.traj.index"), key(f"{tag}.traj.start")))
        assert sorted(b) == ["actions", "returns", "rewards", "states"] and b["returns"].dtype == torch.float64
        for k in b:
            assert _same(b[k], key(f"{tag}.traj.{k}")), (tag, k)
        assert buf.split()[0] == int(key(f"{tag}.trans.n_online"))
        t = buf.trans_sample(indices=key(f"{tag}.trans.index"))
        for k, x in zip(KEYS5, t):
            assert x.dtype == torch.float32 and _same(x, key(f"{tag}.trans.{k}")), (tag, k)

    assert _same(buf.path_lengths, key("init.path_lengths")) and _same(buf.p, key("init.p"))
    assert _same(buf.values_up_bound, key("init.values_up_bound")) and buf.counts() == (5, 16, 0)
    check("first")
    for k in range(2):  # the two online episodes, as host dicts and as online transitions
        tr = R.golden_trajectory(seed, k, buf.discount, buf.use_avg)
        obs, n = R.golden_rollout(seed, k)[0], R.GOLDEN_ROLLOUTS[k]
        buf.update_buffer([tr])
        buf.append_transitions(obs[:n], tr["actions"][:n], tr["rewards"][:n, 0], obs[1:n + 1], np.zeros((n,), np.float32), online=True)
    assert _same(buf.path_lengths, key("updated.path_lengths")) and _same(buf.p, key("updated.p"))
    assert _same(buf.values_up_bound, key("updated.values_up_bound")) and buf.total_step == int(key("updated.total_step"))
    check("second")
    torch.cuda.synchronize()
    buf.close()
    hd.close()


def test_rollout_into_the_buffer():
    """values_up_bound is what evaluate_plan takes as episode_rtg_ref; online_rollout: one exploring episode per environment through
    the episode store, pushed device to device."""
    from fake_learner import ToyEnv

    S, A, T, Msteps = 11, 3, 8, 12
    cfg = types.SimpleNamespace(traj_length=T, action_samples=64, horizon=4, discount=0.99, temperature=0.01, lmbda=0.6, plan_guidance="rtg_guiding",
                                device="cuda", index_jump=4, traj_batch_size=4, traj_buffer_size=4, trans_batch_size=6, trans_buffer_size=64,
                                select_mode="prob", mtm_iter_per_rollout=2, using_online_threshold=4)
    dims = synth.Dims(S, A, T, n_embd=64, n_head=2)
    p = HipPlanner(cfg, synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), None, n_embd=64, n_head=2, precision="fp32",
                   generator=torch.Generator(device="cuda").manual_seed(11), max_batch=3, max_windows=3)
    rng = np.random.RandomState(3)
    buf = DeviceReplayBuffer(p, cfg, 4, Msteps, discount=0.99)
    for n in (9, 12):
        obs, act, rew = np.zeros((Msteps, S), np.float32), np.zeros((Msteps, A), np.float32), np.zeros((Msteps, 1), np.float32)
        obs[:n], act[:n], rew[:n, 0] = rng.normal(size=(n, S)), rng.uniform(-1, 1, size=(n, A)), rng.normal(size=(n,))
        buf.update_buffer([{"observations": obs, "actions": act, "rewards": rew, "values": R.online_values(rew[:, 0], 0.99)[:, None], "path_length": n}])
    ub = buf.values_up_bound
    assert ub.shape == (Msteps, 1) and ub.dtype == np.float64
    lengths = [7, 12, 10]
    out = evaluate_plan(p, [ToyEnv(S, A, i, length=lengths[i]) for i in range(3)], ub, max_steps=Msteps, lockstep="native")
    assert out["plan_steps"] == sum(lengths)
    out = buf.online_rollout(p, [ToyEnv(S, A, i, length=lengths[i]) for i in range(3)])
    assert out["plan_steps"] == sum(lengths) and out["taken"] == 2  # (7 < traj_length = 8)
    assert buf.counts() == (4, 0, sum(lengths)) and buf.path_lengths.tolist() == [9, 12, 12, 10] and buf.total_step == 21 + sum(lengths)
    for i, n in ((2, 12), (3, 10)):  # the pushed trajectories are the rollout's
        tr = out["trajectories"][i - 1]
        b = buf.traj_sample(indices=([i], [n - T]))
        assert _same(b["actions"][0], tr["actions"][n - T:n]) and _same(b["states"][0], tr["observations"][n - T:n])
    buf.append_transitions(*[rng.normal(size=(5,) + w).astype(np.float32) for w in ((S,), (A,), (), (S,), ())], online=False)
    assert buf.trans_sample()[0].shape == (6, S) and buf.traj_sample()["returns"].shape == (4, T, 1)
    torch.cuda.synchronize()
    buf.close()
    p.handle.close()


# ---------------------------------------------------------------------------------------------- 11: the C example
def test_replay_loop_example(tmp_path):
    """examples/replay_loop.c compiled with gcc -Wall -Werror against include/m3pc_hip.h, linked to the built library and run: what it
    prints -- counts, path lengths, the library's indices and the checksums of both batches -- is what the restatement makes of the same
    toy episodes (exact integer arithmetic on both sides)."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = tmp_path / "replay_loop"
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "examples", "replay_loop.c"), "-o", str(exe), "-L", libdir, "-l:" + os.path.basename(capi.LIB_PATH),
                           "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.join(rocm, "lib")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = {ln.split()[0] + (" index" if " index" in ln[:18] else ""): ln.split()[(2 if " index" in ln[:18] else 1):] for ln in out.stdout.splitlines()}
    E, S, A, Ms, Ls, lengths = 4, 11, 3, 16, 8, [16, 5, 11, 8]
    model = R.HostReplay(S, A, E, Ms, Ls, 0, 24)
    for e, n in enumerate(lengths):
        obs = np.float32([[((131 * e + 17 * t + 7 * j) % 64 - 32) / 32 for j in range(S)] for t in range(n + 1)])
        act = np.clip(np.float32([[((29 * e + 5 * t + 3 * j) % 80 - 40) / 32 for j in range(A)] for t in range(n)]), -1, 1)
        rew = np.float32([((e + 3 * t) % 16 - 8) / 8 for t in range(n)])
        pad = lambda x, w: np.vstack([x[:n].reshape(n, w), np.zeros((Ms - n, w), np.float32)])
        model.push_episode(np.vstack([pad(obs, S)]), pad(act, A), pad(rew, 1), n, 0.5, False, final_obs=obs[n])
    assert lines["taken"] == ["3", "trajectories", "3", "online", "24", "lengths", "16", "11", "8"] and len(model.trans[True]) == 24
    ti, si = R.draw_segments(7, 0, 6, R.LENGTH, model.lens, Ls)
    assert lines["segment index"] == [f"{i}:{k}" for i, k in zip(ti, si)]
    seq = lambda x: float(np.cumsum(np.asarray(x, dtype=np.float64).reshape(-1))[-1])  # the sum in index order, in double
    assert [float(v) for v in lines["segments"]] == [seq(x) for x in model.segments(ti, si)]
    idx = R.draw_transitions(7, 1, 8, 0, 24, 0)
    assert lines["transition index"] == [str(i) for i in idx] and len(set(idx.tolist())) == 8
    assert [float(v) for v in lines["transitions"]] == [seq(x) for x in model.transitions(idx, 8)]
