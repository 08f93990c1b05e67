"""The episode store on the device (m3pc_episodes_*, m3pc_amd/episodes.py) against its NumPy restatement (tests/episodes_ref.py):
windows bit for bit after every step of random episodes, the clip's bits, the values to one fp32 ulp, a full episode refused
with nothing written, and the callers that take ``store=`` against the same calls without it.

Shapes: T = 8, H = 4, n_envs = 5, max_steps = 40 -- the smallest that reach every branch (the shrinking horizon of the first
T - H steps, the sliding window, the end of the buffer where smart < T) -- with (S, A) = (11, 3) and (17, 6): rows that are not
16-byte aligned; one case with 300 environments for more than one block per launch and many staged ids."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import episodes_ref as R
from m3pc_amd import capi, synth
from m3pc_amd.episodes import EpisodeStore
from m3pc_amd.planner import HipPlanner
from m3pc_amd.rollout import evaluate_plan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H = 8, 4


def _handle(S, A, **kw):
    return capi.Handle(S, A, T, n_embd=64, n_head=2, max_candidates=64, **kw)


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


class _Host:
    """The host model of a store: one trajectory dict per environment, stepped beside it."""

    def __init__(self, n, M, S, A):
        self.n, self.M, self.S, self.A = n, M, S, A
        self.tr = [self.fresh() for _ in range(n)]

    def fresh(self, table=None):
        obs = np.zeros((self.M, self.S), dtype=np.float64) if table is None else np.array(table, dtype=np.float64)
        return {"observations": obs, "actions": np.zeros((self.M, self.A), dtype=np.float32),
                "rewards": np.zeros((self.M, 1), dtype=np.float32), "path_length": 0}

    def observe(self, e, o):
        self.tr[e]["observations"][self.tr[e]["path_length"]] = np.float32(o)  # (what the store keeps: one rounding)

    def record(self, e, a, r, lo=-1.0, hi=1.0):
        t = self.tr[e]
        t["actions"][t["path_length"]] = R.clip(a, lo, hi)
        t["rewards"][t["path_length"]] = r
        t["path_length"] += 1


def _check_windows(store, host, ids, mode):
    s, a, r, h = store.windows(None if ids is None else ids, horizon=H, mode=mode)
    s, a, r = _np(s), _np(a), _np(r)
    envs = range(store.n_envs) if ids is None else ids
    assert s.shape == (len(envs), T, host.S) and a.shape == (len(envs), T, host.A) and r.shape == (len(envs), T, 1)
    fn = R.window_plan if mode == "plan" else R.window_goal
    for i, e in enumerate(envs):
        ws, wa, wr, wh = fn(host.tr[e], T, H)
        assert int(h[i]) == wh, (mode, e, host.tr[e]["path_length"])
        for got, want, key in ((s[i], ws, "states"), (a[i], wa, "actions"), (r[i], wr, "rewards")):
            assert np.array_equal(_bits(got), _bits(want)), (mode, key, e, host.tr[e]["path_length"])


@pytest.mark.parametrize("S,A", [(11, 3), (17, 6)])
def test_windows_are_the_restatement_after_every_step(S, A):
    n, M = 5, 40
    rng = np.random.RandomState(S)
    hd = _handle(S, A)
    store = EpisodeStore(hd, n, M)
    host = _Host(n, M, S, A)
    tables = {1: rng.normal(size=(M, S)), 3: rng.normal(size=(M, S)) * 1e3}  # fp64 way-points: rounded by the store
    store.reset()
    store.reset([3, 1], np.stack([tables[3], tables[1]]))  # float64, host
    for e, tb in tables.items():
        host.tr[e] = host.fresh(tb)
    lengths = {0: M, 1: 13, 2: 27, 3: M, 4: 33}  # the steps each episode takes; 0 and 3 run to the end of the buffer
    seen_h, seen_smart = set(), False
    for step in range(M + 9):
        if step == 9:  # a reset in mid-run: environment 2 starts over, with a float32 table on the device
            tb = rng.normal(size=(M, S)).astype(np.float32)
            store.reset([2], torch.from_numpy(tb).cuda())
            host.tr[2] = host.fresh(tb)
            lengths[2] = 27
        live = [e for e in range(n) if host.tr[e]["path_length"] < lengths[e]]
        if not live:
            break
        ids = [int(e) for e in rng.permutation(live)]
        obs = rng.normal(size=(len(ids), S))
        kind = step % 3  # the observations as float64 host rows, float32 host rows, float32 device rows
        if kind == 0:
            store.observe(obs, ids)
        elif kind == 1:
            obs = obs.astype(np.float32)
            store.observe(obs, ids)
        else:
            obs = obs.astype(np.float32)
            store.observe(torch.from_numpy(obs).cuda(), ids)
        for i, e in enumerate(ids):
            host.observe(e, obs[i])
        for mode in ("plan", "goal"):
            _check_windows(store, host, None if len(live) == n and step % 2 == 0 else ids, mode)  # NULL ids = 0 .. n-1
            _check_windows(store, host, [ids[-1]], mode)                                           # n = 1
            if len(ids) > 2:
                _check_windows(store, host, ids[1:][::-1], mode)                                   # a subset, another order
        for e in live:
            end = host.tr[e]["path_length"]
            seen_h.add(R.horizon_of(end, T, H))
            seen_smart |= end + R.horizon_of(end, T, H) > M
        acts = rng.uniform(-1.5, 1.5, size=(len(ids), A)).astype(np.float32)
        rews = rng.normal(size=(len(ids),)).astype(np.float32)
        if step % 2:
            store.record(torch.from_numpy(acts).cuda(), torch.from_numpy(rews).cuda(), ids)
        else:
            store.record(acts, rews, ids)
        for i, e in enumerate(ids):
            host.record(e, acts[i], rews[i])
        assert [int(v) for v in store.path_length] == [t["path_length"] for t in host.tr]
    assert seen_h == {4, 5, 6, 7, 8} and seen_smart  # every horizon of the shrinking start, and the end of the buffer
    assert [t["path_length"] for t in host.tr] == [lengths[e] for e in range(n)]
    for e in range(n):  # the export: the three blocks and the path length
        out = store.export(e)
        assert out["path_length"] == lengths[e]
        assert np.array_equal(_bits(_np(out["observations"])), _bits(host.tr[e]["observations"].astype(np.float32)))
        assert np.array_equal(_bits(_np(out["actions"])), _bits(host.tr[e]["actions"]))
        assert np.array_equal(_bits(_np(out["rewards"])), _bits(host.tr[e]["rewards"]))
    store.close()
    hd.close()


def test_clip_has_numpy_bits_and_host_and_device_inputs_agree():
    S, A, n = 11, 3, 5
    hd = _handle(S, A)
    special = np.float32([-2.0, -1.0, -0.0, 0.0, 0.3, 1.0, 1.7, np.nan, np.inf, -np.inf, 1.0000001, -1.0000001, 1e-45, -1e-45, 0.99999994])
    acts = special.reshape(n, A)
    rews = np.float32([0.5, -0.0, np.inf, 1e-45, -3.25])
    for lo, hi in ((-1.0, 1.0), (0.0, 0.5), (-0.0, 0.0), (-0.25, -0.25)):
        a, b = EpisodeStore(hd, n, T), EpisodeStore(hd, n, T)
        a.record(acts, rews, clip_min=lo, clip_max=hi)
        b.record(torch.from_numpy(acts).cuda(), torch.from_numpy(rews).cuda(), clip_min=lo, clip_max=hi)
        want = np.clip(acts, np.float32(lo), np.float32(hi))
        for e in range(n):
            ea, eb = a.export(e), b.export(e)
            assert ea["path_length"] == eb["path_length"] == 1
            assert np.array_equal(_bits(_np(ea["actions"])[0]), _bits(want[e])), (lo, hi, e, _np(ea["actions"])[0], want[e])
            assert np.array_equal(_bits(_np(ea["rewards"])[0]), _bits(rews[e : e + 1]))
            assert not _np(ea["actions"])[1:].any() and not _np(ea["rewards"])[1:].any()
            for k in ("observations", "actions", "rewards"):
                assert np.array_equal(_bits(_np(ea[k])), _bits(_np(eb[k])))
        a.close()
        b.close()
    hd.close()


def _ulps(a, b):
    """Distance in fp32 steps between two float32 arrays (finite values)."""
    def order(x):
        i = _bits(x).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(order(a) - order(b))


@pytest.mark.parametrize("S,A", [(11, 3), (17, 6)])
def test_values_are_the_restatement_to_one_ulp_and_repeat_bit_for_bit(S, A):
    n, M = 5, 40
    rng = np.random.RandomState(7 + S)
    hd = _handle(S, A)
    store = EpisodeStore(hd, n, M)
    lengths = [39, 1, 17, 40, 28]  # episodes shorter than max_steps (and one full one): the rewards behind them are zero
    rew = np.zeros((n, M), dtype=np.float32)
    for step in range(M):
        ids = [e for e in range(n) if step < lengths[e]]
        r = (rng.normal(size=(len(ids),)) * 10 ** rng.uniform(-1, 1, size=(len(ids),))).astype(np.float32)
        store.record(np.zeros((len(ids), A), dtype=np.float32), r, ids)
        rew[ids, step] = r
    worst = 0
    for discount, use_avg, ids in ((0.99, False, None), (1.0, True, None), (0.5, False, [4, 0, 2]), (0.997, True, [1]), (0.0, False, [3, 2])):
        v1 = _np(store.values(discount, use_avg, ids))
        v2 = _np(store.values(discount, use_avg, ids))
        assert np.array_equal(_bits(v1), _bits(v2))  # two runs: identical bits
        envs = range(n) if ids is None else ids
        assert v1.shape == (len(envs), M)
        for i, e in enumerate(envs):
            want = R.values(rew[e], discount, use_avg)
            d = int(_ulps(v1[i], want).max())
            worst = max(worst, d)
            assert d <= 1, (discount, use_avg, e, d)
            assert v1[i, M - 1] == 0 and not v1[i, lengths[e] - 1 if lengths[e] > 0 else 0 :].any()
    print(f"values: largest distance to the fp64 pairwise sum {worst} ulp")
    store.close()
    hd.close()


def test_three_hundred_environments_cross_block_and_staging_boundaries():
    S, A, n, M = 11, 3, 300, 40
    rng = np.random.RandomState(300)
    hd = _handle(S, A)
    store = EpisodeStore(hd, n, M)
    host = _Host(n, M, S, A)
    for step in range(6):
        ids = [int(e) for e in rng.permutation(n)]
        if step == 3:
            ids = ids[:170]  # from here on the environments differ in length: mixed horizons in one call
        obs = rng.normal(size=(len(ids), S)).astype(np.float32)
        store.observe(obs, ids)
        for i, e in enumerate(ids):
            host.observe(e, obs[i])
        if step == 5:
            break
        acts = rng.uniform(-1.5, 1.5, size=(len(ids), A)).astype(np.float32)
        rews = rng.normal(size=(len(ids),)).astype(np.float32)
        store.record(acts, rews, ids)
        for i, e in enumerate(ids):
            host.record(e, acts[i], rews[i])
    for mode in ("plan", "goal"):
        _check_windows(store, host, None, mode)
        _check_windows(store, host, [int(e) for e in rng.permutation(n)], mode)
    v = _np(store.values(0.99, False, [int(e) for e in rng.permutation(n)[:290]]))
    assert v.shape == (290, M)
    store.close()
    hd.close()


def test_a_full_episode_is_refused_and_the_store_is_unchanged():
    S, A = 11, 3
    hd = _handle(S, A)
    store = EpisodeStore(hd, 2, T)  # max_steps == T: the smallest store
    rng = np.random.RandomState(1)
    for step in range(T):
        store.observe(rng.normal(size=(1, S)), [0])
        store.record(rng.uniform(-1, 1, size=(1, A)), rng.normal(size=(1,)), [0])
    assert [int(v) for v in store.path_length] == [T, 0]
    before = [store.export(e) for e in range(2)]
    a, r = rng.uniform(-1, 1, size=(2, A)).astype(np.float32), np.float32([1.0, 2.0])
    for call in (lambda: store.record(a[:1], r[:1], [0]), lambda: store.record(a, r),        # alone, and beside an environment with room
                 lambda: store.record(a, r, [1, 0]), lambda: store.observe(np.ones((1, S)), [0]),
                 lambda: store.observe(np.ones((2, S))), lambda: store.windows([0], horizon=H), lambda: store.windows(None, horizon=H)):
        with pytest.raises(capi.M3pcError, match="m3pc error -2.*full"):
            call()
    assert [int(v) for v in store.path_length] == [T, 0]
    after = [store.export(e) for e in range(2)]
    for b, f in zip(before, after):
        assert b["path_length"] == f["path_length"]
        for k in ("observations", "actions", "rewards"):
            assert torch.equal(b[k], f[k]), k
    # the environment with room goes on, a repeated id is refused per call only, and a reset makes room again
    store.record(a[1:], r[1:], [1])
    with pytest.raises(capi.M3pcError, match="m3pc error -1.*repeated"):
        store.record(a, r, [1, 1])
    store.record(a[1:], r[1:], [1])
    assert [int(v) for v in store.path_length] == [T, 2] and store.export(1)["path_length"] == 2
    store.reset([0])
    store.record(a[:1], r[:1], [0])
    assert store.export(0)["path_length"] == 1 and not _np(store.export(0)["actions"])[1:].any()
    store.close()
    hd.close()


# ---------------------------------------------------------------------------------------------- the callers that take store=
def _cfg(N, guidance="rtg_guiding"):
    return types.SimpleNamespace(traj_length=T, action_samples=N, horizon=H, discount=0.99, temperature=0.01, lmbda=0.6,
                                 plan_guidance=guidance, device="cuda", index_jump=4)


def _planner(N=64, precision="fp32", **kw):
    dims = synth.Dims(11, 3, T, n_embd=64, n_head=2)
    return HipPlanner(_cfg(N), synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), None, n_embd=64, n_head=2,
                      precision=precision, generator=torch.Generator(device="cuda").manual_seed(11), **kw)


@pytest.mark.parametrize("precision,lockstep,kw", [("fp32", "native", {}), ("bf16", "native", {}),
                                                   ("fp32", True, dict(refine=dict(iterations=2, top_k=16)))])
def test_evaluate_plan_with_a_store_is_the_rollout_without_it(precision, lockstep, kw):
    """lockstep="native": one m3pc_plan_steps_certified call per round; the third case is a planner that plans by refinement
    (m3pc_refine_plans per round, the warm start keyed by environment, path lengths from the store's mirror)."""
    from fake_learner import ToyEnv

    lengths = [7, 12, 10]  # past T - H: shrinking horizons, sliding windows and rounds of fewer live environments
    rtg_ref = np.linspace(3.0, 1.0, 1000)

    def run(store):
        p = _planner(precision=precision, max_batch=3, max_windows=3, **kw)
        envs = [ToyEnv(11, 3, i, length=lengths[i]) for i in range(3)]
        out = evaluate_plan(p, envs, rtg_ref, max_steps=12, lockstep=lockstep, store=store)
        torch.cuda.synchronize()
        p.handle.close()
        return out

    a, b = run(False), run(True)
    assert a["plan_steps"] == b["plan_steps"] == sum(lengths)
    assert a["lengths"] == b["lengths"] == [float(v) for v in lengths]
    assert a["returns"] == b["returns"]
    for ta, tb, n in zip(a["trajectories"], b["trajectories"], lengths):
        assert tb["path_length"] == ta["path_length"] == n
        for k in ("actions", "rewards", "observations"):
            assert tb[k].shape == ta[k].shape and tb[k].dtype == ta[k].dtype
            assert np.array_equal(_bits(ta[k]), _bits(tb[k])), k
        assert np.abs(ta["actions"][:n]).sum() > 0
        # the values ReplayBuffer.online_rollout computes; the store-less rollout leaves them zero, as before
        assert not ta["values"].any()
        want = R.values(tb["rewards"], 0.99)
        assert tb["values"].shape == (12, 1) and int(_ulps(tb["values"][:, 0], want).max()) <= 1 and tb["values"].any()


def test_evaluate_plan_store_needs_a_lockstep_form():
    p = _planner()
    with pytest.raises(ValueError, match="lock-step"):
        evaluate_plan(p, [], np.ones(10), store=True)
    with pytest.raises(ValueError, match="lock-step"):
        p.action_sample_batch(None, store=object())
    p.handle.close()


def test_act_batch_with_a_store_equals_act_batch_without_it(tmp_path):
    """12 zero-shot windows with mixed horizons (path lengths 0 .. 5 at T = 8, H = 4: h = 8, 7, 6, 5, 4, 4), float64 way-points."""
    from m3pc_amd.zeroshot import WaypointFollower

    E, S, A = 12, 11, 3
    rng = np.random.RandomState(12)
    path = tmp_path / "waypoints.txt"
    np.savetxt(path, rng.normal(size=(1000, S)))
    for precision, kw in (("fp32", dict(max_batch=E)), ("bf16", dict(goal_batch=E))):
        p = _planner(N=1, precision=precision, **kw)
        fo = WaypointFollower(p, str(path), index_jump=4, goal_mask="piid")
        trajs = [fo.new_trajectory() for _ in range(E)]
        store = fo.new_store(E)
        ahead = [e % 6 for e in range(E)]
        for step in range(5):  # environment e is e % 6 steps into its episode
            ids = [e for e in range(E) if step < ahead[e]]
            obs = rng.normal(size=(len(ids), S)).astype(np.float32)
            acts = rng.uniform(-1.2, 1.2, size=(len(ids), A)).astype(np.float32)
            rews = rng.normal(size=(len(ids),)).astype(np.float32)
            store.observe(obs, ids)
            store.record(acts, rews, ids)
            for i, e in enumerate(ids):
                trajs[e]["observations"][step] = obs[i]
                fo.record(trajs[e], step, np.clip(acts[i], -1, 1), rews[i])
        obs = rng.normal(size=(E, S))
        rtgs = [2.5] * E
        want = fo.act_batch(trajs, list(obs), ahead, rtgs)
        got = fo.act_batch(None, list(obs), ahead, rtgs, store=store)
        assert want.shape == got.shape == (E, A) and np.array_equal(_bits(want), _bits(got)), precision
        assert np.abs(want).sum() > 0
        pruned = precision == "bf16"
        assert p.last["pruned"] == pruned
        # a subset in another order, through env_ids
        sub = [7, 2, 11, 4]
        got2 = fo.act_batch(None, [obs[e] for e in sub], [ahead[e] for e in sub], [2.5] * 4, store=store, env_ids=sub)
        want2 = fo.act_batch([trajs[e] for e in sub], [obs[e] for e in sub], [ahead[e] for e in sub], [2.5] * 4)
        assert np.array_equal(_bits(want2), _bits(got2))
        with pytest.raises(ValueError, match="path lengths"):
            fo.act_batch(None, list(obs), [t + 1 for t in ahead], rtgs, store=store)
        store.close()
        p.handle.close()


def test_c_example_runs_a_closed_loop_on_the_store(tmp_path):
    """examples/episode_loop.c compiled with gcc -Wall -Werror against include/m3pc_hip.h, linked to the built library and run for
    11 rounds of E = 3 (T = 8, H = 4: the shrinking horizons, then sliding windows): what it exports from the store is what its
    own log of actions and rewards says, its horizons are the rule's, its values the restatement's, and its first round is the
    binding's m3pc_plan_steps_certified on the store's first windows."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    so = tmp_path / "libepisode_loop.so"
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(rocm, "include"), os.path.join(ROOT, "examples", "episode_loop.c"), "-o", str(so),
                           "-L", libdir, "-l:" + os.path.basename(capi.LIB_PATH), "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-lm",
                           "-Wl,-rpath," + libdir])
    p = _planner(N=64, precision="fp32", max_batch=3, max_windows=3)
    hd, dims = p.handle, synth.Dims(11, 3, T, n_embd=64, n_head=2)
    S, A, N, K, E, M, seed, tau = 11, 3, 64, 11, 3, 16, 77, 0.01
    fp, vp, ip = C.POINTER(C.c_float), C.c_void_p, C.POINTER(C.c_int)

    class IO(C.Structure):
        _fields_ = [("dims", C.POINTER(capi.Dims)), ("weights", C.POINTER(capi.NamedTensor)), ("n_weights", C.c_int),
                    ("tok_mean", fp * 4), ("tok_std", fp * 4), ("tok_dim", C.c_int * 4), ("tok_normalize", C.c_int * 4),
                    ("n_rounds", C.c_int), ("n_envs", C.c_int), ("max_steps", C.c_int), ("n", C.c_int), ("horizon", C.c_int),
                    ("lmbda", C.c_double), ("discount", C.c_double), ("rtg", C.c_double), ("temperature", C.c_float),
                    ("seed", C.c_ulonglong),
                    ("states", vp), ("actions", vp), ("rewards", vp), ("eps", vp), ("expo", vp), ("sample_actions", vp),
                    ("scores_low", vp), ("merged", vp), ("sample_action", vp),
                    ("obs_host", vp), ("act_host", vp), ("rew_host", vp), ("rtg_host", vp), ("horizons_host", vp),
                    ("records", C.POINTER(capi.CertRecord)),
                    ("actions_log", vp), ("rewards_log", vp), ("horizons_log", vp), ("values", vp),
                    ("obs_out", vp), ("act_out", vp), ("rew_out", vp), ("path_length", vp)]

    sd = synth.make_state_dict(dims, 0)
    arr, keep = capi._named(sd)
    io = IO()
    io.dims, io.weights, io.n_weights = C.pointer(hd.dims), C.cast(arr, C.POINTER(capi.NamedTensor)), len(sd)
    toks = []
    for k, name in enumerate(capi.KEYS):
        t = p.tokenizer_manager.tokenizers[name]
        m, sdv = t._data_mean.float().contiguous().reshape(-1), t._data_std.float().contiguous().reshape(-1)
        toks.append((m, sdv))
        io.tok_mean[k], io.tok_std[k] = C.cast(m.data_ptr(), fp), C.cast(sdv.data_ptr(), fp)
        io.tok_dim[k], io.tok_normalize[k] = m.numel(), int(bool(t.normalize))
    dev = dict(device="cuda", dtype=torch.float32)
    bufs = dict(states=torch.empty((E, T, S), **dev), actions=torch.empty((E, T, A), **dev), rewards=torch.empty((E, T, 1), **dev),
                eps=torch.empty((E, N, T * A), **dev), expo=torch.empty((E, N), **dev), sample_actions=torch.empty((E, N, T, A), **dev),
                scores_low=torch.empty((E, N), **dev), merged=torch.empty((E, N), **dev), sample_action=torch.empty((E, A), **dev),
                values=torch.empty((E, M), **dev), obs_out=torch.empty((E, M, S), **dev), act_out=torch.empty((E, M, A), **dev),
                rew_out=torch.empty((E, M), **dev))
    host = dict(obs_host=np.zeros((E, S), np.float32), act_host=np.zeros((E, A), np.float32), rew_host=np.zeros((E,), np.float32),
                rtg_host=np.zeros((E,), np.float64), horizons_host=np.zeros((E,), np.int32), actions_log=np.zeros((K, E, A), np.float32),
                rewards_log=np.zeros((K, E), np.float32), horizons_log=np.zeros((K,), np.int32), path_length=np.full((E,), -1, np.int32))
    for name, t in bufs.items():
        setattr(io, name, t.data_ptr())
    for name, a in host.items():
        setattr(io, name, a.ctypes.data)
    records = (capi.CertRecord * E)()
    io.records = C.cast(records, C.POINTER(capi.CertRecord))
    io.n_rounds, io.n_envs, io.max_steps, io.n, io.horizon = K, E, M, N, H
    io.lmbda, io.discount, io.rtg, io.temperature, io.seed = 0.6, 0.99, 2.5, tau, seed
    torch.cuda.synchronize()
    lib = C.CDLL(str(so))
    lib.episode_loop.restype = C.c_int
    lib.episode_loop.argtypes = [C.POINTER(IO), C.c_int, vp]
    rc = lib.episode_loop(C.byref(io), torch.cuda.current_device(), vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, hd.lib.m3pc_last_error()
    torch.cuda.synchronize()
    assert host["path_length"].tolist() == [K] * E
    assert host["horizons_log"].tolist() == [R.horizon_of(k, T, H) for k in range(K)] == [8, 7, 6, 5, 4, 4, 4, 4, 4, 4, 4]
    act, rew, obs = _np(bufs["act_out"]), _np(bufs["rew_out"]), _np(bufs["obs_out"])
    for e in range(E):
        assert np.array_equal(_bits(act[e, :K]), _bits(np.clip(host["actions_log"][:, e], np.float32(-1), np.float32(1))))
        assert np.array_equal(_bits(rew[e, :K]), _bits(host["rewards_log"][:, e]))
        assert not act[e, K:].any() and not rew[e, K:].any() and not obs[e, K:].any() and obs[e, :K].all()
        assert int(_ulps(_np(bufs["values"])[e], R.values(rew[e], 0.99)).max()) <= 1
    assert np.abs(host["actions_log"]).sum() > 0 and np.isfinite(host["rewards_log"]).all()
    # round 0 again through the binding: the windows of a store with the example's first observations, the variates of steps 0 .. E-1
    store = EpisodeStore(hd, E, M)
    store.observe(obs[:, 0])
    s, a, r, hz = store.windows(horizon=H)
    var = [hd.draw_variates(seed, w, N, T * A) for w in range(E)]
    res, _ = hd.plan_steps_certified(capi.MODE_RTG, s, a, r, [2.5] * E, torch.stack([v[0] for v in var]), torch.stack([v[1] for v in var]),
                                     int(hz[0]), 0.6, 0.99, N, tau, kmin=1, kmax=1, rfirst=0, rmax=0, precision=capi.PREC_FP32)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(_np(res["sel"][4])), _bits(host["actions_log"][0]))
    store.close()
    p.handle.close()
    del keep, toks
