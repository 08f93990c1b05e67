"""The IQL trainer on the device (m3pc_iql_*, m3pc_amd/iql.py) against the float64 restatement of the reference's train()
(tests/iql_ref.py, which tests/test_iql_cpu.py ties to the real class through tests/golden/g7_iql.npz).

Parameters after an Adam step are NOT compared elementwise with the float64 run: at t = 1 the update is lr g / (|g| + eps), and where
|g| is near eps a relative gradient error of 1e-6 moves the parameter by a visible fraction of lr.  Three things are tested apart:
  (a) gradients: from zero moments the first step's exp_avg is (1 - beta1) g; per tensor max|g_dev - g64| / max|g64| is within 16 x what
      the reference's own float32 run loses on that tensor (golden ref32_grad_dev).  16: an MFMA chain sums K <= 256 fp32 terms one after
      the other where the CPU GEMM sums in blocks, a worst-case error ratio of about K / log2 K = 32 and typically far less; a wrong
      term shows at 1e-3 or more.
  (b) Adam, from the device's own moments: the parameter formula in float64 within 2 ulp, the moment recurrences within 4 ulp (a second
      step on the same batch with all rates 0 repeats the gradient bits), the soft update bit for bit.
  (c) the trajectory: 20 steps; losses relatively and final parameters absolutely within 16 x the float32 reference's deviation.
Cases (S, A, hidden, batch): (11, 3, 64, 37) a partial 32-row tile; (27, 8, 128, 33) S + A = 35, a second feature tile, one row past a
tile; (11, 3, 256, 1) a single row; (17, 6, 256, 256) the reference's own batch; (40, 6, 128, 33) states wider than one feature tile;
(32, 32, 64, 64) both input widths and the batch whole tiles, the widest actor, a log_std component below the lower clamp as well;
(11, 3, 64, 1024) the largest batch."""
import ctypes as C
import math
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import iql_ref as R
import replay_ref
from m3pc_amd import capi, checkpoint, synth
from m3pc_amd.iql import ACTOR_NAMES, QF_NAMES, VF_NAMES, DeviceIQL
from m3pc_amd.planner import HipPlanner
from m3pc_amd.replay import DeviceReplayBuffer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PART_CODES = {"qf": (capi.IQL_QF, capi.IQL_QF_ADAM_M, capi.IQL_QF_ADAM_V), "vf": (capi.IQL_VF, capi.IQL_VF_ADAM_M, capi.IQL_VF_ADAM_V),
              "actor": (capi.IQL_ACTOR, capi.IQL_ACTOR_ADAM_M, capi.IQL_ACTOR_ADAM_V)}
OMB1, B2, OMB2 = float(np.float32(1.0 - 0.9)), float(np.float32(0.999)), float(np.float32(1.0 - 0.999))  # the device's fp32 constants (iql.h)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "g7_iql.npz"))


def _handle(S, A, critic_hidden=0):
    if S > 32:
        return _stand_in_handle(S, A)
    return capi.Handle(S, A, 8, n_embd=64, n_head=2, max_candidates=64, critic_hidden=critic_hidden)


def _stand_in_handle(S, A):
    """m3pc_create takes state_dim <= 32; the trainer's own rule is S + A <= 64.  m3pc_iql_create reads the m3pc_dims a handle starts
    with and the device index behind them, and never refers to the handle again: this is what DeviceIQL needs of one."""
    torch.cuda.init()
    buf = C.create_string_buffer(256)
    C.memmove(buf, C.byref(capi.Dims(S, A, 8, 64, 2, 2, 1, 64, 1, 0, 64, 0)), C.sizeof(capi.Dims))
    return types.SimpleNamespace(lib=capi.load_library(), device=torch.device("cuda", 0), S=S, A=A, _h=C.c_void_p(C.addressof(buf)), _keep=buf)


def _trainer(case, handle=None):
    S, A, H, _ = R.CASES[case]
    hd = handle or _handle(S, A)
    hp = R.HP
    q = DeviceIQL(hd, H, v_lr=hp["v_lr"], critic_lr=hp["q_lr"], actor_lr=hp["actor_lr"], expectile=hp["expectile"], beta=hp["beta"],
                  discount=hp["discount"], tau=hp["tau"], max_steps=hp["max_steps"])
    state, om, os_ = R.make_state(case)
    q.load_part(capi.IQL_QF, state["qf"], om, os_)
    q.load_part(capi.IQL_Q_TARGET, state["q_target"])
    q.load_part(capi.IQL_VF, state["vf"])
    q.load_part(capi.IQL_ACTOR, state["actor"])
    return q


def _export(q):
    """Everything a trainer holds, as {"p/part/name" | "m/part/name" | "v/part/name": float32 array}."""
    out = {}
    for part, (cp, cm, cv) in PART_CODES.items():
        for tag, code in (("p", cp), ("m", cm), ("v", cv)):
            for k, t in q.export_part(code, part).items():
                out["%s/%s/%s" % (tag, part, k)] = t.cpu().numpy()
    for k, t in q.export_part(capi.IQL_Q_TARGET, "qf").items():
        out["p/q_target/" + k] = t.cpu().numpy()
    return out


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _same_state(x, y):
    assert x.keys() == y.keys()
    for k in x:
        assert _bits(x[k], y[k]), k


def _trajectory(case):
    q = _trainer(case)
    losses = [q.train(b) for b in R.make_batches(case)]
    losses = np.array([[float(l[k]) for k in ("value_loss", "q_loss", "actor_loss")] for l in losses], np.float32)
    out = _export(q)
    assert q.total_it == R.N_STEPS
    q.close()
    return losses, out


_CACHE = {}


def _device_run(case):
    """Per case, once: the state before and after the first step; the state after one and after two steps on that batch with every
    rate 0 (nothing moves, so both see the first step's parameters); and two independent 20-step trajectories."""
    if case not in _CACHE:
        b0 = R.make_batches(case, 1)[0]
        q = _trainer(case)
        before = _export(q)
        l1 = q.train(b0)
        after1 = _export(q)
        q.close()
        z = _trainer(case)
        zero = dict(v_lr=0.0, q_lr=0.0, actor_lr=0.0, tau=0.0)
        z1l = z.train(b0, **zero)
        zero1 = _export(z)
        z2l = z.train(b0, **zero)
        zero2 = _export(z)
        z.close()
        first = np.array([[float(l[k]) for k in ("value_loss", "q_loss", "actor_loss")] for l in (l1, z1l, z2l)], np.float32)
        _CACHE[case] = types.SimpleNamespace(before=before, after1=after1, zero1=zero1, zero2=zero2, first=first, traj=_trajectory(case),
                                             again=_trajectory(case), ref=R.run(case))
        print("\n%s: device deviation from float64" % case)
    return _CACHE[case]


@pytest.mark.parametrize("case", list(R.CASES))
def test_a_first_step_gradients(golden, case):
    run = _device_run(case)
    g64 = run.ref[2]
    names, tol = [str(n) for n in golden[case + "/grad_names"]], 16.0 * golden[case + "/ref32_grad_dev"]
    worst = 0.0
    for n, t in zip(names, tol):
        part, name = n.split("/")
        want = g64[part][name]
        got = run.after1["m/" + n].astype(np.float64).reshape(want.shape) / OMB1
        dev = np.abs(got - want).max() / np.abs(want).max() if np.abs(want).max() > 0 else np.abs(got).max()
        worst = max(worst, dev)
        print("  grad %-24s device %.2e  reference float32 %.2e" % (n, dev, t / 16.0))
        assert dev <= t, (n, dev, t)
    print("  %s: largest gradient deviation %.2e" % (case, worst))
    # a clamped component of log_std gets no gradient at all (component 0, above the clamp, in every case; component 2, below it, in a32)
    ls = run.before["p/actor/log_std"]
    out = (ls > R.LOG_STD_MAX) | (ls < R.LOG_STD_MIN)
    assert out[0] and out.sum() == (2 if case in R.LOG_STD_BELOW else 1) and (not out[2:].any() or ls[2] < R.LOG_STD_MIN)
    assert (run.after1["m/actor/log_std"][out] == 0.0).all() and (run.after1["v/actor/log_std"][out] == 0.0).all() and (run.after1["m/actor/log_std"][~out] != 0).all()


@pytest.mark.parametrize("case", list(R.CASES))
def test_b_adam_from_the_devices_own_moments(case):
    run = _device_run(case)
    hp, (S, A, H, B) = R.HP, R.CASES[case]
    bc1, bc2 = 1.0 - R.BETA1 ** 1, 1.0 - R.BETA2 ** 1
    lr = dict(vf=hp["v_lr"], qf=hp["q_lr"], actor=R.actor_lr(hp["actor_lr"], 0, hp["max_steps"]))
    for key in [k for k in run.before if k.startswith("p/") and not k.startswith("p/q_target")]:
        part, name = key.split("/")[1:]
        p, p1 = run.before[key].astype(np.float64), run.after1[key]
        m1, v1 = run.after1["m/%s/%s" % (part, name)].astype(np.float64), run.after1["v/%s/%s" % (part, name)].astype(np.float64)
        # the parameter formula in float64 from the exported fp32 moments.  The ulp is that of the larger of |p| and |p'|: where the
        # update is larger than the parameter, half an ulp of the RESULT is the best any fp32 store can do
        want = p - (lr[part] / bc1) * m1 / (np.sqrt(v1) / math.sqrt(bc2) + R.EPS)
        ulp = np.maximum(R.ulp(p), R.ulp(p1))
        assert (np.abs(p1.astype(np.float64) - want) <= 2.0 * ulp).all(), (key, (np.abs(p1 - want) / ulp).max())
        # the moment recurrences, on the steps with all rates 0: nothing moves, so the second step repeats the gradient bits of the
        # first, g = m' / (1 - beta1) -- which are also the bits of the ordinary first step
        z1m, z1v = run.zero1["m/%s/%s" % (part, name)], run.zero1["v/%s/%s" % (part, name)]
        assert _bits(z1m, run.after1["m/%s/%s" % (part, name)]) and _bits(z1v, run.after1["v/%s/%s" % (part, name)]), key
        assert _bits(run.zero1[key], run.before[key]) and _bits(run.zero2[key], run.before[key]), key
        g = m1 / OMB1
        m2, v2 = run.zero2["m/%s/%s" % (part, name)], run.zero2["v/%s/%s" % (part, name)]
        want_m, want_v = m1 + OMB1 * (g - m1), B2 * v1 + OMB2 * g * g
        assert (np.abs(m2 - want_m) <= 4.0 * R.ulp(want_m)).all(), (key, (np.abs(m2 - want_m) / R.ulp(want_m)).max())
        assert (np.abs(v2 - want_v) <= 4.0 * R.ulp(want_v)).all(), (key, (np.abs(v2 - want_v) / R.ulp(want_v)).max())
    assert _bits(run.first[0], run.first[1]) and _bits(run.first[1], run.first[2])   # the losses repeat
    tau = hp["tau"]
    omt, tf = np.float32(1.0 - tau), np.float32(tau)
    for name in QF_NAMES:
        want = omt * run.before["p/q_target/" + name] + tf * run.after1["p/qf/" + name]   # fp32: two products, one sum
        assert want.dtype == np.float32 and _bits(run.after1["p/q_target/" + name], want), name
        assert _bits(run.zero2["p/q_target/" + name], run.before["p/q_target/" + name]), name   # tau 0


@pytest.mark.parametrize("case", list(R.CASES))
def test_c_twenty_steps_follow_the_float64_run(golden, case):
    """Measured on an MI355X.  Losses, largest relative deviation over the 20 steps (reference float32 in brackets): h64 7.2e-7 / 8.4e-7 /
    1.4e-6 (8.3e-7 / 7.5e-7 / 1.3e-6); h128 8.5e-7 / 4.0e-7 / 1.4e-6 (7.9e-7 / 3.3e-7 / 1.0e-6); h256_1 6.3e-6 / 6.8e-6 / 3.1e-6 (3.4e-5 /
    3.3e-6 / 3.1e-6); h256 2.3e-6 / 1.9e-6 / 4.2e-6 (2.2e-6 / 1.9e-6 / 4.1e-6).  Final parameters, largest absolute deviation: h64 3.1e-7,
    h128 2.3e-7, h256_1 2.5e-7, h256 3.1e-6 (3.4e-7, 2.3e-7, 2.4e-7, 6.3e-7).  The recipes keep every pre-activation of all 20 steps 1e-4
    from zero (iql_ref.make_batches): one ReLU that float32 puts on the other side moves a row of weights by 0.1 lr per step.
    s40: losses 5.8e-7 / 4.2e-7 / 2.0e-6 (5.4e-7 / 4.2e-7 / 1.8e-6), parameters 1.3e-6 (5.7e-7) -- one element of v.net.2.weight whose
    first gradient is -3.405e-9 in float64 and -3.481e-9 on the device: lr g / (|g| + eps) moves it by 0.004 lr in the first step."""
    run = _device_run(case)
    ref, l64, _ = run.ref
    losses, state = run.traj
    dev = (np.abs(losses.astype(np.float64) - l64) / np.abs(l64)).max(0)
    tol = 16.0 * golden[case + "/ref32_loss_dev"]
    print("  %s: loss deviation %s (reference float32 %s)" % (case, dev, tol / 16.0))
    assert (dev <= tol).all(), (dev, tol)
    # the bound of the parameters is the case's, not the tensor's: which tensor holds an element whose first gradients lie near
    # Adam's eps, where lr g / (|g| + eps) turns a gradient error of 1e-10 into 0.01 lr (the module docstring), differs between two
    # float32 evaluations, and a tensor without one deviates by its roundings alone (6e-8)
    worst, t = 0.0, 16.0 * float(golden[case + "/ref32_traj_dev"])
    for n in [str(n) for n in golden[case + "/param_names"]]:
        part, name = n.split("/")
        want = ref.p[part][name]
        d = np.abs(state["p/" + n].astype(np.float64).reshape(want.shape) - want).max()
        worst = max(worst, d)
        assert d <= t, (n, d, t)
    print("  %s: largest parameter deviation after 20 steps %.2e" % (case, worst))


@pytest.mark.parametrize("case", list(R.CASES))
def test_two_runs_give_the_same_bits(case):
    run = _device_run(case)
    assert _bits(run.traj[0], run.again[0])
    _same_state(run.traj[1], run.again[1])
    assert np.isfinite(run.traj[0]).all()


EVAL_ROWS = {"h64": (1024, 1025, 2049), "h256": (1030,)}   # (the other cases: their own batch)


@pytest.mark.parametrize("case", ["h64", "h128", "h256", "s40"])
def test_evaluate_against_the_restatement(case):
    """Q_MIN, Q_TARGET_MIN, V and ACTOR_MEAN at the loaded weights; at hidden 64 on exactly one pass of rows (1024), one row more and
    two passes and a row (2049), at hidden 256 on 1030 rows (the second pass takes 6).  Tolerance: three layers of fp32 sums of at most
    256 terms, each off by at most K 2^-24 of the sum of its terms' magnitudes -- 2e-5 of the largest output."""
    S, A, H, B = R.CASES[case]
    q = _trainer(case)
    state, om, os_ = R.make_state(case)
    ref = R.RefIQL(state, om, os_)
    most = max(EVAL_ROWS.get(case, (B,)))
    bs = R.make_batches(case, 1)
    rng = np.random.RandomState(17)
    reps = (most + B - 1) // B    # the recipe's rows, jittered: every row its own
    s_all = (np.concatenate([bs[0][0]] * reps) + rng.normal(size=(reps * B, S)) * 0.1).astype(np.float32)
    a_all = np.clip(np.concatenate([bs[0][1]] * reps) + rng.normal(size=(reps * B, A)) * 0.05, -1, 1).astype(np.float32)
    for rows in EVAL_ROWS.get(case, (B,)):
        s, a = s_all[:rows], a_all[:rows]
        s64, a64 = s.astype(np.float64), a.astype(np.float64)
        for which, want in ((capi.IQL_Q_MIN, ref.q_min("qf", s64, a64)), (capi.IQL_Q_TARGET_MIN, ref.q_min("q_target", s64, a64)),
                            (capi.IQL_V, ref.value(s64)), (capi.IQL_ACTOR_MEAN, ref.actor_mean(s64))):
            got = q.evaluate(which, torch.from_numpy(s), None if which in (capi.IQL_V, capi.IQL_ACTOR_MEAN) else torch.from_numpy(a)).cpu().numpy()
            assert got.shape == want.shape and np.abs(got - want).max() <= 2e-5 * max(1.0, np.abs(want).max()), (rows, which, np.abs(got - want).max())
    assert np.allclose(q.act(s_all[0]), np.clip(ref.actor_mean(s_all[:1].astype(np.float64))[0], -1, 1), atol=2e-5)
    q.close()


def _planner(case, max_batch=1, max_windows=1, **cfg_over):
    S, A, H, _ = R.CASES[case]
    T = 8
    cfg = dict(traj_length=T, action_samples=64, horizon=4, discount=0.99, temperature=0.01, lmbda=0.6, plan_guidance="critic_lambda_guiding",
               device="cuda", index_jump=4, traj_batch_size=4, traj_buffer_size=4, trans_batch_size=6, trans_buffer_size=64, select_mode="prob",
               mtm_iter_per_rollout=2, using_online_threshold=4)
    cfg.update(cfg_over)
    dims = synth.Dims(S, A, T, n_embd=64, n_head=2)
    state, om, os_ = R.make_state(case)
    q_sd = {k: torch.from_numpy(v) for k, v in state["qf"].items()}
    p = HipPlanner(types.SimpleNamespace(**cfg), synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), q_sd, om, os_, n_embd=64,
                   n_head=2, precision="fp32", generator=torch.Generator(device="cuda").manual_seed(11), max_batch=max_batch, max_windows=max_windows)
    return p, dims


@pytest.mark.parametrize("case", ["h64", "h128", "h256_1"])
def test_publish_is_the_host_route(case):
    """A critic-guided fp32 plan step after m3pc_iql_publish_critic, and after m3pc_set_critic with the exported qf: every output bit
    for bit (pred_boot is min(q1, q2) itself).  hidden 64 with S + A = 14: the MFMA critic, so the packed operand streams are compared
    through their only reader; hidden 128 with S + A = 35, which critic_mfma_covers does not cover: the scalar critic kernel, the only
    reader of the transposed copies; hidden 256 with S + A = 14: the MFMA critic again, with streams long enough (289308 elements
    in all) that the grid-stride loop of iql_publish_kernel runs."""
    S, A, H, _ = R.CASES[case]
    p, dims = _planner(case)
    q = _trainer(case, p.handle)
    for b in R.make_batches(case, 3):
        q.train(b)
    hist = synth.make_history(dims, 0)
    hist["path_length"] = 500
    s, a, r, h, rtg = p.assemble_window(hist, rtg=3.0)
    eps = synth.make_eps(64, dims, 1).cuda().reshape(64, -1, A)

    def step():
        res = p.handle.plan_step(capi.MODE_CRITIC, s, a, r, eps, h, rtg, 0.6, 0.99, 64, 0, 64, want_debug=True)
        return {k: v.cpu().numpy() for k, v in res.items()}

    before = step()                                   # the critic the planner was built with: the initial qf
    q.publish(p)
    published = step()
    _, om, os_ = R.make_state(case)
    p.handle.set_critic(q.export_part(capi.IQL_QF, "qf"), om, os_)
    hosted = step()
    for k in hosted:
        assert _bits(published[k], hosted[k]), k
    assert not _bits(before["expect_return"], published["expect_return"])   # three steps moved the critic
    assert np.isfinite(published["expect_return"]).all()
    q.close()
    p.handle.close()


@pytest.mark.parametrize("k", [500, 1000, 1500])
def test_adam_from_loaded_moments_at_a_late_step(k):
    """The ADAM_M / ADAM_V parts loaded, set_step(k) with actor_t_max = 1000, one step: the moments move by the recurrences, every
    parameter is the formula in float64 from the exported moments (2 ulp of the larger of |p| and |p'|, as in
    test_b_adam_from_the_devices_own_moments) with bias corrections of step k + 1 and, for the actor, the cosine rate at k -- half the
    rate at 500, EXACTLY 0 at 1000 (cos(pi) = -1 in double: the actor's parameters keep their bits, its moments move), and the rate on
    the way back up at 1500."""
    case = "h64"
    q = _trainer(case)
    hp = R.HP
    assert q.max_steps == 1000 == hp["max_steps"]
    rng = np.random.RandomState(100 + k)
    loaded = {}
    for part, (cp, cm, cv) in PART_CODES.items():
        shapes = q.shapes(part)
        m = {n: (rng.normal(size=sh) * 0.05).astype(np.float32) for n, sh in shapes.items()}
        v = {n: (rng.uniform(size=sh) * 0.01).astype(np.float32) for n, sh in shapes.items()}
        q.load_part(cm, m)
        q.load_part(cv, v)
        loaded[part] = (m, v)
    q.total_it = k
    before = _export(q)
    zero1 = _device_run(case).zero1      # exp_avg = (1 - b1) g of the same weights and batch, from zero moments
    for part, (m, v) in loaded.items():
        for n in m:
            assert _bits(before["m/%s/%s" % (part, n)], m[n]) and _bits(before["v/%s/%s" % (part, n)], v[n]), (part, n)
    q.train(R.make_batches(case, 1)[0])
    after = _export(q)
    assert q.total_it == k + 1
    t = k + 1
    bc1, bc2 = 1.0 - R.BETA1 ** t, 1.0 - R.BETA2 ** t
    alr = R.actor_lr(hp["actor_lr"], k, 1000)
    assert (alr == 0.0) == (k == 1000) and (k != 500 or abs(alr - hp["actor_lr"] / 2) < 1e-18) and (k != 1500 or abs(alr - hp["actor_lr"] / 2) < 1e-18)
    lr = dict(vf=hp["v_lr"], qf=hp["q_lr"], actor=alr)
    for key in [x for x in before if x.startswith("p/") and not x.startswith("p/q_target")]:
        part, name = key.split("/")[1:]
        p, p1 = before[key].astype(np.float64), after[key]
        m0, v0 = before["m/%s/%s" % (part, name)], before["v/%s/%s" % (part, name)]
        m1, v1 = after["m/%s/%s" % (part, name)], after["v/%s/%s" % (part, name)]
        assert not _bits(m0, m1) and not _bits(v0, v1), key
        # the recurrences from the loaded moments: the gradient is the one of the first step from zero moments (the same weights and
        # batch), g = exp_avg / (1 - b1) to one rounding.  Three fp32 roundings each, of operands no larger than `mag`, and g's own
        m064, v064 = m0.astype(np.float64), v0.astype(np.float64)
        g = zero1["m/%s/%s" % (part, name)].astype(np.float64) / OMB1
        want_m, want_v = m064 + OMB1 * (g - m064), B2 * v064 + OMB2 * g * g
        mag = np.abs(m064) + OMB1 * (np.abs(g) + np.abs(m064))
        assert (np.abs(m1 - want_m) <= 4.0 * R.ulp(mag)).all(), (key, (np.abs(m1 - want_m) / R.ulp(mag)).max())
        assert (np.abs(v1 - want_v) <= 4.0 * R.ulp(want_v)).all(), (key, (np.abs(v1 - want_v) / R.ulp(want_v)).max())
        want = p - (lr[part] / bc1) * m1.astype(np.float64) / (np.sqrt(v1.astype(np.float64)) / math.sqrt(bc2) + R.EPS)
        ulp = np.maximum(R.ulp(p), R.ulp(p1))
        assert (np.abs(p1.astype(np.float64) - want) <= 2.0 * ulp).all(), (key, (np.abs(p1 - want) / ulp).max())
        if part == "actor" and k == 1000:
            assert _bits(p1, before[key]), key
        elif name != "log_std":
            assert not _bits(p1, before[key]), key
    q.close()


@pytest.mark.parametrize("threshold", [1000, 4])
def test_train_from_a_replay_buffer_is_sample_then_step(threshold):
    """m3pc_iql_train over a DeviceReplayBuffer (offline 37, online 64; n_online 0 and batch // 2) for 5 steps against the loop of
    trans_sample + train: exported state and losses bit for bit."""
    case = "h64"
    S, A, H, _ = R.CASES[case]
    hd = _handle(S, A)
    cfg = types.SimpleNamespace(traj_length=8, traj_batch_size=4, traj_buffer_size=4, trans_batch_size=8, trans_buffer_size=64, select_mode="uniform",
                                mtm_iter_per_rollout=1, using_online_threshold=threshold)
    buf = DeviceReplayBuffer(hd, cfg, 0, 16, seed=5, offline_capacity=37, online_capacity=64)
    rng = np.random.RandomState(9)
    for n, online in ((37, False), (64, True)):
        buf.append_transitions(rng.normal(size=(n, S)).astype(np.float32), rng.uniform(-1, 1, size=(n, A)).astype(np.float32),
                               rng.normal(size=(n,)).astype(np.float32), rng.normal(size=(n, S)).astype(np.float32),
                               (rng.uniform(size=(n,)) < 0.2).astype(np.float32), online=online)
    assert buf.split() == ((0, 8) if threshold == 1000 else (4, 4))
    step0 = buf.step
    qa, qb = _trainer(case, hd), _trainer(case, hd)
    la = []
    for _ in range(5):
        batch, idx = buf.trans_sample(return_indices=True)
        assert idx.shape == (8,)
        l = qa.train(batch)
        la.append(torch.stack([l["value_loss"], l["q_loss"], l["actor_loss"]]))
    assert buf.step == step0 + 5
    buf.step = step0
    lb = qb.train_from(buf, 5)
    assert buf.step == step0 + 5 and qb.total_it == 5 == qa.total_it
    assert _bits(torch.stack(la).cpu().numpy(), lb.cpu().numpy()) and np.isfinite(lb.cpu().numpy()).all()
    _same_state(_export(qa), _export(qb))
    for q in (qa, qb):
        q.close()
    buf.close()
    hd.close()


class _MLP(torch.nn.Module):
    def __init__(self, i, h, o):
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.Linear(i, h), torch.nn.ReLU(), torch.nn.Linear(h, h), torch.nn.ReLU(), torch.nn.Linear(h, o))


class _TwinQ(torch.nn.Module):
    def __init__(self, S, A, H):
        super().__init__()
        self.q1, self.q2 = _MLP(S + A, H, 1), _MLP(S + A, H, 1)


def test_state_dict_round_trip(tmp_path):
    """state_dict() -> torch.save -> torch.load -> load_state_dict() -> one more step: the bits of not having round-tripped (with
    q_target = qf on both sides, as the reference's load_state_dict leaves it); the file is an iql_{step}.pt checkpoint.load_iql_qf
    reads, and its parts load into a TwinQ-shaped module and its torch.optim.Adam."""
    case = "h64"
    S, A, H, _ = R.CASES[case]
    hd = _handle(S, A)
    bs = R.make_batches(case, 4)
    qa = _trainer(case, hd)
    for b in bs[:3]:
        qa.train(b)
    path = str(tmp_path / "iql_3.pt")
    torch.save(qa.state_dict(), path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert list(sd) == ["qf", "q_optimizer", "vf", "v_optimizer", "actor", "actor_optimizer", "actor_lr_schedule", "total_it"] and sd["total_it"] == 3
    assert list(sd["qf"]) == list(QF_NAMES) and list(sd["vf"]) == list(VF_NAMES) and list(sd["actor"]) == list(ACTOR_NAMES)
    _, om, os_ = R.make_state(case)
    qb = DeviceIQL(hd, H)
    qb.load_state_dict(sd, om, os_)
    assert qb.total_it == 3 and qb.max_steps == R.HP["max_steps"] and qb.actor_lr == R.HP["actor_lr"] and qb.critic_lr == R.HP["q_lr"]
    qb.expectile, qb.beta, qb.discount, qb.tau = (R.HP[k] for k in ("expectile", "beta", "discount", "tau"))
    qa.load_part(capi.IQL_Q_TARGET, qa.export_part(capi.IQL_QF, "qf"))   # model.py:325
    la, lb = qa.train(bs[3]), qb.train(bs[3])
    for k in la:
        assert _bits(la[k].cpu().numpy(), lb[k].cpu().numpy()), k
    _same_state(_export(qa), _export(qb))
    # the reference's shapes
    qf = checkpoint.load_iql_qf(path)
    assert list(qf) == list(QF_NAMES)
    twin = _TwinQ(S, A, H)
    twin.load_state_dict(sd["qf"])
    opt = torch.optim.Adam(twin.parameters(), lr=1.0)
    opt.load_state_dict(sd["q_optimizer"])
    params = dict(twin.named_parameters())
    for j, n in enumerate(QF_NAMES):
        st = opt.state[params[n]]
        assert float(st["step"]) == 3.0 and st["exp_avg"].shape == params[n].shape and torch.equal(st["exp_avg_sq"], sd["q_optimizer"]["state"][j]["exp_avg_sq"])
    assert opt.param_groups[0]["lr"] == R.HP["q_lr"] and opt.param_groups[0]["betas"] == (0.9, 0.999)
    assert abs(sd["actor_optimizer"]["param_groups"][0]["lr"] - R.actor_lr(R.HP["actor_lr"], 3, R.HP["max_steps"])) < 1e-18
    for q in (qa, qb):
        q.close()
    hd.close()


class _Actor(torch.nn.Module):
    def __init__(self, S, A, H):
        super().__init__()
        self.log_std = torch.nn.Parameter(torch.zeros(A))
        self.net = _MLP(S, H, A)


class _V(torch.nn.Module):
    def __init__(self, S, H):
        super().__init__()
        self.v = _MLP(S, H, 1)


class _LiveIQL:
    """What from_iql reads of an ImplicitQLearning (model.py:194-226, :310-320), with real torch optimizers that have made two steps."""

    def __init__(self, S, A, H, om, os_):
        torch.manual_seed(5)
        self.qf, self.q_target, self.vf, self.actor = _TwinQ(S, A, H), _TwinQ(S, A, H), _V(S, H), _Actor(S, A, H)
        self.qf.obs_mean, self.qf.obs_std = torch.from_numpy(om), torch.from_numpy(os_)
        self.q_optimizer = torch.optim.Adam(self.qf.parameters(), lr=2e-4)
        self.v_optimizer = torch.optim.Adam(self.vf.parameters(), lr=4e-4)
        self.actor_optimizer = torch.optim.Adam(self.actor.parameters(), lr=5e-4)
        self.actor_lr_schedule = torch.optim.lr_scheduler.CosineAnnealingLR(self.actor_optimizer, 50)
        self.iql_tau, self.beta, self.discount, self.tau, self.total_it = 0.8, 2.0, 0.98, 0.01, 0
        for _ in range(2):
            for net, opt in ((self.qf, self.q_optimizer), (self.vf, self.v_optimizer), (self.actor, self.actor_optimizer)):
                for prm in net.parameters():
                    prm.grad = torch.randn_like(prm)
                opt.step()
            self.actor_lr_schedule.step()
            self.total_it += 1

    def state_dict(self):
        return {"qf": self.qf.state_dict(), "q_optimizer": self.q_optimizer.state_dict(), "vf": self.vf.state_dict(),
                "v_optimizer": self.v_optimizer.state_dict(), "actor": self.actor.state_dict(), "actor_optimizer": self.actor_optimizer.state_dict(),
                "actor_lr_schedule": self.actor_lr_schedule.state_dict(), "total_it": self.total_it}


def test_from_iql_reads_a_live_learner():
    """DeviceIQL.from_iql: the networks, the live q_target, the three optimizers' moments and rates, the schedule and total_it of an
    ImplicitQLearning-shaped object with real torch.optim.Adam state; a checkpoint with another Adam than the default is refused."""
    case = "h64"
    S, A, H, _ = R.CASES[case]
    _, om, os_ = R.make_state(case)
    live = _LiveIQL(S, A, H, om, os_)
    hd = _handle(S, A)
    q = DeviceIQL.from_iql(hd, live)
    assert q.hidden == H and q.total_it == 2 and q.max_steps == 50
    assert (q.critic_lr, q.v_lr, q.actor_lr) == (2e-4, 4e-4, 5e-4) and (q.expectile, q.beta, q.discount, q.tau) == (0.8, 2.0, 0.98, 0.01)
    assert abs(q.actor_lr_at(2) - live.actor_optimizer.param_groups[0]["lr"]) <= 1e-12 * 5e-4
    got = _export(q)
    for part, net, opt in (("qf", live.qf, live.q_optimizer), ("vf", live.vf, live.v_optimizer), ("actor", live.actor, live.actor_optimizer)):
        for name, prm in net.named_parameters():
            assert _bits(got["p/%s/%s" % (part, name)], prm.detach().numpy()), (part, name)
            assert _bits(got["m/%s/%s" % (part, name)], opt.state[prm]["exp_avg"].numpy()), (part, name)
            assert _bits(got["v/%s/%s" % (part, name)], opt.state[prm]["exp_avg_sq"].numpy()), (part, name)
    for name, prm in live.q_target.named_parameters():
        assert _bits(got["p/q_target/" + name], prm.detach().numpy()), name      # (the live target, not a copy of qf)
    assert torch.equal(q.obs_mean, torch.from_numpy(om)) and torch.equal(q.obs_std, torch.from_numpy(os_))
    sd = live.state_dict()
    sd["q_optimizer"]["param_groups"][0]["betas"] = (0.8, 0.999)
    with pytest.raises(ValueError, match="defaults"):
        DeviceIQL(hd, H).load_state_dict(sd, om, os_)
    q.close()
    hd.close()


def test_the_closed_loop_runs():
    """Rollout into a store, push to the replay buffer, train_from, publish, a second rollout -- at toy size, with finite values."""
    from fake_learner import ToyEnv

    case = "h64"
    S, A, H, _ = R.CASES[case]
    Msteps = 12
    p, dims = _planner(case, max_batch=3, max_windows=3)
    rng = np.random.RandomState(3)
    cfg = types.SimpleNamespace(traj_length=8, traj_batch_size=4, traj_buffer_size=4, trans_batch_size=6, trans_buffer_size=64, select_mode="prob",
                                mtm_iter_per_rollout=2, using_online_threshold=4)
    buf = DeviceReplayBuffer(p, cfg, 4, Msteps, discount=0.99)
    for n in (9, 12):
        obs, act, rew = np.zeros((Msteps, S), np.float32), np.zeros((Msteps, A), np.float32), np.zeros((Msteps, 1), np.float32)
        obs[:n], act[:n], rew[:n, 0] = rng.normal(size=(n, S)), rng.uniform(-1, 1, size=(n, A)), rng.normal(size=(n,))
        buf.update_buffer([{"observations": obs, "actions": act, "rewards": rew, "values": replay_ref.online_values(rew[:, 0], 0.99)[:, None],
                            "path_length": n}])
    buf.append_transitions(*[rng.normal(size=(5,) + w).astype(np.float32) for w in ((S,), (A,), (), (S,), ())], online=False)
    lengths = [7, 12, 10]
    out1 = buf.online_rollout(p, [ToyEnv(S, A, i, length=lengths[i]) for i in range(3)])
    assert out1["plan_steps"] == sum(lengths) and buf.counts()[2] == sum(lengths)
    q = _trainer(case, p.handle)
    losses = q.train_from(buf, 4)
    q.publish(p)
    out2 = buf.online_rollout(p, [ToyEnv(S, A, i + 3, length=lengths[i]) for i in range(3)])
    torch.cuda.synchronize()
    assert losses.shape == (4, 3) and torch.isfinite(losses).all() and q.total_it == 4
    assert out2["plan_steps"] == sum(lengths) and buf.counts()[2] == 2 * sum(lengths)
    for tr in out2["trajectories"]:
        assert np.isfinite(tr["actions"]).all() and np.isfinite(tr["rewards"]).all()
    q.close()
    buf.close()
    p.handle.close()


def test_critic_loop_example(tmp_path):
    """examples/critic_loop.c compiled with gcc -Wall -Werror against include/m3pc_hip.h, linked to the built library and run: five steps
    from the buffer its rollout filled, finite losses, the published critic evaluated."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = tmp_path / "critic_loop"
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "examples", "critic_loop.c"), "-o", str(exe), "-L", libdir, "-l:" + os.path.basename(capi.LIB_PATH),
                           "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.join(rocm, "lib")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "online 40 total_it 5", lines[0]
    steps = [ln.split() for ln in lines if ln.startswith("step ")]
    assert len(steps) == 5 and all(np.isfinite([float(s[3]), float(s[5]), float(s[7])]).all() for s in steps)
    qmin = [float(x) for x in lines[-1].split()[1:]]
    assert lines[-1].startswith("q_min") and len(qmin) == 4 and np.isfinite(qmin).all()
