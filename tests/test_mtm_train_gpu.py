"""Training the masked-trajectory model on the device (m3pc_mtm_opt_*, m3pc_mtm_train*, DeviceMTMTrainer) on the g1_tiny sizes of the
g8 / g9 goldens (S 11, A 3, T 8, d 64, 2 heads; the g8 batch under its mask case c2).

No test compares updated weights elementwise across two gradient arithmetics: where a gradient is below the gradient arithmetic's
noise (the K-bias third of every in_proj_bias is analytically zero) Adam normalises rounding noise to +-lr.  The chain is (1) the
device gradient against float64 (tests/test_mtm_grad_gpu.py) and (2) here, the device optimizer on the device's OWN exported gradient
against the float64 restatement tests/mtm_opt_ref.py, within the per-element bound derived there."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import mtm_grad_cases as MC
import mtm_loss_ref as R
import mtm_opt_ref as OR
from m3pc_amd import capi, synth
from m3pc_amd.mtm_train import EXP_AVG, EXP_AVG_SQ, DeviceMTMTrainer
from m3pc_amd.planner import HipPlanner
from test_mtm_loss_gpu import _filled_buffer

pytestmark = pytest.mark.gpu
S, A, T, B = 11, 3, 8, 3
DIMS = synth.Dims(S, A, T, n_embd=64, n_head=2)
FINETUNE_BITS = 0b0001  # loss_keys of the fine-tuning form: states (m3pc_amd.mtm.form_settings("finetune"))
HYPER = dict(learning_rate=1e-3, weight_decay=5e-3, num_train_steps=10, target_entropy=-3.0, init_log_temperature=math.log(0.1))
ESTATE, EINVAL = -2, -1


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir + "/g8_mtm_loss.npz")


@pytest.fixture(scope="module")
def g10(golden_dir):
    return np.load(golden_dir + "/g10_mtm_train.npz")


def _cfg(golden, traj_length=T):
    return types.SimpleNamespace(traj_length=traj_length, action_samples=64, horizon=4, discount=0.99, temperature=0.01, lmbda=0.6,
                                 plan_guidance="rtg_guiding", device="cuda", index_jump=4, traj_batch_size=B, traj_buffer_size=4, trans_batch_size=6,
                                 trans_buffer_size=64, select_mode="prob", mtm_iter_per_rollout=2, using_online_threshold=4,
                                 mask_ratio=tuple(golden["mask_ratio"].tolist()), p_weights=tuple(golden["p_weights"].tolist()))


@pytest.fixture(scope="module")
def sd():
    return synth.make_state_dict(DIMS, 0)


@pytest.fixture(scope="module")
def planner(golden, sd):
    p = HipPlanner(_cfg(golden), sd, synth.make_tokenizer_stats(DIMS, 0), None, n_embd=64, n_head=2, precision="fp32",
                   generator=torch.Generator(device="cuda").manual_seed(11), max_batch=4, max_windows=1)
    yield p
    torch.cuda.synchronize()
    p.handle.close()


@pytest.fixture
def fresh(planner, sd):
    """-> make(): a new trainer on the planner with the recipe weights loaded; all of them are closed afterwards."""
    made = []

    def make(max_batch=4, **kw):
        torch.cuda.synchronize()
        planner.load_state_dict(sd)
        tr = DeviceMTMTrainer(planner, max_batch, **{**HYPER, **kw})
        made.append(tr)
        return tr

    yield make
    torch.cuda.synchronize()
    for tr in made:
        tr.close()
    planner.load_state_dict(sd)


def _g8(golden, case="c2"):
    batch = {k: torch.from_numpy(golden["batch/" + k]).cuda() for k in R.KEYS}
    masks = {k: golden[f"{case}/mask/{k}"] for k in R.KEYS}
    return batch, masks, torch.from_numpy(golden[f"{case}/eps"]).cuda()


def _np(d):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in d.items()}


def _snapshot(tr):
    """Everything a step can move, as host arrays / bit strings."""
    w, (m, steps), v = tr.export_weights(), tr.export_moments(EXP_AVG, steps=True), tr.export_moments(EXP_AVG_SQ)
    torch.cuda.synchronize()
    return dict(w={k: t.cpu().numpy() for k, t in w.items()}, m={k: t.cpu().numpy() for k, t in m.items()},
                v={k: t.cpu().numpy() for k, t in v.items()}, steps=steps, state=tr.get_state())


def _same_bits(a, b, what):
    for part in ("w", "m", "v"):
        for n in a[part]:
            assert a[part][n].tobytes() == b[part][n].tobytes(), (what, part, n)
    assert a["steps"] == b["steps"], what
    assert a["state"] == b["state"], (what, a["state"], b["state"])


def _check_step(before, after, grads, entropy, loss_bits, what, hyper=HYPER):
    """One device step against the restatement started from the device's own exported state.  -> worst err / bound."""
    k = before["state"]["sched_step"]
    lr_t = OR.lr_at(k, hyper["learning_rate"], hyper["num_train_steps"])
    out = OR.adamw(before["w"], grads, before["m"], before["v"], before["steps"], lr_t, hyper["weight_decay"], loss_bits)
    worst = 0.0
    for n, (pr, mr, vr, st, bp, bm, bv) in out.items():
        assert after["steps"][n] == st, (what, n, after["steps"][n], st)
        if not OR.active(n, loss_bits):
            for part in ("w", "m", "v"):
                assert after[part][n].tobytes() == before[part][n].tobytes(), (what, "inactive", part, n)
            continue
        for part, ref, bound in (("w", pr, bp), ("m", mr, bm), ("v", vr, bv)):
            w = OR.worst(after[part][n], ref, bound)
            worst = max(worst, w)
            assert w <= 1.0, (what, n, part, w)
    s0, s1 = before["state"], after["state"]
    lt, tm, tv, ts, tb = OR.temperature_step(s0["log_temperature"], s0["temp_exp_avg"], s0["temp_exp_avg_sq"], s0["temp_step"], entropy,
                                             hyper["target_entropy"])
    assert s1["sched_step"] == k + 1 and s1["temp_step"] == ts
    assert abs(s1["log_temperature"] - lt) <= tb, (what, s1["log_temperature"], lt, tb)
    assert abs(s1["temp_exp_avg"] - tm) <= 64 * OR.D * abs(tm) and abs(s1["temp_exp_avg_sq"] - tv) <= 64 * OR.D * abs(tv)
    assert abs(s1["temperature"] / math.exp(s1["log_temperature"]) - 1) <= 2.0 ** -23  # (the float the next gradient call reads)
    return worst, lr_t


# ------------------------------------------------------------------------------------------------ (a)
def test_four_optimizer_steps_on_the_devices_own_gradient(golden, fresh):
    tr = fresh()
    batch, masks, eps = _g8(golden)
    names = list(tr.shapes)
    assert len(names) == 90 and sum(tr.decays(n) for n in names) == 28
    for k in range(4):
        before = _snapshot(tr)
        assert abs(tr.lr(k) - OR.lr_at(k, HYPER["learning_rate"], HYPER["num_train_steps"])) <= np.spacing(tr.lr(k))
        rec = tr.grad.grad_record(batch, masks, before["state"]["temperature"], "finetune", eps)
        grads = _np(tr.grad.export())
        tr.opt_step()
        after = _snapshot(tr)
        assert not grads["output_head_dict.rewards.1.weight"].any() and grads["encoder.layers.0.linear1.weight"].any()
        worst, lr_t = _check_step(before, after, grads, float(rec.cpu()[12]), FINETUNE_BITS, f"step {k}")
        moved = max(float(np.abs(after["w"][n] - before["w"][n]).max()) for n in names)
        print(f"step {k}: lr {lr_t:.10e}  temperature {after['state']['temperature']:.9e}  worst err / bound {worst:.3f}  largest move {moved:.2e}")
        assert moved > 1e-5
        assert after["steps"]["output_head_dict.returns.3.bias"] == 0 and after["steps"]["mask_token_dict.rewards"] == k + 1


# ------------------------------------------------------------------------------------------------ (b)
def test_train_step_is_grad_then_opt_step(golden, fresh):
    batch, masks, eps = _g8(golden)
    tr = fresh()
    recs = [tr.train_step_record(batch, masks, eps) for _ in range(2)]
    one = _snapshot(tr)
    recs = [(r.cpu().numpy(), t.cpu().numpy()) for r, t in recs]
    tr2 = fresh()
    for k in range(2):
        temp = tr2.get_state()["temperature"]
        rec = tr2.grad.grad_record(batch, masks, temp, "finetune", eps)
        tr2.opt_step()
        st = tr2.get_state()
        assert rec.cpu().numpy().tobytes() == recs[k][0].tobytes(), k
        assert recs[k][1][0] == tr2.lr(k) and recs[k][1][2] == st["log_temperature"] and float(np.float32(recs[k][1][1])) == st["temperature"]
    _same_bits(one, _snapshot(tr2), "train_step vs grad + opt_step")


def test_train_is_n_single_calls(golden, planner, fresh):
    masks = {k: torch.from_numpy(golden[f"c2/mask/{k}"].astype(np.float64)) for k in R.KEYS}
    other = {k: torch.from_numpy(golden[f"c0/mask/{k}"].astype(np.float64)) for k in R.KEYS}
    per_step = [masks, other, masks]
    buf, _ = _filled_buffer(planner)
    try:
        tr = fresh()
        step0 = buf.step
        recs, trecs = buf.mtm_train(tr, 3, per_step, batch_size=B)
        assert buf.step == step0 + 3
        many = _snapshot(tr)
        recs, trecs = recs.cpu().numpy(), trecs.cpu().numpy()
        assert np.isfinite(recs[:, 14]).all()
        # the plan path sees the trained weights: the bf16 copies behind the last step are those of a load of the exported weights
        tr2 = fresh()
        buf.step = step0
        for i in range(3):
            temp = tr2.get_state()["temperature"]
            rec = buf.mtm_grad(tr2.grad, per_step[i], temp, batch_size=B)
            tr2.opt_step()
            assert rec.cpu().numpy().tobytes() == recs[i].tobytes(), i
            st = tr2.get_state()
            assert trecs[i][0] == tr2.lr(i) and trecs[i][2] == st["log_temperature"]
        _same_bits(many, _snapshot(tr2), "m3pc_mtm_train vs three single calls")
    finally:
        torch.cuda.synchronize()
        buf.close()


# ------------------------------------------------------------------------------------------------ (c)
def _plan_outputs(handle, dims, s, a, r, eps, N, H):
    out = {}
    for prec in (capi.PREC_FP32, capi.PREC_BF16, capi.PREC_BF16X3):
        res = handle.plan_step(capi.MODE_RTG, s, a, r, eps, H, 3.0, 0.6, 0.99, N, precision=prec)
        out[prec] = {k: v.clone() for k, v in res.items()}
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("d, nh, batch", [(64, 2, 3), (512, 4, 2)], ids=["g1_tiny", "d512"])
def test_derived_forms_are_those_of_a_load_of_the_trained_weights(golden, d, nh, batch):
    """After training, a plan step on the trained handle equals, bit for bit in fp32, bf16 and bf16x3, the step of a fresh handle
    given the exported weights through m3pc_load_weights -- on g1_tiny and on a size where the fused layer tail runs (d 512, ff
    2048): hi / lo bf16 copies, fragment streams, K|V streams, embedding tables, mask tokens.  m3pc_load_stats of a plain load is
    what it was."""
    dims = synth.Dims(S, A, T, n_embd=d, n_head=nh)
    N, H = 64, 4
    sd0, stats = synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0)
    p = HipPlanner(_cfg(golden), sd0, stats, None, n_embd=d, n_head=nh, precision="fp32", max_batch=4, max_windows=1)
    fused = d == 512
    plain = dict(tensors=len(sd0), tail_streams=4 if fused else 0, kv_streams=4 if fused else 0, tables_invalidated=True)
    assert p.handle.load_stats() == plain, p.handle.load_stats()
    tr = DeviceMTMTrainer(p, 4, **HYPER)
    h2 = None
    try:
        hist = synth.make_history(dims, 0)
        hist["path_length"] = 100
        s, a, r, h, rtg = p.assemble_window(hist, rtg=3.0)
        s, a, r = s.clone(), a.clone(), r.clone()
        eps = synth.make_eps(N, dims, 7)[:, 0, :, 0, :].cuda().contiguous()
        before = _plan_outputs(p.handle, dims, s, a, r, eps, N, H)  # (plans and shared decoder tables are cached now: the step invalidates them)
        b = {k: v.cuda() for k, v in MC.make_batch(dims, batch, 41).items()}
        for i in range(2):
            tr.train_step_record(b, MC.random_masks(T, 43 + i), MC.make_eps(dims, batch, 45 + i).cuda())
        trained = _plan_outputs(p.handle, dims, s, a, r, eps, N, H)
        w = tr.export_weights()
        torch.cuda.synchronize()
        assert not torch.equal(trained[capi.PREC_FP32]["expect_return"], before[capi.PREC_FP32]["expect_return"]), "the plan step saw the step"
        full = {k: v.cpu() for k, v in w.items()}
        full["pos_embed"] = sd0["pos_embed"]
        h2 = capi.Handle(dims.state_dim, dims.action_dim, dims.traj_length, dims.n_embd, dims.n_head, dims.n_enc_layer, dims.n_dec_layer,
                         max_candidates=N, max_batch=4, critic_hidden=256)
        h2.load_weights(full)
        assert h2.load_stats() == plain, h2.load_stats()
        for k, name in enumerate(synth.KEYS):
            h2.set_tokenizer(k, stats[name]["mean"], stats[name]["std"], normalize=(name != "actions"))
        loaded = _plan_outputs(h2, dims, s, a, r, eps, N, H)
        for prec, name in ((capi.PREC_FP32, "fp32"), (capi.PREC_BF16, "bf16"), (capi.PREC_BF16X3, "bf16x3")):
            for k in ("loc", "std", "sample_actions", "expect_return"):
                assert torch.equal(trained[prec][k].view(torch.int32), loaded[prec][k].view(torch.int32)), (name, k)
            assert torch.isfinite(trained[prec]["expect_return"]).all()
    finally:
        torch.cuda.synchronize()
        tr.close()
        if h2 is not None:
            h2.close()
        p.handle.close()


# ------------------------------------------------------------------------------------------------ (d)
def test_pinned_to_the_real_reference(golden, g10, fresh):
    tr = fresh()
    names = [str(n) for n in g10["names"]]
    assert sorted(names) == sorted(tr.shapes)
    dec = {str(n) for n in g10["decay_names"]}
    assert [n for n in names if tr.decays(n)] == [n for n in names if n in dec]
    out = C.c_int(7)
    assert tr.lib.m3pc_mtm_opt_decays(tr._o, b"pos_embed", C.byref(out)) == EINVAL and out.value == -1 and b"pos_embed" in tr.lib.m3pc_last_error()
    stateless = {str(n) for n in g10["stateless_names"]} - {"log_temperature"}
    K = int(g10["K"])
    batch, masks, eps = _g8(golden, str(g10["case"]))
    w0 = _snapshot(tr)
    logs = [tr.train_step(batch, masks, eps) for _ in range(K)]
    w1 = _snapshot(tr)
    assert {n for n in names if w1["steps"][n] == 0} == stateless
    for n in stateless:
        assert w1["w"][n].tobytes() == w0["w"][n].tobytes(), n
    t_dev = np.abs(g10["temperature32"] / g10["temperature64"] - 1.0)
    l_dev = float((np.abs(g10["loss32"] - g10["loss64"]) / np.abs(g10["loss64"])).max())
    for k, log in enumerate(logs):
        assert abs(log["train/lr"] - float(g10["lr"][k])) <= np.spacing(float(g10["lr"][k])), k
        t_tol = max(16 * float(t_dev[k]), 1e-9)
        t_got = abs(log["train/temperature"] / float(g10["temperature64"][k]) - 1.0)
        l_tol = max(16 * l_dev, 1e-4)  # (floor: the tolerance tests/test_mtm_grad_gpu.py gives `total`)
        l_got = abs(log["train/loss"] - float(g10["loss64"][k])) / max(1.0, abs(float(g10["loss64"][k])))
        print(f"step {k}: temperature rel dev {t_got:.2e} (tol {t_tol:.2e})  loss dev {l_got:.2e} (tol {l_tol:.2e})  entropy {log['train/entropy']:.6f}")
        assert t_got <= t_tol and l_got <= l_tol, k
    ref_dev = dict(zip(names, g10["ref32_upd_dev"].tolist()))
    sums = dict(zip(names, g10["sums"]))
    med = float(np.median([ref_dev[n] for n in names if sums[n][1] > 0]))
    skipped, bad, ratio = [], [], 0.0
    for n in names:
        if n in stateless:
            continue
        if ref_dev[n] >= 1.0 / 16:
            skipped.append(n)
            print(f"skipped {n}: ref32_upd_dev {ref_dev[n]:.3f}")
            continue
        upd = (w1["w"][n].astype(np.float64) - w0["w"][n].astype(np.float64)).reshape(-1)
        head = g10["head/" + n]
        if sums[n][1] == 0:  # the reference did not move it (an exact-zero gradient on a tensor that does not decay): nor does the device
            assert not upd.any(), n
            continue
        if upd.size <= head.size:  # the whole update is in the file
            dev = math.sqrt(((upd - head) ** 2).sum() / sums[n][1])
        else:  # leading entries against their own norm, and the whole tensor's sum and sum of squares
            dev = math.sqrt(((upd[:head.size] - head) ** 2).sum() / (head ** 2).sum())
            assert abs((upd ** 2).sum() / sums[n][1] - 1.0) <= 2 * 16 * max(ref_dev[n], med) + 1e-6, n
        bound = 16 * max(ref_dev[n], med)
        ratio = max(ratio, dev / bound)
        if not dev <= bound:
            bad.append((n, dev, bound))
    print("largest dev / bound over the compared tensors: %.3f (median ref32_upd_dev %.2e)" % (ratio, med))
    assert sorted(skipped) == sorted(n for n in names if n.endswith("self_attn.in_proj_bias")) and len(skipped) == 3
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ (e)
def test_round_trip_through_a_torch_learner(golden, planner, sd, fresh):
    from test_mtm_grad_gpu import GradModule, _optimizers
    batch, masks, eps = _g8(golden)
    tmasks = {k: torch.from_numpy(m.astype(np.float64)) for k, m in masks.items()}
    shapes = {"states": (1, S), "actions": (1, A), "rewards": (1, 1), "returns": (1, 1)}
    no = {k: False for k in R.KEYS}
    planner.load_state_dict(sd)
    model = GradModule(sd)
    opt, sched, topt = _optimizers(dict(zip(model.names, model.ps)), model.log_temperature, t_max=10)
    ln = types.SimpleNamespace(cfg=planner.cfg, mtm=model, mtm_optimizer=opt, mtm_scheduler=sched, temp_optimizer=topt)
    tr = None
    try:
        for _ in range(2):  # two torch steps (the device's gradient, torch's optimizers)
            planner.mtm_update(batch, shapes, no, model, opt, sched, topt, masks=tmasks, eps=eps)
        planner.load_state_dict({k: v.detach() for k, v in model.state_dict().items()})
        tr = DeviceMTMTrainer.from_learner(ln, planner=planner, max_batch=4, num_train_steps=10)
        assert tr.args.temp_learning_rate == 1e-2 and tr.args.weight_decay == 5e-3 and tr.args.learning_rate == 1e-3
        before = _snapshot(tr)
        assert before["state"]["sched_step"] == 2 and before["state"]["temp_step"] == 2
        assert before["steps"]["encoder.layers.0.linear1.weight"] == 2 and before["steps"]["output_head_dict.rewards.1.bias"] == 0
        for n, p in zip(model.names, model.ps):
            assert before["w"][n].tobytes() == p.detach().cpu().numpy().tobytes(), n
            if before["steps"][n]:
                assert before["m"][n].tobytes() == opt.state[p]["exp_avg"].cpu().numpy().tobytes(), n
        rec, trec = tr.train_step_record(batch, masks, eps)
        grads = _np(tr.grad.export())
        after = _snapshot(tr)
        lt, _, _, _, tb = OR.temperature_step(before["state"]["log_temperature"], before["state"]["temp_exp_avg"], before["state"]["temp_exp_avg_sq"],
                                              before["state"]["temp_step"], float(rec.cpu()[12]), model.target_entropy, lr=1e-2)
        assert abs(after["state"]["log_temperature"] - lt) <= tb
        out = OR.adamw(before["w"], grads, before["m"], before["v"], before["steps"], OR.lr_at(2, 1e-3, 10), 5e-3, FINETUNE_BITS)
        worst = 0.0
        for n, (pr, mr, vr, st, bp, bm, bv) in out.items():
            assert after["steps"][n] == st
            worst = max(worst, OR.worst(after["w"][n], pr, bp), OR.worst(after["m"][n], mr, bm), OR.worst(after["v"][n], vr, bv))
        print("device step from the imported torch state: worst err / bound %.3f" % worst)
        assert worst <= 1.0
        tr.to_learner(ln)
        assert sched.last_epoch == 3 and opt.param_groups[0]["lr"] == pytest.approx(OR.lr_at(3, 1e-3, 10), rel=1e-15)
        for n, p in zip(model.names, model.ps):
            assert after["w"][n].tobytes() == p.detach().cpu().numpy().tobytes(), n
        planner.mtm_update(batch, shapes, no, model, opt, sched, topt, masks=tmasks, eps=eps, sync=False)  # one more torch step
        assert sched.last_epoch == 4 and int(topt.state[model.log_temperature]["step"]) == 4
        for n, p in zip(model.names, model.ps):
            outside = n.startswith("output_head_dict.rewards.") or n.startswith("output_head_dict.returns.")
            st = opt.state.get(p, {})
            if outside:
                assert not len(st), n
            else:
                assert int(st["step"]) == 4 and st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape and st["exp_avg"].device == p.device, n
    finally:
        torch.cuda.synchronize()
        if tr is not None:
            tr.close()
        if getattr(planner, "_mtm_grad", None) is not None:
            planner._mtm_grad.close()
            planner._mtm_grad = None
        planner.load_state_dict(sd)


def test_native_mtm_update_returns_the_reference_log(golden, planner, sd):
    from test_mtm_grad_gpu import LOG_KEYS, GradModule, _optimizers
    batch, masks, eps = _g8(golden)
    tmasks = {k: torch.from_numpy(m.astype(np.float64)) for k, m in masks.items()}
    planner.load_state_dict(sd)
    model = GradModule(sd)
    opt, sched, topt = _optimizers(dict(zip(model.names, model.ps)), model.log_temperature)
    planner.cfg.num_train_steps = 10
    try:
        logs = [planner.mtm_update(batch, None, {k: False for k in R.KEYS}, model, opt, sched, topt, masks=tmasks, eps=eps, native=True) for _ in range(2)]
        assert set(logs[0]) == LOG_KEYS and logs[1]["train/lr"] == planner._mtm_trainer.lr(1) and logs[1]["train/loss"] != logs[0]["train/loss"]
        assert torch.equal(model.ps[0].detach().cpu(), sd[model.names[0]]), "the native step leaves the torch module alone"
        planner._mtm_trainer.to_learner(planner._mtm_trainer._shim)
        assert not torch.equal(model.ps[0].detach().cpu(), sd[model.names[0]]) and sched.last_epoch == 2
    finally:
        del planner.cfg.num_train_steps
        torch.cuda.synchronize()
        if getattr(planner, "_mtm_trainer", None) is not None:
            planner._mtm_trainer.close()
            planner._mtm_trainer = None
        planner.load_state_dict(sd)


# ------------------------------------------------------------------------------------------------ (f)
def test_refusals(golden, planner, fresh):
    batch, masks, eps = _g8(golden)
    tr = fresh(max_batch=2)
    lib = tr.lib
    stream = capi._stream(tr.device)
    assert lib.m3pc_mtm_opt_step(tr._o, stream) == ESTATE and b"no gradient call" in lib.m3pc_last_error()
    with pytest.raises(capi.M3pcError, match="batch 3 outside"):
        tr.train_step_record(batch, masks, eps)  # max_batch exceeded
    small = {k: v[:2] for k, v in batch.items()}
    tr.grad.grad_record(small, masks, 0.1, "finetune", eps[:2])
    tr.opt_step()
    assert lib.m3pc_mtm_opt_step(tr._o, stream) == ESTATE and b"already applied" in lib.m3pc_last_error()
    with pytest.raises(capi.M3pcError, match="mask keeps no token"):
        tr.train_step_record(small, {k: np.zeros(T, np.uint8) for k in R.KEYS}, eps[:2])
    buf, _ = _filled_buffer(planner)
    try:
        with pytest.raises(capi.M3pcError, match="2 mask sets for 3 steps"):
            tr.train_from(buf, 3, 2, [masks, masks])
        with pytest.raises(capi.M3pcError, match="mask row has 7 entries"):
            tr.train_from(buf, 1, 2, {k: m[:7] for k, m in masks.items()})
        mp = (C.c_void_p * 4)(*[np.ascontiguousarray(masks[k]).ctypes.data for k in R.KEYS])
        assert lib.m3pc_mtm_train(tr._o, buf._rb, 0, 2, 0, 0, 0, mp, 0, 3, None, None, stream) == EINVAL and b"n_steps 0" in lib.m3pc_last_error()
    finally:
        buf.close()
    # a certified step between _begin and _end on the handle
    N, H = 64, 4
    hist = synth.make_history(DIMS, 0)
    hist["path_length"] = 100
    s, a, r, h, rtg = planner.assemble_window(hist, rtg=3.0)
    e = synth.make_eps(N, DIMS, 1).cuda().reshape(N, -1).contiguous()
    q = torch.empty(N, dtype=torch.float32).exponential_(1, generator=torch.Generator().manual_seed(7)).cuda()
    hd = planner.handle
    before = _snapshot(tr)
    hd.plan_step_certified_begin(capi.MODE_RTG, s.clone(), a.clone(), r.clone(), e, q, h, rtg, 0.6, 0.99, N, 0.01, precision=capi.PREC_FP32, slot=0)
    try:
        with pytest.raises(capi.M3pcError, match="m3pc error -2.*certified step"):
            tr.train_step_record(small, masks, eps[:2])
        tr.grad.grad_record(small, masks, 0.1, "finetune", eps[:2])  # (the gradient call itself never writes to the handle)
        assert lib.m3pc_mtm_opt_step(tr._o, stream) == ESTATE and b"certified step" in lib.m3pc_last_error()
    finally:
        hd.plan_step_certified_end(0)
        torch.cuda.synchronize()
    tr.opt_step()  # afterwards the same gradients are applied
    after = _snapshot(tr)
    assert after["state"]["sched_step"] == before["state"]["sched_step"] + 1
    arr = (capi.NamedTensor * 1)(capi.NamedTensor(b"nope", 1, 1, 0))
    assert lib.m3pc_mtm_opt_export(tr._o, 1, arr, 1, None, stream) == EINVAL and b"nope" in lib.m3pc_last_error()
    assert lib.m3pc_mtm_opt_export(tr._o, 3, arr, 1, None, stream) == EINVAL and b"which" in lib.m3pc_last_error()
    assert lib.m3pc_mtm_weights_export(tr.handle._h, arr, 1, stream) == EINVAL and b"nope" in lib.m3pc_last_error()
    st = capi.MtmOptState(-1, 0, 0.0, 0.0, 0.0, 0.0)
    assert lib.m3pc_mtm_opt_set_state(tr._o, C.byref(st)) == EINVAL and b"sched_step" in lib.m3pc_last_error()


ENTRIES = ("m3pc_mtm_loss", "m3pc_mtm_loss_replay", "m3pc_mtm_grad", "m3pc_mtm_grad_replay", "m3pc_mtm_train_step", "m3pc_mtm_train")
REPLAY_ENTRIES = tuple(e for e in ENTRIES if e.endswith("replay") or e == "m3pc_mtm_train")


def _six_entries(lib, handle, tr, dims_T=T):
    """-> call(entry, rb, b, mk, flags, keys): the same call through one of the six batch entries of the handle / of the trainer ``tr`` on
    it, on zero-filled device rows, under the mask rows ``mk`` ((C.c_void_p * 4) of host bytes), eps given (raw) or library-drawn."""
    dev, stream = handle.device, capi._stream(handle.device)
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
    n = 5  # (rows for max_batch + 1: a refused call reads none of them, a call that runs has batch <= 4)
    s, a, r, v, e = z(n, dims_T, S), z(n, dims_T, A), z(n, dims_T, 1), z(n, dims_T, 1, dtype=torch.float64), z(n, dims_T, A)
    rec, trec = z(capi.MTM_LOSS_FLOATS), z(3, dtype=torch.float64)
    ptr = capi._ptr

    def call(entry, rb=None, b=2, mk=None, flags=0, keys=FINETUNE_BITS):
        if entry == "m3pc_mtm_loss":
            return lib.m3pc_mtm_loss(handle._h, b, ptr(s), ptr(a), ptr(r), ptr(v), 1, mk, ptr(e), 0.1, flags, keys, capi.PREC_FP32, ptr(rec),
                                     None, None, None, None, None, stream)
        if entry == "m3pc_mtm_loss_replay":
            return lib.m3pc_mtm_loss_replay(handle._h, rb, b, 0, None, None, 0, 5, 0, mk, None, 0.1, flags, keys, capi.PREC_FP32, ptr(rec),
                                            None, None, stream)
        if entry == "m3pc_mtm_grad":
            return lib.m3pc_mtm_grad(tr.grad._g, b, ptr(s), ptr(a), ptr(r), ptr(v), 1, mk, ptr(e), 0.1, flags, keys, ptr(rec), stream)
        if entry == "m3pc_mtm_grad_replay":
            return lib.m3pc_mtm_grad_replay(tr.grad._g, rb, b, 0, None, None, 0, 5, 0, mk, None, 0.1, flags, keys, ptr(rec), None, None, stream)
        if entry == "m3pc_mtm_train_step":
            return lib.m3pc_mtm_train_step(tr._o, b, ptr(s), ptr(a), ptr(r), ptr(v), 1, mk, ptr(e), flags, keys, ptr(rec), ptr(trec), stream)
        assert entry == "m3pc_mtm_train"
        return lib.m3pc_mtm_train(tr._o, rb, 1, b, 0, 5, 0, mk, flags, keys, ptr(rec), ptr(trec), stream)

    call.keep = (s, a, r, v, e, rec, trec)
    return call


def _mask_ptrs(*rows):
    bufs = [None if row is None else C.create_string_buffer(bytes(bytearray(row)), len(row)) for row in rows]
    return (C.c_void_p * 4)(*[None if b is None else C.addressof(b) for b in bufs]), bufs


def test_the_six_batch_entries_refuse_alike(golden, planner, sd, fresh):
    """One faulty call through m3pc_mtm_loss, _loss_replay, _grad, _grad_replay, _train_step and _train: the same code and, behind the
    entry's name, the same text; the first of two faults is reported; a refusal leaves the gradient object's have_grad / consumed
    state (probed with m3pc_mtm_opt_step, which refuses in both states used here) and ``replay.step`` where they were.  An all-hidden
    mask set is refused by name in the four gradient and trainer entries, accepted by m3pc_mtm_loss_terms, and refused without the
    entry's name by the two loss entries that run the forward (the plan lookup behind their tokenise launches refuses it)."""
    tr = fresh(max_batch=4)  # (the handle's max_batch is 4 too: "max_batch=4" in every entry's text)
    lib, err = tr.lib, tr.lib.m3pc_last_error
    stream = capi._stream(tr.device)
    call = _six_entries(lib, planner.handle, tr)
    good, k0 = _mask_ptrs(*[[1, 0] * (T // 2)] * 4)
    byte2, k1 = _mask_ptrs([1, 0] * (T // 2), [1, 0, 2, 0, 0, 0, 0, 0], [0] * T, [1] * T)
    hidden, k2 = _mask_ptrs(*[[0] * T] * 4)
    buf, _ = _filled_buffer(planner)
    short, empty = C.c_void_p(), C.c_void_p()
    assert lib.m3pc_replay_create(planner.handle._h, 4, 40, T - 1, 0, 0, C.byref(short)) == 0
    assert lib.m3pc_replay_create(planner.handle._h, 4, 40, T, 0, 0, C.byref(empty)) == 0

    def alike(entries, code, text, **kw):
        for entry in entries:
            kw.setdefault("rb", buf._rb)
            kw.setdefault("mk", good)
            rc, msg = call(entry, **kw), err()
            assert rc == code and msg.startswith(entry.encode() + b": "), (entry, kw, rc, msg)
            assert msg[len(entry) + 2:] == text, (entry, kw, msg)

    def every_refusal(probe):
        """Each shared refusal through the entries that can meet it; after each, m3pc_mtm_opt_step still answers ``probe``."""
        for kw, code, text, entries in (
                (dict(b=0), EINVAL, b"batch 0 outside [1, max_batch=4]", ENTRIES),
                (dict(b=5), EINVAL, b"batch 5 outside [1, max_batch=4]", ENTRIES),
                (dict(mk=byte2), EINVAL, b"mask byte 2 of 'actions' is 2, not 0 or 1", ENTRIES),
                (dict(flags=4), EINVAL, b"unknown flag bits 0x4", ENTRIES),
                (dict(keys=16), EINVAL, b"loss_keys 16 outside [0, 15]", ENTRIES),
                (dict(b=0, flags=4), EINVAL, b"batch 0 outside [1, max_batch=4]", ENTRIES),  # two faults: the batch is reported
                (dict(rb=short), EINVAL, b"the buffer (S 11, A 3, segment_length 7, device 0) does not fit the handle (11, 3, T 8, 0)", REPLAY_ENTRIES),
                (dict(rb=empty), ESTATE, b"the buffer holds no trajectory", REPLAY_ENTRIES),
                (dict(mk=hidden), EINVAL, b"mask keeps no token", ENTRIES[2:])):
            alike(entries, code, text, **kw)
            assert lib.m3pc_mtm_opt_step(tr._o, stream) == ESTATE and probe in err(), (kw, err())

    try:
        every_refusal(b"no gradient call was made")  # have_grad stays false
        for entry in ENTRIES[:2]:  # as observed on the parent commit: M3PC_EINVAL from the plan lookup, no entry name in front
            assert call(entry, rb=buf._rb, mk=hidden) == EINVAL and err() == b"mask keeps no token", (entry, err())
        c = call.keep
        four = (C.c_void_p * 4)(*[capi._ptr(t) for t in (c[0], c[1], c[2], c[2])])
        one = torch.ones_like(c[4])
        assert lib.m3pc_mtm_loss_terms(planner.handle._h, 2, capi._ptr(c[0]), capi._ptr(c[2]), capi._ptr(c[2]), capi._ptr(c[4]), capi._ptr(one),
                                       four, hidden, capi._ptr(c[4]), 0.1, 0, FINETUNE_BITS, capi._ptr(c[5]), stream) == 0, err()
        step0 = buf.step
        for wrapper in (lambda: buf.mtm_loss(_g8(golden)[1], 0.1, batch_size=5), lambda: buf.mtm_grad(tr.grad, _g8(golden)[1], 0.1, batch_size=5),
                        lambda: buf.mtm_train(tr, 2, _g8(golden)[1], batch_size=5)):
            with pytest.raises(capi.M3pcError, match="batch 5 outside"):
                wrapper()
            assert buf.step == step0
        batch, masks, eps = _g8(golden)
        tr.grad.grad_record({k: v[:2] for k, v in batch.items()}, masks, 0.1, "finetune", eps[:2])
        tr.opt_step()
        every_refusal(b"already applied")  # consumed stays true

        # a bare handle: the state refusals, behind every argument refusal
        bare = capi.Handle(S, A, T, 64, 2, 2, 1, max_candidates=64, max_batch=4)
        tr2 = buf2 = None
        try:
            tr2 = DeviceMTMTrainer(bare, 4, **HYPER)
            buf2 = type(buf)(bare, planner.cfg, 4, 40, discount=0.99, seed=5)
            buf2.append(np.zeros((1, 40, S), np.float32), np.zeros((1, 40, A), np.float32), np.zeros((1, 40), np.float32), np.zeros((1, 40)), [20])
            call2 = _six_entries(lib, bare, tr2)
            for entry in ENTRIES:
                assert call2(entry, rb=buf2._rb, mk=good) == ESTATE and err() == entry.encode() + b": weights not loaded", (entry, err())
            bare.load_weights(sd)
            for entry in ENTRIES:
                assert call2(entry, rb=buf2._rb, mk=good) == ESTATE and err() == entry.encode() + b": tokenizer 'states' not set", (entry, err())
        finally:
            torch.cuda.synchronize()
            for x in (buf2, tr2, bare):
                if x is not None:
                    x.close()
    finally:
        torch.cuda.synchronize()
        buf.close()
        for rb in (short, empty):
            assert lib.m3pc_replay_destroy(rb) == 0
    del k0, k1, k2


# ------------------------------------------------------------------------------------------------ the C example
def test_mtm_train_example(planner, golden, fresh, tmp_path):
    """examples/mtm_train.c compiled with gcc -Wall -Werror against include/m3pc_hip.h, linked to the built library and run on a handle
    of its own: a three-step loop from a replay buffer.  Its records, its {lr, temperature, log_temperature} rows and the weight it
    exports are DeviceReplayBuffer.mtm_train's on the same trajectories, masks, seed and step, bit for bit."""
    import os
    import subprocess
    from m3pc_amd.replay import DeviceReplayBuffer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    so = tmp_path / "libmtm_train_example.so"
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(root, "include"),
                           "-I", os.path.join(rocm, "include"), os.path.join(root, "examples", "mtm_train.c"), "-o", str(so),
                           "-L", libdir, "-l:" + os.path.basename(capi.LIB_PATH), "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-lm",
                           "-Wl,-rpath," + libdir])
    fp, vp = C.POINTER(C.c_float), C.c_void_p

    class IO(C.Structure):
        _fields_ = [("dims", C.POINTER(capi.Dims)), ("weights", C.POINTER(capi.NamedTensor)), ("n_weights", C.c_int),
                    ("tok_mean", fp * 4), ("tok_std", fp * 4), ("tok_dim", C.c_int * 4), ("tok_normalize", C.c_int * 4),
                    ("n_traj", C.c_int), ("max_steps", C.c_int), ("obs", vp), ("act", vp), ("rew", vp), ("val", vp), ("lens", vp),
                    ("batch", C.c_int), ("masks", vp * 4), ("learning_rate", C.c_double), ("weight_decay", C.c_double),
                    ("num_train_steps", C.c_longlong), ("seed", C.c_ulonglong), ("step0", C.c_ulonglong), ("records_dev", vp),
                    ("train_records_dev", vp), ("records", vp), ("train_records", vp), ("weight_name", C.c_char_p), ("weight", vp),
                    ("weight_numel", C.c_longlong)]

    n_traj, Ms, seed = 3, 40, 5
    rng = np.random.RandomState(9)
    lens = np.array([8, 40, 23], np.int32)
    obs, act, rew = np.zeros((n_traj, Ms, S), np.float32), np.zeros((n_traj, Ms, A), np.float32), np.zeros((n_traj, Ms), np.float32)
    for i, n in enumerate(lens):
        obs[i, :n], act[i, :n], rew[i, :n] = rng.normal(size=(n, S)), rng.uniform(-1, 1, size=(n, A)), rng.normal(size=(n,))
    val = rng.normal(size=(n_traj, Ms)) * 10.0
    sd0 = synth.make_state_dict(DIMS, 0)
    arr, keep = capi._named(sd0)
    io = IO()
    dims = capi.Dims(S, A, T, 64, 2, 2, 1, 64, 4, 0, 64, 0)
    io.dims, io.weights, io.n_weights = C.pointer(dims), C.cast(arr, C.POINTER(capi.NamedTensor)), len(sd0)
    toks = []
    for k, name in enumerate(capi.KEYS):
        t = planner.tokenizer_manager.tokenizers[name]
        m, sdv = t._data_mean.float().contiguous().reshape(-1), t._data_std.float().contiguous().reshape(-1)
        toks.append((m, sdv))
        io.tok_mean[k], io.tok_std[k] = C.cast(m.data_ptr(), fp), C.cast(sdv.data_ptr(), fp)
        io.tok_dim[k], io.tok_normalize[k] = m.numel(), int(bool(t.normalize))
    io.n_traj, io.max_steps, io.batch, io.seed, io.step0 = n_traj, Ms, B, seed, 0
    io.learning_rate, io.weight_decay, io.num_train_steps = HYPER["learning_rate"], HYPER["weight_decay"], HYPER["num_train_steps"]
    io.obs, io.act, io.rew, io.val, io.lens = obs.ctypes.data, act.ctypes.data, rew.ctypes.data, val.ctypes.data, lens.ctypes.data
    mrows = [np.ascontiguousarray(golden[f"c0/mask/{k}"]) for k in R.KEYS]
    for k in range(4):
        io.masks[k] = mrows[k].ctypes.data
    recs_dev = torch.zeros(3 * capi.MTM_LOSS_FLOATS, dtype=torch.float32, device="cuda")
    trecs_dev = torch.zeros(9, dtype=torch.float64, device="cuda")
    records, train_records = np.zeros((3, capi.MTM_LOSS_FLOATS), np.float32), np.zeros((3, 3), np.float64)
    name = "encoder.layers.0.linear1.weight"
    weight = np.zeros(int(np.prod(sd0[name].shape)), np.float32)
    io.records_dev, io.train_records_dev, io.records, io.train_records = recs_dev.data_ptr(), trecs_dev.data_ptr(), records.ctypes.data, train_records.ctypes.data
    io.weight_name, io.weight, io.weight_numel = name.encode(), weight.ctypes.data, weight.size
    torch.cuda.synchronize()
    lib = C.CDLL(str(so))
    lib.mtm_train_example.restype = C.c_int
    lib.mtm_train_example.argtypes = [C.POINTER(IO), C.c_int, vp]
    rc = lib.mtm_train_example(C.byref(io), torch.cuda.current_device(), vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, planner.handle.lib.m3pc_last_error()
    tr = fresh(target_entropy=-float(A))
    buf = DeviceReplayBuffer(planner, planner.cfg, n_traj, Ms, discount=0.99, seed=seed)
    try:
        buf.append(obs, act, rew, val, lens)
        recs, trecs = buf.mtm_train(tr, 3, {k: torch.from_numpy(golden[f"c0/mask/{k}"].astype(np.float64)) for k in R.KEYS}, batch_size=B)
        want = tr.export_weights()[name]
        torch.cuda.synchronize()
        assert np.isfinite(records[:, 14]).all() and records.tobytes() == recs.cpu().numpy().tobytes()
        assert train_records.tobytes() == trecs.cpu().numpy().tobytes() and train_records[1, 0] == tr.lr(1)
        assert weight.tobytes() == want.cpu().numpy().reshape(-1).tobytes() and not np.array_equal(weight, sd0[name].numpy().reshape(-1))
    finally:
        buf.close()
    del keep, toks
