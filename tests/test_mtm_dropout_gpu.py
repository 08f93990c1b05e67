"""Dropout in the gradient of the masked-trajectory loss end to end (m3pc_mtm_grad_set_dropout / _get_dropout and everything that steps
on them) on the g1_tiny sizes: every tensor against the float64 restatement under the SAME keep masks (tests/mtm_dropout_ref.py) within
16 x max(dev32[tensor], median dev32) -- dev32 the REAL training-mode reference's own float32 deviation for the golden cases
(tests/golden/g11_mtm_dropout.npz; the fine-tuning form: ref32_grad_dev_f32clip, as tests/test_mtm_grad_gpu.py explains), the float32
restatement's otherwise -- then what the stream promises: same (seed, draw) same bits, whatever ran before and on whichever object;
p = 0 is the object that never had dropout; n steps in one call are n single calls; state round trips; the learner entry points."""
import math
import types

import numpy as np
import pytest
import torch

import mtm_dropout_ref as DR
import mtm_grad_cases as MC
import mtm_grad_ref as GR
import mtm_loss_ref as R
from m3pc_amd import capi, synth
from m3pc_amd.mtm_grad import DeviceMTMGrad
from m3pc_amd.mtm_train import DeviceMTMTrainer
from m3pc_amd.planner import HipPlanner, attach
from oracle import mtm_oracle as O
from test_mtm_grad_gpu import LOG_KEYS, NO, SHAPES, GradModule, _optimizers
from test_mtm_loss_gpu import _filled_buffer
from test_mtm_train_gpu import HYPER, _same_bits, _snapshot

pytestmark = pytest.mark.gpu
S, A, T, B = 11, 3, 8, 3
DIMS = synth.Dims(S, A, T, n_embd=64, n_head=2)
CASES = (("ft_c0_p10", "c0", "finetune"), ("ft_c0_p50", "c0", "finetune"), ("pt_c3_p10", "c3", "pretrain"))
EINVAL = -1


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir + "/g8_mtm_loss.npz")


@pytest.fixture(scope="module")
def g11(golden_dir):
    return np.load(golden_dir + "/g11_mtm_dropout.npz")


@pytest.fixture(scope="module")
def g9p(golden_dir):
    return np.load(golden_dir + "/g9_mtm_grad_pretrain.npz")


def _cfg(golden):
    return types.SimpleNamespace(traj_length=T, action_samples=64, horizon=4, discount=0.99, temperature=0.01, lmbda=0.6, plan_guidance="rtg_guiding",
                                 device="cuda", index_jump=4, traj_batch_size=B, traj_buffer_size=4, trans_batch_size=6, trans_buffer_size=64,
                                 select_mode="prob", mtm_iter_per_rollout=2, using_online_threshold=4,
                                 mask_ratio=tuple(golden["mask_ratio"].tolist()), p_weights=tuple(golden["p_weights"].tolist()))


@pytest.fixture(scope="module")
def sd():
    return synth.make_state_dict(DIMS, 0)


@pytest.fixture(scope="module")
def ostats():
    return O.make_stats(synth.make_tokenizer_stats(DIMS, 0))


@pytest.fixture(scope="module")
def planner(golden, sd):
    p = HipPlanner(_cfg(golden), sd, synth.make_tokenizer_stats(DIMS, 0), None, n_embd=64, n_head=2, precision="fp32",
                   generator=torch.Generator(device="cuda").manual_seed(11), max_batch=4, max_windows=1)
    yield p
    torch.cuda.synchronize()
    p.handle.close()


@pytest.fixture
def objs(planner):
    """-> make(max_batch): a new gradient object; all of them are closed afterwards."""
    made = []

    def make(max_batch=4):
        g = DeviceMTMGrad(planner, max_batch)
        made.append(g)
        return g

    yield make
    torch.cuda.synchronize()
    for g in made:
        g.close()


@pytest.fixture
def fresh(planner, sd):
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


def _bits(gd):
    return {k: v.tobytes() for k, v in gd.items()}


# ------------------------------------------------------------------------------------------------ against float64 under the same masks
@pytest.mark.parametrize("tag,case,form", CASES)
def test_golden_cases(objs, golden, g9p, g11, sd, ostats, tag, case, form):
    obj = objs()
    p, seed, draw = float(g11[tag + "/p"]), int(g11["seed"]), int(g11["draw"])
    batch = {k: torch.from_numpy(golden["batch/" + k]) for k in R.KEYS}
    if case == "c3":
        batch["actions"] = torch.from_numpy(g9p["c3/actions"])
    mcase = "c2" if case == "c3" else case
    masks, eps, reg = {k: golden[f"{mcase}/mask/{k}"] for k in R.KEYS}, torch.from_numpy(golden[f"{mcase}/eps"]), float(golden["entropy_reg"])
    obj.set_dropout(p, seed, draw)
    rec, got = MC.device_grads(obj, batch, masks, eps, reg, form)
    assert obj.get_dropout() == (p, seed, draw + 1)
    flags, bits = GR.FORMS[form]
    t64, g64 = DR.grads_dropout(sd, ostats, batch, masks, eps, reg, flags, bits, DIMS.n_head, p, seed, draw, torch.float64, True)
    assert abs(rec[R.TOTAL] - t64) <= 1e-4 * max(1.0, abs(t64)), "the record is that of the dropped forward"
    names = [str(n) for n in g11["grad_names"]]
    key = "ref32_grad_dev_f32clip" if form == "finetune" else "ref32_grad_dev"
    dev32 = {n: (np.nan if g11[tag + "/none"][i] else float(g11[f"{tag}/{key}"][i])) for i, n in enumerate(names)}
    MC.compare(got, g64, dev32, f"dropout golden {tag}")


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_odd_row_mask_set(objs, sd, ostats, p):
    """7 encoder rows and 32 decoder rows per sequence, batch 3: 21 encoder rows (the last row quad of every matrix site is ragged, and
    so is the last key quad of every encoder attention row); rewards fully hidden: structural zeros stay exact zeros."""
    obj = objs()
    masks = MC.rows(T, states=[0, 2, 5], actions=[1], rewards="none", returns=[0, 3, 4])
    batch, eps, seed, draw = MC.make_batch(DIMS, B, 131), MC.make_eps(DIMS, B, 132), 77 + 2 ** 40, 2 ** 33 + 5
    for form in ("finetune", "pretrain"):
        flags, bits = GR.FORMS[form]
        obj.set_dropout(p, seed, draw)
        rec, got = MC.device_grads(obj, batch, masks, eps, 0.1, form)
        t64, g64 = DR.grads_dropout(sd, ostats, batch, masks, eps, 0.1, flags, bits, DIMS.n_head, p, seed, draw, torch.float64, True)
        _, g32 = DR.grads_dropout(sd, ostats, batch, masks, eps, 0.1, flags, bits, DIMS.n_head, p, seed, draw, torch.float32, True)
        dev32 = {n: np.nan if g is None else GR.deviation(g32[n], g) for n, g in g64.items()}
        assert np.isfinite(t64) and abs(rec[R.TOTAL] - t64) <= 1e-4 * max(1.0, abs(t64))
        MC.compare(got, g64, dev32, f"dropout odd rows p {p} {form}")
        for n in ("encoder_embed_dict.rewards.weight", "encoder_embed_dict.rewards.bias", "encoder_per_dim_encoding.rewards"):
            assert not got[n].any(), n
        # the eval-mode gradient is another one
        _, g0 = GR.grads(sd, ostats, batch, masks, eps, 0.1, flags, bits, DIMS.n_head)
        n = "decoder.layers.0.linear1.weight"
        assert GR.deviation(got[n], g0[n]) > 1e-2


# ------------------------------------------------------------------------------------------------ the stream
def test_same_seed_and_draw_same_bits(objs):
    obj = objs(4)
    masks = MC.random_masks(T, 141)
    small, eps_s = MC.make_batch(DIMS, 2, 142), MC.make_eps(DIMS, 2, 143)
    big, eps_b = MC.make_batch(DIMS, 4, 144), MC.make_eps(DIMS, 4, 145)
    obj.set_dropout(0.1, 9, 40)
    rec_a, a = MC.device_grads(obj, small, masks, eps_s, 0.1, "pretrain")
    assert obj.get_dropout()[2] == 41
    _, b = MC.device_grads(obj, small, masks, eps_s, 0.1, "pretrain")  # draw 41
    assert any(a[n].tobytes() != b[n].tobytes() for n in a), "another draw, other gradients"
    MC.device_grads(obj, big, MC.random_masks(T, 146), eps_b, 0.1, "finetune")  # a larger batch in between (draw 42)
    obj.set_dropout(0.1, 9, 40)
    rec_c, c = MC.device_grads(obj, small, masks, eps_s, 0.1, "pretrain")
    assert _bits(a) == _bits(c) and rec_a.tobytes() == rec_c.tobytes(), "after a larger-batch call"
    other = objs(2)  # a fresh object, another max_batch
    other.set_dropout(0.1, 9, 40)
    rec_d, d = MC.device_grads(other, small, masks, eps_s, 0.1, "pretrain")
    assert _bits(a) == _bits(d) and rec_a.tobytes() == rec_d.tobytes(), "on a fresh object"


def test_p_zero_is_the_object_that_never_had_dropout(objs):
    plain, obj = objs(), objs()
    batch, eps, masks = MC.make_batch(DIMS, B, 151), MC.make_eps(DIMS, B, 152), MC.random_masks(T, 153)
    rec0, g0 = MC.device_grads(plain, batch, masks, eps, 0.1, "finetune")
    assert plain.get_dropout() == (0.0, 0, 0)
    obj.set_dropout(0.5, 3, 7)
    rec1, g1 = MC.device_grads(obj, batch, masks, eps, 0.1, "finetune")
    assert any(g0[n].tobytes() != g1[n].tobytes() for n in g0)
    obj.set_dropout(0.0, 3, 7)
    rec2, g2 = MC.device_grads(obj, batch, masks, eps, 0.1, "finetune")
    assert _bits(g0) == _bits(g2) and rec0.tobytes() == rec2.tobytes()
    assert obj.get_dropout() == (0.0, 3, 7), "without dropout nothing draws"


def test_refusals_leave_the_draw_alone(objs, planner):
    obj = objs()
    lib = planner.handle.lib
    obj.set_dropout(0.1, 5, 11)
    for bad in (-0.5, 1.0, float("nan")):
        with pytest.raises(capi.M3pcError, match="set_dropout: p"):
            obj.set_dropout(bad, 1, 2)
    assert obj.get_dropout() == (0.1, 5, 11), "a refused _set_dropout changes nothing"
    batch, eps, masks = MC.make_batch(DIMS, 5, 161), MC.make_eps(DIMS, 5, 162), MC.random_masks(T, 163)
    with pytest.raises(capi.M3pcError):  # batch 5 > max_batch 4
        MC.device_grads(obj, batch, masks, eps, 0.1, "finetune")
    none = {k: np.zeros(T, np.uint8) for k in R.KEYS}  # masks that keep no token
    with pytest.raises(capi.M3pcError):
        MC.device_grads(obj, MC.make_batch(DIMS, 2, 164), none, MC.make_eps(DIMS, 2, 165), 0.1, "finetune")
    assert obj.get_dropout() == (0.1, 5, 11), "a refused gradient call does not advance the draw"
    assert lib.m3pc_mtm_grad_get_dropout(obj._g, None, None, None) == 0, "the outputs are optional"


# ------------------------------------------------------------------------------------------------ the trainer
def test_train_is_three_train_steps(golden, planner, fresh):
    masks = {k: torch.from_numpy(golden[f"c2/mask/{k}"].astype(np.float64)) for k in R.KEYS}
    other = {k: torch.from_numpy(golden[f"c0/mask/{k}"].astype(np.float64)) for k in R.KEYS}
    per_step = [masks, other, masks]
    buf, _ = _filled_buffer(planner)
    try:
        tr = fresh(dropout=0.1, dropout_seed=21)
        assert tr.grad.get_dropout() == (0.1, 21, 0)
        step0 = buf.step
        recs, trecs = buf.mtm_train(tr, 3, per_step, batch_size=B)
        many = _snapshot(tr)
        assert tr.grad.get_dropout() == (0.1, 21, 3) and many["state"]["dropout_next_draw"] == 3
        recs = recs.cpu().numpy()
        assert np.isfinite(recs[:, 14]).all()
        tr2 = fresh(dropout=0.1, dropout_seed=21)
        buf.step = step0
        for i in range(3):
            eps_lib, _ = planner.handle.draw_variates(buf.seed, buf.step, B * T, A)
            seg = buf.traj_sample(batch_size=B)
            rec, _ = tr2.train_step_record(seg, per_step[i], eps_lib.reshape(B, T, A))
            assert rec.cpu().numpy().tobytes() == recs[i].tobytes(), i
        _same_bits(many, _snapshot(tr2), "m3pc_mtm_train vs three m3pc_mtm_train_step, with dropout")
        # without dropout the same three steps end elsewhere
        tr3 = fresh()
        buf.step = step0
        buf.mtm_train(tr3, 3, per_step, batch_size=B)
        w3 = _snapshot(tr3)["w"]
        assert any(w3[n].tobytes() != many["w"][n].tobytes() for n in w3)
        # a refused train call leaves the draw alone
        with pytest.raises(capi.M3pcError):
            buf.mtm_train(tr, 0, [], batch_size=B)
        assert tr.grad.get_dropout()[2] == 3
    finally:
        torch.cuda.synchronize()
        buf.close()


def test_state_round_trip_continues_the_stream(golden, fresh):
    batch = {k: torch.from_numpy(golden["batch/" + k]).cuda() for k in R.KEYS}
    masks, eps = {k: golden[f"c2/mask/{k}"] for k in R.KEYS}, torch.from_numpy(golden["c2/eps"]).cuda()
    tr = fresh(dropout=0.5, dropout_seed=33)
    tr.train_step_record(batch, masks, eps)
    tr.train_step_record(batch, masks, eps)
    st = tr.get_state()
    assert (st["dropout"], st["dropout_seed"], st["dropout_next_draw"]) == (0.5, 33, 2)
    w, (m, steps), v = tr.export_weights(), tr.export_moments(1, steps=True), tr.export_moments(2)
    torch.cuda.synchronize()
    w, m, v = ({k: t.clone() for k, t in d.items()} for d in (w, m, v))
    rec_a, _ = tr.train_step_record(batch, masks, eps)
    a = _snapshot(tr)
    tr2 = fresh()  # (reloads the recipe weights into the planner)
    full = dict(w)
    full["pos_embed"] = synth.make_state_dict(DIMS, 0)["pos_embed"]
    tr2.planner.load_state_dict({k: t.cpu() for k, t in full.items()})
    tr2.load_moments(1, m, steps)
    tr2.load_moments(2, v)
    tr2.set_state(**st)
    assert tr2.grad.get_dropout() == (0.5, 33, 2)
    rec_b, _ = tr2.train_step_record(batch, masks, eps)
    assert rec_a.cpu().numpy().tobytes() == rec_b.cpu().numpy().tobytes()
    _same_bits(a, _snapshot(tr2), "a resumed trainer continues with identical bits")


# ------------------------------------------------------------------------------------------------ the learner entry points
def test_mtm_update_and_attach_with_device_dropout(golden, sd):
    from fake_learner import make_learner
    cfg = _cfg(golden)
    batch, eps, masks = MC.make_batch(DIMS, B, 171), MC.make_eps(DIMS, B, 172), MC.random_masks(T, 173)
    tmasks = {k: torch.from_numpy(m.astype(np.float64)) for k, m in masks.items()}
    cb = {k: v.cuda() for k, v in batch.items()}

    def learner_with(dropout):
        ln = make_learner(DIMS, cfg, with_critic=False)
        ln.mtm = GradModule(sd, dropout=dropout)
        ln.mtm_optimizer, ln.mtm_scheduler, ln.temp_optimizer = _optimizers(dict(zip(ln.mtm.names, ln.mtm.ps)), ln.mtm.log_temperature)
        return ln

    ln = learner_with(0.1)
    p1 = attach(ln, precision="fp32", max_batch=4, max_windows=1, mtm_update=True)
    try:
        assert ln.mtm.training
        with pytest.raises(capi.M3pcError, match="dropout") as e:
            ln.mtm_update(cb, SHAPES, NO, masks=tmasks, eps=eps.cuda())
        assert '"device"' in str(e.value) and '"eval"' in str(e.value)
        before = ln.mtm.ps[0].detach().clone()
        log = ln.mtm_update(cb, SHAPES, NO, masks=tmasks, eps=eps.cuda(), dropout="device", dropout_seed=5)
        assert set(log) == LOG_KEYS and math.isfinite(log["train/loss"]) and not torch.equal(before, ln.mtm.ps[0].detach())
        assert p1._mtm_grad.get_dropout() == (0.1, 5, 1)
        ln.mtm_update(cb, SHAPES, NO, masks=tmasks, eps=eps.cuda(), dropout="device", dropout_seed=5)
        assert p1._mtm_grad.get_dropout() == (0.1, 5, 2), "the stream goes on from call to call"
        with pytest.raises(ValueError):
            ln.mtm_update(cb, SHAPES, NO, masks=tmasks, eps=eps.cuda(), dropout="torch")
    finally:
        torch.cuda.synchronize()
        if getattr(p1, "_mtm_grad", None) is not None:
            p1._mtm_grad.close()
        p1.handle.close()
    # attach(..., dropout="device") binds it: the rebound method steps without the keyword; the eval-mode step is another one
    logs = {}
    for how in ("device", "eval"):
        ln = learner_with(0.1)
        p2 = attach(ln, precision="fp32", max_batch=4, max_windows=1, mtm_update=True, dropout=how, dropout_seed=6)
        try:
            logs[how] = ln.mtm_update(cb, SHAPES, NO, masks=tmasks, eps=eps.cuda())
            assert p2._mtm_grad.get_dropout() == ((0.1, 6, 1) if how == "device" else (0.0, 0, 0))
        finally:
            torch.cuda.synchronize()
            p2._mtm_grad.close()
            p2.handle.close()
    assert set(logs["device"]) == LOG_KEYS and logs["device"]["train/loss"] != logs["eval"]["train/loss"]
    # the native route: the trainer carries the stream
    cfg.num_train_steps = 10
    ln = learner_with(0.1)
    p3 = attach(ln, precision="fp32", max_batch=4, max_windows=1, mtm_update="native", dropout="device", dropout_seed=8)
    try:
        log = ln.mtm_update(cb, SHAPES, NO, masks=tmasks, eps=eps.cuda())
        assert math.isfinite(log["train/loss"]) and p3._mtm_trainer.grad.get_dropout() == (0.1, 8, 1)
    finally:
        torch.cuda.synchronize()
        p3._mtm_trainer.close()
        p3.handle.close()


# ------------------------------------------------------------------------------------------------ limits and corners of the host state
def test_more_than_64_layers_is_refused_and_leaves_the_draw_alone():
    """The site id 4 layer + s has eight bits.  The refusal is a host check in front of the weights-loaded check: nothing is loaded."""
    hd = capi.Handle(S, A, T, n_embd=64, n_head=2, n_enc_layer=64, n_dec_layer=1, max_candidates=64, max_batch=1)
    g = DeviceMTMGrad(hd, 2)
    try:
        g.set_dropout(0.1, 3, 9)
        batch, eps, masks = MC.make_batch(DIMS, 2, 181), MC.make_eps(DIMS, 2, 182), MC.random_masks(T, 183)
        with pytest.raises(capi.M3pcError, match="65 layers"):
            MC.device_grads(g, batch, masks, eps, 0.1, "finetune")
        assert g.get_dropout() == (0.1, 3, 9)
    finally:
        g.close()
        hd.close()


def test_a_p_below_the_threshold_resolution_is_no_dropout(objs):
    plain, obj = objs(), objs()
    batch, eps, masks = MC.make_batch(DIMS, B, 184), MC.make_eps(DIMS, B, 185), MC.random_masks(T, 186)
    rec0, g0 = MC.device_grads(plain, batch, masks, eps, 0.1, "finetune")
    obj.set_dropout(2.0 ** -33, 3, 7)
    rec1, g1 = MC.device_grads(obj, batch, masks, eps, 0.1, "finetune")
    assert _bits(g0) == _bits(g1) and rec0.tobytes() == rec1.tobytes()
    assert obj.get_dropout() == (2.0 ** -33, 3, 7), "nothing dropped, nothing drawn"


def test_a_refused_trainer_leaves_nothing_open_and_eval_steps_keep_the_stream(golden, planner, fresh, sd):
    with pytest.raises(capi.M3pcError, match="set_dropout: p"):
        fresh(dropout=1.0)
    # HipPlanner.mtm_update: "eval" calls between "device" calls neither use nor reset the draw; another seed restarts it
    model = GradModule(sd, dropout=0.1)
    opt, sched, topt = _optimizers(dict(zip(model.names, model.ps)), model.log_temperature)
    batch, eps, masks = MC.make_batch(DIMS, B, 187), MC.make_eps(DIMS, B, 188), MC.random_masks(T, 189)
    cb = {k: v.cuda() for k, v in batch.items()}
    tm = {k: torch.from_numpy(m.astype(np.float64)) for k, m in masks.items()}
    step = lambda **kw: planner.mtm_update(cb, SHAPES, NO, model, opt, sched, topt, masks=tm, eps=eps.cuda(), **kw)
    try:
        step(dropout="device", dropout_seed=4)
        step(dropout="device", dropout_seed=4)
        assert planner._mtm_grad.get_dropout() == (0.1, 4, 2)
        step(dropout="eval")
        assert planner._mtm_grad.get_dropout() == (0.0, 4, 2)
        step(dropout="device", dropout_seed=4)
        assert planner._mtm_grad.get_dropout() == (0.1, 4, 3)
        step(dropout="device", dropout_seed=5)
        assert planner._mtm_grad.get_dropout() == (0.1, 5, 1)
    finally:
        torch.cuda.synchronize()
        planner.load_state_dict(sd)
        if getattr(planner, "_mtm_grad", None) is not None:
            planner._mtm_grad.close()
            planner._mtm_grad = None
