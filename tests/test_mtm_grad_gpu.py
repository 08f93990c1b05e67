"""The gradient of the masked-trajectory loss end to end (m3pc_mtm_grad, _replay, _export and their Python mirrors) on the g1_tiny
model: every tensor against the float64 restatement (tests/mtm_grad_ref.py) under 16 x max(dev32[tensor], median dev32), dev32 the
REAL reference's own float32 deviation (tests/golden/g9_mtm_grad*.npz) for the golden cases.  The g8 batch has exact +-1 actions, so
what the golden cases pin differs by form: the fine-tuning form (which clips) is compared in every tensor for c0, c1, c2, with dev32 =
ref32_grad_dev_f32clip (both reference runs clipping at the float32 bounds the device and the restatement use; the plain ref32_grad_dev
of c1 is 1.6e-3, a difference of clip bounds, and would bound nothing); of the pretraining form c0 / c1 pin only that total is NaN and
the call returns M3PC_OK, c2 the 19 tensors not upstream of mu; c3 (c2's masks and eps, those actions at +-0.9) pins every tensor
of the pretraining form against the reference.  Then the record against the golden of
m3pc_mtm_loss; the replay form, the refusals, the workspace's independence, the example, and the learner-side mirrors."""
import ctypes as C
import math
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import mtm_grad_cases as MC
import mtm_grad_ref as GR
import mtm_loss_ref as R
from m3pc_amd import capi, synth
from m3pc_amd.mtm_grad import DeviceMTMGrad
from m3pc_amd.planner import HipPlanner, attach
from m3pc_amd.replay import DeviceReplayBuffer
from oracle import mtm_oracle as O
from test_mtm_loss_gpu import _close, _filled_buffer, _scale

pytestmark = pytest.mark.gpu
S, A, T, B = 11, 3, 8, 3
DIMS = synth.Dims(S, A, T, n_embd=64, n_head=2)
CASES = ("c0", "c1", "c2")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"states": (1, S), "actions": (1, A), "rewards": (1, 1), "returns": (1, 1)}
NO = {k: False for k in R.KEYS}
LOG_KEYS = {"train/loss_states", "train/masked_loss_states", "train/masked_c_loss_states", "train/loss_entropy", "train/loss_nll", "train/loss",
            "train/lr", "train/temperature", "train/entropy"}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir + "/g8_mtm_loss.npz")


@pytest.fixture(scope="module")
def g9(golden_dir):
    return np.load(golden_dir + "/g9_mtm_grad.npz")


def _cfg(golden):
    return types.SimpleNamespace(traj_length=T, action_samples=64, horizon=4, discount=0.99, temperature=0.01, lmbda=0.6, plan_guidance="rtg_guiding",
                                 device="cuda", index_jump=4, traj_batch_size=B, traj_buffer_size=4, trans_batch_size=6, trans_buffer_size=64,
                                 select_mode="prob", mtm_iter_per_rollout=2, using_online_threshold=4,
                                 mask_ratio=tuple(golden["mask_ratio"].tolist()), p_weights=tuple(golden["p_weights"].tolist()))


@pytest.fixture(scope="module")
def planner(golden):
    p = HipPlanner(_cfg(golden), synth.make_state_dict(DIMS, 0), synth.make_tokenizer_stats(DIMS, 0), None, n_embd=64, n_head=2, precision="fp32",
                   generator=torch.Generator(device="cuda").manual_seed(11), max_batch=4, max_windows=1)
    yield p
    torch.cuda.synchronize()
    p.handle.close()


@pytest.fixture(scope="module")
def obj(planner):
    g = DeviceMTMGrad(planner, 4)
    yield g
    torch.cuda.synchronize()
    g.close()


@pytest.fixture(scope="module")
def model_ref():
    return synth.make_state_dict(DIMS, 0), O.make_stats(synth.make_tokenizer_stats(DIMS, 0))


@pytest.fixture(scope="module")
def g9p(golden_dir):
    return np.load(golden_dir + "/g9_mtm_grad_pretrain.npz")


def _gbatch(golden):
    return {k: torch.from_numpy(golden["batch/" + k]) for k in R.KEYS}


def _gmasks(golden, case):
    return {k: golden[f"{case}/mask/{k}"] for k in R.KEYS}


def _bits(a):
    return a.tobytes()


@pytest.mark.parametrize("form", ["finetune", "pretrain"])
@pytest.mark.parametrize("case", CASES)
def test_golden_cases(planner, obj, golden, g9, model_ref, case, form):
    sd, ostats = model_ref
    reg, batch, masks, eps = float(golden["entropy_reg"]), _gbatch(golden), _gmasks(golden, case), torch.from_numpy(golden[f"{case}/eps"])
    rec, got = MC.device_grads(obj, batch, masks, eps, reg, form)
    _close(rec, golden[f"{case}/{form}32"], _scale(golden, case, form), golden[f"{case}/{form}_have"], f"{case} {form} record")
    flags, bits = GR.FORMS[form]
    b = {k: v.cuda() for k, v in batch.items()}
    loss = planner.handle.mtm_loss(b["states"], b["actions"], b["rewards"], b["returns"], [masks[k] for k in R.KEYS], eps.cuda(), reg, flags, bits).cpu().numpy()
    print(case, form, "record equals m3pc_mtm_loss(PREC_FP32) bit for bit:", _bits(rec) == _bits(loss))
    pre = f"{case}/{form}/"
    if not np.isfinite(float(g9[pre + "total64"])):  # an exact +-1 action at a hidden timestep, no clip: M3PC_OK, gradients unspecified
        assert not np.isfinite(rec[R.TOTAL])
        return
    names = [str(n) for n in g9["grad_names"]]
    key = "ref32_grad_dev_f32clip" if form == "finetune" else "ref32_grad_dev"
    dev32 = {n: (np.nan if g9[pre + "none"][i] else float(g9[pre + key][i])) for i, n in enumerate(names)}
    t64, g64, _ = MC.reference(sd, ostats, batch, masks, eps, reg, form, DIMS.n_head, want32=False)
    assert abs(rec[R.TOTAL] - t64) <= 1e-4 * max(1.0, abs(t64))
    MC.compare(got, g64, dev32, f"golden {case} {form}")


def test_golden_c3_pins_every_tensor_of_the_pretraining_form(obj, golden, g9p, model_ref):
    """c2's masks and eps on the g8 batch with its four +-1 actions at +-0.9: the real reference's backward is finite in all 90 tensors,
    and every one of them is compared (dev32 = the reference's own ref32_grad_dev of this case)."""
    sd, ostats = model_ref
    reg, batch, masks, eps = float(golden["entropy_reg"]), _gbatch(golden), _gmasks(golden, "c2"), torch.from_numpy(golden["c2/eps"])
    batch["actions"] = torch.from_numpy(g9p["c3/actions"])
    names = [str(n) for n in g9p["grad_names"]]
    ref = g9p["c3/pretrain/ref32_grad_dev"]
    assert len(names) == 90 and np.isfinite(ref).all() and not g9p["c3/pretrain/none"].any()
    rec, got = MC.device_grads(obj, batch, masks, eps, reg, "pretrain")
    t64, g64, _ = MC.reference(sd, ostats, batch, masks, eps, reg, "pretrain", DIMS.n_head, want32=False)
    assert abs(t64 - float(g9p["c3/pretrain/total64"])) <= 1e-9 * abs(t64) and abs(rec[R.TOTAL] - t64) <= 1e-4 * abs(t64)
    assert all(np.isfinite(g64[n]).all() for n in names)
    for n in names:  # the restatement is the stored float64 gradient of the reference (rounded to float32 in the file)
        gold = g9p["c3/pretrain/full/" + n].astype(np.float64).reshape(g64[n].shape)
        assert np.abs(g64[n] - gold).max() <= 2.0 ** -23 * np.abs(gold).max(), n
    MC.compare(got, g64, dict(zip(names, ref.tolist())), "golden c3 pretrain")


@pytest.mark.parametrize("name", ["full_and_empty", "one_token", "all_but_one_action"])
def test_golden_shape_mask_sets(obj, model_ref, name):
    sd, ostats = model_ref
    batch, eps, masks = MC.make_batch(DIMS, B, 31), MC.make_eps(DIMS, B, 32), MC.mask_sets(T)[name]
    for form in ("finetune", "pretrain"):
        rec, got = MC.device_grads(obj, batch, masks, eps, 0.1, form)
        t64, g64, dev32 = MC.reference(sd, ostats, batch, masks, eps, 0.1, form, DIMS.n_head)
        assert np.isfinite(t64) and abs(rec[R.TOTAL] - t64) <= 1e-4 * max(1.0, abs(t64))
        MC.compare(got, g64, dev32, f"golden-shape {name} {form}")
        if name == "full_and_empty":
            for n in ("mask_token_dict.states", "encoder_embed_dict.rewards.weight", "encoder_embed_dict.rewards.bias", "encoder_per_dim_encoding.rewards"):
                assert not got[n].any(), n


def test_total_nan_returns_ok(obj):
    """No hidden action timestep: total is NaN, the call still returns M3PC_OK and nothing faults."""
    batch, eps = MC.make_batch(DIMS, B, 33), MC.make_eps(DIMS, B, 34)
    rec, got = MC.device_grads(obj, batch, MC.rows(T, states=[0, 1], actions="all"), eps, 0.1, "finetune")
    assert np.isnan(rec[R.TOTAL])


def test_the_replay_form_is_sampling_then_grad(planner, obj, golden):
    buf, model = _filled_buffer(planner)
    other = DeviceMTMGrad(planner, 4)
    masks = {k: torch.from_numpy(golden[f"c0/mask/{k}"].astype(np.float64)) for k in R.KEYS}
    eps = torch.randn(B, T, A, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    ti, si = np.array([1, 0, 2], np.int32), np.array([17, 0, 15], np.int32)
    try:
        for form in ("finetune", "pretrain"):
            rec, oi = buf.mtm_grad(obj, masks, 0.2, form=form, indices=(ti, si), eps=eps, return_indices=True)
            ga = obj.export()
            seg = buf.traj_sample(indices=(ti, si))
            rec2, gb = other.grad(seg, masks, 0.2, form=form, eps=eps)
            torch.cuda.synchronize()
            assert torch.equal(rec.view(torch.int32), rec2.view(torch.int32)), form
            assert all(torch.equal(ga[n].view(torch.int32), gb[n].view(torch.int32)) for n in ga), form
            assert oi[0].cpu().tolist() == ti.tolist() and oi[1].cpu().tolist() == si.tolist()
        # the library's draws: rows and eps at (seed, step)
        step0 = buf.step
        rec, oi = buf.mtm_grad(obj, masks, 0.2, batch_size=B, return_indices=True)
        ga = obj.export()
        assert buf.step == step0 + 1
        eps_lib, _ = planner.handle.draw_variates(buf.seed, step0, B * T, A)
        seg = buf.traj_sample(indices=(oi[0].cpu().numpy(), oi[1].cpu().numpy()))
        rec2, gb = other.grad(seg, masks, 0.2, eps=eps_lib.reshape(B, T, A))
        torch.cuda.synchronize()
        assert torch.equal(rec.view(torch.int32), rec2.view(torch.int32))
        assert all(torch.equal(ga[n].view(torch.int32), gb[n].view(torch.int32)) for n in ga)
        with pytest.raises(capi.M3pcError, match="m3pc error -1.*does not fit"):
            wrong = DeviceReplayBuffer(planner, types.SimpleNamespace(**{**vars(planner.cfg), "traj_length": T - 1}), 4, 40)
            wrong.mtm_grad(obj, masks, 0.2)
    finally:
        torch.cuda.synchronize()
        other.close()
        buf.close()


def test_the_handle_computes_the_same_before_and_after(planner, obj, golden):
    """The gradient call never writes to the handle: a plan step and an m3pc_mtm_loss call give the same bits around it."""
    hist = synth.make_history(DIMS, 0)
    hist["path_length"] = 100
    b = {k: v.cuda() for k, v in _gbatch(golden).items()}
    mrows, eps = [golden[f"c1/mask/{k}"] for k in R.KEYS], torch.from_numpy(golden["c1/eps"]).cuda()

    def both():
        planner.generator.manual_seed(21)
        planner._step_index = 0
        acts = [torch.as_tensor(planner.action_sample(hist, plan=True, eval=ev, rtg=3.0)).clone().cuda().float() for ev in (True, False)]
        return acts + [planner.handle.mtm_loss(b["states"], b["actions"], b["rewards"], b["returns"], mrows, eps, 0.1, *R.PRETRAIN).clone()]

    before = both()
    MC.device_grads(obj, _gbatch(golden), _gmasks(golden, "c1"), torch.from_numpy(golden["c1/eps"]), 0.1, "pretrain")
    after = both()
    for x, y in zip(before, after):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_refusals(planner, obj, golden):
    lib, h = planner.handle.lib, planner.handle
    batch, eps = MC.make_batch(DIMS, B, 35), MC.make_eps(DIMS, B, 36)
    masks = MC.random_masks(T, 37)

    def refused(code, fn, *a, **k):
        with pytest.raises(capi.M3pcError, match=f"m3pc error {code}: .+"):
            fn(*a, **k)
        assert lib.m3pc_last_error()  # left set

    fresh = DeviceMTMGrad(planner, 2)
    try:
        refused(-2, fresh.export)  # export before any gradient call
        refused(-1, fresh.grad_record, batch, masks, 0.1, eps=eps)  # batch 3 > max_batch 2
    finally:
        fresh.close()
    out = C.c_void_p()
    for mb in (0, -3):
        assert lib.m3pc_mtm_grad_create(h._h, mb, C.byref(out)) == -1 and lib.m3pc_last_error()
    assert lib.m3pc_mtm_grad_create(None, 2, C.byref(out)) == -1
    refused(-1, obj.grad_record, batch, masks, 0.1, eps=eps, flags=8)
    refused(-1, obj.grad_record, batch, masks, 0.1, eps=eps, loss_keys=16)
    refused(-1, obj.grad_record, batch, MC.rows(T), 0.1, eps=eps)  # masks that keep no token: as m3pc_forward
    with pytest.raises(capi.M3pcError, match="mask keeps no token"):
        h.forward([torch.zeros(B, T, w, device="cuda") for w in (S, A, 1, 1)], [np.zeros(T, np.uint8)] * 4)
    obj.grad_record(batch, masks, 0.1, eps=eps)
    refused(-1, obj.export, {"pos_embed": torch.empty(T * 64, device="cuda")})
    refused(-1, obj.export, {"no.such.tensor": torch.empty(4, device="cuda")})
    refused(-1, obj.export, {"decoder.norm.weight": torch.empty(63, device="cuda")})
    host = obj.export({"decoder.norm.weight": torch.empty(64)})  # a host target
    assert torch.equal(host["decoder.norm.weight"], obj.export()["decoder.norm.weight"].cpu())
    # without weights, and without tokenizers
    bare = capi.Handle(S, A, T, 64, 2, 2, 1, max_candidates=8, max_batch=4)
    g = DeviceMTMGrad(bare, 4)
    try:
        buf = DeviceReplayBuffer(planner, planner.cfg, 4, 40)
        with pytest.raises(capi.M3pcError, match="another handle"):  # a gradient object of another handle with the same sizes
            buf.mtm_grad(g, masks, 0.1)
        buf.close()
        refused(-2, g.grad_record, batch, masks, 0.1, eps=eps)
        bare.load_weights(synth.make_state_dict(DIMS, 0))
        refused(-2, g.grad_record, batch, masks, 0.1, eps=eps)
    finally:
        torch.cuda.synchronize()
        g.close()
        bare.close()


def test_mtm_grad_example(planner, obj, golden, tmp_path):
    """examples/mtm_grad.c compiled with gcc -Wall -Werror against include/m3pc_hip.h, linked to the built library and run on a handle
    of its own: its record and its two exported gradients are DeviceReplayBuffer.mtm_grad's on the same trajectories, masks, seed and
    step, bit for bit."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    so = tmp_path / "libmtm_grad_example.so"
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(rocm, "include"), os.path.join(ROOT, "examples", "mtm_grad.c"), "-o", str(so),
                           "-L", libdir, "-l:" + os.path.basename(capi.LIB_PATH), "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-lm",
                           "-Wl,-rpath," + libdir])
    fp, vp = C.POINTER(C.c_float), C.c_void_p

    class IO(C.Structure):
        _fields_ = [("dims", C.POINTER(capi.Dims)), ("weights", C.POINTER(capi.NamedTensor)), ("n_weights", C.c_int),
                    ("tok_mean", fp * 4), ("tok_std", fp * 4), ("tok_dim", C.c_int * 4), ("tok_normalize", C.c_int * 4),
                    ("n_traj", C.c_int), ("max_steps", C.c_int), ("obs", vp), ("act", vp), ("rew", vp), ("val", vp), ("lens", vp),
                    ("batch", C.c_int), ("masks", vp * 4), ("entropy_reg", C.c_float), ("seed", C.c_ulonglong), ("step", C.c_ulonglong),
                    ("record_dev", vp), ("record", vp), ("grad_name", C.c_char_p * 2), ("grad", vp * 2), ("grad_numel", C.c_longlong * 2)]

    n_traj, Ms, seed, reg = 3, 40, 5, 0.2
    rng = np.random.RandomState(9)
    lens = np.array([8, 40, 23], np.int32)
    obs, act, rew = np.zeros((n_traj, Ms, S), np.float32), np.zeros((n_traj, Ms, A), np.float32), np.zeros((n_traj, Ms), np.float32)
    for i, n in enumerate(lens):
        obs[i, :n], act[i, :n], rew[i, :n] = rng.normal(size=(n, S)), rng.uniform(-1, 1, size=(n, A)), rng.normal(size=(n,))
    val = rng.normal(size=(n_traj, Ms)) * 10.0
    sd = synth.make_state_dict(DIMS, 0)
    arr, keep = capi._named(sd)
    io = IO()
    dims = capi.Dims(S, A, T, 64, 2, 2, 1, 64, 4, 0, 64, 0)
    io.dims, io.weights, io.n_weights = C.pointer(dims), C.cast(arr, C.POINTER(capi.NamedTensor)), len(sd)
    toks = []
    for k, name in enumerate(capi.KEYS):
        t = planner.tokenizer_manager.tokenizers[name]
        m, sdv = t._data_mean.float().contiguous().reshape(-1), t._data_std.float().contiguous().reshape(-1)
        toks.append((m, sdv))
        io.tok_mean[k], io.tok_std[k] = C.cast(m.data_ptr(), fp), C.cast(sdv.data_ptr(), fp)
        io.tok_dim[k], io.tok_normalize[k] = m.numel(), int(bool(t.normalize))
    io.n_traj, io.max_steps, io.batch, io.entropy_reg, io.seed, io.step = n_traj, Ms, B, reg, seed, 0
    io.obs, io.act, io.rew, io.val, io.lens = obs.ctypes.data, act.ctypes.data, rew.ctypes.data, val.ctypes.data, lens.ctypes.data
    mrows = [np.ascontiguousarray(golden[f"c0/mask/{k}"]) for k in R.KEYS]
    for k in range(4):
        io.masks[k] = mrows[k].ctypes.data
    rec_dev = torch.zeros(capi.MTM_LOSS_FLOATS, dtype=torch.float32, device="cuda")
    record = np.zeros(capi.MTM_LOSS_FLOATS, np.float32)
    names = ["encoder.layers.0.linear1.weight", "mask_token_dict.actions"]
    outs = [np.zeros(int(np.prod(obj.shapes[n])), np.float32) for n in names]
    io.record_dev, io.record = rec_dev.data_ptr(), record.ctypes.data
    for i in range(2):
        io.grad_name[i], io.grad[i], io.grad_numel[i] = names[i].encode(), outs[i].ctypes.data, outs[i].size
    torch.cuda.synchronize()
    lib = C.CDLL(str(so))
    lib.mtm_grad_example.restype = C.c_int
    lib.mtm_grad_example.argtypes = [C.POINTER(IO), C.c_int, vp]
    rc = lib.mtm_grad_example(C.byref(io), torch.cuda.current_device(), vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, planner.handle.lib.m3pc_last_error()
    buf = DeviceReplayBuffer(planner, planner.cfg, n_traj, Ms, discount=0.99, seed=seed)
    buf.append(obs, act, rew, val, lens)
    rec = buf.mtm_grad(obj, {k: torch.from_numpy(golden[f"c0/mask/{k}"].astype(np.float64)) for k in R.KEYS}, reg)
    want = obj.export()
    torch.cuda.synchronize()
    assert np.isfinite(record[R.TOTAL]) and _bits(rec.cpu().numpy()) == _bits(record)
    for n, o in zip(names, outs):
        assert o.any() and _bits(want[n].cpu().numpy().reshape(-1)) == _bits(o), n
    buf.close()
    del keep, toks


# ------------------------------------------------------------------------------------------------ the learner-side mirrors
class GradModule(torch.nn.Module):
    """The model as a trainer holds it: Parameters (requires_grad) under their state_dict names, pos_embed a buffer, and the
    temperature of the reference model (mtm_model.py: log_temperature, temperature(), target_entropy)."""

    def __init__(self, sd, dropout=0.0, init_temperature=0.1, device="cuda"):
        super().__init__()
        self.names = [k for k in sd if k != "pos_embed"]
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(sd[k].clone().to(device)) for k in self.names])
        self.register_buffer("pos", sd["pos_embed"].clone().to(device))
        self.log_temperature = torch.nn.Parameter(torch.tensor(math.log(init_temperature), device=device))
        self.target_entropy = -float(A)
        self.config = types.SimpleNamespace(n_embd=64, n_head=2, n_enc_layer=2, n_dec_layer=1, dropout=dropout)

    def temperature(self):
        return self.log_temperature.exp()

    def state_dict(self, *a, keep_vars=False, **k):
        out = {n: (p if keep_vars else p.detach()) for n, p in zip(self.names, self.ps)}
        out["pos_embed"] = self.pos
        return out


def _optimizers(params_by_name, log_temperature, t_max=10):
    """torch.optim.AdamW in two groups (weight decay 5e-3 on the 2-D Linear weights), the cosine LambdaLR, Adam on the temperature."""
    decay = [p for n, p in params_by_name.items() if p.dim() == 2]
    rest = [p for n, p in params_by_name.items() if p.dim() != 2]
    opt = torch.optim.AdamW([{"params": decay, "weight_decay": 5e-3}, {"params": rest, "weight_decay": 0.0}], lr=1e-3, betas=(0.9, 0.999))
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 0.5 * (1.0 + math.cos(math.pi * min(s, t_max) / t_max)))
    return opt, sched, torch.optim.Adam([log_temperature], lr=1e-2)


def _cpu_steps(sd, ostats, steps, dtype):
    """The same three mtm_update steps in the restatement on the CPU: -> {name: float64 ndarray} of the parameters afterwards."""
    p = GR.cast_state_dict(sd, dtype)
    names = GR.param_names(p)
    log_t = torch.tensor(math.log(0.1), dtype=dtype, requires_grad=True)
    opt, sched, topt = _optimizers({n: p[n] for n in names}, log_t)
    flags, bits = GR.FINETUNE
    for batch, masks, eps in steps:
        tokens = GR.tokens_of(batch, ostats)
        out = O.mtm_forward(p, tokens, masks, DIMS.n_head)
        total, parts = GR.loss_total(out, tokens, masks, eps, float(log_t.detach().exp()), flags, bits, dtype, True)
        opt.zero_grad(set_to_none=True)
        total.backward()
        opt.step()
        sched.step()
        topt.zero_grad()
        (log_t.exp() * (parts["entropy"].detach() - (-float(A)))).backward()
        topt.step()
    return {n: p[n].detach().to(torch.float64).numpy() for n in names}


def test_backward_into_fills_every_parameter_and_nothing_else(planner, obj, golden):
    model = GradModule(synth.make_state_dict(DIMS, 0))
    batch, eps, masks = MC.make_batch(DIMS, B, 81), MC.make_eps(DIMS, B, 82), MC.random_masks(T, 83)
    rec = obj.backward_into(model, {k: v.cuda() for k, v in batch.items()}, masks, 0.1, "finetune", eps.cuda())
    want = obj.export()
    torch.cuda.synchronize()
    assert np.isfinite(rec.cpu().numpy()[R.TOTAL])
    for n, p in zip(model.names, model.ps):
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.is_cuda, n
        assert torch.equal(p.grad.reshape(-1), want[n].reshape(-1)), n
    assert model.log_temperature.grad is None and model.pos.grad is None
    obj.backward_into(model, {k: v.cuda() for k, v in batch.items()}, masks, 0.1, "finetune", eps.cuda(), unused="none")
    for n, p in zip(model.names, model.ps):
        outside = n.startswith("output_head_dict.rewards.") or n.startswith("output_head_dict.returns.")
        assert (p.grad is None) == outside, n


def test_three_mtm_update_steps_follow_the_restatement(planner, model_ref):
    sd, ostats = model_ref
    steps = [(MC.make_batch(DIMS, B, 90 + i), MC.random_masks(T, 93 + i), MC.make_eps(DIMS, B, 96 + i)) for i in range(3)]
    model = GradModule(sd)
    opt, sched, topt = _optimizers(dict(zip(model.names, model.ps)), model.log_temperature)
    try:
        for batch, masks, eps in steps:
            log = planner.mtm_update({k: v.cuda() for k, v in batch.items()}, SHAPES, NO, model, opt, sched, topt,
                                     masks={k: torch.from_numpy(m.astype(np.float64)) for k, m in masks.items()}, eps=eps.cuda())
            assert set(log) == LOG_KEYS, sorted(log)
            assert math.isfinite(log["train/loss"]) and isinstance(log["train/loss"], float)
        torch.cuda.synchronize()
        p64, p32 = _cpu_steps(sd, ostats, steps, torch.float64), _cpu_steps(sd, ostats, steps, torch.float32)
        dev32 = {n: GR.deviation(p32[n], p64[n]) for n in p64}
        fin = np.array([v for v in dev32.values() if v > 0])
        med = float(np.median(fin))
        bad = []
        for n, p in zip(model.names, model.ps):
            dev, bound = GR.deviation(p.detach().cpu().numpy().astype(np.float64), p64[n]), MC.FACTOR * max(dev32[n], med)
            print(f"after three steps {n}: dev {dev:.3e} bound {bound:.3e}")
            if not dev <= bound:
                bad.append((n, dev, bound))
        assert not bad, bad
        moved = max(float((p.detach().cpu() - sd[n]).abs().max()) for n, p in zip(model.names, model.ps))
        assert moved > 1e-4, "the optimizer stepped"
    finally:
        planner.load_state_dict(sd)  # the module-scoped planner goes back to the recipe weights
        if getattr(planner, "_mtm_grad", None) is not None:
            planner._mtm_grad.close()
            planner._mtm_grad = None


def test_dropout_refusal_and_attach_rebind(golden):
    from fake_learner import make_learner
    cfg = _cfg(golden)
    sd = synth.make_state_dict(DIMS, 0)
    batch, eps, masks = MC.make_batch(DIMS, B, 84), MC.make_eps(DIMS, B, 85), MC.random_masks(T, 86)
    tmasks = {k: torch.from_numpy(m.astype(np.float64)) for k, m in masks.items()}
    cb = {k: v.cuda() for k, v in batch.items()}

    def learner_with(dropout):
        ln = make_learner(DIMS, cfg, with_critic=False)
        ln.mtm = GradModule(sd, dropout=dropout)
        ln.mtm_optimizer, ln.mtm_scheduler, ln.temp_optimizer = _optimizers(dict(zip(ln.mtm.names, ln.mtm.ps)), ln.mtm.log_temperature)
        ln.mtm_update = "the learner's own"
        return ln

    ln = learner_with(0.1)
    p0 = attach(ln, precision="fp32", max_batch=4, max_windows=1)
    assert ln.mtm_update == "the learner's own", "the default attach leaves mtm_update alone"
    p0.handle.close()
    ln = learner_with(0.1)
    p1 = attach(ln, precision="fp32", max_batch=4, max_windows=1, mtm_update=True)
    try:
        assert callable(ln.mtm_update)
        assert ln.mtm.training
        with pytest.raises(capi.M3pcError, match="dropout"):
            ln.mtm_update(cb, SHAPES, NO, masks=tmasks, eps=eps.cuda())
        before = ln.mtm.ps[0].detach().clone()
        log = ln.mtm_update(cb, SHAPES, NO, masks=tmasks, eps=eps.cuda(), dropout="eval")
        assert set(log) == LOG_KEYS and not torch.equal(before, ln.mtm.ps[0].detach())
        ln.mtm.eval()  # eval mode: nothing to refuse
        log2 = ln.mtm_update(cb, SHAPES, NO, masks=tmasks, eps=eps.cuda())
        assert set(log2) == LOG_KEYS and log2["train/loss"] != log["train/loss"], "the second step saw the stepped weights (_sync)"
    finally:
        torch.cuda.synchronize()
        if getattr(p1, "_mtm_grad", None) is not None:
            p1._mtm_grad.close()
        p1.handle.close()
