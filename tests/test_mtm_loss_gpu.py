"""The masked-trajectory loss end to end (m3pc_mtm_loss, m3pc_mtm_loss_replay and their Python mirrors) on the golden captured from
the real reference (tests/golden/g8_mtm_loss.npz: Learner.compute_mtm_loss and omtm.forward_loss(norm="l2") on the g1_tiny model):
every scalar of both forms in fp32, the reference's dict contents from the mirrors, the record against the restatement on the call's
own head outputs in bf16 and bf16x3, the replay form against the plain one bit for bit, and a plan step before and after."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import mtm_loss_ref as R
import replay_ref
import variates_ref
from m3pc_amd import capi, mtm, synth
from m3pc_amd.planner import HipPlanner
from m3pc_amd.replay import DeviceReplayBuffer

pytestmark = pytest.mark.gpu
S, A, T, B = 11, 3, 8, 3
CASES = ("c0", "c1", "c2")
FORMS = {"finetune": R.FINETUNE, "pretrain": R.PRETRAIN}
HEADS = ("states", "rewards", "returns", "mu", "std")
KERNEL_BOUND = 32.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir + "/g8_mtm_loss.npz")


@pytest.fixture(scope="module")
def planner(golden):
    cfg = types.SimpleNamespace(traj_length=T, action_samples=64, horizon=4, discount=0.99, temperature=0.01, lmbda=0.6, plan_guidance="rtg_guiding",
                                device="cuda", index_jump=4, traj_batch_size=B, traj_buffer_size=4, trans_batch_size=6, trans_buffer_size=64,
                                select_mode="prob", mtm_iter_per_rollout=2, using_online_threshold=4,
                                mask_ratio=tuple(golden["mask_ratio"].tolist()), p_weights=tuple(golden["p_weights"].tolist()))
    dims = synth.Dims(S, A, T, n_embd=64, n_head=2)
    p = HipPlanner(cfg, synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0), None, n_embd=64, n_head=2, precision="fp32",
                   generator=torch.Generator(device="cuda").manual_seed(11), max_batch=4, max_windows=1)
    yield p
    torch.cuda.synchronize()
    p.handle.close()


def _batch(golden, order=R.KEYS):
    return {k: torch.from_numpy(golden["batch/" + k]).cuda() for k in order}


def _masks(golden, case):
    return [golden[f"{case}/mask/{k}"] for k in R.KEYS]


def _mask_dict(golden, case):
    return {k: torch.from_numpy(golden[f"{case}/mask/{k}"].astype(np.float64)) for k in R.KEYS}


def _eps(golden, case):
    return torch.from_numpy(golden[f"{case}/eps"]).cuda()


def _scale(golden, case, form):
    flags, bits = FORMS[form]
    return R.loss_terms(*[golden[f"{case}/head32/{n}"] for n in HEADS], [golden[f"{case}/target/{k}"] for k in R.KEYS], _masks(golden, case),
                        golden[f"{case}/eps"], float(golden["entropy_reg"]), flags, bits)[1]


def _close(got, gold, scale, have, what, tol=1e-4):
    got, gold = np.asarray(got, np.float64), np.asarray(gold, np.float64)
    assert R.same_specials(got[have], gold[have]), (what, got, gold)
    ok = have & np.isfinite(gold)
    dev = np.abs(got[ok] - gold[ok]) / np.maximum(np.abs(gold[ok]), scale[ok])
    print(what, "max |got - golden| / max(|golden|, scale) = %.2e" % dev.max())
    assert dev.max() <= tol, (what, dev)
    return dev.max()


@pytest.mark.parametrize("case", CASES)
def test_both_forms_are_the_reference_in_fp32(planner, golden, case):
    h, reg, b = planner.handle, float(golden["entropy_reg"]), _batch(golden)
    for form, (flags, bits) in FORMS.items():
        rec, heads = h.mtm_loss(b["states"], b["actions"], b["rewards"], b["returns"], _masks(golden, case), _eps(golden, case), reg, flags, bits,
                                want_heads=True)
        have = golden[f"{case}/{form}_have"]
        _close(rec.cpu().numpy(), golden[f"{case}/{form}32"], _scale(golden, case, form), have, f"{case} {form}")
        for name, hd in zip(HEADS, heads):  # the optional outs are the forward's heads
            assert np.abs(hd.cpu().numpy() - golden[f"{case}/head32/{name}"]).max() <= 1e-4 * max(1.0, np.abs(golden[f"{case}/head32/{name}"]).max()), name
        again = h.mtm_loss(b["states"], b["actions"], b["rewards"], b["returns"], _masks(golden, case), _eps(golden, case), reg, flags, bits)
        assert torch.equal(rec.view(torch.int32), again.view(torch.int32)), "with and without the optional outs"
    # float32 returns are the rounded float64 ones through the float32 tokenizer path: the same loss to rounding
    rec32 = h.mtm_loss(b["states"], b["actions"], b["rewards"], b["returns"].float(), _masks(golden, case), _eps(golden, case), reg, *FORMS["finetune"])
    _close(rec32.cpu().numpy(), golden[f"{case}/finetune32"], _scale(golden, case, "finetune"), golden[f"{case}/finetune_have"], f"{case} f32 returns")


@pytest.mark.parametrize("case", CASES)
def test_the_python_mirrors_return_the_reference_dicts(planner, golden, case):
    reg, eps, masks = float(golden["entropy_reg"]), _eps(golden, case), _mask_dict(golden, case)
    shapes = {"states": (1, S), "actions": (1, A), "rewards": (1, 1), "returns": (1, 1)}
    no = {k: False for k in R.KEYS}

    def record(tup):
        loss, losses, masked, masked_c, entropy = tup
        val, have = np.full(15, np.nan), np.zeros(15, bool)
        for j, k in enumerate(R.KEYS):
            for o, d in ((0, losses), (1, masked), (2, masked_c)):
                if k in d:
                    val[3 * j + o], have[3 * j + o] = float(d[k]), True
        val[R.ENTROPY], val[R.NLL], val[R.TOTAL] = float(losses["entropy"]), float(losses["nll"]), float(loss)
        have[[R.ENTROPY, R.NLL, R.TOTAL]] = True
        assert float(entropy) == float(losses["entropy"]) or np.isnan(float(entropy))
        return val, have, losses

    # the learner surface: compute_mtm_loss, the fine-tuning form with its early return
    val, have, losses = record(planner.compute_mtm_loss(_batch(golden), shapes, no, reg, masks=masks, eps=eps))
    assert list(losses) == ["states", "entropy", "nll"] and have.tolist() == golden[f"{case}/finetune_have"].tolist()
    _close(val, golden[f"{case}/finetune32"], _scale(golden, case, "finetune"), have, f"{case} compute_mtm_loss")
    if case != "c2":  # masks=None draws the reference's masks from NumPy's global generator
        np.random.seed(int(golden["case_seeds"][CASES.index(case)]))
        val2, have2, _ = record(planner.compute_mtm_loss(_batch(golden), shapes, no, reg, eps=eps))
        assert np.array_equal(val2[have2], val[have])
    # a batch whose keys start with the actions: the reference would hold actions and states, and add both to the total
    val, have, losses = record(planner.compute_mtm_loss(_batch(golden, ("actions", "states", "rewards", "returns")), shapes, no, reg, masks=masks, eps=eps))
    assert list(losses) == ["actions", "states", "entropy", "nll"]
    gold = golden[f"{case}/finetune32"]
    want_total = gold[R.TOTAL] + golden[f"{case}/pretrain32"][3]  # (loss_actions does not depend on the form)
    assert abs(val[R.TOTAL] - want_total) <= 1e-4 * max(abs(want_total), _scale(golden, case, "finetune")[R.TOTAL])
    # the model surface: omtm.compute_loss (one call) and omtm.forward_loss on forward's preds
    model = object.__new__(mtm.omtm)
    model.handle, model.precision = planner.handle, capi.PREC_FP32
    for form in FORMS:
        val, have, losses = record(model.compute_loss(_batch(golden), masks, reg, form=form, eps=eps))
        assert have.tolist() == golden[f"{case}/{form}_have"].tolist()
        _close(val, golden[f"{case}/{form}32"], _scale(golden, case, form), have, f"{case} compute_loss {form}")
    targets = planner.tokenizer_manager.encode(_batch(golden))
    for k in R.KEYS:
        assert np.abs(targets[k][:, :, 0].cpu().numpy() - golden[f"{case}/target/{k}"]).max() <= 1e-5, k
    preds = model.forward(targets, masks)
    val, have, losses = record(model.forward_loss(targets, preds, masks, reg, no, norm="l2", eps=eps))
    assert list(losses) == list(R.KEYS) + ["entropy", "nll"]
    _close(val, golden[f"{case}/pretrain32"], _scale(golden, case, "pretrain"), have, f"{case} forward_loss")
    val, have, _ = record(model.forward_loss(targets, preds, masks, reg, no, norm="none", loss_keys=["states", "returns"], eps=eps))
    assert val[0] > 0 and np.isclose(val[0], golden[f"{case}/finetune32"][0], rtol=1e-4)  # no normalisation: the fine-tuning form's loss_states


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_low_precision_records_are_the_restatement_on_their_own_heads(planner, golden, precision):
    h, reg, b = planner.handle, float(golden["entropy_reg"]), _batch(golden)
    worst = 0.0
    for case in CASES:
        for form, (flags, bits) in FORMS.items():
            rec, heads = h.mtm_loss(b["states"], b["actions"], b["rewards"], b["returns"], _masks(golden, case), _eps(golden, case), reg, flags, bits,
                                    precision=capi.precision_code(precision), want_heads=True)
            got = rec.cpu().numpy()
            ref, scale = R.loss_terms(*[x.cpu().numpy() for x in heads], [golden[f"{case}/target/{k}"] for k in R.KEYS], _masks(golden, case),
                                      golden[f"{case}/eps"], reg, flags, bits)
            assert R.same_specials(got, ref), (case, form, got, ref)
            ok = np.isfinite(ref)
            ratio = np.abs(got[ok] - ref[ok]) / (2.0 ** -24 * np.where(scale[ok] > 0, scale[ok], 1.0))  # (scale 0: the two empty slots)
            assert ratio.max() <= KERNEL_BOUND, (case, form, ratio)
            gold, have = golden[f"{case}/{form}32"], golden[f"{case}/{form}_have"]
            okg = have & np.isfinite(gold)
            gscale = _scale(golden, case, form)
            dev = (np.abs(got[okg] - gold[okg]) / np.maximum(np.abs(gold[okg]), gscale[okg])).max()
            worst = max(worst, dev)
            print(precision, case, form, "deviation from the golden %.2e (not asserted), kernel ratio %.2f" % (dev, ratio.max()))
    print(precision, "largest deviation from the golden over the cases and forms: %.2e" % worst)


def _filled_buffer(planner):
    cfg = planner.cfg
    buf = DeviceReplayBuffer(planner, cfg, 4, 40, discount=0.99, seed=5)
    model = replay_ref.HostReplay(S, A, 4, 40, T, 64, 64)
    rng = np.random.RandomState(9)
    for n in (8, 40, 23):
        obs, act, rew = np.zeros((40, S), np.float32), np.zeros((40, A), np.float32), np.zeros((40,), np.float32)
        obs[:n], act[:n], rew[:n] = rng.normal(size=(n, S)), rng.uniform(-1, 1, size=(n, A)), rng.normal(size=(n,))
        val = rng.normal(size=(40,)) * 10.0
        buf.append(obs[None], act[None], rew[None], val[None], [n])
        model.append(obs, act, rew, val, n)
    return buf, model


def test_the_replay_form_is_the_plain_one_on_the_drawn_rows(planner, golden):
    buf, model = _filled_buffer(planner)
    masks, reg = _mask_dict(golden, "c0"), 0.2
    rows = [golden[f"c0/mask/{k}"] for k in R.KEYS]
    eps = torch.randn(B, T, A, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    ti, si = np.array([1, 0, 2], np.int32), np.array([17, 0, 15], np.int32)
    for form, (flags, bits) in FORMS.items():
        tup, oi = buf.mtm_loss(masks, reg, form=form, indices=(ti, si), eps=eps, return_indices=True)
        seg = buf.traj_sample(indices=(ti, si))
        plain = planner.handle.mtm_loss(seg["states"], seg["actions"], seg["rewards"], seg["returns"], rows, eps, reg, flags, bits)
        want = mtm.loss_tuple(plain, mtm.form_settings(form, R.KEYS)[2])
        assert list(tup[1]) == list(want[1]) and torch.equal(tup[0].view(torch.int32), want[0].view(torch.int32))
        for d, w in zip(tup[1:4], want[1:4]):
            assert all(torch.equal(d[k].view(torch.int32), w[k].view(torch.int32)) for k in w), form
        assert oi[0].cpu().tolist() == ti.tolist() and oi[1].cpu().tolist() == si.tolist()
        assert torch.isfinite(tup[0]) == torch.isfinite(want[0])
    # the library's draws: the rows of replay_ref at (seed, step), eps of m3pc_draw_variates at the same (seed, step)
    step0 = buf.step
    tup, oi = buf.mtm_loss(masks, reg, batch_size=B, return_indices=True)
    assert buf.step == step0 + 1
    wi, ws = replay_ref.draw_segments(buf.seed, step0, B, replay_ref.LENGTH, model.lens, T)
    assert oi[0].cpu().tolist() == list(wi) and oi[1].cpu().tolist() == list(ws)
    eps_lib, _ = planner.handle.draw_variates(buf.seed, step0, B * T, A)
    assert np.abs(eps_lib.cpu().numpy() - variates_ref.eps(buf.seed, step0, B * T, A)).max() < 1e-5
    seg = buf.traj_sample(indices=(np.asarray(wi, np.int32), np.asarray(ws, np.int32)))
    plain = planner.handle.mtm_loss(seg["states"], seg["actions"], seg["rewards"], seg["returns"], rows, eps_lib.reshape(B, T, A), reg, *FORMS["finetune"])
    assert torch.equal(tup[0].view(torch.int32), plain[R.TOTAL].view(torch.int32)) and torch.equal(tup[4].view(torch.int32), plain[R.ENTROPY].view(torch.int32))
    # a buffer of another segment length is refused
    with pytest.raises(capi.M3pcError, match="m3pc error -1.*does not fit"):
        other = DeviceReplayBuffer(planner, types.SimpleNamespace(**{**vars(planner.cfg), "traj_length": T - 1}), 4, 40)
        other.mtm_loss(masks, reg)
    torch.cuda.synchronize()
    buf.close()


def test_a_plan_step_is_the_same_before_and_after_a_loss_call(planner, golden):
    """The loss call borrows the candidate workspace (its forward) and leaves nothing behind."""
    dims = synth.Dims(S, A, T, n_embd=64, n_head=2)
    hist = synth.make_history(dims, 0)
    hist["path_length"] = 100

    def step():
        planner.generator.manual_seed(21)
        planner._step_index = 0
        return [torch.as_tensor(planner.action_sample(hist, plan=True, eval=ev, rtg=3.0)).clone().cuda().float() for ev in (True, False)]

    before = step()
    b = _batch(golden)
    for precision in (capi.PREC_FP32, capi.PREC_BF16, capi.PREC_BF16X3):
        planner.handle.mtm_loss(b["states"], b["actions"], b["rewards"], b["returns"], _masks(golden, "c1"), _eps(golden, "c1"), 0.1, *FORMS["pretrain"],
                                precision=precision)
    after = step()
    for x, y in zip(before, after):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_mtm_loss_example(planner, golden, tmp_path):
    """examples/mtm_loss.c compiled with gcc -Wall -Werror against include/m3pc_hip.h, linked to the built library and run on a
    handle of its own: the records of its three evaluations are DeviceReplayBuffer.mtm_loss's on the same trajectories, masks, seed
    and steps, bit for bit."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    so = tmp_path / "libmtm_loss_example.so"
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(rocm, "include"), os.path.join(ROOT, "examples", "mtm_loss.c"), "-o", str(so),
                           "-L", libdir, "-l:" + os.path.basename(capi.LIB_PATH), "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-lm",
                           "-Wl,-rpath," + libdir])
    fp, vp = C.POINTER(C.c_float), C.c_void_p

    class IO(C.Structure):
        _fields_ = [("dims", C.POINTER(capi.Dims)), ("weights", C.POINTER(capi.NamedTensor)), ("n_weights", C.c_int),
                    ("tok_mean", fp * 4), ("tok_std", fp * 4), ("tok_dim", C.c_int * 4), ("tok_normalize", C.c_int * 4),
                    ("n_traj", C.c_int), ("max_steps", C.c_int), ("obs", vp), ("act", vp), ("rew", vp), ("val", vp), ("lens", vp),
                    ("n_evals", C.c_int), ("batch", C.c_int), ("masks", vp * 4), ("entropy_reg", C.c_float), ("seed", C.c_ulonglong),
                    ("record_dev", vp), ("records", vp)]

    n_traj, Ms, K, seed, reg = 3, 40, 3, 5, 0.2
    rng = np.random.RandomState(9)
    lens = np.array([8, 40, 23], np.int32)
    obs, act, rew = np.zeros((n_traj, Ms, S), np.float32), np.zeros((n_traj, Ms, A), np.float32), np.zeros((n_traj, Ms), np.float32)
    for i, n in enumerate(lens):
        obs[i, :n], act[i, :n], rew[i, :n] = rng.normal(size=(n, S)), rng.uniform(-1, 1, size=(n, A)), rng.normal(size=(n,))
    val = rng.normal(size=(n_traj, Ms)) * 10.0
    sd = synth.make_state_dict(synth.Dims(S, A, T, n_embd=64, n_head=2), 0)
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
    io.n_traj, io.max_steps, io.n_evals, io.batch, io.entropy_reg, io.seed = n_traj, Ms, K, B, reg, seed
    io.obs, io.act, io.rew, io.val, io.lens = obs.ctypes.data, act.ctypes.data, rew.ctypes.data, val.ctypes.data, lens.ctypes.data
    mrows = [np.ascontiguousarray(golden[f"c0/mask/{k}"]) for k in R.KEYS]
    for k in range(4):
        io.masks[k] = mrows[k].ctypes.data
    rec_dev = torch.zeros(capi.MTM_LOSS_FLOATS, dtype=torch.float32, device="cuda")
    records = np.zeros((K, capi.MTM_LOSS_FLOATS), np.float32)
    io.record_dev, io.records = rec_dev.data_ptr(), records.ctypes.data
    torch.cuda.synchronize()
    lib = C.CDLL(str(so))
    lib.mtm_loss_example.restype = C.c_int
    lib.mtm_loss_example.argtypes = [C.POINTER(IO), C.c_int, vp]
    rc = lib.mtm_loss_example(C.byref(io), torch.cuda.current_device(), vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, planner.handle.lib.m3pc_last_error()
    buf = DeviceReplayBuffer(planner, planner.cfg, n_traj, Ms, discount=0.99, seed=seed)
    buf.append(obs, act, rew, val, lens)
    for k in range(K):
        tup = buf.mtm_loss(_mask_dict(golden, "c0"), reg)
        assert np.isfinite(records[k][[0, 1, 2, 12, 13, 14]]).all()
        assert np.float32(tup[0].item()).tobytes() == records[k][R.TOTAL].tobytes() and np.float32(tup[4].item()).tobytes() == records[k][R.ENTROPY].tobytes()
        assert np.float32(tup[1]["states"].item()).tobytes() == records[k][0].tobytes()
    torch.cuda.synchronize()
    buf.close()
    del keep, toks
