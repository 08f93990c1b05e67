"""The kernels of m3pc_mtm_grad at their edges, against the float64 restatement (tests/mtm_grad_ref.py): row counts that are no
multiple of the 32-row tile and cross 128 (odd), the shipped widths with hd = 128 and K = 2048 products (wide), L = 256 (long),
hd = 64 with feature widths that are multiples of 4 and dW products of 3 and 6 rows (hd64), traj_length 1 (one), the
mask sets with structural zeros, without a states token and with a hidden key between visible ones, and run-to-run determinism.
(The kernels one by one: tests/test_mtm_grad_kernel_edges_gpu.py.)  Bound per tensor: 16 x max(dev32[tensor], median dev32 of the case),
dev32 the float32 restatement's own deviation (tests/mtm_grad_cases.py)."""
import numpy as np
import pytest
import torch

import mtm_grad_cases as MC
import mtm_loss_ref as R
from hip_util import make_handle
from m3pc_amd import capi, synth
from m3pc_amd.mtm_grad import DeviceMTMGrad

pytestmark = pytest.mark.gpu
REG = 0.1
ODD = synth.Dims(17, 6, 5, n_embd=128, n_head=4)
WIDE = synth.Dims(11, 3, 8, n_embd=512, n_head=4)
LONG = synth.Dims(11, 3, 64, n_embd=64, n_head=2)
HD64 = synth.Dims(12, 8, 3, n_embd=64, n_head=1)   # head_dim 64, feature widths that are multiples of 4, dW products of 3 and 6 rows
ONE = synth.Dims(17, 6, 1, n_embd=64, n_head=2)    # traj_length 1: L = 4, one row per row-map group


def _setup(dims, max_batch):
    h, sd, ostats, _ = make_handle(dims, max_candidates=8, max_batch=max_batch)
    return h, sd, ostats, DeviceMTMGrad(h, max_batch)


def _check_record(rec, h, batch, masks, eps, form):
    """the record is m3pc_mtm_loss's on the same batch (its fp32 forward runs other kernels): close at 1e-4; bit equality is reported"""
    flags, bits = R.FINETUNE if form == "finetune" else R.PRETRAIN
    want = h.mtm_loss(*[batch[k].cuda() for k in R.KEYS], [masks[k] for k in R.KEYS], eps.cuda(), REG, flags, bits).cpu().numpy()
    assert R.same_specials(rec, want), (rec, want)
    ok = np.isfinite(want)
    dev = np.abs(rec[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1.0)
    print("record vs m3pc_mtm_loss(PREC_FP32): max dev %.2e, bit for bit: %s" % (dev.max(), rec.tobytes() == want.tobytes()))
    assert dev.max() <= 1e-4


@pytest.fixture(scope="module")
def odd():
    h, sd, ostats, obj = _setup(ODD, 7)
    yield h, sd, ostats, obj
    torch.cuda.synchronize()
    obj.close()
    h.close()


@pytest.mark.parametrize("form", ["finetune", "pretrain"])
@pytest.mark.parametrize("B", [1, 3, 7])
def test_odd_rows(odd, B, form):
    h, sd, ostats, obj = odd
    batch, eps, masks = MC.make_batch(ODD, B, 100 + B), MC.make_eps(ODD, B, 200 + B), MC.random_masks(ODD.traj_length, 300 + B)
    rec, got = MC.device_grads(obj, batch, masks, eps, REG, form)
    t64, g64, dev32 = MC.reference(sd, ostats, batch, masks, eps, REG, form, ODD.n_head)
    assert np.isfinite(t64) and abs(rec[R.TOTAL] - t64) <= 1e-4 * max(1.0, abs(t64))
    _check_record(rec, h, batch, masks, eps, form)
    MC.compare(got, g64, dev32, f"odd B={B} {form}")


@pytest.mark.parametrize("name", ["full_and_empty", "one_token", "all_but_one_action", "states_hidden", "middle_key_hidden"])
def test_odd_mask_sets(odd, name):
    h, sd, ostats, obj = odd
    B = 3
    batch, eps, masks = MC.make_batch(ODD, B, 41), MC.make_eps(ODD, B, 42), MC.mask_sets(ODD.traj_length)[name]
    for form in ("finetune", "pretrain"):
        rec, got = MC.device_grads(obj, batch, masks, eps, REG, form)
        t64, g64, dev32 = MC.reference(sd, ostats, batch, masks, eps, REG, form, ODD.n_head)
        assert np.isfinite(t64) and np.isfinite(rec[R.TOTAL])
        MC.compare(got, g64, dev32, f"odd {name} {form}")
        if name == "full_and_empty":
            for n in ("mask_token_dict.states", "encoder_embed_dict.rewards.weight", "encoder_embed_dict.rewards.bias", "encoder_per_dim_encoding.rewards"):
                assert not got[n].any(), n
        if form == "finetune":
            for n, g in got.items():
                if n.startswith("output_head_dict.rewards") or n.startswith("output_head_dict.returns"):
                    assert not g.any(), n


@pytest.mark.parametrize("form", ["finetune", "pretrain"])
@pytest.mark.parametrize("B", [1, 2])
def test_head_dim_64_and_feature_widths_that_are_multiples_of_four(B, form):
    h, sd, ostats, obj = _setup(HD64, 2)
    try:
        batch, eps, masks = MC.make_batch(HD64, B, 81 + B), MC.make_eps(HD64, B, 82 + B), MC.random_masks(HD64.traj_length, 83 + B)
        rec, got = MC.device_grads(obj, batch, masks, eps, REG, form)
        t64, g64, dev32 = MC.reference(sd, ostats, batch, masks, eps, REG, form, HD64.n_head)
        assert np.isfinite(t64) and abs(rec[R.TOTAL] - t64) <= 1e-4 * max(1.0, abs(t64))
        _check_record(rec, h, batch, masks, eps, form)
        MC.compare(got, g64, dev32, f"hd64 B={B} {form}")
    finally:
        torch.cuda.synchronize()
        obj.close()
        h.close()


def test_traj_length_one():
    """L = 4: the states token visible, the action hidden."""
    h, sd, ostats, obj = _setup(ONE, 3)
    try:
        B = 3
        batch, eps, masks = MC.make_batch(ONE, B, 91), MC.make_eps(ONE, B, 92), MC.rows(1, states="all", rewards="all")
        for form in ("finetune", "pretrain"):
            rec, got = MC.device_grads(obj, batch, masks, eps, REG, form)
            t64, g64, dev32 = MC.reference(sd, ostats, batch, masks, eps, REG, form, ONE.n_head)
            assert np.isfinite(t64) and abs(rec[R.TOTAL] - t64) <= 1e-4 * max(1.0, abs(t64))
            _check_record(rec, h, batch, masks, eps, form)
            MC.compare(got, g64, dev32, f"traj_length 1 {form}")
    finally:
        torch.cuda.synchronize()
        obj.close()
        h.close()


def test_wide():
    h, sd, ostats, obj = _setup(WIDE, 2)
    try:
        batch, eps, masks = MC.make_batch(WIDE, 2, 51), MC.make_eps(WIDE, 2, 52), MC.random_masks(WIDE.traj_length, 53)
        rec, got = MC.device_grads(obj, batch, masks, eps, REG, "pretrain")
        t64, g64, dev32 = MC.reference(sd, ostats, batch, masks, eps, REG, "pretrain", WIDE.n_head)
        assert np.isfinite(t64)
        _check_record(rec, h, batch, masks, eps, "pretrain")
        MC.compare(got, g64, dev32, "wide pretrain")
    finally:
        torch.cuda.synchronize()
        obj.close()
        h.close()


def test_long():
    h, sd, ostats, obj = _setup(LONG, 1)
    try:
        batch, eps, masks = MC.make_batch(LONG, 1, 61), MC.make_eps(LONG, 1, 62), MC.random_masks(LONG.traj_length, 63, p_visible=0.4)
        rec, got = MC.device_grads(obj, batch, masks, eps, REG, "pretrain")
        t64, g64, dev32 = MC.reference(sd, ostats, batch, masks, eps, REG, "pretrain", LONG.n_head)
        assert np.isfinite(t64)
        _check_record(rec, h, batch, masks, eps, "pretrain")
        MC.compare(got, g64, dev32, "long pretrain")
    finally:
        torch.cuda.synchronize()
        obj.close()
        h.close()


def test_two_calls_and_a_smaller_batch_are_bit_identical(odd):
    h, sd, ostats, _ = odd
    big, eps4 = MC.make_batch(ODD, 4, 71), MC.make_eps(ODD, 4, 72)
    small, eps2 = MC.make_batch(ODD, 2, 73), MC.make_eps(ODD, 2, 74)
    masks = MC.random_masks(ODD.traj_length, 75)
    a, b = DeviceMTMGrad(h, 4), DeviceMTMGrad(h, 4)
    try:
        r1, g1 = MC.device_grads(a, big, masks, eps4, REG, "pretrain")
        r2, g2 = MC.device_grads(a, big, masks, eps4, REG, "pretrain")
        assert r1.tobytes() == r2.tobytes() and all(g1[n].tobytes() == g2[n].tobytes() for n in g1)
        r3, g3 = MC.device_grads(a, small, MC.mask_sets(ODD.traj_length)["full_and_empty"], eps2, REG, "finetune")  # behind the batch of 4
        r4, g4 = MC.device_grads(b, small, MC.mask_sets(ODD.traj_length)["full_and_empty"], eps2, REG, "finetune")  # a fresh object
        assert r3.tobytes() == r4.tobytes() and all(g3[n].tobytes() == g4[n].tobytes() for n in g3)
    finally:
        torch.cuda.synchronize()
        a.close()
        b.close()
