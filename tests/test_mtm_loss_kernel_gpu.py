"""m3pc_mtm_loss_terms alone (mtm_loss.hip: mtm_loss_rows_kernel, mtm_loss_reduce_kernel) against the float64 restatement
(tests/mtm_loss_ref.py) on synthetic predictions.

Shapes (B, T, S, A): (1, 4, 11, 3) one row of waves; (3, 8, 17, 6) rows that are no multiple of a block's four; (5, 4, 1, 1) width-1
features everywhere; (64, 32, 11, 3) the fine-tuning loop's own batch, 2048 rows = eight rows per thread of the second stage.  Inputs:
std from exp(-5) to exp(2) with both ends exact, |mu| up to 8 with both ends exact (tanh saturated), target actions with exact +1 and
-1 at a hidden and at a visible timestep.  Masks: mixed; every rewards token visible (x / 0 in masked_loss); every returns token
hidden (x / 0 in masked_c_loss); every action visible (no timestep in the likelihood: NaN).

Bound, per scalar: |got - ref| <= 32 * 2^-24 * scale (scale: tests/mtm_loss_ref.py).  The sums are float64, so what is left is the
<= ~10 fp32 operations of <= 2 ulp each inside a term, and the one rounding of the result."""
import numpy as np
import pytest
import torch

import mtm_loss_ref as R
from m3pc_amd import capi

pytestmark = pytest.mark.gpu
SHAPES = [(1, 4, 11, 3), (3, 8, 17, 6), (5, 4, 1, 1), (64, 32, 11, 3)]
MASKS = ("mixed", "rewards_visible", "returns_hidden", "actions_visible")
SETTINGS = [(R.CLIP_ACTIONS, 1), (R.NORM_L2, 15), (R.CLIP_ACTIONS, 6), (R.NORM_L2, 1)]  # both flag settings, three loss_keys masks
BOUND = 32.0 * 2.0 ** -24
PAD = 16  # rows of batch the handle allows beyond the shape's (the padded determinism case)
_worst = {}


@pytest.fixture(scope="module")
def handles():
    hs = {}

    def get(B, T, S, A):
        if (B, T, S, A) not in hs:
            hs[(B, T, S, A)] = capi.Handle(S, A, T, n_embd=64, n_head=2, max_candidates=8, max_batch=B + PAD)
        return hs[(B, T, S, A)]

    yield get
    torch.cuda.synchronize()
    for h in hs.values():
        h.close()
    print("largest |got - ref| / (2^-24 scale) per scalar:", {R.RECORD_NAMES[i]: round(v, 2) for i, v in sorted(_worst.items())})


def _inputs(B, T, S, A, seed=0):
    rng = np.random.RandomState(1000 * seed + 7 * B + T + S)
    f = lambda *sh: rng.normal(size=sh).astype(np.float32)
    mu = rng.uniform(-8, 8, size=(B, T, A)).astype(np.float32)
    std = np.exp(rng.uniform(-5, 2, size=(B, T, A))).astype(np.float32)
    act = rng.uniform(-0.95, 0.95, size=(B, T, A)).astype(np.float32)
    # the ends: t = 0 is visible and t = T - 1 hidden under every action mask below but the all-visible one
    mu[0, 0, 0], mu[0, T - 1, 0], mu[-1, T - 1, -1] = 8.0, -8.0, 8.0
    std[0, 0, 0], std[0, T - 1, 0], std[-1, T - 1, -1], std[-1, 1, -1] = np.exp(-5.0), np.exp(2.0), np.exp(-5.0), np.exp(2.0)
    act[0, 0, 0], act[0, T - 1, 0], act[-1, 0, -1], act[-1, T - 1, -1] = 1.0, -1.0, -1.0, 1.0
    preds = [f(B, T, S), f(B, T, 1), f(B, T, 1), mu, std]
    targets = [f(B, T, S), act, f(B, T, 1), f(B, T, 1)]
    return preds, targets, f(B, T, A)


def _masks(kind, T, seed=0):
    rng = np.random.RandomState(seed + T)
    rows = []
    for k in range(4):
        m = (rng.uniform(size=T) < 0.5).astype(np.uint8)
        m[0], m[T - 1] = 1, 0
        rows.append(m)
    if kind == "rewards_visible":
        rows[2][:] = 1
    elif kind == "returns_hidden":
        rows[3][:] = 0
    elif kind == "actions_visible":
        rows[1][:] = 1
    return rows


def _cuda(xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def _check(got, ref, scale, what):
    assert R.same_specials(got, ref), (what, got, ref)
    ok = np.isfinite(ref)
    ratio = np.abs(got[ok].astype(np.float64) - ref[ok]) / (2.0 ** -24 * np.where(scale[ok] > 0, scale[ok], 1.0))
    for i, r in zip(np.nonzero(ok)[0], ratio):
        _worst[int(i)] = max(_worst.get(int(i), 0.0), float(r))
    print(what, "max |got - ref| / (2^-24 scale) = %.2f" % (ratio.max() if ratio.size else 0.0))
    bad = ratio > 32.0
    assert not bad.any(), (what, [(R.RECORD_NAMES[i], float(r)) for i, r in zip(np.nonzero(ok)[0][bad], ratio[bad])])
    assert got[4] == 0 and got[5] == 0


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_terms_against_float64(handles, shape, kind):
    B, T, S, A = shape
    h = handles(*shape)
    preds, targets, eps = _inputs(*shape)
    masks = _masks(kind, T)
    dp, dt, de = _cuda(preds), _cuda(targets), _cuda([eps])[0]
    for flags, keys in SETTINGS:
        rec = h.mtm_loss_terms(dp, dt, masks, de, 0.37, flags, keys)
        again = h.mtm_loss_terms(dp, dt, masks, de, 0.37, flags, keys)
        got, got2 = rec.cpu().numpy(), again.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), got2.view(np.uint32)), "two calls differ"
        ref, scale = R.loss_terms(*preds, targets, masks, eps, 0.37, flags, keys)
        _check(got, ref, scale, f"{shape} {kind} flags={flags} keys={keys}")
        # what the cases are there for
        if kind == "rewards_visible":
            assert np.isnan(got[3 * 2 + 1]) and np.isfinite(got[3 * 2 + 2])
        if kind == "returns_hidden":
            assert np.isnan(got[3 * 3 + 2]) and np.isfinite(got[3 * 3 + 1])
        if kind == "actions_visible":
            assert np.isnan(got[R.ENTROPY]) and np.isnan(got[R.NLL]) and np.isnan(got[R.TOTAL]) and np.isfinite(got[3])
        elif flags & R.CLIP_ACTIONS:
            assert np.isfinite(got[R.NLL]) and np.isfinite(got[R.TOTAL])
        else:  # a target of exactly -1 at the hidden timestep T - 1, unclipped: atanh is -inf, the log-probability inf - inf
            assert np.isnan(got[R.NLL]) and np.isnan(got[R.TOTAL]) and np.isfinite(got[R.ENTROPY])


def test_total_follows_entropy_reg_and_loss_keys(handles):
    shape = SHAPES[1]
    h = handles(*shape)
    preds, targets, eps = _inputs(*shape, seed=2)
    masks = _masks("mixed", shape[1])
    dp, dt, de = _cuda(preds), _cuda(targets), _cuda([eps])[0]
    for reg in (0.0, -1.5, 12.0):
        for keys in (0, 2, 9, 15):
            got = h.mtm_loss_terms(dp, dt, masks, de, reg, R.CLIP_ACTIONS, keys).cpu().numpy()
            ref, scale = R.loss_terms(*preds, targets, masks, eps, reg, R.CLIP_ACTIONS, keys)
            _check(got, ref, scale, f"reg={reg} keys={keys}")


def test_the_loops_batch_is_deterministic_and_ignores_rows_beyond_batch(handles):
    """64 x 32: the same bits from a second call, from inputs that live where m3pc_mtm_loss keeps them (other allocations, at
    addresses that are no multiple of a row), and with 16 more batch rows of NaN behind the 64 that count -- a reduction that
    depended on the launch geometry or read past `batch` would differ."""
    shape = SHAPES[3]
    B, T, S, A = shape
    h = handles(*shape)
    preds, targets, eps = _inputs(*shape, seed=1)
    masks = _masks("mixed", T)
    flags, keys = R.CLIP_ACTIONS, 1
    base = h.mtm_loss_terms(_cuda(preds), _cuda(targets), masks, _cuda([eps])[0], 0.1, flags, keys).cpu().numpy()
    assert np.isfinite(base[[0, 1, 2, 3, 12, 13, 14]]).all()

    def shifted(x):  # the same values, three floats into a larger block
        big = torch.full((x.size + 7,), float("nan"), dtype=torch.float32, device="cuda")
        big[3:3 + x.size] = torch.from_numpy(x.reshape(-1)).cuda()
        return big[3:3 + x.size].view(*x.shape)

    def padded(x):  # PAD more batch rows of NaN
        return torch.cat([torch.from_numpy(x).cuda(), torch.full((PAD,) + x.shape[1:], float("nan"), dtype=torch.float32, device="cuda")])

    for name, put in (("shifted", shifted), ("padded", padded)):
        p, t, e = [put(x) for x in preds], [put(x) for x in targets], put(eps)
        assert all(x.is_contiguous() for x in p + t + [e])
        got = h.mtm_loss_terms(p, t, masks, e, 0.1, flags, keys, batch=B).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), (name, got, base)
    # and a smaller batch of the same arrays is the smaller problem, not a slice of the larger one's sums
    got = h.mtm_loss_terms(_cuda(preds), _cuda(targets), masks, _cuda([eps])[0], 0.1, flags, keys, batch=5).cpu().numpy()
    ref, scale = R.loss_terms(*[x[:5] for x in preds], [x[:5] for x in targets], masks, eps[:5], 0.1, flags, keys)
    _check(got, ref, scale, "batch 5 of 64")
