"""Shared by the GPU tests of m3pc_mtm_grad*: synthetic batches, mask sets, the device call, and the per-tensor comparison against the
float64 restatement (tests/mtm_grad_ref.py) under the bound  dev <= 16 x max(dev32[tensor], median of dev32 over the case's tensors)."""
import numpy as np
import torch

import mtm_grad_ref as GR
from m3pc_amd import synth
from m3pc_amd.mtm_grad import DeviceMTMGrad

KEYS = GR.KEYS
FACTOR = 16.0  # what tests/test_iql_gpu.py gives the device over ref32_grad_dev


def make_batch(dims: synth.Dims, B: int, seed: int):
    """A raw batch in the tokenizers' ranges; actions strictly inside (-0.95, 0.95), so both forms are finite without the clip."""
    g = torch.Generator().manual_seed(seed)
    T, S, A = dims.traj_length, dims.state_dim, dims.action_dim
    st = synth.make_tokenizer_stats(dims, 0)
    f = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float32)
    return {"states": torch.randn(B, T, S, generator=g) * f(st["states"]["std"]) + f(st["states"]["mean"]),
            "actions": torch.rand(B, T, A, generator=g) * 1.9 - 0.95,
            "rewards": torch.randn(B, T, 1, generator=g),
            "returns": torch.randn(B, T, 1, generator=g, dtype=torch.float64) * 3.0 + 5.0}


def make_eps(dims, B, seed):
    return torch.randn(B, dims.traj_length, dims.action_dim, generator=torch.Generator().manual_seed(seed))


def rows(T, **vis):
    """{key: (T,) uint8}; vis[key]: the visible timesteps (a list), "all" or "none"."""
    out = {}
    for k in KEYS:
        m = np.zeros(T, np.uint8)
        v = vis.get(k, "none")
        if isinstance(v, str):
            m[:] = 1 if v == "all" else 0
        else:
            m[list(v)] = 1
        out[k] = m
    return out


def mask_sets(T):
    """The edge sets of the issue; every one keeps at least one action timestep hidden."""
    return {
        "full_and_empty": rows(T, states="all", actions=[0, 1], rewards="none", returns=[0]),  # one key fully visible, another fully hidden
        "one_token": rows(T, states=[0]),                                                      # the smallest encoder the forward accepts
        "all_but_one_action": rows(T, states="all", actions=[t for t in range(T) if t != T // 2], rewards="all", returns="all"),
        "states_hidden": rows(T, actions=[0], returns="all"),                                  # no states token: encoder row 0 is an action's
        "middle_key_hidden": rows(T, states="all", rewards="all", returns=[T - 1]),            # a hidden key between two visible ones
    }


def random_masks(T, seed, p_visible=0.5):
    r = np.random.RandomState(seed)
    out = {k: (r.rand(T) < p_visible).astype(np.uint8) for k in KEYS}
    out["actions"][T - 1] = 0  # a hidden action timestep: total is finite
    out["states"][0] = 1
    return out


def device_grads(obj: DeviceMTMGrad, batch, masks, eps, reg, form):
    rec, gd = obj.grad({k: batch[k].cuda() for k in KEYS}, {k: torch.from_numpy(masks[k].astype(np.float64)) for k in KEYS}, reg, form=form, eps=eps.cuda())
    torch.cuda.synchronize()
    return rec.cpu().numpy(), {k: v.cpu().numpy().astype(np.float64) for k, v in gd.items()}


def reference(sd, ostats, batch, masks, eps, reg, form, n_head, want32=True):
    """(total64, g64, dev32 per tensor or None): the float64 restatement at the float32 clip bounds (the header's), and the
    float32 run's own deviation from it."""
    flags, bits = GR.FORMS[form]
    t64, g64 = GR.grads(sd, ostats, batch, masks, eps, reg, flags, bits, n_head, torch.float64, True)
    dev32 = None
    if want32:
        _, g32 = GR.grads(sd, ostats, batch, masks, eps, reg, flags, bits, n_head, torch.float32, True)
        dev32 = {}
        for n, g in g64.items():
            dev32[n] = np.nan if g is None or not np.isfinite(g).all() else GR.deviation(g32[n], g)
    return t64, g64, dev32


def compare(got, g64, dev32, what):
    """Every tensor: identically zero where g64 is (or autograd reaches nothing), else dev <= FACTOR x max(dev32, median dev32).
    A tensor whose float64 gradient is not finite (unspecified) is reported and skipped.  Prints every dev beside its bound."""
    fin = np.array([v for v in dev32.values() if np.isfinite(v) and v > 0])
    med = float(np.median(fin)) if fin.size else 0.0
    worst, bad = 0.0, []
    for n, g in g64.items():
        d = got[n]
        if g is None or not g.any():
            zero = not d.any()
            print(f"{what} {n}: structural zero, device identically zero: {zero}")
            if not zero:
                bad.append((n, "nonzero", float(np.abs(d).max())))
            continue
        if not np.isfinite(g).all():
            print(f"{what} {n}: float64 gradient not finite (unspecified); device finite: {bool(np.isfinite(d).all())}")
            continue
        dev, bound = GR.deviation(d, g), FACTOR * max(dev32[n], med)
        print(f"{what} {n}: dev {dev:.3e} bound {bound:.3e}")
        worst = max(worst, dev / bound)
        if not dev <= bound:
            bad.append((n, dev, bound))
    print(f"{what}: largest dev / bound = {worst:.3f}; median dev32 = {med:.2e}")
    assert not bad, (what, bad)
    return worst
