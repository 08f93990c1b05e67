"""The split-bf16 precision tier (M3PC_PREC_BF16X3) without a GPU: the constant across the header and the binding, the
precision names the planner and attach() take, and the CPU emulation of the x3 arithmetic (tools/bf16x3_study.py) against
bf16 on the oracle's candidate pass."""
import importlib.util
import os
import re
import types

import pytest

from m3pc_amd import capi, planner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(name):
    with open(os.path.join(ROOT, "include", "m3pc_hip.h")) as f:
        m = re.search(rf"#define\s+{name}\s+(\d+)", f.read())
    assert m, name
    return int(m.group(1))


def test_prec_bf16x3_matches_the_header():
    assert capi.PREC_BF16X3 == 2 == _define("M3PC_PREC_BF16X3")
    assert capi.ABI_VERSION == _define("M3PC_ABI_VERSION") == 7
    assert capi.PRECISIONS == {"fp32": capi.PREC_FP32, "bf16": capi.PREC_BF16, "bf16x3": capi.PREC_BF16X3}


def test_precision_names():
    assert capi.precision_code("bf16x3") == capi.PREC_BF16X3
    assert capi.precision_code("bf16") == capi.PREC_BF16
    assert capi.precision_code("fp32") == capi.PREC_FP32
    for bad in ("bf16x2", "x3", "BF16X3", "tf32", ""):
        with pytest.raises(ValueError):
            capi.precision_code(bad)


class _Stop(Exception):
    pass


def test_planner_parses_bf16x3_and_rejects_unknown_names(monkeypatch):
    """HipPlanner checks precision and fallback before it touches the library (the handle is the first GPU object it makes)."""
    from m3pc_amd import synth

    def no_handle(*a, **k):
        raise _Stop
    monkeypatch.setattr(capi, "Handle", no_handle)
    dims = synth.Dims(11, 3, 8, n_embd=64, n_head=2)
    sd, st = synth.make_state_dict(dims, 0), synth.make_tokenizer_stats(dims, 0)
    cfg = types.SimpleNamespace(traj_length=8, action_samples=16, horizon=4, discount=0.99, temperature=0.01, lmbda=0.6,
                                plan_guidance="rtg_guiding")
    for ok in ("bf16x3", "bf16", "fp32"):
        with pytest.raises(_Stop):
            planner.HipPlanner(cfg, sd, st, None, n_embd=64, n_head=2, precision=ok)
    with pytest.raises(_Stop):
        planner.HipPlanner(cfg, sd, st, None, n_embd=64, n_head=2, precision="bf16", fallback="bf16x3")
    with pytest.raises(ValueError):
        planner.HipPlanner(cfg, sd, st, None, n_embd=64, n_head=2, precision="bf16x4")
    with pytest.raises(ValueError):
        planner.HipPlanner(cfg, sd, st, None, n_embd=64, n_head=2, precision="bf16", fallback="bf16")


def test_attach_rejects_unknown_precision_before_reading_the_learner():
    with pytest.raises(ValueError):
        planner.attach(object(), precision="fp16")


def _study():
    spec = importlib.util.spec_from_file_location("bf16x3_study", os.path.join(ROOT, "tools", "bf16x3_study.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_split_is_exact_to_two_bf16_terms():
    import torch
    S = _study()
    x = torch.randn(4096, generator=torch.Generator().manual_seed(0)) * 100
    hi, lo = S.split_bf16(x)
    assert torch.equal(hi, x.to(torch.bfloat16).float()) and torch.equal(lo, lo.to(torch.bfloat16).float())
    assert float(((hi + lo - x).abs() / x.abs()).max()) <= 2.0 ** -16


def test_emulated_x3_deviation_is_a_hundredth_of_bf16():
    """The oracle's candidate pass at N = 256 (C2 shape otherwise), recipe weights of seed 0: the x3 arithmetic's deviation from
    fp32 is at most 1/100 of bf16's (the emulation measured ~500 x), and the arg-max is fp32's."""
    rows = {r["mode"]: r for r in _study().study(256, 0)}
    assert rows["bf16x3"]["dev_max"] <= rows["bf16"]["dev_max"] / 100, rows
    assert rows["bf16x3"]["argmax_match"]
    assert rows["bf16x3"]["dev_max"] <= 1e-4 * rows["bf16x3"]["score_scale"]
