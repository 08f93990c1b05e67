"""CPU checks of the device optimizers of the masked-trajectory model: the float64 restatement (tests/mtm_opt_ref.py) chained
against torch.optim.AdamW(foreach=False) + LambdaLR + torch.optim.Adam on the CPU within the bound it derives; the host-only entries
m3pc_mtm_lr and the refusals that need no GPU; the decay rule and the schedule against the real reference's recorded run
(tests/golden/g10_mtm_train.npz); the names of the new C entries across the header and capi."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import mtm_opt_ref as OR
from m3pc_amd import build, capi, mtm_train
from m3pc_amd.mtm_grad import param_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m3pc_mtm_opt_create", "m3pc_mtm_opt_destroy", "m3pc_mtm_lr", "m3pc_mtm_opt_decays", "m3pc_mtm_opt_step", "m3pc_mtm_train_step",
       "m3pc_mtm_train", "m3pc_mtm_opt_export", "m3pc_mtm_opt_load", "m3pc_mtm_weights_export", "m3pc_mtm_opt_get_state", "m3pc_mtm_opt_set_state")


@pytest.fixture(scope="module")
def lib():
    return capi.load_library(build.build_library())


@pytest.fixture(scope="module")
def g10(golden_dir):
    return np.load(golden_dir + "/g10_mtm_train.npz")


def test_new_entries_are_declared_exported_and_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "m3pc_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
    assert C.sizeof(capi.MtmOptArgs) == 13 * 8 and C.sizeof(capi.MtmOptState) == 6 * 8
    for src in ("mtm_opt.hip",):
        assert src in build.SOURCES


@pytest.mark.parametrize("warmup", [0, 3])
def test_restatement_follows_torch(warmup):
    """K steps of AdamW in two groups, with tensors whose .grad stays None (skipped entirely, step count and all), an all-zero
    gradient (stepped) and both schedules, in float64 on fp32-representable inputs: the restatement, fed its own outputs, stays
    within its own bound of torch at every step; then the float64 Adam of the temperature."""
    rng = np.random.RandomState(3)
    names = ["a.weight", "a.bias", "output_head_dict.rewards.1.weight", "output_head_dict.rewards.1.bias", "blk.norm1.weight", "mask_token_dict.rewards"]
    shapes = [(5, 7), (7,), (4, 4), (4,), (6,), (1, 1, 3)]
    bits = 0b0011  # states, actions: the rewards head is outside
    N, K, lr0, wd = 9, 5, 1e-2, 5e-2
    p = {n: rng.normal(size=s).astype(np.float32).astype(np.float64) for n, s in zip(names, shapes)}
    tp = {n: torch.nn.Parameter(torch.from_numpy(p[n].copy())) for n in names}
    dec = [n for n in names if OR.decays(n)]
    assert dec == ["a.weight", "output_head_dict.rewards.1.weight"]
    opt = torch.optim.AdamW([{"params": [tp[n] for n in dec], "weight_decay": wd}, {"params": [tp[n] for n in names if n not in dec], "weight_decay": 0.0}],
                            lr=lr0, betas=(0.9, 0.999), foreach=False)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: float(OR.lr_lambda(s, N, warmup)))
    m = {n: np.zeros_like(p[n]) for n in names}
    v = {n: np.zeros_like(p[n]) for n in names}
    steps = {n: 0 for n in names}
    worst = 0.0
    for k in range(K):
        g = {n: rng.normal(size=p[n].shape).astype(np.float32).astype(np.float64) * (10.0 ** rng.randint(-6, 3)) for n in names}
        g["mask_token_dict.rewards"][:] = 0.0  # an exact-zero gradient IS stepped
        for n in names:
            tp[n].grad = torch.from_numpy(g[n].copy()) if OR.active(n, bits) else None
        lr_t = OR.lr_at(k, lr0, N, warmup)
        assert sched.get_last_lr()[0] == pytest.approx(lr_t, rel=4e-16)
        out = OR.adamw(p, g, m, v, steps, lr_t, wd, bits)
        opt.step()
        sched.step()
        for n in names:
            pr, mr, vr, st, bp, bm, bv = out[n]
            if not OR.active(n, bits):
                assert st == 0 and not len(opt.state.get(tp[n], {})) and np.array_equal(pr, p[n]) and not bp.any()
                assert np.array_equal(tp[n].detach().numpy(), p[n])
            else:
                assert st == k + 1 == int(opt.state[tp[n]]["step"])
                for got, ref, bound in ((tp[n].detach().numpy(), pr, bp), (opt.state[tp[n]]["exp_avg"].numpy(), mr, bm),
                                        (opt.state[tp[n]]["exp_avg_sq"].numpy(), vr, bv)):
                    worst = max(worst, OR.worst(got, ref, bound))
            p[n], m[n], v[n], steps[n] = pr, mr, vr, st
    print("restatement vs torch float64 AdamW: worst err / bound %.3e" % worst)
    assert worst <= 1.0
    assert steps["mask_token_dict.rewards"] == K and steps["output_head_dict.rewards.1.bias"] == 0
    # the temperature
    log_t = torch.tensor(math.log(0.1), dtype=torch.float64, requires_grad=True)
    topt = torch.optim.Adam([log_t], lr=1e-4, betas=[0.9, 0.999])
    st = (math.log(0.1), 0.0, 0.0, 0)
    for k in range(K):
        ent = float(np.float32(rng.normal() * 3))
        topt.zero_grad()
        (log_t.exp() * (torch.tensor(ent, dtype=torch.float64) - (-3.0))).backward()
        topt.step()
        new = OR.temperature_step(st[0], st[1], st[2], st[3], ent, -3.0)
        assert abs(float(log_t.detach()) - new[0]) <= new[4], (k, float(log_t.detach()), new)
        st = new[:4]


def test_decay_rule_and_schedule_against_the_reference_run(lib, g10):
    names = [str(n) for n in g10["names"]]
    dec, nodec = {str(n) for n in g10["decay_names"]}, {str(n) for n in g10["no_decay_names"]}
    assert len(names) == 90 and len(dec) == 28 and len(nodec - {"log_temperature"}) == 62 and dec | nodec >= set(names)
    shapes = param_shapes(11, 3, 64, 2, 1)
    assert set(shapes) == set(names)
    for n in names:
        assert OR.decays(n) == (n in dec) == mtm_train.decays(n), n
    stateless = sorted(str(n) for n in g10["stateless_names"] if str(n) != "log_temperature")
    assert stateless == sorted(n for n in names if not OR.active(n, 0b0001)) and len(stateless) == 12 and g10["stateless_same_bits"].all()
    args = capi.MtmOptArgs.make(float(g10["learning_rate"]), float(g10["weight_decay"]), int(g10["num_train_steps"]), float(g10["target_entropy"]),
                                float(g10["init_log_temperature"]))
    for k, want in enumerate(g10["lr"].tolist()):
        out = C.c_double()
        assert lib.m3pc_mtm_lr(C.byref(args), k, C.byref(out)) == 0
        assert abs(out.value - want) <= np.spacing(want), (k, out.value, want)
        assert abs(mtm_train.lr_at(k, args.learning_rate, args.num_train_steps) - want) <= np.spacing(want)
    # the temperature of the float64 run from its own recorded entropies, through the restatement
    st = (float(g10["init_log_temperature"]), 0.0, 0.0, 0)
    for k in range(int(g10["K"])):
        new = OR.temperature_step(st[0], st[1], st[2], st[3], float(g10["entropy64"][k]), float(g10["target_entropy"]))
        assert abs(math.exp(new[0]) - float(g10["temperature64"][k])) <= 1e-12 * float(g10["temperature64"][k])
        st = new[:4]


def test_lr_with_warmup_and_refusals_without_gpu(lib):
    args = capi.MtmOptArgs.make(3e-4, 0.01, 100, -3.0, math.log(0.1), warmup_steps=10)
    out = C.c_double()
    for s in (0, 1, 9, 10, 11, 55, 100):
        assert lib.m3pc_mtm_lr(C.byref(args), s, C.byref(out)) == 0
        want = OR.lr_at(s, 3e-4, 100, 10)
        assert abs(out.value - want) <= np.spacing(max(want, 1e-300)), (s, out.value, want)
    assert lib.m3pc_mtm_lr(C.byref(args), 0, None) == -1 and b"lr" in lib.m3pc_last_error()
    assert lib.m3pc_mtm_lr(None, 0, C.byref(out)) == -1 and b"args" in lib.m3pc_last_error()
    assert lib.m3pc_mtm_lr(C.byref(args), -1, C.byref(out)) == -1 and b"sched_step" in lib.m3pc_last_error()
    for field, bad in (("learning_rate", -1.0), ("learning_rate", float("nan")), ("weight_decay", -0.1), ("beta1", 1.0), ("beta2", -0.1), ("eps", 0.0),
                       ("num_train_steps", 0), ("warmup_steps", 100), ("temp_learning_rate", float("inf")), ("temp_beta1", 1.5), ("temp_beta2", 1.0),
                       ("temp_eps", -1.0), ("target_entropy", float("nan")), ("init_log_temperature", float("inf"))):
        a = capi.MtmOptArgs.make(3e-4, 0.01, 100, -3.0, math.log(0.1), warmup_steps=10)
        setattr(a, field, bad)
        assert lib.m3pc_mtm_lr(C.byref(a), 0, C.byref(out)) == -1, field
        assert field.encode() in lib.m3pc_last_error(), (field, lib.m3pc_last_error())
    o = C.c_void_p()
    assert lib.m3pc_mtm_opt_create(None, C.byref(args), C.byref(o)) == -1 and b"null" in lib.m3pc_last_error()
    assert lib.m3pc_mtm_opt_destroy(None) == 0
    assert lib.m3pc_mtm_opt_step(None, None) == -1 and b"opt" in lib.m3pc_last_error()
    assert lib.m3pc_mtm_train_step(None, 1, None, None, None, None, 0, None, None, 0, 1, None, None, None) == -1
    assert lib.m3pc_mtm_train(None, None, 1, 1, 0, 0, 0, None, 0, 1, None, None, None) == -1
    assert lib.m3pc_mtm_opt_export(None, 1, None, 0, None, None) == -1 and lib.m3pc_mtm_opt_load(None, 1, None, 0, None, None) == -1
    assert lib.m3pc_mtm_weights_export(None, None, 0, None) == -1
    assert lib.m3pc_mtm_opt_get_state(None, None) == -1 and lib.m3pc_mtm_opt_set_state(None, None) == -1
    d = C.c_int(5)
    assert lib.m3pc_mtm_opt_decays(None, b"x", C.byref(d)) == -1 and d.value == -1
