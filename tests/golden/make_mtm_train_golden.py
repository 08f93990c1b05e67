#!/usr/bin/env python3
"""Generate tests/golden/g10_mtm_train.npz by running the REAL reference on the CPU: K = 4 calls of ``Learner.mtm_update``
(finetune_omtm/learner.py:506-538) with its real ``omtm.configure_optimizers`` (mtm_model.py:779-841), ``LambdaLR`` and temperature
Adam, built as learner.py:42-58 builds them, on the eval-mode g1_tiny model, the g8 batch and the masks and eps of its case c2 (the
``Eps`` and ``FixedMasks`` devices of make_mtm_loss_golden.py, imported from it) -- lr 1e-3, weight_decay 5e-3, num_train_steps 10 --
once in float32 and once in float64.

Contents (data only): ``decay_names`` / ``no_decay_names`` (the optimizer's two groups, by parameter identity); ``stateless_names``
(parameters without optimizer state after the K steps: .grad stayed None) and ``stateless_same_bits`` (their weights kept their
bits); ``names`` (every parameter, in order); the hyper-parameters, ``target_entropy`` and ``init_log_temperature``; per step
``loss32`` / ``loss64`` (train/loss), ``lr``, ``temperature32`` / ``temperature64``, ``entropy32`` / ``entropy64``; and per tensor of
the update p_K - p_0 of the float64 run ``sums`` ((n, 2): sum, sum of squares), ``head/{name}`` (the leading 1024 entries, float64)
and ``ref32_upd_dev`` (the relative L2 deviation of the float32 run's update from it).

Usage:  python tests/golden/make_mtm_train_golden.py /path/to/reference
"""
import os
import sys
import types

import numpy as np
import torch
from torch.optim.lr_scheduler import LambdaLR

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_mtm_loss_golden as G  # noqa: E402  (parses the reference path and imports the reference)

from research.omtm.models.mtm_model import omtm  # noqa: E402

K = 4
CASE = "c2"
LR, WD, NUM_TRAIN_STEPS = 1e-3, 5e-3, 10
HEAD = 1024


def run(g8, dtype):
    L = G.build(dtype)
    model = L.mtm
    assert not model.training
    L.cfg.learning_rate, L.cfg.weight_decay, L.cfg.num_train_steps = LR, WD, NUM_TRAIN_STEPS
    cfg = L.cfg
    L.mtm_optimizer = omtm.configure_optimizers(model, learning_rate=cfg.learning_rate, weight_decay=cfg.weight_decay, betas=(0.9, 0.999))

    def _schedule(step):
        return 0.5 * (1 + np.cos(step / cfg.num_train_steps * np.pi))

    L.mtm_scheduler = LambdaLR(L.mtm_optimizer, lr_lambda=_schedule)
    L.temp_optimizer = torch.optim.Adam([model.log_temperature], lr=1e-4, betas=[0.9, 0.999])
    assert model.log_temperature.dtype == torch.float64
    names = [n for n, _ in model.named_parameters()]
    by_id = {id(p): n for n, p in model.named_parameters()}
    groups = [[by_id[id(p)] for p in g["params"]] for g in L.mtm_optimizer.param_groups]
    assert [g["weight_decay"] for g in L.mtm_optimizer.param_groups] == [WD, 0.0]
    p0 = {n: p.detach().clone() for n, p in model.named_parameters()}
    init_log_t = float(model.log_temperature.detach())
    batch = {k: torch.from_numpy(g8["batch/" + k]) for k in G.R.KEYS}
    T = G.DIMS.traj_length
    masks = {k: torch.from_numpy(g8[f"{CASE}/mask/{k}"].astype(np.float64)).reshape(T, 1) for k in G.R.KEYS}
    eps = torch.from_numpy(g8[f"{CASE}/eps"])[None, :, :, None, :]
    logs = []
    with torch.enable_grad():
        for _ in range(K):
            with G.Eps(eps), G.FixedMasks(masks):
                log = L.mtm_update(batch, G.DIMS.data_shapes, G.DISCRETE)
            logs.append({k: float(log[k]) for k in ("train/loss", "train/lr", "train/temperature", "train/entropy")})
    upd = {n: (p.detach().to(torch.float64) - p0[n].to(torch.float64)).numpy() for n, p in model.named_parameters()}
    stateless = [n for n, p in model.named_parameters() if len(L.mtm_optimizer.state.get(p, {})) == 0]
    same = [bool(torch.equal(p.detach(), p0[n])) for n, p in model.named_parameters() if n in stateless]
    return dict(names=names, groups=groups, logs=logs, upd=upd, stateless=stateless, same=same, init_log_t=init_log_t,
                target_entropy=float(model.target_entropy), sched=int(L.mtm_scheduler.last_epoch))


def main():
    g8 = np.load(os.path.join(HERE, "g8_mtm_loss.npz"))
    r32, r64 = run(g8, torch.float32), run(g8, torch.float64)
    assert r32["names"] == r64["names"] and r32["groups"] == r64["groups"] and r32["stateless"] == r64["stateless"]
    names = [n for n in r64["names"] if n != "log_temperature"]
    out = {"names": np.array(names), "decay_names": np.array(r64["groups"][0]), "no_decay_names": np.array(r64["groups"][1]),
           "stateless_names": np.array(r64["stateless"]), "stateless_same_bits": np.array(r64["same"]) & np.array(r32["same"]),
           "K": np.int64(K), "learning_rate": np.float64(LR), "weight_decay": np.float64(WD), "num_train_steps": np.int64(NUM_TRAIN_STEPS),
           "init_log_temperature": np.float64(r64["init_log_t"]), "target_entropy": np.float64(r64["target_entropy"]),
           "case": np.array(CASE)}
    for key, tag in (("train/loss", "loss"), ("train/temperature", "temperature"), ("train/entropy", "entropy")):
        out[tag + "32"] = np.array([l[key] for l in r32["logs"]])
        out[tag + "64"] = np.array([l[key] for l in r64["logs"]])
    out["lr"] = np.array([l["train/lr"] for l in r64["logs"]])
    assert out["lr"].tolist() == [l["train/lr"] for l in r32["logs"]]
    sums, dev = np.zeros((len(names), 2)), np.zeros(len(names))
    for i, n in enumerate(names):
        u64, u32 = r64["upd"][n], r32["upd"][n]
        sums[i] = u64.sum(), (u64 * u64).sum()
        nrm = np.sqrt((u64 * u64).sum())
        dev[i] = 0.0 if nrm == 0 else np.sqrt(((u32 - u64) ** 2).sum()) / nrm
        out["head/" + n] = u64.reshape(-1)[:HEAD].copy()
    out["sums"], out["ref32_upd_dev"] = sums, dev
    path = os.path.join(HERE, "g10_mtm_train.npz")
    np.savez_compressed(path, **out)
    moved = dev[sums[:, 1] > 0]
    print("groups: %d decaying / %d non-decaying; stateless: %d (same bits: %s)" % (len(r64["groups"][0]), len(r64["groups"][1]),
                                                                                    len(r64["stateless"]), bool(out["stateless_same_bits"].all())))
    print("lr:", out["lr"].tolist())
    print("temperature 32 vs 64: max rel %.2e" % np.abs(out["temperature32"] / out["temperature64"] - 1).max())
    print("loss 32 vs 64: rel", (np.abs(out["loss32"] - out["loss64"]) / np.abs(out["loss64"])).tolist())
    print("ref32_upd_dev: median %.2e; above 1/16: %s" % (np.median(moved), [(n, float(dev[i])) for i, n in enumerate(names) if dev[i] >= 1 / 16]))
    print("second largest class: max below 1/16 = %.2e" % dev[dev < 1 / 16].max())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
