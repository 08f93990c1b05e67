#!/usr/bin/env python3
"""Generate tests/golden/g6_replay.npz by running the REAL reference ``ReplayBuffer`` (finetune_omtm/replay_buffer.py) on the CPU.

Runs only where the reference checkout exists (pass its path, or set M3PC_REFERENCE); the .npz written here is data only.  The
reference is imported unmodified with empty stub modules for packages that are absent and unused on this path: ``wandb``, ``gym``,
``tqdm``, ``d4rl`` and ``research.jaxrl.datasets.d4rl_dataset``.  The dataset, the config and the two online episodes are the
recipes of tests/replay_ref.py (the golden stores their seed); the dataset and the config are SimpleNamespaces.

Per case ("uniform" with discount 0.99; "prob" with discount 1.5, i.e. use_avg) the capture holds: the buffer after __init__
(arrays, path_lengths, p, values_up_bound, the offline transitions), one traj_sample and one trans_sample with the indices that
np.random.choice / np.random.randint / random.sample returned during the call (the three are wrapped while it runs), the buffer
after two real ``online_rollout`` calls on a toy environment (each ends in ``update_buffer``; the online transitions included), and
a traj_sample and a trans_sample behind them.

Usage:  python tests/golden/make_replay_golden.py /path/to/reference
"""
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("M3PC_REFERENCE")
if not REFERENCE or not os.path.isdir(os.path.join(REFERENCE, "research")):
    sys.exit("usage: make_replay_golden.py /path/to/reference  (the checkout that holds research/finetune_omtm/replay_buffer.py)")
for _name in ("wandb", "gym", "tqdm", "d4rl", "research.jaxrl.datasets.d4rl_dataset"):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules["gym"].Env = object
sys.modules["research.jaxrl.datasets.d4rl_dataset"].D4RLDataset = object
sys.path.insert(0, REFERENCE)

from research.finetune_omtm.replay_buffer import ReplayBuffer  # noqa: E402

import replay_ref as R  # noqa: E402

SEED = 20240611
CASES = (("uniform", 0.99), ("prob", 1.5))


class Tap:
    """Record what np.random.choice / np.random.randint / random.sample return while a reference method runs."""

    def __enter__(self):
        self.choice, self.randint, self.sample = [], [], []
        self._c, self._r, self._s = np.random.choice, np.random.randint, random.sample

        def choice(*a, **k):
            out = self._c(*a, **k)
            self.choice.append(np.array(out))
            return out

        def randint(*a, **k):
            out = self._r(*a, **k)
            self.randint.append(int(out))
            return out

        def sample(population, k):
            # (random.sample picks positions and returns population[position]: on range(len) the same state gives the positions)
            idx = self._s(range(len(population)), k)
            self.sample.append(np.array(idx))
            return [population[i] for i in idx]

        np.random.choice, np.random.randint, random.sample = choice, randint, sample
        return self

    def __exit__(self, *exc):
        np.random.choice, np.random.randint, random.sample = self._c, self._r, self._s


class ToyEnv:
    """Plays back one episode of the recipe: reset() shows row 0, step t returns row t + 1 and reward t; done after the last."""

    def __init__(self, obs, rew):
        self.obs, self.rew, self.t = obs, rew, 0

    def reset(self):
        self.t = 0
        return self.obs[0]

    def step(self, action):
        r = self.rew[self.t]
        self.t += 1
        return self.obs[self.t], r, self.t >= len(self.rew), {}


def transitions(dq):
    return [np.stack([np.asarray(getattr(e, f), dtype=np.float32).reshape(-1) for e in dq])
            for f in ("state", "action", "reward", "next_state", "done")]


def batches(buf, out, tag):
    with Tap() as tap:
        b = buf.traj_sample()
    for k, v in b.items():
        out[f"{tag}.traj.{k}"] = v.numpy()
    out[f"{tag}.traj.index"], out[f"{tag}.traj.start"] = tap.choice[0].astype(np.int32), np.array(tap.randint, dtype=np.int32)
    with Tap() as tap:
        t = buf.trans_sample()
    for k, v in zip(("state", "action", "reward", "next_state", "done"), t):
        out[f"{tag}.trans.{k}"] = v.numpy()
    out[f"{tag}.trans.index"] = np.concatenate(tap.sample).astype(np.int32)
    out[f"{tag}.trans.n_online"] = np.int32(len(tap.sample[0]) if len(tap.sample) == 2 else 0)


def state(buf, out, tag):
    out[f"{tag}.observations"], out[f"{tag}.actions"] = buf.observations_segmented, buf.actions_segmented
    out[f"{tag}.rewards"], out[f"{tag}.values"] = buf.rewards_segmented, buf.values_segmented
    out[f"{tag}.path_lengths"], out[f"{tag}.p"], out[f"{tag}.values_up_bound"] = np.asarray(buf.path_lengths), buf.p, buf.values_up_bound


def capture(mode, discount):
    out = {}
    cfg = R.golden_config(mode)
    np.random.seed(SEED)
    random.seed(SEED)
    buf = ReplayBuffer(cfg, types.SimpleNamespace(env=None, **R.golden_dataset(SEED)), discount=discount, max_path_length=R.GOLDEN_M)
    assert buf.values_segmented.dtype == np.float64 and buf.observations_segmented.dtype == np.float32
    state(buf, out, "init")
    for k, v in zip(("state", "action", "reward", "next_state", "done"), transitions(buf.offline_trans_buffer)):
        out[f"init.offline.{k}"] = v
    batches(buf, out, "first")
    for k in range(len(R.GOLDEN_ROLLOUTS)):
        obs, act, rew = R.golden_rollout(SEED, k)
        buf.env = ToyEnv(obs, rew)
        buf.online_rollout(lambda traj, percentage, plan, a=act: torch.from_numpy(a[traj["path_length"]]), 1)
    state(buf, out, "updated")
    for k, v in zip(("state", "action", "reward", "next_state", "done"), transitions(buf.online_trans_buffer)):
        out[f"updated.online.{k}"] = v
    out["updated.total_step"] = np.int64(buf.total_step)
    batches(buf, out, "second")
    assert out["second.traj.returns"].dtype == np.float64 and out["second.traj.states"].dtype == np.float32
    return out


def main():
    data = {"seed": np.int64(SEED), "torch_version": np.array(torch.__version__), "numpy_version": np.array(np.__version__)}
    for mode, discount in CASES:
        data[f"{mode}.discount"] = np.float64(discount)
        for k, v in capture(mode, discount).items():
            data[f"{mode}.{k}"] = v
    path = os.path.join(HERE, "g6_replay.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes,", len(data), "arrays")


if __name__ == "__main__":
    main()
