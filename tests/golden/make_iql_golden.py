#!/usr/bin/env python3
"""Generate tests/golden/g7_iql.npz by running the REAL reference ``ImplicitQLearning`` (finetune_omtm/model.py) on the CPU, once in
float32 and once as a ``.double()`` copy of itself, from the same weights and batches.

Runs only where the reference checkout exists (pass its path, or set M3PC_REFERENCE); the .npz written here is data only.  The
reference is imported unmodified with an empty stub module for ``gym``, which this path does not use.  Weights and batches are the
recipes of tests/iql_ref.py (which keep every row of every batch away from the ReLU, expectile and clamp kinks at the parameters of
the float64 run); q_target is loaded with a draw of its own after construction.

Per case of iql_ref.CASES the capture holds
  the 20 losses of both runs; the fixture conditions of the float64 run (tests/test_iql_cpu.py asserts them), found by iql_ref on the
  same inputs;
  ref32_grad_dev   per tensor, max|g32 - g64| / max|g64| of the first step's gradient, g = exp_avg / (1 - beta1) in both runs;
  ref32_loss_dev   per loss, the largest relative deviation of the float32 run over the 20 steps;
  ref32_param_dev  per tensor, max|p32 - p64| after the 20 steps; ref32_traj_dev, its largest over the tensors of the case
(what the float32 arithmetic of the reference itself loses: the GPU tests allow the device 16 times that), and for the case h64
the first batch, the first step's exp_avg / exp_avg_sq and the final parameters of both runs (exp_avg_sq of the float32 run only).

Not stored, although a capture could hold them: the initial state and the batches after the first, even for h64 (and for the other
hidden-64 cases, a32 and b1024, not the first batch, moments and final parameters either: the file stays below the size a committed
file may have).
Both are functions of a seed (tests/iql_ref.py), so the capture and the tests build the same arrays; what ties the recipes to this
capture is the equality of the first batch and, for every case, the 20 float64 losses at 1e-10, which no other weights or batches
reproduce (tests/test_iql_cpu.py).

Usage:  python tests/golden/make_iql_golden.py /path/to/reference [--add]
--add keeps what the file already holds and captures only the cases of iql_ref.CASES it lacks: the float32 run of a case depends on
the BLAS of the machine that made it, and the tolerances of the GPU tests are scaled from it, so a new case does not move the old ones.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ADD = "--add" in sys.argv
ARGS = [x for x in sys.argv[1:] if x != "--add"]
REFERENCE = ARGS[0] if ARGS else os.environ.get("M3PC_REFERENCE")
if not REFERENCE or not os.path.isdir(os.path.join(REFERENCE, "research")):
    sys.exit("usage: make_iql_golden.py /path/to/reference  (the checkout that holds research/finetune_omtm/model.py)")
sys.modules.setdefault("gym", types.ModuleType("gym"))
sys.modules["gym"].Env = object
sys.path.insert(0, REFERENCE)

from research.finetune_omtm.model import GaussianPolicy, ImplicitQLearning, TwinQ, ValueFunction  # noqa: E402

import iql_ref as R  # noqa: E402

OPT = {"qf": "q_optimizer", "vf": "v_optimizer", "actor": "actor_optimizer"}


def build(case, dtype):
    S, A, H, _ = R.CASES[case]
    state, om, os_ = R.make_state(case)
    om, os_ = torch.tensor(om, dtype=dtype), torch.tensor(os_, dtype=dtype)
    hp = R.HP
    q = TwinQ(S, A, om, os_, hidden_dim=H).to(dtype)
    v = ValueFunction(S, om, os_, hidden_dim=H).to(dtype)
    actor = GaussianPolicy(S, A, 1.0, om, os_, hidden_dim=H).to(dtype)
    for net, part in ((q, "qf"), (v, "vf"), (actor, "actor")):
        net.load_state_dict({k: torch.tensor(x, dtype=dtype) for k, x in state[part].items()})
    iql = ImplicitQLearning(1.0, actor, torch.optim.Adam(actor.parameters(), lr=hp["actor_lr"]), q, torch.optim.Adam(q.parameters(), lr=hp["q_lr"]),
                            v, torch.optim.Adam(v.parameters(), lr=hp["v_lr"]), iql_tau=hp["expectile"], beta=hp["beta"],
                            max_steps=hp["max_steps"], discount=hp["discount"], tau=hp["tau"])
    iql.q_target.load_state_dict({k: torch.tensor(x, dtype=dtype) for k, x in state["q_target"].items()})
    return iql


def nets(iql):
    return {"qf": iql.qf, "q_target": iql.q_target, "vf": iql.vf, "actor": iql.actor}


def moments(iql, part, key):
    net = nets(iql)[part]
    st = getattr(iql, OPT[part]).state
    return {name: st[p][key].detach().numpy().copy() for name, p in net.named_parameters()}


def run(case, dtype):
    iql = build(case, dtype)
    losses, m1, v1 = [], None, None
    for k, b in enumerate(R.make_batches(case)):
        log = iql.train([torch.tensor(x, dtype=dtype) for x in b])
        losses.append([log["value_loss"], log["q_loss"], log["actor_loss"]])
        if k == 0:
            m1 = {part: moments(iql, part, "exp_avg") for part in OPT}
            v1 = {part: moments(iql, part, "exp_avg_sq") for part in OPT}
    params = {part: {k: x.detach().numpy().copy() for k, x in net.state_dict().items()} for part, net in nets(iql).items()}
    return np.array(losses, np.float64), m1, v1, params


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    path = os.path.join(HERE, "g7_iql.npz")
    out, have = {}, set()
    if ADD and os.path.exists(path):
        with np.load(path) as old:
            out = {k: old[k] for k in old.files}
        have = {str(c) for c in out["cases"]}
    out["cases"], out["n_steps"] = np.array(list(R.CASES)), np.int64(R.N_STEPS)
    for case in R.CASES:
        if case in have:
            continue
        l32, m32, v32, p32 = run(case, torch.float32)
        l64, m64, v64, p64 = run(case, torch.float64)
        ref, lref, _ = R.run(case)
        out[case + "/losses32"], out[case + "/losses64"] = l32, l64
        out[case + "/conditions"] = np.array([ref.min_preact, ref.min_adv, ref.min_clamp_gap, ref.n_clamped, ref.n_done], np.float64)
        gnames, gdev = [], []
        for part in OPT:
            for name in R.part_names(part):
                g32, g64 = m32[part][name].astype(np.float64) / (1 - R.BETA1), m64[part][name] / (1 - R.BETA1)
                gnames.append(part + "/" + name)
                gdev.append(np.abs(g32 - g64).max() / np.abs(g64).max() if np.abs(g64).max() > 0 else 0.0)
        out[case + "/grad_names"], out[case + "/ref32_grad_dev"] = np.array(gnames), np.array(gdev)
        out[case + "/ref32_loss_dev"] = (np.abs(l32 - l64) / np.abs(l64)).max(0)
        pnames = [part + "/" + name for part in R.PARTS for name in R.part_names(part)]
        out[case + "/param_names"] = np.array(pnames)
        out[case + "/ref32_param_dev"] = np.array([np.abs(p32[n.split("/")[0]][n.split("/")[1]].astype(np.float64) - p64[n.split("/")[0]][n.split("/")[1]]).max()
                                                   for n in pnames])
        out[case + "/ref32_traj_dev"] = out[case + "/ref32_param_dev"].max()
        print(case, "grad dev %.2e  loss dev %.2e  param dev %.2e  | restatement vs float64 reference: losses %.1e" % (
            max(gdev), out[case + "/ref32_loss_dev"].max(), out[case + "/ref32_param_dev"].max(), (np.abs(lref - l64) / np.abs(l64)).max()),
            "| conditions", out[case + "/conditions"])
        if case == "h64":
            for j, key in enumerate(("state", "action", "reward", "next_state", "done")):
                out[case + "/batch0/" + key] = R.make_batches(case, 1)[0][j]
            for n in gnames:
                part, name = n.split("/")
                out[case + "/exp_avg32/" + n], out[case + "/exp_avg64/" + n] = m32[part][name], m64[part][name]
                out[case + "/exp_avg_sq32/" + n] = v32[part][name]
            for n in pnames:
                part, name = n.split("/")
                out[case + "/final32/" + n], out[case + "/final64/" + n] = p32[part][name], p64[part][name]
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
