#!/usr/bin/env python3
"""A/B of the IQL trainer (m3pc_iql_*, m3pc_amd/iql.py) against the torch-eager route, in ONE process on one GPU: K critic updates on
batches of a DeviceReplayBuffer and the hand-over of the new TwinQ to the planner's critic, from an idle device until it is idle again.

  eager   K x (buf.trans_sample() + a torch-eager restatement of ImplicitQLearning.train, finetune_omtm/model.py:286-308, WITHOUT its
          three .item() reads), then handle.set_critic(qf.state_dict(), ...): the host round trip of m3pc_set_critic.
  device  DeviceIQL.train_from(buf, K) (m3pc_iql_train: 8 launches per step) + publish (m3pc_iql_publish_critic: one launch).

Batch 256, hidden 256, hopper (S 11, A 3) and walker2d (S 17, A 6) sizes.  The legs alternate call by call; a call is timed by the host
clock between two device synchronisations; medians and the 10 / 90 % quantiles over --calls calls after --warmup.  No bar: the table
is recorded (`--out FILE`, profiles/iql_ab.txt)."""
import argparse
import os
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from m3pc_amd import capi  # noqa: E402
from m3pc_amd.iql import DeviceIQL  # noqa: E402
from m3pc_amd.replay import DeviceReplayBuffer  # noqa: E402

q = lambda v, f: sorted(v)[min(len(v) - 1, int(f * len(v)))]
HP = dict(lr=3e-4, expectile=0.7, beta=3.0, discount=0.99, tau=0.005, max_steps=1000000)


def mlp(i, h, o):
    return torch.nn.Sequential(torch.nn.Linear(i, h), torch.nn.ReLU(), torch.nn.Linear(h, h), torch.nn.ReLU(), torch.nn.Linear(h, o))


class Eager:
    """train() restated with torch modules (names as the reference's state_dict has them)."""

    def __init__(self, S, A, H, om, os_, dev):
        self.q1, self.q2, self.v, self.pi = (mlp(S + A, H, 1).to(dev), mlp(S + A, H, 1).to(dev), mlp(S, H, 1).to(dev), mlp(S, H, A).to(dev))
        self.t1, self.t2 = mlp(S + A, H, 1).to(dev), mlp(S + A, H, 1).to(dev)
        self.t1.load_state_dict(self.q1.state_dict())
        self.t2.load_state_dict(self.q2.state_dict())
        self.log_std = torch.nn.Parameter(torch.zeros(A, device=dev))
        self.om, self.os = om, os_
        self.qo = torch.optim.Adam(list(self.q1.parameters()) + list(self.q2.parameters()), lr=HP["lr"])
        self.vo = torch.optim.Adam(self.v.parameters(), lr=HP["lr"])
        self.ao = torch.optim.Adam(list(self.pi.parameters()) + [self.log_std], lr=HP["lr"])
        self.sched = torch.optim.lr_scheduler.CosineAnnealingLR(self.ao, HP["max_steps"])

    def qf_state_dict(self):
        sd = {"q1.net." + k: v for k, v in self.q1.state_dict().items()}
        sd.update({"q2.net." + k: v for k, v in self.q2.state_dict().items()})
        return sd

    def train(self, batch):
        s, a, r, s2, d = batch
        xs, xn = (s - self.om) / self.os, (s2 - self.om) / self.os
        sa = torch.cat([xs, a], 1)
        with torch.no_grad():
            next_v = self.v(xn).squeeze(-1)
            tq = torch.min(self.t1(sa).squeeze(-1), self.t2(sa).squeeze(-1))
        adv = tq - self.v(xs).squeeze(-1)
        v_loss = torch.mean(torch.abs(HP["expectile"] - (adv < 0).float()) * adv ** 2)
        self.vo.zero_grad()
        v_loss.backward()
        self.vo.step()
        targets = r.squeeze(-1) + (1.0 - d.squeeze(-1)) * HP["discount"] * next_v
        q_loss = (torch.nn.functional.mse_loss(self.q1(sa).squeeze(-1), targets) + torch.nn.functional.mse_loss(self.q2(sa).squeeze(-1), targets)) / 2
        self.qo.zero_grad()
        q_loss.backward()
        self.qo.step()
        with torch.no_grad():
            for t, src in ((self.t1, self.q1), (self.t2, self.q2)):
                for tp, sp in zip(t.parameters(), src.parameters()):
                    tp.data.copy_((1 - HP["tau"]) * tp.data + HP["tau"] * sp.data)
        exp_adv = torch.exp(HP["beta"] * adv.detach()).clamp(max=100.0)
        dist = torch.distributions.Normal(torch.tanh(self.pi(xs)), torch.exp(self.log_std.clamp(-20.0, 2.0)))
        a_loss = torch.mean(exp_adv * -dist.log_prob(a).sum(-1))
        self.ao.zero_grad()
        a_loss.backward()
        self.ao.step()
        self.sched.step()
        return v_loss, q_loss, a_loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40, help="timed calls per leg (after warm-up)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="K: critic updates per call (v_iter_per_mtm)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, H, K = 256, 256, a.steps
    lines = [f"IQL trainer A/B: K = {K} critic updates on replay batches (batch {B}, hidden {H}) + the hand-over of the TwinQ to the planner, from an "
             f"idle device until it is idle again; torch-eager train() + m3pc_set_critic [eager] against m3pc_iql_train + m3pc_iql_publish_critic "
             f"[device]; {a.calls} interleaved calls per leg after {a.warmup} warm-up calls; ms per call; {torch.cuda.get_device_name(0)}",
             f"{'sizes':22s} {'leg':7s} {'median':>9s} {'p10':>9s} {'p90':>9s} {'per step':>9s}"]
    for env, S, A in (("hopper", 11, 3), ("walker2d", 17, 6)):
        cfg = types.SimpleNamespace(traj_length=8, traj_batch_size=4, traj_buffer_size=4, trans_batch_size=B, trans_buffer_size=20000, select_mode="uniform",
                                    mtm_iter_per_rollout=1, using_online_threshold=1000)
        hd = capi.Handle(S, A, 8, n_embd=64, n_head=2, max_candidates=64, critic_hidden=H)
        buf = DeviceReplayBuffer(hd, cfg, 0, 16, seed=1)
        g = torch.Generator(device=dev).manual_seed(1)
        for online, n in ((False, 20000), (True, 5000)):
            buf.append_transitions(torch.randn((n, S), generator=g, device=dev), torch.rand((n, A), generator=g, device=dev) * 1.8 - 0.9,
                                   torch.randn((n,), generator=g, device=dev), torch.randn((n, S), generator=g, device=dev),
                                   (torch.rand((n,), generator=g, device=dev) < 0.1).float(), online=online)
        om, os_ = torch.zeros(S, device=dev), torch.ones(S, device=dev)
        torch.manual_seed(0)
        eager = Eager(S, A, H, om, os_, dev)
        iql = DeviceIQL(hd, H, max_steps=HP["max_steps"])
        qf = eager.qf_state_dict()
        iql.load_part(capi.IQL_QF, qf, om, os_)
        iql.load_part(capi.IQL_Q_TARGET, qf)
        iql.load_part(capi.IQL_VF, {"v.net." + k: v for k, v in eager.v.state_dict().items()})
        actor = {"net.net." + k: v for k, v in eager.pi.state_dict().items()}
        actor["log_std"] = eager.log_std.detach()
        iql.load_part(capi.IQL_ACTOR, actor)

        def leg_eager():
            for _ in range(K):
                out = eager.train(buf.trans_sample())
            hd.set_critic(eager.qf_state_dict(), om, os_)
            return out

        def leg_device():
            out = iql.train_from(buf, K)
            iql.publish(hd)
            return out

        pair = {"eager": leg_eager, "device": leg_device}
        per = {k: [] for k in pair}
        for i in range(a.warmup + a.calls):
            for k, fn in pair.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    per[k].append(1e3 * (time.perf_counter() - t0))
                assert all(bool(torch.isfinite(x).all()) for x in out)
        for k, v in per.items():
            lines.append(f"{env + ' S %d A %d' % (S, A):22s} {k:7s} {q(v, 0.5):9.4f} {q(v, 0.1):9.4f} {q(v, 0.9):9.4f} {q(v, 0.5) / K:9.4f}")
        lines.append(f"{'':22s} device / eager = {q(per['device'], 0.5) / q(per['eager'], 0.5):.4f}")
        torch.cuda.synchronize()
        iql.close()
        buf.close()
        hd.close()
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
