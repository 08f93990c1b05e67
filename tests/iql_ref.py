"""ImplicitQLearning.train (finetune_omtm/model.py:286-308) restated in NumPy float64 -- forward, the three losses, the gradients by
hand, torch.optim.Adam's update, the cosine rate of the actor and the soft update of the target -- and the seeded recipes from which
the capture script (tests/golden/make_iql_golden.py) and the GPU tests build identical weights and batches without storing them.
Does not import the reference: tests/golden/g7_iql.npz holds what the real class computed, and tests/test_iql_cpu.py compares."""
import functools
import math

import numpy as np

# (S, A, hidden, batch): a partial 32-row tile; S + A = 35 (a second feature tile) and one row past a tile; a single row; the
# reference's own batch; S = 40, a second feature tile in V and the actor as well (the widest states the trainer's size rule covers
# are S = 63: wider than a planner handle's, so the GPU tests make this trainer on a stand-in for a handle); S = A = 32, both input
# widths whole feature tiles, the widest actor and a batch of whole row tiles; the largest batch a step takes
CASES = {"h64": (11, 3, 64, 37), "h128": (27, 8, 128, 33), "h256_1": (11, 3, 256, 1), "h256": (17, 6, 256, 256), "s40": (40, 6, 128, 33),
         "a32": (32, 32, 64, 64), "b1024": (11, 3, 64, 1024)}
# picked so that the fixture conditions of test_iql_cpu.py hold and, among those, so that the reference's own float32 gradient of a
# single-number tensor (the bias of an output unit) is at least 2^-27 of it away from the exact one: a smaller deviation (1e-9 was
# seen) is chance, and 16 x it is less than the spacing of float32 there, no tolerance for any float32 evaluation
SEEDS = {"h64": 41, "h128": 71, "h256_1": 38, "h256": 515, "s40": 1, "a32": 2, "b1024": 1}
LOG_STD_BELOW = ("a32",)   # cases whose log_std also has a component below the lower clamp
HP = dict(v_lr=3e-4, q_lr=3e-4, actor_lr=3e-4, expectile=0.7, beta=3.0, discount=0.99, tau=0.005, max_steps=1000)
N_STEPS = 20
PARTS = ("qf", "q_target", "vf", "actor")
FIELDS = ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias")
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
EXP_ADV_MAX, LOG_STD_MIN, LOG_STD_MAX = 100.0, -20.0, 2.0
PREACT_MARGIN, ADV_MARGIN, CLAMP_MARGIN = 1e-4, 1e-4, 1e-3   # the fixture conditions: |z|, |adv|, |beta adv - ln 100|


def part_names(part):
    """The reference's state_dict names of a part (model.py:146-191, :107-133)."""
    if part in ("qf", "q_target"):
        return ["%s.%s" % (q, f) for q in ("q1", "q2") for f in FIELDS]
    if part == "vf":
        return ["v.%s" % f for f in FIELDS]
    return ["net.%s" % f for f in FIELDS] + ["log_std"]


def part_shapes(part, S, A, H):
    i, o = (S + A, 1) if part in ("qf", "q_target") else ((S, 1) if part == "vf" else (S, A))
    mlp = [(H, i), (H,), (H, H), (H,), (o, H), (o,)]
    if part in ("qf", "q_target"):
        return mlp + mlp
    return mlp if part == "vf" else mlp + [(A,)]


def make_state(case, seed=None):
    """{part: {name: float32 array}}, obs_mean, obs_std.  Linear layers as nn.Linear draws them (uniform within 1 / sqrt(fan_in)), the
    output layers of V and Q four times as wide, so that advantages reach both signs and the clamp of exp(beta adv); q_target is a draw
    of its own (not a copy of qf: the soft update then has something to move); log_std has one component above the clamp (and in the
    cases of LOG_STD_BELOW one below it), which gets no gradient, and the others inside it."""
    S, A, H, _ = CASES[case]
    rng = np.random.RandomState(1000 + (SEEDS[case] if seed is None else seed))
    state = {}
    for part in PARTS:
        d = {}
        for name, shape in zip(part_names(part), part_shapes(part, S, A, H)):
            if name == "log_std":
                v = rng.uniform(-1.0, 0.5, size=shape)
                v[0] = 2.5
                v[1] = -0.5
                if case in LOG_STD_BELOW:
                    v[2] = -20.5
            else:
                fan_in = shape[1] if len(shape) == 2 else (H if ".0." not in name else (S + A if part in ("qf", "q_target") else S))
                gain = 4.0 if (".4." in name and part != "actor") else 1.0
                v = rng.uniform(-1.0, 1.0, size=shape) * gain / math.sqrt(fan_in)
            d[name] = v.astype(np.float32)
        state[part] = d
    obs_mean = rng.normal(size=S).astype(np.float32)
    obs_std = rng.uniform(0.5, 2.0, size=S).astype(np.float32)
    return state, obs_mean, obs_std


def _draw_rows(rng, m, S, A):
    s = (rng.normal(size=(m, S)) * 2.0 + 1.0).astype(np.float32)
    a = (rng.uniform(-0.9, 0.9, size=(m, A))).astype(np.float32)
    r = rng.normal(size=(m, 1)).astype(np.float32)
    s2 = (s + rng.normal(size=(m, S)) * 0.3).astype(np.float32)
    d = (rng.uniform(size=(m, 1)) < 0.15).astype(np.float32)
    return [s, a, r, s2, d]


@functools.lru_cache(maxsize=None)
def _batches(case, n, seed):
    S, A, _, B = CASES[case]
    rng = np.random.RandomState(2000 + (SEEDS[case] if seed is None else seed))
    state, om, os_ = make_state(case, seed)
    ref = RefIQL(state, om, os_)
    out = []
    for k in range(n):
        b = _draw_rows(rng, B, S, A)
        while True:
            bad = np.flatnonzero(~ref.rows_clear_of_kinks(b))
            if bad.size == 0:
                break
            for x, y in zip(b, _draw_rows(rng, bad.size, S, A)):
                x[bad] = y
        if k == 0:
            b[4][0, 0] = 1.0
        out.append(tuple(b))
        ref.train(out[-1])
    return out


def make_batches(case, n=N_STEPS, seed=None):
    """n transition batches in the layout of trans_sample (replay_buffer.py:368-420): state, action, reward (B, 1), next_state, done (B, 1).
    A row is drawn again (from the same stream, until it passes) when, at the parameters the float64 run has reached before the step
    that trains on it, it puts a hidden pre-activation within twice PREACT_MARGIN of zero, or the advantage or the clamp of
    exp(beta adv) within twice theirs (twice: the last bits of another BLAS then cannot undo a condition that is asserted): rows are independent in every forward pass, so this keeps all N_STEPS steps of the run away from the kinks, where a
    float32 evaluation may take the other branch of a ReLU (one such flip moves a row of weights by a tenth of the learning rate per
    step).  The batches are a function of the seed alone, like the weights."""
    return list(_batches(case, max(n, N_STEPS), seed)[:n])


def actor_lr(lr, k, t_max):
    """CosineAnnealingLR (model.py:219) in closed form at 0-based step k, eta_min = 0."""
    return lr * 0.5 * (1.0 + math.cos(math.pi * k / t_max))


def _mlp_forward(p, prefix, x):
    z1 = x @ p[prefix + "net.0.weight"].T + p[prefix + "net.0.bias"]
    h1 = np.maximum(z1, 0.0)
    z2 = h1 @ p[prefix + "net.2.weight"].T + p[prefix + "net.2.bias"]
    h2 = np.maximum(z2, 0.0)
    out = h2 @ p[prefix + "net.4.weight"].T + p[prefix + "net.4.bias"]
    return out, (x, z1, h1, z2, h2)


def _mlp_backward(p, prefix, cache, dout):
    x, z1, h1, z2, h2 = cache
    g = {prefix + "net.4.weight": dout.T @ h2, prefix + "net.4.bias": dout.sum(0)}
    d2 = (dout @ p[prefix + "net.4.weight"]) * (z2 > 0)
    g[prefix + "net.2.weight"] = d2.T @ h1
    g[prefix + "net.2.bias"] = d2.sum(0)
    d1 = (d2 @ p[prefix + "net.2.weight"]) * (z1 > 0)
    g[prefix + "net.0.weight"] = d1.T @ x
    g[prefix + "net.0.bias"] = d1.sum(0)
    return g


class RefIQL:
    """The reference's ImplicitQLearning with its three Adam optimizers, in float64."""

    def __init__(self, state, obs_mean, obs_std, hp=HP):
        self.p = {part: {k: np.asarray(v, np.float64).copy() for k, v in state[part].items()} for part in PARTS}
        self.m = {part: {k: np.zeros_like(v) for k, v in self.p[part].items()} for part in ("qf", "vf", "actor")}
        self.v = {part: {k: np.zeros_like(v) for k, v in self.p[part].items()} for part in ("qf", "vf", "actor")}
        self.om, self.os = np.asarray(obs_mean, np.float64), np.asarray(obs_std, np.float64)
        self.hp = dict(hp)
        self.total_it = 0
        self.min_preact = np.inf      # the fixture conditions, over every step made
        self.min_adv = np.inf
        self.min_clamp_gap = np.inf
        self.n_clamped = 0
        self.n_done = 0

    def q_min(self, which, s, a):
        x = np.concatenate([(s - self.om) / self.os, a], 1)
        return np.minimum(_mlp_forward(self.p[which], "q1.", x)[0][:, 0], _mlp_forward(self.p[which], "q2.", x)[0][:, 0])

    def value(self, s):
        return _mlp_forward(self.p["vf"], "v.", (s - self.om) / self.os)[0][:, 0]

    def actor_mean(self, s):
        return np.tanh(_mlp_forward(self.p["actor"], "net.", (s - self.om) / self.os)[0])

    def rows_clear_of_kinks(self, batch):
        """Per row of a batch, at the current parameters: whether every hidden pre-activation of the seven forward passes of a step,
        the advantage and beta adv - ln 100 keep the margins of the fixture conditions."""
        s, a, s2 = [np.asarray(batch[j], np.float64) for j in (0, 1, 3)]
        xs, xn = (s - self.om) / self.os, (s2 - self.om) / self.os
        xsa = np.concatenate([xs, a], 1)
        fw = [_mlp_forward(self.p["vf"], "v.", xn), _mlp_forward(self.p["vf"], "v.", xs), _mlp_forward(self.p["actor"], "net.", xs)]
        fw += [_mlp_forward(self.p[part], q, xsa) for part in ("q_target", "qf") for q in ("q1.", "q2.")]
        z = np.min([np.minimum(np.abs(c[1]).min(1), np.abs(c[3]).min(1)) for _, c in fw], 0)
        adv = np.minimum(fw[3][0][:, 0], fw[4][0][:, 0]) - fw[1][0][:, 0]
        gap = np.abs(self.hp["beta"] * adv - math.log(EXP_ADV_MAX))
        return (z > 2 * PREACT_MARGIN) & (np.abs(adv) > 2 * ADV_MARGIN) & (gap > 2 * CLAMP_MARGIN)

    def grads(self, batch):
        """(losses, {part: {name: gradient}}) of one batch at the current parameters: every forward reads pre-step parameters."""
        hp = self.hp
        s, a, r, s2, d = [np.asarray(x, np.float64) for x in batch]
        B = s.shape[0]
        r, d = r[:, 0], d[:, 0]
        xs, xn = (s - self.om) / self.os, (s2 - self.om) / self.os
        xsa = np.concatenate([xs, a], 1)
        next_v, cn = _mlp_forward(self.p["vf"], "v.", xn)
        v, cv = _mlp_forward(self.p["vf"], "v.", xs)
        q1t, c1t = _mlp_forward(self.p["q_target"], "q1.", xsa)
        q2t, c2t = _mlp_forward(self.p["q_target"], "q2.", xsa)
        q1, c1 = _mlp_forward(self.p["qf"], "q1.", xsa)
        q2, c2 = _mlp_forward(self.p["qf"], "q2.", xsa)
        z, ca = _mlp_forward(self.p["actor"], "net.", xs)
        adv = np.minimum(q1t[:, 0], q2t[:, 0]) - v[:, 0]
        # (the reference forms |tau - 1[adv < 0]| and (1 - done) * discount from float32 tensors and Python floats: both are float32
        # values whatever the dtype of the networks, model.py:60 and :251)
        w = np.abs(np.float32(hp["expectile"]) - (adv < 0).astype(np.float32)).astype(np.float64)
        v_loss = np.mean(w * adv ** 2)
        targets = r + ((1.0 - d).astype(np.float32) * np.float32(hp["discount"])).astype(np.float64) * next_v[:, 0]
        e1, e2 = q1[:, 0] - targets, q2[:, 0] - targets
        q_loss = (np.mean(e1 ** 2) + np.mean(e2 ** 2)) / 2
        exp_adv = np.minimum(np.exp(hp["beta"] * adv), EXP_ADV_MAX)
        ls = self.p["actor"]["log_std"]
        lsc = np.clip(ls, LOG_STD_MIN, LOG_STD_MAX)
        sigma = np.exp(lsc)
        mu = np.tanh(z)
        diff = a - mu
        bc = np.sum(0.5 * diff ** 2 / sigma ** 2 + lsc + 0.5 * math.log(2 * math.pi), 1)
        actor_loss = np.mean(exp_adv * bc)
        g = {"vf": _mlp_backward(self.p["vf"], "v.", cv, (-2.0 * w * adv / B)[:, None])}
        g["qf"] = _mlp_backward(self.p["qf"], "q1.", c1, (e1 / B)[:, None])
        g["qf"].update(_mlp_backward(self.p["qf"], "q2.", c2, (e2 / B)[:, None]))
        wa = (exp_adv / B)[:, None]
        g["actor"] = _mlp_backward(self.p["actor"], "net.", ca, -wa * diff / sigma ** 2 * (1.0 - mu ** 2))
        inside = (ls >= LOG_STD_MIN) & (ls <= LOG_STD_MAX)
        g["actor"]["log_std"] = np.where(inside, np.sum(wa * (1.0 - diff ** 2 / sigma ** 2), 0), 0.0)
        # the fixture conditions (a kink within rounding distance would make the gradient itself discontinuous)
        for c in (cn, cv, c1t, c2t, c1, c2, ca):
            self.min_preact = min(self.min_preact, np.abs(c[1]).min(), np.abs(c[3]).min())
        self.min_adv = min(self.min_adv, np.abs(adv).min())
        self.min_clamp_gap = min(self.min_clamp_gap, np.abs(hp["beta"] * adv - math.log(EXP_ADV_MAX)).min())
        self.n_clamped += int((hp["beta"] * adv > math.log(EXP_ADV_MAX)).sum())
        self.n_done += int((d == 1).sum())
        return np.array([v_loss, q_loss, actor_loss]), g

    def train(self, batch, rates=None, tau=None):
        """One step; returns (losses (3,), gradients)."""
        hp = self.hp
        losses, g = self.grads(batch)
        k = self.total_it
        t = k + 1
        lr = dict(vf=hp["v_lr"], qf=hp["q_lr"], actor=actor_lr(hp["actor_lr"], k, hp["max_steps"])) if rates is None else rates
        bc1, bc2 = 1.0 - BETA1 ** t, 1.0 - BETA2 ** t
        for part in ("vf", "qf", "actor"):
            for name, grad in g[part].items():
                m, v = self.m[part][name], self.v[part][name]
                m += (1.0 - BETA1) * (grad - m)
                v *= BETA2
                v += (1.0 - BETA2) * grad * grad
                self.p[part][name] -= (lr[part] / bc1) * m / (np.sqrt(v) / math.sqrt(bc2) + EPS)
        tau = hp["tau"] if tau is None else tau
        for name in self.p["q_target"]:
            self.p["q_target"][name] = (1.0 - tau) * self.p["q_target"][name] + tau * self.p["qf"][name]
        self.total_it = t
        return losses, g


def run(case, n=N_STEPS):
    """The float64 run of a case from its recipe: (RefIQL after n steps, losses (n, 3), the first step's gradients)."""
    state, om, os_ = make_state(case)
    ref = RefIQL(state, om, os_)
    losses, g1 = [], None
    for k, b in enumerate(make_batches(case, n)):
        l, g = ref.train(b)
        losses.append(l)
        if k == 0:
            g1 = g
    return ref, np.array(losses), g1


def ulp(x):
    """The spacing of float32 at |x| (elementwise)."""
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)
