"""NumPy restatement of the replay buffer (include/m3pc_hip.h: m3pc_replay_*) for the tests to compare the kernels against: the
library's index draws in exact integer arithmetic on the Philox words of tests/variates_ref.py, the values of an online episode
(replay_buffer.py:234-243, fp64 ``use_avg`` quotient included), and ``HostReplay``, a host model of the three rings with the library's
FIFO rules.  Also the deterministic recipes (dataset, toy rollouts, config) that tests/golden/make_replay_golden.py fed to the real
reference ``ReplayBuffer`` -- the golden stores the recipe's seed, not the arrays."""
import types

import numpy as np

import episodes_ref
import variates_ref as V

ARRAY_SEGMENTS, ARRAY_ONLINE, ARRAY_OFFLINE = 2, 3, 4
UNIFORM, LENGTH = 0, 1
MASK = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------- the draws
def mulshift(w, n):
    """(w * n) >> 32 for a 32-bit word: python integers, exact."""
    return (int(w) * int(n)) >> 32


def segment_words(seed, step, batch):
    """Row j's words w0 .. w3: Philox block j of (seed, step), array 2.  -> four uint32 arrays (batch,)."""
    return V._words(seed, step, ARRAY_SEGMENTS, batch)


def pick_trajectory(w0, mode, lens):
    lens = [int(x) for x in lens]
    if mode == UNIFORM:
        return mulshift(w0, len(lens))
    cum = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))])
    r = mulshift(w0, cum[-1])
    return int(np.searchsorted(cum, r, side="right") - 1)  # cum[i] <= r < cum[i+1]


def pick_start(w2, length, L):
    return mulshift(w2, int(length) - L + 1)


def draw_segments(seed, step, batch, mode, lens, L):
    """(trajectory (batch,), start (batch,)) int32, lens in logical order."""
    w = segment_words(seed, step, batch)
    ti = np.array([pick_trajectory(w[0][j], mode, lens) for j in range(batch)], dtype=np.int32)
    si = np.array([pick_start(w[2][j], lens[ti[j]], L) for j in range(batch)], dtype=np.int32)
    return ti, si


def round_keys(seed, step, online):
    w = V._words(seed, step, ARRAY_ONLINE if online else ARRAY_OFFLINE, 1)
    return [int(x[0]) for x in w]


def pi(j, n, keys):
    """The keyed bijection of [0, n): a 4-round balanced Feistel network on 2 * half bits, cycle-walked."""
    if n <= 1:
        return 0
    bits = (n - 1).bit_length()
    half = (bits + 1) // 2
    mask = (1 << half) - 1
    x = j
    while True:
        l, r = x >> half, x & mask
        for k in keys:
            f = ((((r + k) & MASK) * 0x9E3779B1) & MASK) >> (32 - half)
            l, r = r, l ^ f
        x = (l << half) | r
        if x < n:
            return x


def draw_transitions(seed, step, n_online, n_offline, count_online, count_offline):
    """(n_online + n_offline,) int32 logical indices: the online rows first."""
    kon, koff = round_keys(seed, step, True), round_keys(seed, step, False)
    return np.array([pi(j, count_online, kon) for j in range(n_online)] + [pi(j, count_offline, koff) for j in range(n_offline)], dtype=np.int32)


# ---------------------------------------------------------------------------------------------- values
def online_values(rewards, discount, use_avg=False):
    """rewards (M,) float32 -> (M,) FLOAT64: the fp64 sums rounded to float32 on assignment (replay_buffer.py:238), widened; with
    use_avg divided in float64 by (M - t) and NOT rounded again (:240-242: float32 array / int64 array is a float64 array)."""
    v = episodes_ref.values(rewards, discount, False).astype(np.float64)
    if use_avg:
        v = v / np.arange(v.shape[0], 0, -1)
    return v


# ---------------------------------------------------------------------------------------------- the rings
class HostReplay:
    """The three rings on the host, logical order (index 0 = oldest)."""

    def __init__(self, S, A, C, M, L, cap_offline, cap_online):
        self.S, self.A, self.C, self.M, self.L = S, A, C, M, L
        self.traj = []  # (obs (M,S) f32, act (M,A) f32, rew (M,) f32, val (M,) f64, len)
        self.cap = {False: cap_offline, True: cap_online}
        self.trans = {False: [], True: []}  # (s, a, r, s2, d)

    def append(self, obs, act, rew, val, length):
        assert self.L <= length <= self.M
        self.traj.append((np.float32(obs).reshape(self.M, self.S).copy(), np.float32(act).reshape(self.M, self.A).copy(),
                          np.float32(rew).reshape(self.M).copy(), np.float64(val).reshape(self.M).copy(), int(length)))
        self.traj = self.traj[-self.C:] if self.C else []

    def append_transition(self, online, s, a, r, s2, d):
        if self.cap[online]:
            self.trans[online].append((np.float32(s).copy(), np.float32(a).copy(), np.float32(r), np.float32(s2).copy(), np.float32(d)))
            self.trans[online] = self.trans[online][-self.cap[online]:]

    def push_episode(self, obs, act, rew, length, discount, use_avg, final_obs=None):
        """One episode of a store: m3pc_replay_push_episodes.  -> 1 if the trajectory was taken."""
        rew = np.float32(rew).reshape(self.M)
        for t in range(length if final_obs is not None else length - 1):
            self.append_transition(True, obs[t], act[t], rew[t], final_obs if t == length - 1 else obs[t + 1], 0.0)
        if length < self.L or not self.C:
            return 0
        self.append(obs, act, rew, online_values(rew, discount, use_avg), length)
        return 1

    @property
    def lens(self):
        return [t[4] for t in self.traj]

    def segments(self, ti, si, returns_f32=False):
        L = self.L
        s = np.stack([self.traj[i][0][k:k + L] for i, k in zip(ti, si)])
        a = np.stack([self.traj[i][1][k:k + L] for i, k in zip(ti, si)])
        r = np.stack([self.traj[i][2][k:k + L] for i, k in zip(ti, si)])[..., None]
        v = np.stack([self.traj[i][3][k:k + L] for i, k in zip(ti, si)])[..., None]
        return s, a, r, (v.astype(np.float32) if returns_f32 else v)

    def transitions(self, index, n_online):
        rows = [self.trans[j < n_online][int(i)] for j, i in enumerate(index)]
        return (np.stack([e[0] for e in rows]), np.stack([e[1] for e in rows]), np.float32([[e[2]] for e in rows]),
                np.stack([e[3] for e in rows]), np.float32([[e[4]] for e in rows]))

    def values_up_bound(self):
        return np.stack([t[3] for t in self.traj]).max(axis=0)


# ---------------------------------------------------------------------------------------------- the golden's recipes
GOLDEN_LENGTHS = [20, 7, 3, 20, 12, 5, 20, 9]
GOLDEN_S, GOLDEN_A, GOLDEN_M = 5, 2, 20
GOLDEN_ROLLOUTS = [9, 20]  # the lengths of the two online episodes (the second runs into max_path_length)


def golden_config(select_mode):
    return types.SimpleNamespace(traj_length=4, traj_batch_size=6, traj_buffer_size=5, trans_batch_size=8, trans_buffer_size=32,
                                 buffer_init_ratio=0.5, select_mode=select_mode, mtm_iter_per_rollout=2, v_iter_per_mtm=1,
                                 using_online_threshold=4, env_name="toy", device="cpu", rtg_percent=1.0, plan=True, clip_min=-1.0,
                                 clip_max=1.0)


def golden_dataset(seed):
    """What the reference's constructor reads of a D4RLDataset, as float32 arrays."""
    rng = np.random.RandomState(seed)
    n = sum(GOLDEN_LENGTHS)
    ends = np.cumsum(GOLDEN_LENGTHS) - 1
    dones = np.zeros((n,), dtype=np.float32)
    dones[ends] = 1.0
    terminals = np.zeros((n,), dtype=np.float32)
    terminals[[e for e, l in zip(ends, GOLDEN_LENGTHS) if l < GOLDEN_M]] = 1.0
    return dict(observations=rng.normal(size=(n, GOLDEN_S)).astype(np.float32), actions=rng.uniform(-1, 1, size=(n, GOLDEN_A)).astype(np.float32),
                rewards=rng.normal(size=(n,)).astype(np.float32), dones_float=dones, terminals_float=terminals,
                next_observations=rng.normal(size=(n, GOLDEN_S)).astype(np.float32))


def golden_rollout(seed, k):
    """Online episode k: observations (len + 1, S) float32 (row t is what the environment shows at step t), the policy's raw actions
    (len, A) float32 in [-1.5, 1.5] (the reference clips them), rewards (len,) float64."""
    rng = np.random.RandomState(seed + 1000 + k)
    n = GOLDEN_ROLLOUTS[k]
    return (rng.normal(size=(n + 1, GOLDEN_S)).astype(np.float32), rng.uniform(-1.5, 1.5, size=(n, GOLDEN_A)).astype(np.float32),
            rng.normal(size=(n,)))


def golden_trajectory(seed, k, discount, use_avg):
    """That episode as the host dict ReplayBuffer.online_rollout hands to update_buffer (replay_buffer.py:189-248)."""
    obs, act, rew = golden_rollout(seed, k)
    n, M = GOLDEN_ROLLOUTS[k], GOLDEN_M
    tr = {"observations": np.zeros((M, GOLDEN_S), dtype=np.float32), "actions": np.zeros((M, GOLDEN_A), dtype=np.float32),
          "rewards": np.zeros((M, 1), dtype=np.float32), "path_length": n}
    tr["observations"][:n] = obs[:n]
    tr["actions"][:n] = np.clip(act, -1.0, 1.0)
    tr["rewards"][:n, 0] = rew
    tr["values"] = online_values(tr["rewards"][:, 0], discount, use_avg)[:, None]
    tr["total_return"] = tr["rewards"].sum()
    return tr
