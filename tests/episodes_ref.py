"""NumPy restatement of the episode store (include/m3pc_hip.h: m3pc_episodes_*): the two window rules and the discounted values,
for the tests to compare the kernels against.

``window_plan`` is action_sample's window (finetune_omtm/learner.py:342-366), ``window_goal`` action_piid_sample's
(zeroshot_omtm/learner.py:164-223, with ``max_steps`` where the reference has the literal 1000); both take a trajectory dict as
``m3pc_amd.rollout.new_trajectory`` makes it (arrays of max_steps rows, float32 or -- way-point observations -- float64) and
return float32 (T,S), (T,A), (T,1) and the effective horizon.  ``values`` is replay_buffer.py:234-243: float32 rewards times a
float64 ``discounts`` array, summed in float64, ONE rounding to float32 (and, with use_avg, one division in float64 of the
rounded value and one more rounding)."""
import numpy as np


def horizon_of(end: int, T: int, H: int) -> int:
    return H if end + H >= T else T - end


def _history(traj, T: int, H: int):
    obs, act = np.asarray(traj["observations"]), np.asarray(traj["actions"])
    rew = np.asarray(traj["rewards"]).reshape(obs.shape[0])
    end = int(traj["path_length"])
    M = obs.shape[0]
    assert 0 <= end < M, "the window of a full episode would read row max_steps"
    h = horizon_of(end, T, H)
    hl = T - h + 1
    lo = end - hl + 1
    s = np.zeros((T, obs.shape[1]), dtype=np.float32)
    a = np.zeros((T, act.shape[1]), dtype=np.float32)
    r = np.zeros((T, 1), dtype=np.float32)
    for t in range(hl):
        s[t] = obs[lo + t]  # (a float64 row is rounded by the assignment)
        a[t] = act[lo + t]
        r[t, 0] = rew[lo + t]
    return s, a, r, h, lo, end, M


def window_plan(traj, T: int, H: int):
    s, a, r, h, _, _, _ = _history(traj, T, H)
    return s, a, r, h


def window_goal(traj, T: int, H: int):
    s, a, r, h, lo, end, M = _history(traj, T, H)
    smart = T - max(0, end + h - M)
    obs = np.asarray(traj["observations"])
    s[:] = 0.0
    for t in range(smart):
        s[t] = obs[lo + t]
    return s, a, r, h


def values(rewards, discount: float, use_avg: bool = False) -> np.ndarray:
    """rewards (M,) float32 -> (M,) float32."""
    rew = np.asarray(rewards, dtype=np.float32).reshape(-1)
    M = rew.shape[0]
    discounts = float(discount) ** np.arange(M)  # float64, replay_buffer.py:70
    out = np.zeros((M,), dtype=np.float32)
    for t in range(M):
        out[t] = (rew[t + 1 :] * discounts[: M - t - 1]).sum()  # float32 * float64 -> float64 sum, one rounding
    if use_avg:
        out = (out.astype(np.float64) / np.arange(M, 0, -1)).astype(np.float32)
    return out


def clip(a, lo, hi) -> np.ndarray:
    return np.clip(np.asarray(a, dtype=np.float32), np.float32(lo), np.float32(hi))
