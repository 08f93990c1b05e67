"""float64 NumPy restatement of the masked-trajectory loss (include/m3pc_hip.h: m3pc_mtm_loss*; the reference:
finetune_omtm/learner.py:419-504 and omtm/models/mtm_model.py:440-532) on given predictions.

``loss_terms`` returns the record -- RECORD_NAMES, the layout of M3PC_MTM_LOSS_FLOATS -- and, per scalar, its SCALE: the mean, over
the scalar's terms, of the sum of the absolute values of the term's addends, every product expanded:
    (p - t)^2                          -> (|p| + |t|)^2
    Normal(mu, std).log_prob(x)        -> (|x| + |mu|)^2 / (2 std^2) + |log std| + log sqrt(2 pi)
    2 (log 2 - x - softplus(-2 x))     -> 2 (log 2 + |x| + softplus(-2 x))
with |x| itself expanded where x is a sum: z = (log1p(a) - log1p(-a)) / 2 -> (|log1p(a)| + |log1p(-a)|) / 2, u = mu + std eps ->
|mu| + |std eps|.  An fp32 evaluation of a term errs by a few 2^-24 of that sum, whatever cancels inside it, so a bound on a scalar is
a multiple of 2^-24 * scale.  total's scale is the sum of the scales of what it adds up.
"""
import numpy as np

KEYS = ("states", "actions", "rewards", "returns")
NORM_L2, CLIP_ACTIONS = 1, 2
RECORD_NAMES = tuple(f"{kind}_{k}" for k in KEYS for kind in ("loss", "masked_loss", "masked_c_loss")) + ("entropy", "nll", "total")
ENTROPY, NLL, TOTAL = 12, 13, 14
LOG_SQRT_2PI = float(np.log(np.sqrt(2 * np.pi)))
LOG2 = float(np.log(2.0))
FINETUNE = (CLIP_ACTIONS, 1)  # (flags, loss_keys) of Learner.compute_mtm_loss for the key order states, actions, ...
PRETRAIN = (NORM_L2, 15)      # of omtm.forward_loss(norm="l2", loss_keys=None)


def early_return_keys(order):
    """What Learner.compute_mtm_loss has in its dicts when it returns: lines 488-504 sit inside the key loop, behind the ``continue``
    of the actions."""
    out = []
    for k in order:
        out.append(k)
        if k != "actions":
            return out
    return out


def _softplus(y):
    with np.errstate(over="ignore"):
        return np.where(y > 20.0, y, np.log1p(np.exp(np.minimum(y, 700.0))))


def _squashed_log_prob(x, absx, mu, sd):
    """(value, scale) of Normal(mu, sd).log_prob(x) - 2 (log 2 - x - softplus(-2 x)); absx: the expanded |x|."""
    var = sd * sd
    sp = _softplus(-2.0 * x)
    with np.errstate(invalid="ignore", over="ignore"):
        normal = -((x - mu) ** 2) / (2.0 * var) - np.log(sd) - LOG_SQRT_2PI
        ladj = 2.0 * (LOG2 - x - sp)
        val = normal - ladj
        scale = (absx + np.abs(mu)) ** 2 / (2.0 * var) + np.abs(np.log(sd)) + LOG_SQRT_2PI + 2.0 * (LOG2 + absx + np.abs(sp))
    return val, scale


def loss_terms(pred_states, pred_rewards, pred_returns, mu, std, targets, masks, eps, entropy_reg, flags, loss_keys, f32_clip=True):
    """preds (B,T,D), targets: four (B,T,D) tokenised arrays in KEYS order, masks: four (T,) 0/1 rows, eps (B,T,A).  f32_clip: the
    clip bounds rounded to float32 (torch.clip on a float32 tensor); False: the float64 reference's.  -> (record (15,), scale (15,))."""
    f8 = lambda x: np.asarray(x, dtype=np.float64)
    preds = {"states": f8(pred_states), "rewards": f8(pred_rewards), "returns": f8(pred_returns)}
    mu, std, eps = f8(mu), f8(std), f8(eps)
    B, T, A = mu.shape
    tg = {k: f8(t).reshape(B, T, -1) for k, t in zip(KEYS, targets)}
    m = {k: f8(np.asarray(x).reshape(T)) for k, x in zip(KEYS, masks)}
    rec, scale = np.zeros(15), np.zeros(15)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in ("states", "rewards", "returns"):
            i = 3 * KEYS.index(k)
            t, p = tg[k], preds[k].reshape(B, T, -1)
            if flags & NORM_L2:
                t = t / np.sqrt((t * t).sum(axis=-1, keepdims=True))
            raw, s = (p - t) ** 2, (np.abs(p) + np.abs(t)) ** 2
            mk = m[k][None, :, None]
            n_vis = m[k].sum()
            rec[i], scale[i] = raw.mean(), s.mean()
            rec[i + 1] = ((raw * (1 - mk)).sum(axis=(1, 2)) / (T - n_vis)).mean()
            scale[i + 1] = ((s * (1 - mk)).sum(axis=(1, 2)) / (T - n_vis)).mean()
            rec[i + 2] = ((raw * mk).sum(axis=(1, 2)) / n_vis).mean()
            scale[i + 2] = ((s * mk).sum(axis=(1, 2)) / n_vis).mean()
        a = tg["actions"]
        ma = m["actions"][None, :, None]
        th = np.tanh(mu)
        rec[3], scale[3] = ((th - a) ** 2 * ma).mean(), ((np.abs(th) + np.abs(a)) ** 2 * ma).mean()
        ac = a
        if flags & CLIP_ACTIONS:
            lo, hi = (np.float32(-1 + 1e-6), np.float32(1 - 1e-6)) if f32_clip else (-1 + 1e-6, 1 - 1e-6)
            ac = np.clip(a, np.float64(lo), np.float64(hi))
        l1, l2 = np.log1p(ac), np.log1p(-ac)
        z = 0.5 * (l1 - l2)
        lp, lp_s = _squashed_log_prob(z, 0.5 * (np.abs(l1) + np.abs(l2)), mu, std)
        u = mu + eps * std
        lq, lq_s = _squashed_log_prob(u, np.abs(mu) + np.abs(eps * std), mu, std)
        hidden = m["actions"] == 0
        mean = lambda x: x[:, hidden, :].mean() if hidden.any() else np.float64(np.nan)
        ll, ent = mean(lp), -mean(lq)
        rec[ENTROPY], scale[ENTROPY] = ent, mean(lq_s)
        rec[NLL], scale[NLL] = -ll, mean(lp_s)
        bits = [j for j in range(4) if (loss_keys >> j) & 1]
        rec[TOTAL] = sum(rec[3 * j] for j in bits) - (ll + entropy_reg * ent)
        scale[TOTAL] = sum(scale[3 * j] for j in bits) + scale[NLL] + abs(entropy_reg) * scale[ENTROPY]
    return rec, scale


def same_specials(a, b):
    """NaN, +inf and -inf stand at the same positions."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b)) and
                np.array_equal(np.isneginf(a), np.isneginf(b)))
