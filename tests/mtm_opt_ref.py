"""A float64 restatement of one optimizer step of the masked-trajectory model (m3pc_amd/csrc/mtm_opt.h): AdamW with torch's
per-tensor skip rule, both LambdaLR schedules and the float64 Adam step of log_temperature -- and a per-element bound on what the
device's arithmetic may differ from it by, from a running error analysis of the order mtm_opt.h states.  Nothing here is read from a
device.

THE BOUND (u = 2^-24, the unit roundoff of fp32; eta = 2^-150, half the smallest subnormal; gamma_k = k u / (1 - k u)).
The device computes, for an active tensor with fp32 inputs p, g, m, v and fp32 constants omb1 = fl(1 - beta1), b2 = fl(beta2),
omb2 = fl(1 - beta2) (each within u relative of the float64 constant):
    m' = fl(m + fl(omb1 fl(g - m)))        three roundings and the constant's:   |m' - m_ref| <= gamma_3 (1 - beta1) |g - m| + u |m_ref| + 3 eta
    v' = fl(fl(b2 v) + fl(fl(omb2 g) g))   |v' - v_ref| <= gamma_2 beta2 |v| + gamma_3 (1 - beta2) g^2 + u |v_ref| + 4 eta
(the rounding of the final sum is taken on the reference value, its first-order size; the second-order remainder is inside the
gamma's slack of one extra u, added below as a factor 1 + 8 u).  The parameter is ONE float64 expression of the fp32 m', v':
    p' = fl32( p k - s m' / (sqrt(v') / c + eps) ),   k = 1 - lr wd or 1,  s = lr / (1 - beta1^t),  c = sqrt(1 - beta2^t)
so against p_ref (the same expression of m_ref, v_ref) the update quotient is enclosed by evaluating it at the four corners of
[m_ref -+ bm] x [max(v_ref - bv, 0), v_ref + bv] (it is monotone in m and in v on that box), plus the float64 slop of the
expression and of the device's pow (64 units of 2^-53 on the magnitudes involved), plus the one fp32 rounding u |p_ref| + eta.
"""
import math

import numpy as np

U = 2.0 ** -24
ETA = 2.0 ** -150
D = 2.0 ** -53


def gamma(k):
    return k * U / (1.0 - k * U)


def decays(name):
    """omtm.configure_optimizers on this architecture (mtm_model.py:779-841)."""
    return name.endswith("weight") and ".norm" not in name and not name.endswith(".0.weight")


def head_key(name):
    """The loss key whose output head ``name`` belongs to (never the actions head: it takes part in every loss), or None."""
    for k in ("states", "rewards", "returns"):
        if name.startswith(f"output_head_dict.{k}."):
            return k
    return None


def active(name, loss_keys_bits, keys=("states", "actions", "rewards", "returns")):
    k = head_key(name)
    return k is None or bool((loss_keys_bits >> keys.index(k)) & 1)


def lr_lambda(step, num_train_steps, warmup_steps=0):
    if warmup_steps > 0:
        if step < warmup_steps:
            return step / warmup_steps
        step = step - warmup_steps
        return 0.5 * (1 + np.cos(step / (num_train_steps - warmup_steps) * np.pi))
    return 0.5 * (1 + np.cos(step / num_train_steps * np.pi))


def lr_at(step, learning_rate, num_train_steps, warmup_steps=0):
    return learning_rate * float(lr_lambda(step, num_train_steps, warmup_steps))


def adamw_tensor(p, g, m, v, step, lr_t, wd, decay, is_active, beta1=0.9, beta2=0.999, eps=1e-8):
    """One tensor, float64: -> (p', m', v', step', bound_p, bound_m, bound_v).  Inputs are the fp32 values the device holds (any
    float dtype; converted exactly).  An inactive tensor comes back unchanged with zero bounds: its bits must not move."""
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    if not is_active:
        z = np.zeros_like(p)
        return p.copy(), m.copy(), v.copy(), int(step), z, z.copy(), z.copy()
    t = int(step) + 1
    m_ref = m + (1.0 - beta1) * (g - m)
    v_ref = beta2 * v + (1.0 - beta2) * g * g
    bm = (gamma(3) * (1.0 - beta1) * np.abs(g - m) + U * np.abs(m_ref)) * (1 + 8 * U) + 3 * ETA
    bv = (gamma(2) * beta2 * np.abs(v) + gamma(3) * (1.0 - beta2) * g * g + U * np.abs(v_ref)) * (1 + 8 * U) + 4 * ETA
    bc1 = 1.0 - beta1 ** t
    c = math.sqrt(1.0 - beta2 ** t)
    s = lr_t / bc1
    k = (1.0 - lr_t * wd) if decay else 1.0

    def quot(mm, vv):
        return s * mm / (np.sqrt(vv) / c + eps)

    q_ref = quot(m_ref, v_ref)
    p_ref = p * k - q_ref
    v_lo, v_hi = np.maximum(v_ref - bv, 0.0), v_ref + bv
    spread = np.zeros_like(p)
    for mm in (m_ref - bm, m_ref + bm):
        for vv in (v_lo, v_hi):
            spread = np.maximum(spread, np.abs(quot(mm, vv) - q_ref))
    bp = spread + 64 * D * (np.abs(p * k) + np.abs(q_ref) + spread) + U * np.abs(p_ref) + ETA
    return p_ref, m_ref, v_ref, t, bp, bm, bv


def adamw(params, grads, exp_avg, exp_avg_sq, steps, lr_t, wd, loss_keys_bits, beta1=0.9, beta2=0.999, eps=1e-8):
    """Every tensor of {name: array} dicts -> dict name -> the tuple of adamw_tensor."""
    return {n: adamw_tensor(params[n], grads[n], exp_avg[n], exp_avg_sq[n], steps[n], lr_t, wd, decays(n), active(n, loss_keys_bits), beta1,
                            beta2, eps) for n in params}


def temperature_step(log_t, m, v, step, entropy, target_entropy, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam on the float64 scalar log_temperature with grad = exp(log_t) (entropy - target_entropy): -> (log_t', m', v',
    step', bound).  The bound: the device evaluates the same ~20 float64 operations with its own exp and pow (a few units in the
    last place each); every intermediate is bounded by the step's size |lr / bc1 * m / denom| <= ~lr / (1 - beta1) or by |log_t|, so
    64 units of 2^-53 on |log_t'| + the step cover it, and as much again relative for exp(log_t')."""
    t = int(step) + 1
    g = math.exp(log_t) * (entropy - target_entropy)
    m2 = m + (g - m) * (1.0 - beta1)
    v2 = v * beta2 + ((1.0 - beta2) * g) * g
    step_size = lr / (1.0 - beta1 ** t)
    denom = math.sqrt(v2) / math.sqrt(1.0 - beta2 ** t) + eps
    delta = (step_size * m2) / denom
    out = log_t - delta
    return out, m2, v2, t, 64 * D * (abs(out) + abs(delta) + abs(log_t))


def bf16_split(p32):
    """hi = bf16(p), lo = bf16(p - hi) by torch's round-to-nearest-even conversion: -> two int16 bit arrays."""
    import torch
    p = torch.from_numpy(np.ascontiguousarray(np.asarray(p32, np.float32)))
    hi = p.to(torch.bfloat16)
    lo = (p - hi.to(torch.float32)).to(torch.bfloat16)
    return hi.view(torch.int16).numpy(), lo.view(torch.int16).numpy()


def worst(got, ref, bound):
    """max |got - ref| / bound over the elements with a positive bound; elements with bound 0 must be equal."""
    got, ref, bound = (np.asarray(x, np.float64).reshape(-1) for x in (got, ref, bound))
    err = np.abs(got - ref)
    zero = bound == 0
    if zero.any() and err[zero].max() > 0:
        return float("inf")
    if zero.all():
        return 0.0
    return float((err[~zero] / bound[~zero]).max())
