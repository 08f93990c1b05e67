"""The eval_action certificate of include/m3pc_hip.h (m3pc_eval_bound) restated in fp64 numpy: the bound, bound(n') for every
prefix of the score list, and need_eval.  Everything is computed in the plainest possible way from the definitions:

    p = softmax(tau (m - max m)),  e = sum_j p_j a0_j,  eps = |tau| delta
    S_k = sum_{j in U} p_j |a0_jk - e_k|,  P_U = sum_{j in U} p_j
    B_k = expm1(eps) S_k / (1 - (1 - exp(-eps)) P_U),  bound = max_k B_k

with U = the candidates that are neither one of the r race entries nor one of the first n' score entries of the list."""
import numpy as np


def softmax_mean(m, a0, tau):
    """(p, e): the select's weights and eval_action on the score vector m."""
    m = np.asarray(m, dtype=np.float64)
    z = float(tau) * (m - m.max())
    w = np.exp(z)
    p = w / w.sum()
    return p, p @ np.asarray(a0, dtype=np.float64)


def bound_given(p, e, a0, in_U, eps):
    """(B_k for every k, P_U) for one set U (boolean mask)."""
    a0 = np.asarray(a0, dtype=np.float64)
    S = (p[in_U, None] * np.abs(a0[in_U] - e[None, :])).sum(axis=0)
    PU = p[in_U].sum()
    return np.expm1(eps) * S / (1.0 - (1.0 - np.exp(-eps)) * PU), PU


def eval_bound(m, a0, lst, r, n, n_listed, tau, delta, eval_tol=np.inf):
    """lst: r race entries (re-scored), then n_listed score entries of which the first n are re-scored.  Returns a dict:
    eval_bound = bound(n), need_eval, P_U, k (arg-max component of bound(n)), eps, bound_listed = bound(n_listed), n_U = |U| at n,
    bounds = [bound(n'), n' = n .. n_listed], e (the eval_action on m), p.  (``eval_bound_fast`` adds B = the B_k of bound(n).)"""
    m = np.asarray(m, dtype=np.float64)
    a0 = np.asarray(a0, dtype=np.float64).reshape(m.size, -1)
    lst = np.asarray(lst, dtype=np.int64)
    N = m.size
    p, e = softmax_mean(m, a0, tau)
    eps = abs(float(tau)) * float(delta)
    race, score = lst[:r], lst[r : r + n_listed]
    bounds, first = [], None
    for t in range(n, n_listed + 1):
        in_U = np.ones(N, dtype=bool)
        in_U[race[(race >= 0) & (race < N)]] = False
        s = score[:t]
        in_U[s[(s >= 0) & (s < N)]] = False
        B, PU = bound_given(p, e, a0, in_U, eps)
        bounds.append(float(B.max()) if B.size else 0.0)
        if t == n:
            first = dict(P_U=float(PU), k=int(np.argmax(B)), n_U=int(in_U.sum()))
    bounds = np.array(bounds)
    ok = np.nonzero(bounds <= eval_tol)[0]
    need = n + int(ok[0]) if ok.size else N
    return dict(eval_bound=float(bounds[0]), need_eval=need, eps=eps, bound_listed=float(bounds[-1]), bounds=bounds, e=e, p=p, **first)


def eval_bound_fast(m, a0, lst, r, n, n_listed, tau, delta, eval_tol=np.inf):
    """``eval_bound`` with the prefixes by cumulative sums (fp64; the same numbers to ~1e-13, for the large cases of the tests)."""
    m = np.asarray(m, dtype=np.float64)
    a0 = np.asarray(a0, dtype=np.float64).reshape(m.size, -1)
    lst = np.asarray(lst, dtype=np.int64)
    N = m.size
    p, e = softmax_mean(m, a0, tau)
    eps = abs(float(tau)) * float(delta)
    in_U = np.ones(N, dtype=bool)
    in_U[lst[: r + n]] = False
    score = lst[r + n : r + n_listed]
    live = in_U[score].copy()  # listed entries that are still in U (not re-scored as race entries)
    contrib = p[:, None] * np.abs(a0 - e[None, :])
    # taking entries out one by one: suffix sums of what is still in, so that nothing is subtracted
    rest = in_U.copy()
    rest[score] = False
    Srest, Prest = contrib[rest].sum(axis=0), p[rest].sum()
    c = contrib[score] * live[:, None]
    q = p[score] * live
    Ssuf = np.concatenate([np.cumsum(c[::-1], axis=0)[::-1], np.zeros((1, a0.shape[1]))], axis=0) + Srest[None, :]
    Psuf = np.concatenate([np.cumsum(q[::-1])[::-1], [0.0]]) + Prest
    B = np.expm1(eps) * Ssuf / (1.0 - (1.0 - np.exp(-eps)) * Psuf)[:, None]
    bounds = B.max(axis=1)
    ok = np.nonzero(bounds <= eval_tol)[0]
    need = n + int(ok[0]) if ok.size else N
    return dict(eval_bound=float(bounds[0]), need_eval=need, eps=eps, bound_listed=float(bounds[-1]), bounds=bounds, e=e, p=p,
                P_U=float(Psuf[0]), k=int(np.argmax(B[0])), n_U=int(in_U.sum()), B=B[0])
