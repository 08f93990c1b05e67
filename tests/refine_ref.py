"""fp64 restatement of the CEM / MPPI refinement of include/m3pc_hip.h (m3pc_refit_resample, m3pc_refine_plan), in numpy:
the refit of the sampling distribution on the elite candidates, the resample, and the loop around a scoring callback.  The
formulae are the header's; nothing here looks at the library."""
import numpy as np

CEM, MPPI = 0, 1


def weights(scores_elite, weighting, tau):
    """w (k,) fp64: 1 / k, or the softmax of tau * score over the elites (about their maximum, as the header states it)."""
    e = np.asarray(scores_elite, dtype=np.float64)
    if weighting == CEM:
        return np.full(e.shape, 1.0 / e.size)
    u = np.exp(float(tau) * (e - e.max()))
    return u / u.sum()


def spread_denominator(w):
    """D = sum w (1 - w): 1 - sum w^2 without the cancellation."""
    return float((w * (1.0 - w)).sum())


def refit(cand, elites, scores=None, weighting=CEM, tau=0.0, min_std=0.0):
    """cand (n, h, A), elites (k,) ids, scores (n,) -> (mean (h, A), std (h, A), D) in fp64:
    mean = sum w x;  S = sum w (x - mean)^2;  std = max(sqrt(S / D) if D > 1e-6 else 0, min_std)."""
    x = np.asarray(cand, dtype=np.float64)[np.asarray(elites, dtype=np.int64)]  # (k, h, A)
    k = x.shape[0]
    w = weights(np.zeros(k) if weighting == CEM else np.asarray(scores, dtype=np.float64)[np.asarray(elites, dtype=np.int64)],
                weighting, tau)
    wb = w.reshape(k, 1, 1)
    mean = (wb * x).sum(axis=0)
    S = (wb * (x - mean[None]) ** 2).sum(axis=0)
    D = spread_denominator(w)
    std = np.sqrt(S / D) if D > 1e-6 else np.zeros_like(S)
    return mean, np.maximum(std, float(min_std)), D


def resample(mean, std, noise):
    """min(1, max(-1, mean + std * noise)) in the dtype of the inputs (fp32 in: product and sum rounded separately, in fp32)."""
    return np.clip(mean[None] + std[None] * noise, -1.0, 1.0)


def top_k(scores, k):
    """ids of the k largest scores, descending, ties to the lower index."""
    s = np.asarray(scores)
    return np.lexsort((np.arange(s.size), -s.astype(np.float64)))[:k]


def loop(score_fn, mean0, init_std, noise, iterations, k, weighting=CEM, tau=0.0, min_std=0.0):
    """The refinement around ``score_fn(cand fp32 (n, h, A)) -> scores (n,)``: the distributions are refitted in fp64 and
    rounded to fp32 once, the candidates are resampled from them in fp32 (what the library does on its own distributions).
    noise (iterations + 1, n, h, A) fp32.  -> dict(mean, std (iterations + 1, h, A) fp32, trace [expect_return, top, mean, std],
    candidates, sample_action (1, A), eval_action (A,))."""
    noise = np.asarray(noise, dtype=np.float32)
    mean = np.asarray(mean0, dtype=np.float32)
    std = np.full_like(mean, np.float32(init_std))
    means, stds, trace = [mean], [std], []
    cand = resample(mean, std, noise[0])
    for it in range(iterations):
        er = np.asarray(score_fn(cand))
        top = top_k(er, k)
        m64, s64, _ = refit(cand, top, er, weighting, tau, min_std)
        mean, std = m64.astype(np.float32), s64.astype(np.float32)
        trace.append(dict(expect_return=er, top=top, mean=mean, std=std))
        means.append(mean)
        stds.append(std)
        cand = resample(mean, std, noise[it + 1])
    return dict(mean=np.stack(means), std=np.stack(stds), trace=trace, candidates=cand, sample_action=cand[0, 0][None],
                eval_action=mean[0])
