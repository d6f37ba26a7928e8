"""Numpy restatement of the risk-aware candidate scores (cadm_amd/csrc/score.hip, `cadm_particle_score`).  Generic over dtype: it
computes in the dtype of `rows`.  The tests use it at float64 on the float32 inputs, where every float32 comparison is exact: rank
selection and ties are then the device's.

rows [..., p] -> scores [...]:
    mean        mu = sum_j r_j / p
    mean_std    mu - kappa sqrt(sum_j (r_j - mu)^2 / p)
    member_std  mu - kappa sqrt(sum_e (mu_e - mu)^2 / E),  mu_e = the mean of particles [e q, (e + 1) q), q = p / E
    cvar        the mean of the k particles of lowest rank,  rank_j = #{i : r_i < r_j or (r_i == r_j and i < j)}
A candidate with a NaN or infinite particle return scores its plain mean (numpy's: NaN, or +-inf) in every mode."""
import math

import numpy as np

MODES = ("mean", "mean_std", "member_std", "cvar")


def cvar_k(alpha, p):
    """The tail fraction alpha in (0, 1] as a particle count (the model classes' rule)."""
    return int(min(p, max(1, math.ceil(round(float(alpha) * p, 6)))))


def ranks(rows):
    """rank_j = #{i : r_i < r_j or (r_i == r_j and i < j)} along the last axis"""
    r = np.asarray(rows)
    ri, rj = r[..., None, :], r[..., :, None]                         # [..., j, i]
    idx = np.arange(r.shape[-1])
    lower = (ri < rj) | ((ri == rj) & (idx[None, :] < idx[:, None]))
    return lower.sum(axis=-1)


def score(rows, mode, kappa=0.0, k=None, E=None):
    r = np.asarray(rows)
    p = r.shape[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        mu = r.sum(axis=-1) / r.dtype.type(p)
        if mode == "mean":
            return mu
        if mode == "mean_std":
            s = mu - r.dtype.type(kappa) * np.sqrt(((r - mu[..., None]) ** 2).sum(axis=-1) / r.dtype.type(p))
        elif mode == "member_std":
            assert E is not None and p % E == 0
            mu_e = r.reshape(r.shape[:-1] + (E, p // E)).sum(axis=-1) / r.dtype.type(p // E)
            s = mu - r.dtype.type(kappa) * np.sqrt(((mu_e - mu[..., None]) ** 2).sum(axis=-1) / r.dtype.type(E))
        elif mode == "cvar":
            assert k is not None and 1 <= k <= p
            s = np.where(ranks(r) < k, r, r.dtype.type(0)).sum(axis=-1) / r.dtype.type(k)
        else:
            raise ValueError("unknown mode %r" % (mode,))
    return np.where(np.isfinite(r).all(axis=-1), s, mu)


def top_elites(cand, num_elites):
    """[m, num_elites] candidate ids by score descending, ties to the lower index (finite scores)."""
    return np.argsort(-np.asarray(cand, np.float64), axis=1, kind="stable")[:, :num_elites].astype(np.int32)
