"""numpy restatement of the resampling stage and of the bootstrap confidence bands
(tda-multimodal_amd/bootstrap.py, include/tda_rips.h tda_resample), the checker of
test_resample*.py.  Written from the definitions:

    H(dm, ix)   = max_i min_j dm[ix[j]][i]          the resample is a subset: one direction only
    sub(dm, ix) = dm[ix][:, ix]
    quantile    = the ceil((1 - alpha) * B)-th smallest of B statistics, no interpolation
    significant = persistence > 2 * radius, or an essential bar

Every value is an f32 distance copied, compared, subtracted or doubled, so comparisons with the
library are ``==``.  Test infrastructure only."""
import math

import numpy as np


def tables(idx, L):
    """The (L, B, m) view of a shared (B, m) or per-layer (L, B, m) index table."""
    idx = np.asarray(idx)
    return idx if idx.ndim == 3 else np.broadcast_to(idx[None], (L,) + idx.shape)


def hausdorff(dm, idx) -> np.ndarray:
    """(L, B) float64 of the f32 values max_i min_j dm[l][idx[b][j]][i]."""
    dm = np.asarray(dm)
    L = dm.shape[0]
    T = tables(idx, L)
    H = np.empty((L, T.shape[1]), dtype=np.float64)
    for l in range(L):
        for b in range(T.shape[1]):
            H[l, b] = dm[l][T[l, b]].min(axis=0).max()
    return H


def sub(dm_l, ix) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(dm_l)[np.ix_(ix, ix)])


def rank(B: int, alpha: float) -> int:
    return min(max(math.ceil((1.0 - alpha) * B), 1), B)


def quantile(stat, alpha: float) -> np.ndarray:
    """Along the last axis, by counting: the smallest value with at least rank(B, alpha) values <= it."""
    stat = np.asarray(stat, dtype=np.float64)
    B = stat.shape[-1]
    k = rank(B, alpha)
    out = np.empty(stat.shape[:-1])
    for pos in np.ndindex(*stat.shape[:-1]):
        row = stat[pos]
        out[pos] = min(v for v in row if np.count_nonzero(row <= v) >= k)
    return out


def significant(dgm, radius: float) -> np.ndarray:
    dgm = np.asarray(dgm, dtype=np.float64).reshape(-1, 2)
    return np.array([bool(np.isinf(d) or d - b > 2.0 * radius) for b, d in dgm], dtype=bool)


def bands(full_dgms, stat, alpha, dims):
    """(quantile, significant[l][k], n_significant) from the full clouds' diagrams
    (full_dgms[l][dim]) and the (len(dims), L, B) statistics."""
    q = quantile(stat, alpha)
    L = len(full_dgms)
    sig = [[significant(full_dgms[l][d], q[k, l]) for k, d in enumerate(dims)] for l in range(L)]
    n = np.array([[int(sig[l][k].sum()) for l in range(L)] for k in range(len(dims))], dtype=np.int64).reshape(len(dims), L)
    return q, sig, n
