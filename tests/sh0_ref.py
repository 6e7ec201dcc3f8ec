"""The numpy restatement of tda_subsample_h0 (include/tda_rips.h): Prim's algorithm from position 0
with np.argmin (the first minimum: the lowest position among equal keys), a sequential Python-float
sum in step order, and the persistent-homology dimension's regression in closed form.  Nothing here
imports the package."""
import numpy as np


def term(w, alpha):
    w = float(w)
    if alpha == 1:
        return w
    if alpha == 2:
        return w * w
    return w ** float(alpha)  # Python's float pow is the C library's


def prim(dm, pts, alpha=1.0):
    """dm: one layer's (N, N) f32 matrix; pts: the subsample's points by position.
    -> (E as a Python float, the s - 1 deaths in step order as float32)."""
    pts = np.asarray(pts, dtype=np.int64)
    s = len(pts)
    W = np.asarray(dm, dtype=np.float32)[np.ix_(pts, pts)]
    key = W[0].copy()
    out = np.ones(s, dtype=bool)
    out[0] = False
    deaths = np.zeros(s - 1, dtype=np.float32)
    acc = 0.0
    for t in range(1, s):
        j = int(np.argmin(np.where(out, key, np.inf)))  # the first of the smallest: `<`, lowest position
        if not out[j]:  # every remaining key is +inf: the first position outside the tree
            j = int(np.flatnonzero(out)[0])
        deaths[t - 1] = key[j]
        acc += term(key[j], alpha)
        out[j] = False
        upd = W[j] < key
        key[upd] = W[j][upd]
    return acc, deaths


def h0_subsamples(dm, idx, sizes=None, alpha=1.0):
    """dm (L, N, N) f32; idx (B, m) or (L, B, m); sizes (B,) or None (whole rows).
    -> E (L, B) float64 and deaths[l][b] (float32, step order)."""
    dm, idx = np.asarray(dm), np.asarray(idx)
    L, B, m = dm.shape[0], idx.shape[-2], idx.shape[-1]
    sizes = np.full(B, m) if sizes is None else np.asarray(sizes)
    E = np.zeros((L, B))
    deaths = []
    for l in range(L):
        tab = idx[l] if idx.ndim == 3 else idx
        row = []
        for b in range(B):
            E[l, b], d = prim(dm[l], tab[b, :sizes[b]], alpha)
            row.append(d)
        deaths.append(row)
    return E, deaths


def default_sizes(N):
    s = np.unique(np.round(np.linspace(N / 4, N, 10)).astype(int))
    return s[s >= 2]


def subsample_indices(N, sizes, n_trials, seed=0):
    """The draw order of the contract: sizes in the given order, then trials, rng.permutation(N)[:n]."""
    rng = np.random.default_rng(seed)
    sizes = [int(n) for n in sizes]
    idx = np.zeros((len(sizes) * n_trials, max(sizes)), dtype=np.int32)
    sz = np.zeros(len(sizes) * n_trials, dtype=np.int32)
    b = 0
    for n in sizes:
        for _ in range(n_trials):
            idx[b, :n] = rng.permutation(N)[:n]
            sz[b] = n
            b += 1
    return idx, sz


def regression(E, sizes, alpha=1.0):
    """Ordinary least squares of log E against log n over all B points, in closed form.
    -> (dimension, slope, intercept); nan where any E <= 0."""
    E = np.asarray(E, dtype=np.float64)
    if (E <= 0).any():
        return float("nan"), float("nan"), float("nan")
    x, y = np.log(np.asarray(sizes, dtype=np.float64)), np.log(E)
    n = len(x)
    sx, sy, sxx, sxy = x.sum(), y.sum(), (x * x).sum(), (x * y).sum()
    slope = (n * sxy - sx * sy) / (n * sxx - sx * sx)
    intercept = (sy - slope * sx) / n
    return alpha / (1.0 - slope), slope, intercept


def distances(X):
    """f32 Euclidean distances of one cloud for the CPU estimator tests (float64 differences, one
    rounding to f32; symmetric, zero diagonal)."""
    X = np.asarray(X, dtype=np.float64)
    d = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)).astype(np.float32)
    return np.maximum(d, d.T)


def ph_dimension(dm, alpha=1.0, sizes=None, n_trials=8, seed=0):
    """One layer's dimension through this file alone."""
    N = dm.shape[0]
    sizes = default_sizes(N) if sizes is None else sizes
    idx, sz = subsample_indices(N, sizes, n_trials, seed)
    E, _ = h0_subsamples(dm[None], idx, sz, alpha)
    return regression(E[0], sz, alpha), E, idx, sz
