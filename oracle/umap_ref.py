"""CPU restatement of umap-learn's fuzzy simplicial set -- TEST INFRASTRUCTURE
ONLY (checker for the k_umap_* kernels; the product never imports it).

umap-learn (third-party, unpinned; not vendored in the reference, not
installed here) is what the reference calls at debug_tda_pipeline.py:96-104.
Its published small-data path (N < 4096) is restated step by step:
  * distances: sklearn pairwise_distances with umap's own metric function
    (umap.distances.cosine: 1 - <x,y> / sqrt(|x|^2 |y|^2), f64), or euclidean;
  * kNN: argsort of each distance row (self included), first n_neighbors;
  * smooth_knn_dist: rho = smallest non-zero neighbour distance
    (local_connectivity 1), sigma by 64-step bisection of
    sum_{j>=1} exp(-(d_j - rho) / sigma) = log2(k) (tolerance 1e-5), floor
    1e-3 * mean neighbour distance;
  * compute_membership_strengths: 0 for self, 1 if d - rho <= 0, else
    exp(-(d - rho) / sigma);
  * fuzzy union (set_op_mix_ratio 1) in float32: (P + P^T) - P o P^T;
  * simplicial_set_embedding's pruning: entries < max / n_epochs -> 0.
Also a kNN-preservation measure for the distributional layout checks.

The layout itself (csrc/umap_kernels.h: k_umap_spectral, k_umap_sgd and the
SGD half of k_umap_transform) is restated in numpy float64 as that header
states it -- umap_hash / rnd_unit (the random streams, part of the kernels'
contract: they depend on the seed only), init_random, spectral_init,
sgd_fit and sgd_transform:
  * spectral_init: scipy eigh of D^-1/2 S D^-1/2 (D = f32 row sums of the
    pruned graph), eigenvectors 1..c after the trivial one, 10 / max|.|,
    the 1e-4 N(0, 1) noise of the Box-Muller streams 2 and 3, f32 min-max to
    [0, 10]; both sign choices of every column are returned;
  * sgd: the epoch-synchronous optimize_layout_euclidean -- every sample of
    an epoch reads the epoch-start layout, squared distances are rounded to
    f32, gradients clipped at 4, moves summed exactly as integers of
    rint(v * 2^40), the layout rounded to f32 once per epoch.
"""
from __future__ import annotations

import numpy as np


def distances(X: np.ndarray, metric: str = "euclidean") -> np.ndarray:
    X64 = np.asarray(X, dtype=np.float64)
    if metric == "cosine":
        G = X64 @ X64.T
        nrm = np.diag(G).copy()
        with np.errstate(divide="ignore", invalid="ignore"):
            D = 1.0 - G / np.sqrt(np.outer(nrm, nrm))
        zx = nrm == 0.0
        D[np.outer(zx, ~zx) | np.outer(~zx, zx)] = 1.0
        D[np.outer(zx, zx)] = 0.0
        D = np.maximum(D, 0.0)
    else:
        sq = np.sum(X64 * X64, axis=1)
        D = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * (X64 @ X64.T), 0.0))
    np.fill_diagonal(D, 0.0)
    return D.astype(np.float32)


def smooth_knn(kd: np.ndarray, k: int):
    n = kd.shape[0]
    target = np.log2(k)
    rho = np.zeros(n)
    sigma = np.zeros(n)
    mean_all = float(np.mean(kd.astype(np.float64)))
    for i in range(n):
        d = kd[i].astype(np.float64)
        nz = d[d > 0.0]
        rho[i] = nz[0] if nz.size else 0.0
        lo, hi, mid = 0.0, np.inf, 1.0
        for _ in range(64):
            dd = d[1:] - rho[i]
            psum = float(np.sum(np.where(dd > 0, np.exp(-(np.maximum(dd, 0) / mid)), 1.0)))
            if abs(psum - target) < 1e-5:
                break
            if psum > target:
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2.0 if np.isinf(hi) else (lo + hi) / 2.0
        s = mid
        floor = 1e-3 * (np.mean(d) if rho[i] > 0.0 else mean_all)
        sigma[i] = max(s, floor)
    return rho, sigma


def fuzzy_graph(X: np.ndarray, n_neighbors: int, metric: str = "euclidean", n_epochs: int = 500) -> np.ndarray:
    """Dense (N, N) float32 pruned fuzzy union, as the GPU returns it."""
    D = distances(X, metric)
    n = D.shape[0]
    idx = np.stack([np.lexsort((np.arange(n), D[i]))[:n_neighbors] for i in range(n)])
    kd = np.take_along_axis(D, idx, 1)
    rho, sigma = smooth_knn(kd, n_neighbors)
    P = np.zeros((n, n), np.float32)
    for i in range(n):
        for j in range(n_neighbors):
            c = idx[i, j]
            if c == i:
                v = 0.0
            elif kd[i, j] - rho[i] <= 0.0 or sigma[i] == 0.0:
                v = 1.0
            else:
                v = np.exp(-((kd[i, j] - rho[i]) / sigma[i]))
            P[i, c] = np.float32(v)
    S = (P + P.T) - P * P.T
    S[S < S.max() / float(n_epochs)] = 0.0
    return S.astype(np.float32)


def knn_preservation(X: np.ndarray, Y: np.ndarray, k: int, metric: str = "euclidean") -> float:
    """Mean fraction of each point's k nearest input neighbours that are among
    its k nearest neighbours in the layout."""
    DX = distances(X, metric)
    DY = distances(Y, "euclidean")
    n = DX.shape[0]
    np.fill_diagonal(DX, np.inf)
    np.fill_diagonal(DY, np.inf)
    a = np.argsort(DX, 1)[:, :k]
    b = np.argsort(DY, 1)[:, :k]
    return float(np.mean([len(set(a[i]) & set(b[i])) / k for i in range(n)]))


def transform_graph(X_train: np.ndarray, Y: np.ndarray, n_neighbors: int, metric: str = "euclidean",
                    disconnection: float = np.inf):
    """The bipartite graph of umap-learn's UMAP.transform: for each of the M
    new points its n_neighbors nearest training points (ties: smaller index)
    and their memberships -- smooth_knn_dist with local_connectivity 0 (rho =
    0; slot 0 skipped in the bisection as umap does), 0 for a neighbour at >=
    the disconnection distance.  Returns (idx, vals), both (M, k), vals f32."""
    Z = np.concatenate([np.asarray(X_train), np.asarray(Y)]).astype(np.float32)
    D = distances(Z, metric)
    N, M, k = X_train.shape[0], Y.shape[0], n_neighbors
    C = D[N:, :N]
    idx = np.stack([np.lexsort((np.arange(N), C[i]))[:k] for i in range(M)])
    kd = np.take_along_axis(C, idx, 1)
    mean_all = float(np.mean(kd.astype(np.float64)))
    target = np.log2(k)
    vals = np.empty((M, k), np.float32)
    for i in range(M):
        d = kd[i].astype(np.float64)
        lo, hi, mid = 0.0, np.inf, 1.0
        for _ in range(64):
            psum = float(np.sum(np.where(d[1:] > 0, np.exp(-(np.maximum(d[1:], 0) / mid)), 1.0)))
            if abs(psum - target) < 1e-5:
                break
            if psum > target:
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2.0 if np.isinf(hi) else (lo + hi) / 2.0
        sigma = max(mid, 1e-3 * mean_all)
        vals[i] = [0.0 if not kd[i, j] < disconnection else (1.0 if kd[i, j] <= 0.0 else np.exp(-(float(kd[i, j]) / sigma)))
                   for j in range(k)]
    return idx, vals


def transform_init(X_train: np.ndarray, emb: np.ndarray, Y: np.ndarray, n_neighbors: int, metric: str = "euclidean",
                   disconnection: float = np.inf) -> np.ndarray:
    """umap-learn UMAP.transform up to the initial embedding (what the GPU
    returns with learning_rate 0): transform_graph, then init_graph_transform
    (f32 weighted mean, or the neighbour's own embedding at membership 1, NaN
    without neighbours), over each row's entries in ascending training index
    (graph.tocsr() order)."""
    idx, V = transform_graph(X_train, Y, n_neighbors, metric, disconnection)
    M, k = idx.shape
    out = np.empty((M, emb.shape[1]), np.float32)
    for i in range(M):
        vals = V[i]
        nz = vals != 0.0
        if not nz.any():
            out[i] = np.nan
            continue
        # graph.tocsr() row order: ascending training index
        order = [j for j in np.argsort(idx[i], kind="stable") if nz[j]]
        rs = np.float32(0.0)
        for j in order:
            rs = np.float32(rs + vals[j])
        r = np.zeros(emb.shape[1], np.float32)
        for j in order:
            if vals[j] == 1.0:
                r = emb[idx[i, j]].astype(np.float32).copy()
                break
            r = (r + np.float32(vals[j] / rs) * emb[idx[i, j]]).astype(np.float32)
        out[i] = r
    return out


# ---------------------------------------------------------------- the layout
_M64 = (1 << 64) - 1


def _mix64(x: np.ndarray) -> np.ndarray:
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xFF51AFD7ED558CCD)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xC4CEB9FE1A85EC53)
    return x ^ (x >> np.uint64(33))


def _u64(x) -> np.ndarray:
    if isinstance(x, int):
        return np.asarray(x & _M64, dtype=np.uint64)
    return np.asarray(x).astype(np.uint64)  # integer arrays wrap mod 2^64


def umap_hash(a, b) -> np.ndarray:
    """umap_hash of csrc/umap_kernels.h (mix64 of csrc/rips_device.h): integer
    arithmetic mod 2^64 on Python ints or integer arrays -> uint64 array."""
    a, b = _u64(a), _u64(b)
    with np.errstate(over="ignore"):
        return _mix64(a * np.uint64(0x9E3779B97F4A7C15) ^ _mix64(b + np.uint64(0x632BE59BD9B4E019)))


def rnd_unit(seed: int, stream: int, idx) -> np.ndarray:
    """Uniform in [0, 1): stream 1 the subspace start block, 2 and 3 the
    Box-Muller pair of the spectral noise, 4 the random init."""
    h = umap_hash(seed, stream * 1000003 + np.asarray(idx, dtype=np.int64))
    return (h >> np.uint64(11)).astype(np.float64) * 2.0**-53


def _minmax_f32(E: np.ndarray) -> np.ndarray:
    """Per-column min-max to [0, 10], every operation in f32."""
    E = E.astype(np.float32)
    lo, hi = E.min(0), E.max(0)
    span = (hi - lo).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (np.float32(10.0) * (E - lo)).astype(np.float32) / span
    return np.where(span > 0, out, np.float32(0.0)).astype(np.float32)


def init_random(n: int, c: int, seed: int) -> np.ndarray:
    """init='random': uniform in [-10, 10) in f32, min-max to [0, 10]."""
    u = rnd_unit(seed, 4, np.arange(n * c)).reshape(n, c)
    return _minmax_f32((20.0 * u - 10.0).astype(np.float32))


def normalized_graph(S: np.ndarray, dtype=np.float64) -> np.ndarray:
    """D^-1/2 S D^-1/2 with D the f32 row sums of the pruned graph."""
    deg = np.sum(np.asarray(S, np.float64), axis=1).astype(np.float32)
    with np.errstate(divide="ignore"):
        dis = np.where(deg > 0, 1.0 / np.sqrt(deg.astype(np.float64)), 0.0)
    return (dis[:, None] * np.asarray(S, np.float64) * dis[None, :]).astype(dtype)


def spectral_init(S: np.ndarray, c: int, seed: int, dtype=np.float64) -> np.ndarray:
    """init='spectral' -> (2, n, c) float32: column d of [0] uses eigenvector
    d + 1 as eigh returns it, column d of [1] its negation (an eigenvector's
    sign is free; scale and min-max act per column, so the choices are
    independent).  ``dtype`` is the precision eigh runs in (float32 measures
    the layout's own sensitivity to rounding)."""
    from scipy.linalg import eigh

    n = S.shape[0]
    _, vec = eigh(normalized_graph(S, dtype))
    W = vec[:, ::-1][:, 1:c + 1].astype(np.float64)  # eigenvalues descending, the trivial one dropped
    m = float(np.max(np.abs(W)))
    expn = 10.0 / m if m > 0.0 else 1.0
    e = np.arange(n * c)
    u1 = np.maximum(rnd_unit(seed, 2, e), 1e-300)
    u2 = rnd_unit(seed, 3, e)
    noise = (1e-4 * np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)).astype(np.float32).reshape(n, c)
    return np.stack([_minmax_f32((sg * W * expn).astype(np.float32) + noise) for sg in (1.0, -1.0)])


_FIX = 2.0**40


def epochs_per_sample(w: np.ndarray, wmax, n_epochs: int) -> np.ndarray:
    """make_epochs_per_sample: n_samples = n_epochs * (w / w_max) in f32,
    n_epochs / n_samples in f64."""
    ns = np.float32(n_epochs) * (np.asarray(w, np.float32) / np.float32(wmax)).astype(np.float32)
    return float(n_epochs) / ns.astype(np.float64)


def _clip(v):
    return np.clip(v, -4.0, 4.0)


def _sgd(E0, T, head, tail, eps, n_epochs, a, b, lr, gamma, neg_rate, seed):
    """optimize_layout_euclidean, epoch-synchronous.  T None: fit (heads and
    tails in one embedding, both move; negative samples among its points);
    else transform (tails and negative samples in the fixed T)."""
    E = np.array(E0, dtype=np.float32)
    n, c = E.shape
    fit = T is None
    nv = n if fit else T.shape[0]
    live = eps >= 0.0
    slot = np.arange(eps.shape[0], dtype=np.int64)
    nxt = eps.copy()
    epsn = eps / float(neg_rate)
    nxn = epsn.copy()
    for ep in range(n_epochs):
        alpha = lr * (1.0 - float(ep) / float(n_epochs))
        O = E.astype(np.float64) if fit else np.asarray(T, np.float32).astype(np.float64)
        E64 = E.astype(np.float64)
        acc = np.zeros((n, c), np.int64)
        s = np.flatnonzero(live & (nxt <= float(ep)))
        j, k = head[s], tail[s]
        cur = E64[j]
        df = cur - O[k]
        d2 = np.zeros(s.shape[0])
        for d in range(c):
            d2 = d2 + df[:, d] * df[:, d]
        d2f = d2.astype(np.float32).astype(np.float64)
        pos = d2f > 0.0
        sd = np.where(pos, d2f, 1.0)
        gc = np.where(pos, -2.0 * a * b * np.power(sd, b - 1.0) / (a * np.power(sd, b) + 1.0), 0.0)
        gd = _clip(gc[:, None] * df)
        np.add.at(acc, j, np.rint(gd * alpha * _FIX).astype(np.int64))
        if fit:
            np.add.at(acc, k, np.rint(-gd * alpha * _FIX).astype(np.int64))
        nxt[s] += eps[s]
        nneg = ((float(ep) - nxn[s]) / epsn[s]).astype(np.int64)
        for p in range(int(nneg.max()) if s.size else 0):
            m = nneg > p
            q = (umap_hash(seed, (ep << 32) ^ (slot[s][m] << 8) ^ p) % np.uint64(nv)).astype(np.int64)
            dfn = cur[m] - O[q]
            r2 = np.zeros(q.shape[0])
            for d in range(c):
                r2 = r2 + dfn[:, d] * dfn[:, d]
            r2f = r2.astype(np.float32).astype(np.float64)
            posn = r2f > 0.0
            sr = np.where(posn, r2f, 1.0)
            g2 = np.where(posn, 2.0 * gamma * b / ((0.001 + sr) * (a * np.power(sr, b) + 1.0)), 0.0)
            gdn = np.where((g2 > 0.0)[:, None], _clip(g2[:, None] * dfn), 4.0)
            keep = posn | (j[m] != q)  # a coincident sample that is the head itself is skipped
            np.add.at(acc, j[m][keep], np.rint(gdn[keep] * alpha * _FIX).astype(np.int64))
        nxn[s] += nneg.astype(np.float64) * epsn[s]
        E = (E64 + acc.astype(np.float64) * (1.0 / _FIX)).astype(np.float32)
    return E


def sgd_fit(S: np.ndarray, E0: np.ndarray, n_epochs: int, a: float, b: float, lr: float = 1.0, gamma: float = 1.0,
            neg_rate: int = 5, seed: int = 42) -> np.ndarray:
    """k_umap_sgd on the pruned graph S from the layout E0: edges in
    row-major order of S > 0, head and tail both move."""
    head, tail = np.nonzero(S > 0)
    eps = epochs_per_sample(S[head, tail], S.max(), n_epochs)
    return _sgd(E0, None, head, tail, eps, n_epochs, a, b, lr, gamma, neg_rate, seed)


def transform_edges(idx: np.ndarray, vals: np.ndarray, n_epochs: int):
    """The transform's edge list: the M * k kNN slots in row-major order, with
    epochs_per_sample -1 for a dropped slot (membership 0) or one pruned below
    max / n_epochs."""
    M, k = idx.shape
    w = vals.reshape(-1).astype(np.float32)
    vm = np.float32(w.max())
    keep = (w != 0.0) & ~(w.astype(np.float64) < float(vm) / float(n_epochs))
    eps = np.full(M * k, -1.0)
    eps[keep] = epochs_per_sample(w[keep], vm, n_epochs)
    return np.repeat(np.arange(M), k), idx.reshape(-1).astype(np.int64), eps


def sgd_transform(idx: np.ndarray, vals: np.ndarray, emb_train: np.ndarray, E0: np.ndarray, n_epochs: int, a: float, b: float,
                  lr: float = 0.25, gamma: float = 1.0, neg_rate: int = 5, seed: int = 42) -> np.ndarray:
    """The SGD half of k_umap_transform (move_other=False) on the bipartite
    graph of transform_graph, from the initial embedding E0: only the new
    points move; tails and negative samples are training points, fixed."""
    head, tail, eps = transform_edges(idx, vals, n_epochs)
    return _sgd(E0, np.asarray(emb_train, np.float32), head, tail, eps, n_epochs, a, b, lr, gamma, neg_rate, seed)
