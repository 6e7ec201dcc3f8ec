"""Float64 restatements of the reference's spectral metrics (test infrastructure
only): matrix_entropy (metrics.py:344-399), compute_fixed_window_ed (:47-109)
and compute_fixed_window_id (:211-265), on LAPACK through numpy.

The entropy's spectrum is taken from the singular values of Z in float64
(lambda_i = s_i^2, min(N, D) of them): the N x N Gram matrix's further
eigenvalues are exact zeros for N > D and add nothing at the orders alpha > 0
that the library supports.
"""
from __future__ import annotations

import numpy as np


F32_ULP = 2.0 ** -23  # spacing of float32 at p = 1: entropies below it are not resolved by float32 arithmetic on p
F64_ULP = 2.0 ** -52  # the same for float64


def rel_gap(a: float, b: float, floor: float) -> float:
    """|a - b| / |b|.  Non-finite values must be equal (gap 0, else inf).  Where
    |b| <= floor -- an entropy that is zero but for the eps in the trace, which
    arithmetic of that precision on p = lambda / (trace + eps) cannot resolve
    (m = 1, the zero matrix) -- a within floor of b counts as gap 0."""
    a, b = float(a), float(b)
    if not (np.isfinite(a) and np.isfinite(b)):
        return 0.0 if (a == b or (np.isnan(a) and np.isnan(b))) else float("inf")
    d = abs(a - b)
    if abs(b) <= floor:
        return 0.0 if d <= floor else float("inf")
    return d / abs(b)


def matrix_entropy(Z, alpha: float = 1.0, eps: float = 1e-10) -> np.ndarray:
    """(..., N, D) -> (...) float64."""
    Z = np.asarray(Z, dtype=np.float64)
    lam = np.linalg.svd(Z, compute_uv=False) ** 2
    p = lam / (lam.sum(axis=-1, keepdims=True) + eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        if abs(alpha - 1.0) < eps:
            return -np.sum(np.where(p > 0.0, p * np.log(np.where(p > 0.0, p, 1.0)), 0.0), axis=-1)
        return np.log(np.sum(p ** alpha, axis=-1)) / (1.0 - alpha)


def effective_dimensionality(X) -> np.ndarray:
    """metrics.py:5-44: (batch, n, d) -> (batch,) float64."""
    X = np.asarray(X, dtype=np.float64)
    S = np.linalg.svd(X, compute_uv=False)
    s1, s2 = S.sum(axis=-1), (S * S).sum(axis=-1)
    return s1 * s1 / np.maximum(s2, 1e-10) / max(float(min(X.shape[1:])), 1.0)


def windows(X, n_windows: int) -> np.ndarray:
    """The reference's window split: (B, S, D) -> (B, W, S // W, D), W =
    min(n_windows, S), the last S % W rows of every item dropped."""
    X = np.asarray(X)
    B, S, D = X.shape
    W = min(n_windows, S)
    ws = S // W
    return X[:, : W * ws].reshape(B, W, ws, D)


def fixed_window_ed(X, n_windows: int) -> np.ndarray:
    """(B, S, D) -> (B, W) float64."""
    w = windows(X, n_windows)
    B, W = w.shape[:2]
    return effective_dimensionality(w.reshape((B * W,) + w.shape[2:])).reshape(B, W)


def twonn(x, discard_fraction: float = 0.1, eps: float = 1e-10) -> float:
    """metrics.py:113-208 for one (n, d) cloud, in float64."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    if n <= 5:
        return float("nan")
    d = np.sqrt(np.maximum(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1), 0.0))
    np.fill_diagonal(d, np.inf)
    r = np.sort(d, axis=1)[:, :2]
    ok = (r[:, 0] > eps) & (r[:, 1] > eps)
    mu = np.sort(r[ok, 1] / r[ok, 0])
    if mu.size < 5:
        return float("nan")
    keep = max(int(mu.size * (1.0 - discard_fraction)), 5)
    mu = mu[:keep]
    f = np.arange(1, mu.size + 1, dtype=np.float64) / float(n)
    xs, ys = np.log(mu + eps), -np.log(1.0 - f + eps)
    if xs.size < 2 or xs.var(ddof=1) < eps or ys.var(ddof=1) < eps:
        return float("nan")
    den = float((xs * xs).sum())
    if abs(den) < eps:
        return float("nan")
    slope = float((xs * ys).sum()) / den
    return slope if np.isfinite(slope) and 0.0 < slope < 1000.0 else float("nan")


def fixed_window_id(X, n_windows: int, discard_fraction: float = 0.1) -> np.ndarray:
    """(B, S, D) -> (B, n_windows) float64, NaN in the reference's cases."""
    X = np.asarray(X)
    B, S, _ = X.shape
    if n_windows <= 0 or S < n_windows or S < 6 or S // n_windows < 6:
        return np.full((B, max(n_windows, 0)), np.nan)
    w = windows(X, n_windows)
    return np.array([[twonn(w[b, k], discard_fraction) for k in range(n_windows)] for b in range(B)])
