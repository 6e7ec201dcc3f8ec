"""CPU reference of the persistence landscape (include/tda_dgm.h tda_landscape):
a numpy float64 restatement of the definition, test infrastructure only.

    f_p(t)      = max(0, min(t - b_p, d_p - t))
    lambda_k(t) = the k-th largest of the f_p(t), 0 beyond the diagram's points

Per grid value the tents are sorted descending, the first K taken and the rest
padded with zeros.  Every value is one rounded float64 subtraction or +0.0, so
the library is compared with ``np.array_equal``."""
import numpy as np


def finite_points(D) -> np.ndarray:
    D = np.asarray(D, dtype=np.float64).reshape(-1, 2)
    return D[np.isfinite(D).all(axis=1)]


def landscape(D, grid, K: int) -> np.ndarray:
    """(K, G) float64: lambda_1 .. lambda_K of diagram D at the grid values."""
    D = finite_points(D)
    grid = np.asarray(grid, dtype=np.float64)
    out = np.zeros((K, len(grid)))
    if not len(D):
        return out
    with np.errstate(over="ignore"):
        tents = np.minimum(grid[None, :] - D[:, :1], D[:, 1:] - grid[None, :])  # (n, G)
    tents = np.where(tents > 0, tents, 0.0)  # +0.0, never -0.0
    top = -np.sort(-tents, axis=0)[:K]
    out[:len(top)] = top
    return out


def landscapes(dgms, grid, K: int) -> np.ndarray:
    return np.stack([landscape(D, grid, K) for D in dgms]) if len(dgms) else np.zeros((0, K, len(grid)))
