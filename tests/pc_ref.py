"""CPU reference of the persistence curves (include/tda_dgm.h tda_persistence_curve):
the definition in numpy float64, test infrastructure only.

    acc = +0.0; for p in row order: where K_p(t) > 0: acc = acc + c_p * K_p(t)

K the indicator of b <= t < d or the tent max(0, min(t - b, d - t)).  The loop
runs over the points and is vectorised over the grid only, so every value sees
the additions of the definition in their order, each product and each sum
rounded once; the library is compared with ``np.array_equal``.  Also here: the
coefficient formulas of the named curves, as the docstrings of diagrams.py state
them."""
import numpy as np


def kept_rows(D, essential: bool = False) -> np.ndarray:
    """The mask of the rows a call keeps: finite b and finite d or, with ``essential``, d = +inf."""
    D = np.asarray(D, dtype=np.float64).reshape(-1, 2)
    ok_d = np.isfinite(D[:, 1]) | (D[:, 1] == np.inf) if essential else np.isfinite(D[:, 1])
    return np.isfinite(D[:, 0]) & ok_d


def accumulate(D, grid, coef=None, kernel: str = "indicator", essential: bool = False):
    """(acc (G,), W): the sums of the definition before TDA_PC_NORMALIZE, and the divisor it would use."""
    assert kernel in ("indicator", "tent") and not (essential and kernel == "tent")
    D = np.asarray(D, dtype=np.float64).reshape(-1, 2)
    grid = np.asarray(grid, dtype=np.float64)
    keep = kept_rows(D, essential)
    c = None if coef is None else np.asarray(coef, dtype=np.float64).reshape(-1)[keep]
    D = D[keep]
    acc = np.zeros(len(grid))
    W = np.float64(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for p, (b, d) in enumerate(D):
            if kernel == "tent":
                K = np.minimum(grid - b, d - grid)
                K = np.where(K > 0, K, 0.0)
            else:
                K = np.where((b <= grid) & (grid < d), 1.0, 0.0)
            term = K if c is None else c[p] * K
            acc = np.where(K > 0, acc + term, acc)  # outside the support nothing is added
            if c is not None:
                W = W + c[p]  # row order
    return acc, (W if c is not None else np.float64(len(D)))


def normalized(acc, W) -> np.ndarray:
    """acc / W; zeros for W == 0, and a zero quotient of either sign is +0.0."""
    if W == 0:
        return np.zeros(len(acc))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        q = acc / W
    return np.where(q == 0, 0.0, q)


def curve(D, grid, coef=None, kernel: str = "indicator", normalize: bool = False, essential: bool = False) -> np.ndarray:
    """(G,) float64: the curve of diagram D at the grid values; coef holds one value per row of D."""
    acc, W = accumulate(D, grid, coef, kernel, essential)
    return normalized(acc, W) if normalize else acc


def curves(dgms, grid, coef=None, **kw) -> np.ndarray:
    if not len(dgms):
        return np.zeros((0, len(grid)))
    return np.stack([curve(D, grid, None if coef is None else coef[s], **kw) for s, D in enumerate(dgms)])


# ---------------------------------------------------------------- the named curves' coefficients
def finite(D) -> np.ndarray:
    D = np.asarray(D, dtype=np.float64).reshape(-1, 2)
    return D[kept_rows(D)]


def lifespan_coef(D) -> np.ndarray:
    D = finite(D)
    return D[:, 1] - D[:, 0]


def entropy_coef(D) -> np.ndarray:
    D = finite(D)
    l = D[:, 1] - D[:, 0]  # noqa: E741
    p = l / l.sum()
    return -p * np.log(p)


def silhouette_coef(D, power: float = 1.0) -> np.ndarray:
    D = finite(D)
    return np.power(D[:, 1] - D[:, 0], power)


def betti(D, grid, essential: bool = True) -> np.ndarray:
    return curve(D, grid, essential=essential)


def lifespan(D, grid) -> np.ndarray:
    return curve(finite(D), grid, lifespan_coef(D))


def entropy(D, grid) -> np.ndarray:
    return curve(finite(D), grid, entropy_coef(D))


def silhouette(D, grid, power: float = 1.0) -> np.ndarray:
    return curve(finite(D), grid, silhouette_coef(D, power), kernel="tent", normalize=True)
