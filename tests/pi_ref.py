"""CPU reference of the persistence image (include/tda_dgm.h
tda_persistence_image) in mpmath at 40 digits, and the accuracy bound the header
derives; test infrastructure only.

    pi_p     = the float64 d_p - b_p              (finite rows only)
    w_p      = pi_p ^ weight_power for pi_p > 0, else 0
    gx_p[i]  = (erf((x_edges[i + 1] - b_p) r) - erf((x_edges[i] - b_p) r)) / 2,  r = 1 / (sigma sqrt(2))
    gy_p[j]  = the same with y_edges and pi_p
    out[i][j] = sum_p w_p gx_p[i] gy_p[j]

The erf values are computed in mpmath and then held as integers scaled by 2^140
(40 digits are 133 bits), so that the n W H products and sums run on exact
Python integers: the result's error is that of the erf values, some 1e-40."""
import mpmath
import numpy as np

U = 2.0 ** -53
ERF_ULP = 16  # E: the OpenCL conformance bound of double erf (tda_dgm.h says why this one)
SHIFT = 140


def C(n: int) -> int:
    """tda_dgm.h: C(n) = 2 E + 9 + n."""
    return 2 * ERF_ULP + 9 + n


def finite_points(D) -> np.ndarray:
    D = np.asarray(D, dtype=np.float64).reshape(-1, 2)
    return D[np.isfinite(D).all(axis=1)]


def weights(D, weight_power: float = 1.0):
    """The exact weights (mpf) of the finite rows of D."""
    D = finite_points(D)
    with mpmath.workdps(40):
        return [mpmath.mpf(float(p)) ** mpmath.mpf(float(weight_power)) if p > 0 else mpmath.mpf(0) for p in D[:, 1] - D[:, 0]]


def bound(D, n=None, weight_power: float = 1.0) -> float:
    """C(n) u sum_p w_p, n the finite rows of D unless given."""
    w = weights(D, weight_power)
    with mpmath.workdps(40):
        return float(C(len(w) if n is None else n) * mpmath.mpf(U) * mpmath.fsum(w))


def _masses(centres, edges, sigma):
    """(n, len(edges) - 1) integers: the Gaussian's mass per pixel, times 2^(SHIFT + 1)."""
    r = 1 / (mpmath.mpf(float(sigma)) * mpmath.sqrt(2))
    rows = []
    for c in centres:
        e = [int(mpmath.floor(mpmath.ldexp(mpmath.erf((mpmath.mpf(float(x)) - mpmath.mpf(float(c))) * r), SHIFT))) for x in edges]
        rows.append([e[k + 1] - e[k] for k in range(len(edges) - 1)])
    return np.array(rows, dtype=object).reshape(len(centres), len(edges) - 1)


def image(D, x_edges, y_edges, sigma: float, weight_power: float = 1.0) -> np.ndarray:
    """(W, H) object array of mpf: the image of diagram D at 40 digits."""
    D = finite_points(D)
    W, H = len(x_edges) - 1, len(y_edges) - 1
    with mpmath.workdps(40):
        if not len(D):
            return np.array([[mpmath.mpf(0)] * H for _ in range(W)], dtype=object).reshape(W, H)
        pers = D[:, 1] - D[:, 0]  # float64, as the library forms it
        w = np.array([int(mpmath.floor(mpmath.ldexp(x, SHIFT))) for x in weights(D, weight_power)], dtype=object)
        gx, gy = _masses(D[:, 0], x_edges, sigma), _masses(pers, y_edges, sigma)
        acc = np.dot((gx * w[:, None]).T, gy)  # exact integers, times 2^(3 SHIFT + 2)
        return np.array([[mpmath.ldexp(mpmath.mpf(int(v)), -(3 * SHIFT + 2)) for v in row] for row in acc], dtype=object).reshape(W, H)


def errors(out, exact) -> np.ndarray:
    """|out - exact| per pixel as float64 (out float64, exact from image())."""
    with mpmath.workdps(40):
        return np.array([[float(abs(mpmath.mpf(float(o)) - e)) for o, e in zip(ro, re)] for ro, re in zip(np.asarray(out), exact)],
                        dtype=np.float64).reshape(np.asarray(out).shape)


def restatement(D, x_edges, y_edges, sigma: float, weight_power: float = 1.0) -> np.ndarray:
    """The same in plain float64 with libm's erf (context for the bound, and the profiler's CPU figure)."""
    from math import erf

    D = finite_points(D)
    pers = D[:, 1] - D[:, 0]
    w = np.where(pers > 0, np.power(np.where(pers > 0, pers, 1.0), weight_power), 0.0)
    r = 0.70710678118654752440 / sigma
    ex = np.array([[erf((x - b) * r) for x in x_edges] for b in D[:, 0]]).reshape(len(D), len(x_edges))
    ey = np.array([[erf((y - p) * r) for y in y_edges] for p in pers]).reshape(len(D), len(y_edges))
    gx, gy = 0.5 * np.diff(ex, axis=1), 0.5 * np.diff(ey, axis=1)
    return (gx * w[:, None]).T @ gy
