"""CPU reference of the 1-Wasserstein distance between two persistence
diagrams, the checker of test_wasserstein*.py.  Written from the definition
(include/tda_dgm.h):

    drop the points with a non-finite coordinate
    c(p, q) = sqrt((b_p - b_q)^2 + (d_p - d_q)^2)     p in A, q in B
    c(p)    = (d_p - b_p) * 0.70710678118654752440    the L2 distance to the diagonal
    W       = min over partial matchings of the sum of the costs paid

in the full augmented formulation: A joined with one diagonal copy per point of
B against B joined with one diagonal copy per point of A, a point reaches only
its own copy (at c(p)), copies reach each other at 0, and W is the cost of a
minimum-cost perfect matching (scipy.optimize.linear_sum_assignment; where
there is no edge the matrix holds a finite constant larger than the cost of
sending every point to the diagonal, so no optimum uses one).  ``value_reduced``
solves the n1 x (n2 + n1) form instead.  The library's kernel shares the cost
expressions with this file and nothing else.  Sums are taken in
``np.longdouble`` over the float64 costs.  Test infrastructure only."""
import numpy as np
from scipy.optimize import linear_sum_assignment

SQRT1_2 = 0.70710678118654752440
U = 2.0 ** -53


def finite_points(D) -> np.ndarray:
    D = np.asarray(D, dtype=np.float64).reshape(-1, 2)
    return D[np.isfinite(D).all(axis=1)]


def costs(A, B):
    """(cross (n1, n2), diagonal of A (n1,), diagonal of B (n2,)) of finite diagrams: float64, each
    operation rounded on its own."""
    db, dd = A[:, None, 0] - B[None, :, 0], A[:, None, 1] - B[None, :, 1]
    return np.sqrt(db * db + dd * dd), (A[:, 1] - A[:, 0]) * SQRT1_2, (B[:, 1] - B[:, 0]) * SQRT1_2


def augmented(A, B):
    """The (n1 + n2)^2 cost matrix and the constant it holds where there is no edge."""
    n1, n2 = len(A), len(B)
    C, cA, cB = costs(A, B)
    big = 1.0 + float(np.abs(cA).sum() + np.abs(cB).sum())
    F = np.full((n1 + n2, n1 + n2), big)
    F[:n1, :n2] = C
    F[np.arange(n1), n2 + np.arange(n1)] = cA
    F[n1 + np.arange(n2), np.arange(n2)] = cB
    F[n1:, n2:] = 0.0
    return F, big


def solve(A, B) -> np.ndarray:
    """The reference's optimal matching as a map: per finite point of A the index of its partner among
    the finite points of B, or -1 for the diagonal."""
    A, B = finite_points(A), finite_points(B)
    n1, n2 = len(A), len(B)
    F, big = augmented(A, B)
    rows, cols = linear_sum_assignment(F)
    assert not (F[rows, cols] == big).any()
    m = np.full(n1 + n2, -1, np.int64)
    m[rows] = cols
    return np.where(m[:n1] < n2, m[:n1], -1)


def check_matching(A, B, match) -> np.longdouble:
    """Validates a map as `solve` returns it (one entry per finite point of A, in [-1, n2), no point of
    B named twice) and returns its cost: the longdouble sum of the float64 costs."""
    A, B = finite_points(A), finite_points(B)
    n1, n2 = len(A), len(B)
    match = np.asarray(match)
    assert match.shape == (n1,) and match.dtype.kind == "i", (match.shape, match.dtype)
    assert ((match >= -1) & (match < n2)).all()
    hit = match >= 0
    assert len(np.unique(match[hit])) == hit.sum(), "a point of the second diagram is matched twice"
    C, cA, cB = costs(A, B)
    free = np.ones(n2, bool)
    free[match[hit]] = False
    ld = np.longdouble
    return (C[np.nonzero(hit)[0], match[hit]].astype(ld).sum() + cA[~hit].astype(ld).sum() + cB[free].astype(ld).sum() + ld(0))


def value(A, B) -> np.longdouble:
    """W(A, B): the cost of the reference's optimal matching."""
    return check_matching(A, B, solve(A, B))


def value_reduced(A, B) -> np.longdouble:
    """W(A, B) by a second formulation: the n1 x (n2 + n1) problem in which row p reaches every q at
    c(p, q) - c(q) and its own extra column at c(p), plus the constant sum of c(q)."""
    A, B = finite_points(A), finite_points(B)
    n1, n2 = len(A), len(B)
    C, cA, cB = costs(A, B)
    big = 1.0 + float(np.abs(cA).sum() + np.abs(cB).sum())
    F = np.full((n1, n2 + n1), big)
    F[:, :n2] = C - cB[None, :]
    F[np.arange(n1), n2 + np.arange(n1)] = cA
    rows, cols = linear_sum_assignment(F)
    m = np.full(n1, -1, np.int64)
    m[rows] = np.where(cols < n2, cols, -1)
    return check_matching(A, B, m)


def cmax(A, B) -> float:
    A, B = finite_points(A), finite_points(B)
    return float(max([0.0] + [x.max() for x in costs(A, B) if x.size]))


def bound(A, B) -> float:
    """The tolerance of an exact float64 solver's matching against the optimum: 4 K^2 u cmax, K = n1 + n2."""
    K = len(finite_points(A)) + len(finite_points(B))
    return 4.0 * K * K * U * cmax(A, B)

