"""CPU reference of the Frechet mean (2-Wasserstein barycenter) of persistence diagrams, the
checker of test_frechet*.py.  Written from the definition (include/tda_dgm.h):

    drop the points with a non-finite coordinate
    c(p, q) = db*db + dd*dd            db = b_p - b_q, dd = d_p - d_q
    c(p)    = (pers*pers)*0.5          pers = d - b
    W2^2(Y, X) = min over partial matchings of the sum of the costs paid
    F(Y)    = (1/S) sum_j W2^2(Y, X_j)

A matching is solved in the full augmented formulation of tests/ws_ref.py: Y joined with one
diagonal copy per point of X against X joined with one diagonal copy per point of Y, a point
reaches only its own copy, copies reach each other at 0 (scipy.optimize.linear_sum_assignment on
the (K + n)^2 matrix; where there is no edge the matrix holds a finite constant no optimum uses).
``update`` is steps 2 - 3 of the definition in numpy scalar arithmetic, every operation rounded on
its own, in the pinned order.  The library's kernels share the cost expressions with this file
and nothing else.  Sums for checking are taken in ``np.longdouble`` over the float64 costs.
Test infrastructure only."""
import numpy as np
from scipy.optimize import linear_sum_assignment

U = 2.0 ** -53
f64 = np.float64


def finite_points(D) -> np.ndarray:
    D = np.asarray(D, dtype=np.float64).reshape(-1, 2)
    return D[np.isfinite(D).all(axis=1)]


def costs(Y, X):
    """(cross (K, n), diagonal of Y (K,), diagonal of X (n,)) of finite diagrams: float64, each
    operation rounded on its own."""
    db, dd = Y[:, None, 0] - X[None, :, 0], Y[:, None, 1] - X[None, :, 1]
    py, px = Y[:, 1] - Y[:, 0], X[:, 1] - X[:, 0]
    return db * db + dd * dd, (py * py) * 0.5, (px * px) * 0.5


def solve(Y, X) -> np.ndarray:
    """The reference's optimal matching as a map: per finite point of Y the index of its partner
    among the finite points of X, or -1 for the diagonal."""
    Y, X = finite_points(Y), finite_points(X)
    K, n = len(Y), len(X)
    C, cY, cX = costs(Y, X)
    big = 1.0 + float(np.abs(cY).sum() + np.abs(cX).sum())
    F = np.full((K + n, K + n), big)
    F[:K, :n] = C
    F[np.arange(K), n + np.arange(K)] = cY
    F[K + np.arange(n), np.arange(n)] = cX
    F[K:, n:] = 0.0
    rows, cols = linear_sum_assignment(F)
    assert not (F[rows, cols] == big).any()
    m = np.full(K + n, -1, np.int64)
    m[rows] = cols
    return np.where(m[:K] < n, m[:K], -1)


def terms(Y, X, match):
    """The float64 costs a map pays in the pinned order: the columns (points of Y) in increasing
    index, then the points of X at the diagonal in increasing index."""
    C, cY, cX = costs(Y, X)
    hit = match >= 0
    free = np.ones(len(X), bool)
    free[match[hit]] = False
    col = cY.copy()
    col[hit] = C[np.nonzero(hit)[0], match[hit]]
    return np.concatenate([col, cX[free]])


def check_matching(Y, X, match) -> np.longdouble:
    """Validates a map as `solve` returns it (one entry per finite point of Y, in [-1, n), no point
    of X named twice) and returns its cost: the longdouble sum of the float64 costs."""
    Y, X = finite_points(Y), finite_points(X)
    K, n = len(Y), len(X)
    match = np.asarray(match)
    assert match.shape == (K,) and match.dtype.kind == "i", (match.shape, match.dtype)
    assert ((match >= -1) & (match < n)).all()
    hit = match >= 0
    assert len(np.unique(match[hit])) == hit.sum(), "a point of the diagram is matched twice"
    return terms(Y, X, match).astype(np.longdouble).sum() + np.longdouble(0)


def cost_f64(Y, X, match) -> float:
    """cost_j as the library adds it: the float64 terms left to right from +0.0."""
    s = f64(0.0)
    for t in terms(finite_points(Y), finite_points(X), np.asarray(match)):
        s = s + t
    return float(s)


def cmax(Y, X) -> float:
    Y, X = finite_points(Y), finite_points(X)
    return float(max([0.0] + [x.max() for x in costs(Y, X) if x.size]))


def bound(Y, X) -> float:
    """Promise (a): 4 K_j^2 u cmax_j, K_j = K + n_j."""
    Kj = len(finite_points(Y)) + len(finite_points(X))
    return 4.0 * Kj * Kj * U * cmax(Y, X)


def point(sb, sd, k: int, S: int):
    """The update of k >= 1 points with coordinate sums (sb, sd) among S diagrams (step 2)."""
    kd, rd, Sd = f64(k), f64(S - k), f64(S)
    mb, md = f64(sb) / kd, f64(sd) / kd
    w = (mb + md) * f64(0.5)
    rw = rd * w
    return (kd * mb + rw) / Sd, (kd * md + rw) / Sd


def update(Y, Xs, G) -> np.ndarray:
    """Steps 2 - 3: the next diagram from the maps G[j] (one per diagram, as `solve` returns them)."""
    Y = finite_points(Y)
    Xs = [finite_points(X) for X in Xs]
    S, out = len(Xs), []
    for y in range(len(Y)):
        k, sb, sd = 0, None, None
        for j in range(S):
            g = int(G[j][y])
            if g < 0:
                continue
            b, d = Xs[j][g]
            sb, sd = (b, d) if k == 0 else (sb + b, sd + d)  # left to right, from the first partner
            k += 1
        if k:
            out.append(point(sb, sd, k, S))
    for j in range(S):
        taken = np.zeros(len(Xs[j]), bool)
        g = np.asarray(G[j], np.int64)
        taken[g[g >= 0]] = True
        for i in np.nonzero(~taken)[0]:
            out.append(point(Xs[j][i, 0], Xs[j][i, 1], 1, S))
    return np.array(out, np.float64).reshape(-1, 2)


def energy(Y, Xs, G) -> float:
    """E of a step as the library forms it: (the cost_j added in increasing j from +0.0) / S."""
    s = f64(0.0)
    for X, g in zip(Xs, G):
        s = s + f64(cost_f64(Y, X, g))
    return float(s / f64(len(Xs)))


def energy_ld(Y, Xs, G) -> np.longdouble:
    """The same in longdouble over the float64 costs."""
    return sum((check_matching(Y, X, g) for X, g in zip(Xs, G)), np.longdouble(0)) / np.longdouble(len(Xs))


def energy_bound(Y, Xs, G) -> float:
    """Promise (c) through the sum over j and the division: every cost_j within K_j u cost_j, the S
    additions and the division one rounding each of a value of at most the total."""
    Y = finite_points(Y)
    tot = sum(float(check_matching(Y, X, g)) for X, g in zip(Xs, G))
    Kmax = max(len(Y) + len(finite_points(X)) for X in Xs)
    return (Kmax + len(Xs) + 2) * U * tot / len(Xs)


def step(Y, Xs):
    """One step from Y: (next diagram, E, G) with the reference's own matchings."""
    Y = finite_points(Y)
    Xs = [finite_points(X) for X in Xs]
    G = [solve(Y, X) for X in Xs]
    return update(Y, Xs, G), energy(Y, Xs, G), G


def run(Xs, init=0, max_iter: int = 100):
    """The whole iteration: (mean, converged, energies)."""
    Xs = [finite_points(X) for X in Xs]
    Y = Xs[init] if isinstance(init, (int, np.integer)) else finite_points(init)
    energies = []
    for _ in range(max_iter):
        Yn, E, _ = step(Y, Xs)
        energies.append(E)
        same = Yn.shape == Y.shape and Yn.tobytes() == Y.tobytes()
        Y = Yn
        if same:
            return Y, True, energies
    return Y, False, energies
