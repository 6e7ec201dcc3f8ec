"""GPU tests of the 1-Wasserstein distance between persistence diagrams
(include/tda_dgm.h, diagrams.py) against the CPU reference tests/ws_ref.py.

What is compared, with K = n1 + n2, u = 2^-53 and cmax the pair's largest cost
(tda_dgm.h): the returned matching is a valid partial matching whose cost,
summed in longdouble over the float64 costs, lies within 4 K^2 u cmax of the
reference's optimum (bound 1: both are float64 solvers); the returned value
lies within K u value of that sum (bound 2: K non-negative terms added in some
order); and the bitwise promises (symmetry, a pair alone / among others /
shuffled / run to run) are ``==``.

Sizes: empty and one-point diagrams, 63 / 64 / 65 points (one wave and two),
the 512 limit, and both sides of the kernel's launch classes (max(n1, n2) <= 64
/ <= 256 / <= 512: another workgroup size), in either orientation.  No test
here calls the persistence pipeline (known limits)."""
import ctypes

import numpy as np
import pytest

import ws_ref

pytestmark = pytest.mark.gpu

SIZES = [(0, 0), (0, 1), (1, 0), (1, 1), (3, 5), (63, 64), (64, 64), (65, 64), (64, 65), (65, 1), (100, 157), (129, 127),
         (256, 256), (257, 256), (3, 257), (300, 212), (512, 511), (512, 512)]
GENERATORS = ("spread", "near")
LD = np.longdouble
E = np.zeros((0, 2))


def diagram(n: int, seed: int) -> np.ndarray:
    """n seeded (b, d) with d > b, values up to about 10; every third point is
    rounded to f32 and every fifth repeats the point before it (ties)."""
    rng = np.random.default_rng(seed)
    b = rng.uniform(0.0, 5.0, n)
    D = np.stack([b, b + rng.uniform(1e-3, 5.0, n)], 1)
    D[::3] = D[::3].astype(np.float32)
    D[4::5] = D[3::5][:len(D[4::5])]
    assert np.all(D[:, 1] > D[:, 0])
    return D


def near_pair(n1: int, n2: int, seed: int):
    """Two diagrams of short bars (persistence <= 0.2) whose first
    min(n1, n2) / 8 rows are long bars (persistence 2 .. 5), those of B being
    A's moved by up to 0.3 per coordinate: the long bars must be matched with
    each other."""
    rng = np.random.default_rng(seed)
    k = min(n1, n2) // 8

    def one(n):
        b = rng.uniform(0.0, 5.0, n)
        pers = rng.uniform(1e-3, 0.2, n)
        pers[:k] = rng.uniform(2.0, 5.0, k)
        return np.stack([b, b + pers], 1)

    A, B = one(n1), one(n2)
    B[:k] = A[:k] + rng.uniform(-0.3, 0.3, (k, 2))
    return A, B[rng.permutation(n2)]


_cases = {}


def case(n1, n2, gen):
    """The two diagrams of a size and their reference value, computed once."""
    if (n1, n2, gen) not in _cases:
        A, B = (diagram(n1, 1000 + n1), diagram(n2, 2000 + n2)) if gen == "spread" else near_pair(n1, n2, 3000 + n1 + n2)
        _cases[n1, n2, gen] = A, B, ws_ref.value(A, B)
    return _cases[n1, n2, gen]


def solve(pkg, A, B):
    """(value, the map of A's finite points, the rows) of one call with the matching; the rows are
    checked to be persim's: A's points in order, then the points of B no row names."""
    d, M = pkg.wasserstein(A, B, matching=True)
    n1, n2 = len(ws_ref.finite_points(A)), len(ws_ref.finite_points(B))
    assert isinstance(d, float) and M.dtype == np.float64 and M.ndim == 2 and M.shape[1] == 3
    assert M[:n1, 0].tolist() == list(range(n1)) and (M[n1:, 0] == -1).all()
    match = M[:n1, 1].astype(np.int64)
    assert (match == M[:n1, 1]).all()
    assert M[n1:, 1].tolist() == sorted(set(range(n2)) - set(match.tolist()))
    return d, match, M


def check_against(A, B, d, match, ref):
    """bounds 1 and 2 of a returned value and map against the reference optimum; returns the figures"""
    cost = ws_ref.check_matching(A, B, match)
    K = len(match) + len(ws_ref.finite_points(B))
    b1, b2 = ws_ref.bound(A, B), K * ws_ref.U * d
    e1, e2 = float(abs(cost - ref)), float(abs(LD(d) - cost))
    assert e1 <= b1 and e2 <= b2, (e1, b1, e2, b2)
    return e1, b1, e2, b2


@pytest.mark.parametrize("gen", GENERATORS)
@pytest.mark.parametrize("n1,n2", SIZES)
def test_matches_reference(pkg, n1, n2, gen):
    A, B, ref = case(n1, n2, gen)
    d, match, M = solve(pkg, A, B)
    print(f"n1={n1} n2={n2} {gen}: gpu={d!r} ref={float(ref)!r} matched={(match >= 0).sum()}")
    e1, b1, e2, b2 = check_against(A, B, d, match, ref)
    print(f"  |cost - ref| = {e1:.3e} (bound {b1:.3e}); |dist - cost| = {e2:.3e} (bound {b2:.3e})")
    assert pkg.wasserstein(A, B) == d  # without the matching: the same bits
    C, cA, cB = ws_ref.costs(ws_ref.finite_points(A), ws_ref.finite_points(B))
    hit = match >= 0
    assert np.array_equal(M[:n1, 2], np.where(hit, C[np.arange(n1), np.where(hit, match, 0)] if n2 else 0.0, cA))
    assert np.array_equal(M[n1:, 2], cB[M[n1:, 1].astype(np.int64)])


def chain(k, seed):
    """A_i = (2i, 2i + 100), B_i = (2i + 1, 2i + 101), rows shuffled."""
    rng = np.random.default_rng(seed)
    i = np.arange(k, dtype=np.float64)
    A, B = np.stack([2 * i, 2 * i + 100], 1), np.stack([2 * i + 1, 2 * i + 101], 1)
    return A[rng.permutation(k)], B[rng.permutation(k)]


@pytest.mark.parametrize("k", (2, 65, 200, 512))
def test_chain_needs_long_augmenting_paths(pkg, k):
    """A_i is at sqrt(2) from B_i and B_(i-1) and at 3 sqrt(2) or more from every other point, and the
    diagonal costs 100 / sqrt(2): the optimum matches A_i with B_i, and a row added where its two
    neighbours are taken moves the matching along the chain.  With one row of A removed, k - 1 pairs
    stay at sqrt(2) and one point of B pays the diagonal.  Each cost is a rounded sqrt (relative error
    <= u / 2) and the sum adds k terms: 2 k u W covers both."""
    A, B = chain(k, 40 + k)
    W = k * np.sqrt(LD(2))
    W1 = (k - 1) * np.sqrt(LD(2)) + 100 * LD(ws_ref.SQRT1_2)
    sa, sb = A[np.argsort(A[:, 0])], B[np.argsort(B[:, 0])]
    for X, Y in ((A, B), (B, A), (sa, sb), (sa[::-1].copy(), sb), (sb, sa[::-1].copy())):
        d, match, _ = solve(pkg, X, Y)
        assert abs(LD(d) - W) <= 2 * k * ws_ref.U * W, (d, W)
        assert (match >= 0).all() and sorted(match.tolist()) == list(range(k))
    for X, Y in ((A[1:], B), (B, A[1:]), (sa[1:], sb), (sb[::-1].copy(), sa[:-1])):
        d, match, M = solve(pkg, X, Y)
        assert abs(LD(d) - W1) <= 2 * k * ws_ref.U * W1, (d, W1)
        assert (M[:, :2] == -1).any(axis=1).sum() == 1  # exactly one point at the diagonal: one of B
        assert (match < 0).sum() == (1 if len(X) == k else 0)
    assert pkg.wasserstein(A, B) == pkg.wasserstein(B, A) and pkg.wasserstein(A[1:], B) == pkg.wasserstein(B, A[1:])


def abi(pkg, dgms, pairs, matching=True):
    """One library call on arrays: (dist (P,), per pair the map of its first diagram)."""
    dg = __import__("importlib").import_module(pkg.__name__ + ".diagrams")
    off = np.concatenate([[0], np.cumsum([len(d) for d in dgms])]).astype(np.int64)
    pts = np.ascontiguousarray(np.concatenate(dgms))
    pairs = None if pairs is None else np.ascontiguousarray(pairs, np.int32)
    dist, ms, moff, match = dg._call_ws(pts, off, pairs, 0, want_matching=matching)
    assert ms > 0
    return dist, [match[moff[p]:moff[p + 1]] for p in range(len(dist))] if matching else None


def inverse(match, n2):
    inv = np.full(n2, -1, np.int32)
    inv[match[match >= 0]] = np.nonzero(match >= 0)[0]
    return inv


def test_bitwise_invariants(pkg):
    """A pair's value and matching alone == among all pairs of 9 diagrams (all three launch classes in
    one call) == in a second run == in a shuffled explicit list holding both orientations; W(A, B) ==
    W(B, A), the matching of (B, A) being the inverse map; the matrix is symmetric with a zero diagonal."""
    dg = [diagram(n, 30 + n) for n in (5, 70, 300, 0, 500, 17, 64, 257, 512)]
    S = len(dg)
    D = pkg.wasserstein_matrix(dg)
    assert D.shape == (S, S) and D.dtype == np.float64 and np.array_equal(D, D.T) and not np.diag(D).any()
    assert (D[~np.eye(S, dtype=bool)] > 0).all()
    assert np.array_equal(D, pkg.wasserstein_matrix(dg))  # two runs of the same call
    iu = np.stack(np.triu_indices(S, 1), 1)
    dist, maps = abi(pkg, dg, None)
    assert np.array_equal(dist, D[iu[:, 0], iu[:, 1]])
    dist2, maps2 = abi(pkg, dg, None)
    assert np.array_equal(dist, dist2) and all(np.array_equal(a, b) for a, b in zip(maps, maps2))
    assert np.array_equal(abi(pkg, dg, None, matching=False)[0], dist)
    # every ordered pair, shuffled, in one explicit list
    rng = np.random.default_rng(3)
    both = np.concatenate([iu, iu[:, ::-1]])[rng.permutation(2 * len(iu))]
    dist3, maps3 = abi(pkg, dg, both)
    where = {(int(i), int(j)): p for p, (i, j) in enumerate(iu)}
    for p, (i, j) in enumerate(both):
        assert dist3[p] == D[i, j]
        fwd = maps[where[min(i, j), max(i, j)]]
        assert np.array_equal(maps3[p], fwd if i < j else inverse(fwd, len(dg[i]))), (i, j)
    # the other-list form, shuffled, and every pair alone in both orientations
    perm = rng.permutation(S)
    X = pkg.wasserstein_matrix([dg[i] for i in perm], other=[dg[i] for i in perm[::-1]])
    assert np.array_equal(X, D[np.ix_(perm, perm[::-1])])
    for i in range(S):
        for j in range(S):
            if i != j:
                d, match, _ = solve(pkg, dg[i], dg[j])
                fwd = maps[where[min(i, j), max(i, j)]]
                assert d == D[i, j] and np.array_equal(match, fwd if i < j else inverse(fwd, len(dg[i]))), (i, j)
    for i, j in ((0, 5), (1, 6), (2, 7), (4, 8)):
        check_against(dg[i], dg[j], D[i, j], maps[where[i, j]].astype(np.int64), ws_ref.value(dg[i], dg[j]))


def test_empty_and_equal_diagrams(pkg):
    """W(A, empty) == W(empty, A), within K u W of the sum of A's diagonal costs; W(A, A) and W(A, A
    reversed) are not promised to be 0.0, only to lie within bound 1 of it."""
    assert pkg.wasserstein(E, E) == 0.0
    d, M = pkg.wasserstein(E, E, matching=True)
    assert d == 0.0 and M.shape == (0, 3)
    for n in (1, 5, 70, 300, 512):
        A = diagram(n, 30 + n)
        total = ((A[:, 1] - A[:, 0]) * ws_ref.SQRT1_2).astype(LD).sum()
        d, match, M = solve(pkg, A, E)
        assert d == pkg.wasserstein(E, A) > 0 and (match == -1).all()
        assert abs(LD(d) - total) <= n * ws_ref.U * d
        assert solve(pkg, E, A)[2][:, 1].tolist() == list(range(n))
        for B in (A, A[::-1].copy()):
            d, match, _ = solve(pkg, A, B)
            print(f"n={n}: W(A, A') = {d!r} (bound {ws_ref.bound(A, B):.3e})")
            assert 0.0 <= d <= ws_ref.bound(A, B)
            check_against(A, B, d, match, LD(0))


def test_non_finite_points_are_dropped(pkg):
    A, B = diagram(40, 7), diagram(25, 8)
    Ainf = np.concatenate([A[:10], [[0.0, np.inf]], A[10:], [[0.5, np.inf]]])
    with pytest.warns(UserWarning, match="non-finite"):
        got, M = pkg.wasserstein(Ainf, B, matching=True)
    d, _, M0 = solve(pkg, A, B)
    assert got == d and np.array_equal(M, M0)  # the indices count the finite rows
    with pytest.warns(UserWarning, match="non-finite"):
        assert pkg.wasserstein(B, Ainf) == d
    with pytest.warns(UserWarning, match="non-finite"):
        assert pkg.wasserstein(np.array([[0.0, np.inf]]), E) == 0.0  # two empty diagrams
    with pytest.warns(UserWarning, match="non-finite"):
        assert np.array_equal(pkg.wasserstein_matrix([Ainf, B, A]), pkg.wasserstein_matrix([A, B, A]))


def test_limit_through_the_abi(pkg):
    """513 finite points in a diagram return TDA_E_UNSUPPORTED with no result, 512 are computed; the
    matching's arrays are NULL unless asked for."""
    L, lb = pkg.lib(), pkg._lib
    A, B, ref = case(512, 512, "spread")
    pts = np.ascontiguousarray(np.concatenate([A, B, [[1.0, 2.0]]]))
    res = ctypes.POINTER(lb.WsResult)()
    a = lb.WsArgs()
    a.points, a.S, a.device = pts.ctypes.data, 2, 0
    off = np.array([0, 512, 1025], np.int64)
    a.offsets = off.ctypes.data
    for flags in (0, 1):
        a.flags = flags
        assert L.tda_wasserstein(ctypes.byref(a), ctypes.byref(res)) == -2 and not res
        assert b"512" in L.tda_last_error()
    off = np.array([0, 512, 1024], np.int64)
    a.offsets = off.ctypes.data
    a.flags = 0
    assert L.tda_wasserstein(ctypes.byref(a), ctypes.byref(res)) == 0 and res
    try:
        r = res.contents
        assert r.P == 1 and r.device_ms > 0 and not r.match and not r.match_off
        d = r.dist[0]
    finally:
        L.tda_ws_free(res)
    a.flags = lb.TDA_WS_WANT_MATCHING
    assert L.tda_wasserstein(ctypes.byref(a), ctypes.byref(res)) == 0 and res
    try:
        r = res.contents
        assert r.P == 1 and r.device_ms > 0 and r.dist[0] == d
        assert [r.match_off[0], r.match_off[1]] == [0, 512]
        check_against(A, B, d, np.array(r.match[:512], np.int64), ref)
    finally:
        L.tda_ws_free(res)
