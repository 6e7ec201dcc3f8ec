"""GPU tests of the persistence Fisher distance (include/tda_dgm.h tda_persistence_fisher,
diagrams.py) against the CPU restatement of tests/pf_ref.py.  Arrays only: nothing here calls
the persistence pipeline.

What is compared, with u = 2^-53 (tda_dgm.h, promise 3): the affinity formed from a pair's a, b
and h in the header's order lies within B(n1, n2) of the restatement's (which
tests/test_fisher_cpu.py holds to the same bound against mpmath, and which differs from the
device by the exponential alone), and dist within the bound that follows through arccos.  The
bitwise promises (symmetry, identity, a pair alone / among others / anywhere in the list / with
and without `pairs` / with other= / run to run) are ``==``.

Sizes: empty and one point; 63 / 64 / 65 (the 64 evaluation points of a part, one wave);
127 / 128 / 129 (the 128 sources staged at a time), each diagram with one non-finite row, all
pairs of them (n1 + n2 from 1 to 258: the launch classes <= 64 and <= 512, 1 to 9 parts); the
1024 x 1024 limit once (the class <= 2048, 64 parts: every lane of the second kernel).

The largest share of the bound seen, recorded in DESIGN 6.31: printed by
test_values_within_the_bound and test_the_limit."""
import importlib

import numpy as np
import pytest

import pf_ref
from test_wasserstein import diagram

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:the diagrams hold")]  # every diagram here has a non-finite row

E = np.zeros((0, 2))
SIZES = [0, 1, 63, 64, 65, pf_ref.CHUNK - 1, pf_ref.CHUNK, pf_ref.CHUNK + 1]
SIGMAS = (0.05, 1.0, 5.0)
JUNK = ([[0.5, np.inf]], [[np.nan, 1.0]], [[-np.inf, 2.0]])


def dgm(n: int, k: int = 0) -> np.ndarray:
    """n seeded finite points and one non-finite row in the middle."""
    D = diagram(n, 9000 + 10 * n + k)
    return np.concatenate([D[:n // 2], JUNK[(n + k) % 3], D[n // 2:]])


def call(pkg, dgms, pairs, sigma, other=None):
    """One library call: (a, b, h, dist) of `pairs` ((P, 2), or None for every i < j; with `other` the block)."""
    dg = importlib.import_module(pkg.__name__ + ".diagrams")
    pts, off, blk, S, S2 = dg._inputs(dgms, other, 1, 1 << 30)
    pairs = blk if pairs is None else np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    a, b, h, dist, ms = dg._call_pf(pts, off, pairs, float(sigma), 0)
    P = len(a)
    assert ms > 0 and len(b) == len(h) == len(dist) == P == (S * (S - 1) // 2 if pairs is None else len(pairs))
    return a, b, h, dist


_ref = {}


def ref(x, y, sigma):
    """(a, b, h) of the restatement on dgm(*x), dgm(*y), computed once."""
    key = (x, y, sigma)
    if key not in _ref:
        _ref[key] = pf_ref.sums(dgm(*x), dgm(*y), sigma)
        _ref[(y, x, sigma)] = (_ref[key][1], _ref[key][0], _ref[key][2])  # test_fisher_cpu.py: bit for bit
    return _ref[key]


def check_pair(got, x, y, sigma):
    """One pair's (a, b, h, dist) against the restatement; returns the error's share of the bound."""
    a, b, h, dist = (float(v) for v in got)
    B = pf_ref.bound(x[0], y[0])
    A, Aref = pf_ref.affinity_of(a, b, h), pf_ref.affinity_of(*ref(x, y, sigma))
    err = abs(A - Aref)
    assert err <= B, (x, y, sigma, err, B)
    dref = float(np.arccos(Aref)) if x[0] + y[0] else 0.0
    assert abs(dist - dref) <= pf_ref.bound_dist(A, B), (x, y, sigma, dist, dref)
    assert abs(dist - (float(np.arccos(A)) if x[0] + y[0] else 0.0)) <= 4 * pf_ref.U_  # dist is the host's arccos of this affinity
    assert 0.0 <= dist <= np.arccos(0.0) and not np.signbit(dist)
    assert a >= x[0] + y[0] and b >= x[0] + y[0] and 0.0 <= h  # every z of U holds e(z, z) = 1 in rhoU
    return err / B


@pytest.mark.parametrize("sigma", SIGMAS)
def test_values_within_the_bound(pkg, sigma):
    ids = [(n, 0) for n in SIZES]
    got = call(pkg, [dgm(*i) for i in ids], None, sigma)
    iu = np.triu_indices(len(ids), 1)
    worst = max(check_pair([v[p] for v in got], ids[i], ids[j], sigma) for p, (i, j) in enumerate(zip(*iu)))
    print(f"sigma={sigma}: all pairs of {SIZES}: largest share of the bound B: {worst:.3e}")


@pytest.mark.parametrize("sigma", SIGMAS)
def test_the_limit(pkg, sigma):
    x, y = (1024, 1), (1024, 2)
    got = call(pkg, [dgm(*x), dgm(*y)], None, sigma)
    share = check_pair([v[0] for v in got], x, y, sigma)
    print(f"sigma={sigma}: 1024 x 1024: share of the bound B: {share:.3e}")


def test_the_point_limit_counts_only_where_a_pair_names_the_diagram(pkg):
    big, A, B = dgm(1025), dgm(5), dgm(7)  # 1025 finite rows
    for pairs in ([(0, 1)], [(1, 0)], [(0, 0)], [(1, 2), (2, 0)]):
        with pytest.raises(NotImplementedError, match="1024"):
            call(pkg, [big, A, B], pairs, 1.0)  # the library's refusal
    with pytest.raises(NotImplementedError, match="1024"):
        pkg.fisher_matrix([big, A, B])  # and the Python entry's
    alone = call(pkg, [A, B], [(0, 1)], 1.0)
    beside = call(pkg, [big, A, B], [(1, 2)], 1.0)
    assert all(u[0] == v[0] for u, v in zip(alone, beside))


def test_known_answers_bit_for_bit(pkg):
    # two single points with every cross argument below -708: h == 0.0 and the distance is arccos(0)
    p, q = np.array([[0.0, 10.0]]), np.array([[100.0, 130.0]])
    assert pkg.fisher(p, q, 0.05) == np.arccos(0.0) == pkg.fisher(q, p, 0.05)
    dg = importlib.import_module(pkg.__name__ + ".diagrams")
    a, b, h, dist, _ = dg._call_pf(np.concatenate([p, q]), np.array([0, 1, 2]), None, 0.05, 0)
    assert (a[0], b[0], h[0], dist[0]) == (2.0, 2.0, 0.0, np.arccos(0.0))
    # F = {p}, G empty: affinity 2 sqrt(g) / (1 + g); here a == b by the symmetry of the two points
    a, b, h, dist, _ = dg._call_pf(np.array([[1.0, 3.0]]), np.array([0, 1, 1]), None, 1.0, 0)
    g = np.exp(-1.0)
    assert a[0] == b[0] and abs(a[0] - (1 + g)) <= 8 * pf_ref.U_ and abs(pf_ref.affinity_of(a[0], b[0], h[0]) - 2 * np.sqrt(g) / (1 + g)) <= pf_ref.bound(1, 0)
    # (F, F): exactly +0.0, named by one index or as two equal diagrams, repeated points included
    rep = np.tile([[0.25, 1.5]], (5, 1))
    same = [dgm(1), dgm(64), dgm(65), dgm(129), diagram(300, 3), rep, np.concatenate([rep, dgm(70), rep])]
    for sigma in SIGMAS:
        n = len(same)
        D = pkg.fisher_matrix(same + [d.copy() for d in same], sigma)
        a, b, h, dist = call(pkg, same + [dgm(3)], [(i, i) for i in range(n)], sigma)
        for i in range(n):
            assert D[i, n + i] == 0.0 and not np.signbit(D[i, n + i]) and D[n + i, i] == 0.0
            assert dist[i] == 0.0 and not np.signbit(dist[i]) and a[i] == b[i] == h[i] and a[i] >= 2 * np.isfinite(same[i]).all(axis=1).sum()
    assert pkg.fisher(E, E) == 0.0 and not np.signbit(pkg.fisher(E, E))
    assert pkg.fisher(np.array([[0.0, np.inf]]), E, 0.3) == 0.0  # nothing finite: two empty diagrams


def test_symmetry_bit_for_bit(pkg):
    ids = [(n, 1) for n in SIZES] + [(64, 2), (129, 2)]  # equal counts too: the lexicographic orientation
    dgms = [dgm(*i) for i in ids]
    S = len(ids)
    fwd = [(i, j) for i in range(S) for j in range(S) if i < j]
    for sigma in SIGMAS:
        a, b, h, dist = call(pkg, dgms, fwd, sigma)
        a2, b2, h2, dist2 = call(pkg, dgms, [(j, i) for i, j in fwd], sigma)
        assert np.array_equal(a, b2) and np.array_equal(b, a2) and np.array_equal(h, h2) and np.array_equal(dist, dist2)
        D = pkg.fisher_matrix(dgms, sigma)
        assert np.array_equal(D, D.T) and np.array_equal(D[np.triu_indices(S, 1)], dist) and not D.diagonal().any()


def test_independence_of_the_call_bit_for_bit(pkg):
    sigma = 1.0
    X, Y = dgm(65, 3), dgm(129, 3)
    alone = [v[0] for v in call(pkg, [X, Y], None, sigma)]
    others = [dgm(n, 4) for n in (0, 1, 300, 64, 1000, 128)]
    mixed = others[:3] + [X] + others[3:] + [Y]
    ix, iy = 3, len(mixed) - 1
    allp = call(pkg, mixed, None, sigma)  # every i < j, no explicit pairs
    iu = np.triu_indices(len(mixed), 1)
    at = int(np.flatnonzero((iu[0] == ix) & (iu[1] == iy))[0])
    assert [v[at] for v in allp] == alone
    pairs = [(i, j) for i, j in zip(*iu)]
    rev = call(pkg, mixed, pairs[::-1], sigma)  # the reversed pair list: every pair at another position
    assert all(np.array_equal(u, v[::-1]) for u, v in zip(allp, rev))
    few = call(pkg, mixed, [(6, 4), (ix, iy), (0, 1), (iy, ix), (ix, iy)], sigma)
    assert [v[1] for v in few] == alone == [v[4] for v in few] and [few[1][3], few[0][3], few[2][3], few[3][3]] == alone
    blk = call(pkg, [others[2], X], None, sigma, other=[others[4], Y, others[1]])  # other=: the (2, 3) block
    assert [v[1 * 3 + 1] for v in blk] == alone
    again = call(pkg, mixed, None, sigma)
    assert all(np.array_equal(u, v) for u, v in zip(allp, again))  # run to run
    assert pkg.fisher(X, Y, sigma) == alone[3] == pkg.fisher_matrix([Y, others[0]], sigma, other=[X])[0, 0]


def test_two_row_orders_agree_within_the_bound(pkg):
    rng = np.random.default_rng(11)
    for n1, n2 in ((65, 129), (128, 128), (300, 7)):
        F, G = dgm(n1, 5), dgm(n2, 6)
        for sigma in SIGMAS:
            a, b, h, _ = call(pkg, [F, G, F[rng.permutation(len(F))], G[rng.permutation(len(G))]], [(0, 1), (2, 1), (0, 3), (2, 3)], sigma)
            A = [pf_ref.affinity_of(a[p], b[p], h[p]) for p in range(4)]
            assert max(A) - min(A) <= pf_ref.bound(n1, n2), (n1, n2, sigma, A)


def test_the_kernel_matrix_is_the_exponential_of_the_distances(pkg):
    dgms = [dgm(n, 7) for n in (0, 1, 64, 65, 129, 300)]
    D = pkg.fisher_matrix(dgms, 0.5)
    for bw in (1.0, 0.25):
        K = pkg.fisher_kernel_matrix(dgms, 0.5, bw)
        assert np.array_equal(K, np.exp(-D / bw)) and np.array_equal(K.diagonal(), np.ones(len(dgms))) and np.array_equal(K, K.T)
    Kb, ms = pkg.fisher_kernel_matrix(dgms[:2], 0.5, 2.0, other=dgms[2:], return_time=True)
    assert ms > 0 and np.array_equal(Kb, np.exp(-D[:2, 2:] / 2.0)) and (K > 0).all() and (K <= 1).all()
