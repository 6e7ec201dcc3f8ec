"""GPU tests of the heat (persistence scale-space) kernel and its distance
(include/tda_dgm.h tda_heat_kernel, diagrams.py) against the CPU references of tests/hk_ref.py.

What is compared, with u = 2^-53 (tda_dgm.h, promise 3): kern and self lie within
C(n1, n2) u cn of the longdouble reference (which tests/test_heat_cpu.py holds to 1 / 16 of
that bound against mpmath), the squared distance formed from them in the header's order
within B2, and dist is the correctly rounded root of its clamp.  The bitwise promises
(symmetry, identity, a pair alone / among others / anywhere in the list / with and without
`pairs` / run to run) are ``==``.

Sizes: empty, one and two points; 63 / 64 / 65 (the 64 rows of a part, one wave); 255 / 256 /
257 (the 256 columns a part stages in LDS); 512 / 513 (the launch classes <= 64 / <= 512 /
<= 4096); 1024 / 1025 (many parts, the second pass over the parts' lanes); the 4096 limit
once.  No test but the last calls the persistence pipeline."""
import importlib

import numpy as np
import pytest

import hk_ref
from test_wasserstein import diagram

pytestmark = pytest.mark.gpu

E = np.zeros((0, 2))
LD = np.longdouble
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 512, 513, 1024, 1025]
LOPSIDED = [(1, 1025), (65, 257), (0, 64)]
SIGMAS = (0.01, 0.4, 5.0)


def dgm(n: int, k: int = 0) -> np.ndarray:
    return diagram(n, 7000 + 10 * n + k)


def call(pkg, dgms, pairs, sigma, other=None):
    """One library call: (kern, self, dist) of `pairs` ((P, 2), or None for every i < j)."""
    dg = importlib.import_module(pkg.__name__ + ".diagrams")
    pts, off, _, _, _ = dg._hk_inputs(dgms, None, 1)
    pairs = None if pairs is None else np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    kern, self_, dist, ms = dg._call_hk(pts, off, pairs, float(sigma), 0)
    assert ms > 0 and len(self_) == len(dgms) and len(kern) == len(dist) == (len(dgms) * (len(dgms) - 1) // 2 if pairs is None else len(pairs))
    return kern, self_, dist


_ref = {}


def ref_k(a, b, sigma):
    """The longdouble k of dgm(*a) and dgm(*b), computed once."""
    key = (min(a, b), max(a, b), sigma)
    if key not in _ref:
        _ref[key] = hk_ref.ld_k(dgm(*key[0]), dgm(*key[1]), sigma)
    return _ref[key]


def check_pairs(pkg, ids, pairs, sigma):
    """kern, self and the squared distance of `pairs` (indices into ids = [(n, k), ...]) within the
    header's bounds of the reference; dist the root of the clamp.  Returns the largest error over bound."""
    dgms = [dgm(*i) for i in ids]
    kern, self_, dist = call(pkg, dgms, pairs, sigma)
    worst = 0.0
    for s, i in enumerate(ids):
        err, tol = abs(LD(self_[s]) - ref_k(i, i, sigma)), hk_ref.bound_k(i[0], i[0], sigma)
        worst = max(worst, float(err) / tol if tol else float(err))
        assert err <= tol, ("self", i, sigma, float(err), tol)
        assert i[0] or (self_[s] == 0.0 and not np.signbit(self_[s]))
    for p, (x, y) in enumerate(pairs):
        a, b = ids[x], ids[y]
        err, tol = abs(LD(kern[p]) - ref_k(a, b, sigma)), hk_ref.bound_k(a[0], b[0], sigma)
        worst = max(worst, float(err) / tol if tol else float(err))
        assert err <= tol, ("kern", a, b, sigma, float(err), tol)
        if not (a[0] and b[0]):
            assert kern[p] == 0.0 and not np.signbit(kern[p])  # an empty diagram: +0.0 against anything
        q = (self_[x] + self_[y]) - 2.0 * kern[p]  # the header's order, in float64
        assert dist[p] == (np.sqrt(q) if q > 0 else 0.0)
        want = hk_ref.d2(ref_k(a, a, sigma), ref_k(b, b, sigma), ref_k(a, b, sigma))
        err, tol = abs(LD(q) - want), hk_ref.bound_d2(a[0], b[0], sigma, self_[x], self_[y], kern[p])
        worst = max(worst, float(err) / tol if tol else float(err))
        assert err <= tol, ("d2", a, b, sigma, float(err), tol)
    return worst


@pytest.mark.parametrize("sigma", SIGMAS)
def test_values_within_the_bound(pkg, sigma):
    ids = [(n, 0) for n in SIZES] + [(n, 1) for n in SIZES]
    pairs = [(s, len(SIZES) + s) for s in range(len(SIZES))]  # n x n, two different diagrams
    for n1, n2 in LOPSIDED:
        pairs += [(SIZES.index(n1), len(SIZES) + SIZES.index(n2))]
        pairs += [pairs[-1][::-1]]
    worst = check_pairs(pkg, ids, pairs, sigma)
    print(f"sigma={sigma}: {len(pairs)} pairs and {len(ids)} selfs, largest error over bound {worst:.3e}")
    assert worst > 0  # something was compared


def test_the_limit(pkg):
    """4096 x 4096 and 1 x 4096 once, against the longdouble reference (the two large selfs are
    compared with the pairs (s, s) only: a reference of 4096 x 4096 terms takes seconds); 4097
    finite points are refused."""
    F, G, one = dgm(4096), dgm(4096, 1), dgm(1)
    kern, self_, dist = call(pkg, [F, G, one], [(0, 1), (2, 0), (1, 0), (0, 0), (1, 1)], 0.4)
    worst = 0.0
    for p, (X, Y) in enumerate(((F, G), (one, F))):
        err, tol = float(abs(LD(kern[p]) - hk_ref.ld_k(X, Y, 0.4))), hk_ref.bound_k(len(X), len(Y), 0.4)
        worst = max(worst, err / tol)
        assert err <= tol, (len(X), len(Y), err, tol)
    assert kern[2] == kern[0] and dist[2] == dist[0] > 0 and kern[3] == self_[0] and kern[4] == self_[1] and not dist[3:].any()
    assert abs(LD(self_[2]) - hk_ref.ld_k(one, one, 0.4)) <= hk_ref.bound_k(1, 1, 0.4)
    print(f"the 4096 limit: largest error over bound {worst:.3e}")
    big = np.concatenate([dgm(4096), [[1.0, 2.0]]])
    with pytest.raises(NotImplementedError, match="4096"):
        pkg.heat(big, dgm(5))
    with pytest.warns(UserWarning, match="non-finite"):  # 4096 finite rows and one that is not
        assert pkg.heat(np.concatenate([dgm(4096), [[1.0, np.inf]]]), dgm(4096)) == 0.0


def lattice(n: int, seed: int):
    """n points out of distinct points of the 0.25-spaced lattice with persistence >= 0.25, some of
    them repeated, shuffled; and the number of ordered coincident pairs."""
    rng = np.random.default_rng(seed)
    k = max(1, (2 * n) // 3) if n else 0
    i = np.arange(k)
    base = np.stack([0.25 * i, 0.25 * i + 0.25 * (1 + i % 5)], 1)
    which = np.concatenate([i, rng.integers(0, max(k, 1), n - k)]) if n else i
    which = which[rng.permutation(n)]
    mult = np.bincount(which, minlength=k)
    return base[which], int((mult.astype(np.int64) ** 2).sum())


def test_known_answer_counts_coincident_points(pkg):
    """sigma = 1e-6: every term between different points underflows to zero and a point against itself
    gives 1 - 0, so self / cn is the number of ordered coincident pairs: a dropped or doubled row or
    column at any tile edge changes it by at least 1."""
    sigma = 1e-6
    cn = hk_ref.constants(sigma)[1]
    sizes = SIZES + [1000]
    dgms, counts = zip(*(lattice(n, 40 + n) for n in sizes))
    assert counts[sizes.index(65)] > 65 and counts[0] == 0
    _, self_, _ = call(pkg, list(dgms), [(0, 0)], sigma)
    worst = 0.0
    for n, c, v in zip(sizes, counts, self_):
        err, tol = float(abs(LD(v) - LD(cn) * c)), hk_ref.bound_k(n, n, sigma)
        assert err <= tol and (n == 0 or tol < 0.5 * cn), (n, c, v / cn)
        worst = max(worst, err / tol if tol else err)
    print(f"known answer: largest error over bound {worst:.3e}")
    # two diagrams: the coincident pairs across them, in both orientations
    A, B = dgms[sizes.index(257)], dgms[sizes.index(1025)]
    cross = sum(int((np.all(B == p, axis=1)).sum()) for p in A)
    kern, _, _ = call(pkg, [A, B], [(0, 1), (1, 0)], sigma)
    assert cross > 0 and kern[0] == kern[1] and abs(LD(kern[0]) - LD(cn) * cross) <= hk_ref.bound_k(1025, 257, sigma)


CLASS_SIZES = [0, 1, 5, 63, 64, 65, 100, 256, 300, 512, 513, 700, 1025, 2048]  # every launch class, several part shapes


def test_bitwise_symmetry_identity_and_independence_of_the_call(pkg):
    sigma = 0.4
    dgms = [dgm(n, 2) for n in CLASS_SIZES]
    S = len(dgms)
    iu = np.stack(np.triu_indices(S, 1), 1)
    kern, self_, dist = call(pkg, dgms, None, sigma)
    k2, s2, d2 = call(pkg, dgms, None, sigma)  # two runs
    assert np.array_equal(kern, k2) and np.array_equal(self_, s2) and np.array_equal(dist, d2)
    ke, se, de = call(pkg, dgms, iu, sigma)  # pairs == NULL against the explicit list
    assert np.array_equal(kern, ke) and np.array_equal(self_, se) and np.array_equal(dist, de)
    kt, st, dt = call(pkg, dgms, iu[:, ::-1], sigma)  # (j, i) against (i, j)
    assert np.array_equal(kern, kt) and np.array_equal(dist, dt) and np.array_equal(self_, st)
    perm = np.random.default_rng(3).permutation(len(iu))  # any position in the list; first against last
    kp, _, dp = call(pkg, dgms, iu[perm], sigma)
    assert np.array_equal(kp, kern[perm]) and np.array_equal(dp, dist[perm])
    kr, _, dr = call(pkg, dgms, iu[::-1], sigma)
    assert kr[-1] == kern[0] and kr[0] == kern[-1] and np.array_equal(dr, dist[::-1])
    # identity: kern(s, s) is self[s] and heat(F, F) is exactly 0.0
    ks, ss, ds = call(pkg, dgms, [(s, s) for s in range(S)], sigma)
    assert np.array_equal(ks, self_) and np.array_equal(ss, self_) and not ds.any() and not np.signbit(ds).any()
    assert (self_[1:] > 0).all() and self_[0] == 0.0
    # a pair alone, in either orientation, against the same pair among the others
    for x, y in ((5, 3), (12, 13), (9, 10), (13, 1), (8, 8), (0, 4), (13, 13)):
        ka, sa, da = call(pkg, [dgms[x], dgms[y]], [(0, 1), (1, 0)], sigma)
        p = int(np.flatnonzero((iu == sorted((x, y))).all(axis=1))[0]) if x != y else None
        want_k, want_d = (kern[p], dist[p]) if x != y else (self_[x], 0.0)
        assert ka[0] == ka[1] == want_k and da[0] == da[1] == want_d and sa[0] == self_[x] and sa[1] == self_[y], (x, y)
    # the Python matrices: the Gram diagonal is self, other= is the block of the full matrix
    K, D = pkg.heat_kernel_matrix(dgms, sigma), pkg.heat_matrix(dgms, sigma)
    assert np.array_equal(np.diag(K), self_) and np.array_equal(K[iu[:, 0], iu[:, 1]], kern) and np.array_equal(K, K.T)
    assert np.array_equal(D[iu[:, 0], iu[:, 1]], dist) and np.array_equal(D, D.T) and not np.diag(D).any()
    assert np.array_equal(pkg.heat_kernel_matrix(dgms[:5], sigma, other=dgms[3:]), K[:5, 3:])
    assert np.array_equal(pkg.heat_matrix(dgms[9:], sigma, other=dgms[:9]), D[9:, :9])
    assert pkg.heat(dgms[5], dgms[12], sigma) == D[5, 12] == pkg.heat(dgms[12], dgms[5], sigma)
    assert pkg.heat(dgms[5], dgms[5], sigma) == 0.0 and pkg.heat(E, E) == 0.0


@pytest.mark.parametrize("sigma", SIGMAS)
def test_row_order_moves_a_value_within_the_bound(pkg, sigma):
    rng = np.random.default_rng(11)
    for n, m in ((65, 65), (300, 257), (1025, 64)):
        F, G = dgm(n, 3), dgm(m, 4)
        Fs = F[rng.permutation(n)]
        assert not np.array_equal(F, Fs)
        kern, self_, dist = call(pkg, [F, Fs, G], [(0, 2), (1, 2), (0, 1)], sigma)
        # bound 3 itself (tda_dgm.h, promise 4), not twice it: both values sum the same terms
        assert abs(kern[0] - kern[1]) <= hk_ref.bound_k(n, m, sigma)
        assert abs(self_[0] - self_[1]) <= hk_ref.bound_k(n, n, sigma) and abs(kern[2] - self_[0]) <= hk_ref.bound_k(n, n, sigma)
        B2 = hk_ref.bound_d2(n, n, sigma, self_[0], self_[1], kern[2])
        assert dist[2] <= np.sqrt(B2) * (1 + 2.0 ** -50), (n, sigma, dist[2], np.sqrt(B2))


def test_gram_matrix_is_positive_semidefinite_within_the_bound(pkg):
    """Positive semi-definiteness is the point: no eigenvalue of the Gram matrix of 8 diagrams lies
    below -(the sum of the eight diagonal bounds)."""
    for sigma in SIGMAS:
        ns = [5, 40, 64, 65, 130, 257, 300, 513]
        dgms = [dgm(n, 5) for n in ns]
        K = pkg.heat_kernel_matrix(dgms + [dgms[2].copy()], sigma)[:8, :8]  # the ninth: an equal diagram elsewhere in the call
        floor = -sum(hk_ref.bound_k(n, n, sigma) for n in ns)
        lo = float(np.linalg.eigvalsh(K).min())
        print(f"sigma={sigma}: smallest eigenvalue {lo:.3e}, allowed {floor:.3e}, trace {np.trace(K):.3e}")
        assert lo >= floor and np.array_equal(K, K.T) and (np.diag(K) > 0).all()


def test_python_entries_and_a_real_sweep(pkg, ref_clouds):
    A, B = dgm(70, 6), dgm(33, 6)
    withinf = np.concatenate([A[:7], [[0.0, np.inf]], A[7:]])
    D = pkg.heat_matrix([A, B])
    assert pkg.heat(A, B) == D[0, 1] == D[1, 0] > 0 and pkg.heat(A, B, sigma=0.4, device=0) == D[0, 1]
    assert pkg.heat(A, B, 5.0) == pkg.heat_matrix([A], 5.0, other=[B])[0, 0] != D[0, 1]
    with pytest.warns(UserWarning, match="non-finite"):
        assert pkg.heat(withinf, B) == D[0, 1]
    D1, ms = pkg.heat_matrix([A, B, E], return_time=True)
    assert ms > 0 and D1[0, 1] == D[0, 1] and D1[2, 2] == 0.0 and D1[0, 2] == np.sqrt(pkg.heat_kernel_matrix([A])[0, 0])
    results = pkg.ripser_batch(ref_clouds[:4], maxdim=1)
    h1 = [r.dgms[1] for r in results]
    L = pkg.layer_distance_matrix(results, metric="heat")
    assert L.shape == (4, 4) and np.array_equal(L, L.T) and not np.diag(L).any()
    assert np.array_equal(L, pkg.heat_matrix(h1)) and np.array_equal(L, pkg.heat_matrix(results[::-1], dim=1)[::-1, ::-1])
    assert np.array_equal(pkg.layer_distance_matrix(results, metric="heat", sigma=0.05), pkg.heat_matrix(h1, 0.05))
    for i in range(4):
        for j in range(i + 1, 4):
            n1, n2 = len(h1[i]), len(h1[j])
            k = [hk_ref.ld_k(h1[a], h1[b], 0.4) for a, b in ((i, i), (j, j), (i, j))]
            K = pkg.heat_kernel_matrix([h1[i], h1[j]])
            B2 = hk_ref.bound_d2(n1, n2, 0.4, K[0, 0], K[1, 1], K[0, 1])
            assert abs(LD((K[0, 0] + K[1, 1]) - 2.0 * K[0, 1]) - hk_ref.d2(*k)) <= B2
