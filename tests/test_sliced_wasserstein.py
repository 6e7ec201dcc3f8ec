"""GPU tests of the sliced Wasserstein distance between persistence diagrams
(include/tda_dgm.h, diagrams.py) against the float64 restatement tests/sw_ref.py.

Tolerance (sw_ref.bound): |gpu - ref| <= 64 * eps * n * xmax with eps = 2^-52,
n = n1 + n2 and xmax the largest absolute finite coordinate -- each projected
value is two products and a sum of numbers bounded by xmax (the kernel uses
fma, numpy does not), each |a - b| term doubles that, n terms are added, the
average over directions does not grow it.  Absolute, because the L1 sum can
cancel far below n * xmax.

Sizes: empty and one-point diagrams, sums of exactly 64 and of 65, one below
a power of two, the 4096 limit, and both sides of the kernel's launch classes
(next_pow2(n) <= 128 / <= 1024 / <= 4096: another workgroup size and another
count of directions per workgroup)."""
import ctypes

import numpy as np
import pytest

import sw_ref

pytestmark = pytest.mark.gpu

SIZES = [(0, 0), (0, 1), (1, 0), (1, 1), (3, 5), (32, 32), (33, 31), (40, 25), (64, 64), (65, 64), (100, 157), (500, 524),
         (512, 513), (1000, 1047), (2048, 2048)]
MS = (1, 7, 50)  # 7 and 50 are no multiple of the 8 directions a small pair's workgroup takes


def diagram(n: int, seed: int) -> np.ndarray:
    """n seeded (b, d) with d > b, values up to about 10; every third point is
    rounded to f32 and every fifth repeats the point before it."""
    rng = np.random.default_rng(seed)
    b = rng.uniform(0.0, 5.0, n)
    D = np.stack([b, b + rng.uniform(1e-3, 5.0, n)], 1)
    D[::3] = D[::3].astype(np.float32)
    D[4::5] = D[3::5][:len(D[4::5])]
    assert np.all(D[:, 1] > D[:, 0])
    return D


_cases = {}


def case(n1, n2):
    """The two diagrams of a size and their reference values, computed once."""
    if (n1, n2) not in _cases:
        A, B = diagram(n1, 1000 + n1), diagram(n2, 2000 + n2)
        _cases[n1, n2] = A, B, {M: sw_ref.sliced_wasserstein(A, B, M) for M in MS}
    return _cases[n1, n2]


def close(got, A, B, M, ref=None):
    ref = sw_ref.sliced_wasserstein(A, B, M) if ref is None else ref
    bd = sw_ref.bound(A, B)
    err = abs(got - ref)
    print(f"n1={len(A)} n2={len(B)} M={M} gpu={got!r} ref={ref!r} err={err:.3e} bound={bd:.3e} ratio={err / bd if bd else err:.4f}")
    return err <= bd and np.isfinite(got)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("n1,n2", SIZES)
def test_matches_restatement(pkg, n1, n2, M):
    A, B, ref = case(n1, n2)
    assert close(pkg.sliced_wasserstein(A, B, M=M), A, B, M, ref[M])


def test_exact_invariants(pkg):
    """Bitwise: SW(A, A) = 0, symmetry, a pair's value alone / among all pairs
    of 9 diagrams / in a shuffled explicit list, and run to run.  The 9
    diagrams put pairs into all three launch classes of one call."""
    dg = [diagram(n, 30 + n) for n in (5, 70, 600, 0, 1500, 17, 64, 300, 2000)]
    for A in (dg[0], dg[1], dg[2], dg[8]):
        assert pkg.sliced_wasserstein(A, A) == 0.0
        assert pkg.sliced_wasserstein(A, A[::-1].copy(), M=7) == 0.0  # the same multiset in another order
    for i, j in ((0, 1), (1, 2), (2, 8), (3, 5)):
        assert pkg.sliced_wasserstein(dg[i], dg[j]) == pkg.sliced_wasserstein(dg[j], dg[i]) > 0.0
    D = pkg.sliced_wasserstein_matrix(dg, M=7)
    assert D.shape == (9, 9) and np.array_equal(D, D.T) and not np.diag(D).any()
    assert np.array_equal(D, pkg.sliced_wasserstein_matrix(dg, M=7))  # two runs of the same call
    alone = np.array([[pkg.sliced_wasserstein(a, b, M=7) if i != j else 0.0 for j, b in enumerate(dg)] for i, a in enumerate(dg)])
    assert np.array_equal(D, alone)
    # an explicit pairs list in shuffled order, both orientations, through the other-list form
    perm = np.random.default_rng(3).permutation(9)
    X = pkg.sliced_wasserstein_matrix([dg[i] for i in perm], M=7, other=[dg[i] for i in perm[::-1]])
    assert np.array_equal(X, D[np.ix_(perm, perm[::-1])])
    for i, j in ((0, 3), (1, 6), (2, 7), (4, 8), (2, 4)):
        assert close(D[i, j], dg[i], dg[j], 7)


def test_non_finite_points_are_dropped(pkg):
    A, B = diagram(40, 7), diagram(25, 8)
    Ainf = np.concatenate([A[:10], [[0.0, np.inf]], A[10:], [[0.5, np.inf]]])
    with pytest.warns(UserWarning, match="non-finite"):
        got = pkg.sliced_wasserstein(Ainf, B)
    assert got == pkg.sliced_wasserstein(A, B)
    with pytest.warns(UserWarning, match="non-finite"):
        assert pkg.sliced_wasserstein(np.array([[0.0, np.inf]]), np.zeros((0, 2))) == 0.0  # two empty diagrams


def test_all_pairs_order_with_an_empty_diagram(pkg):
    dg = [diagram(6, 1), diagram(11, 2), np.zeros((0, 2)), diagram(4, 3), diagram(9, 4)]
    D = pkg.sliced_wasserstein_matrix(dg)
    assert D.shape == (5, 5) and D.dtype == np.float64 and np.array_equal(D, D.T) and not np.diag(D).any()
    for i in range(5):
        for j in range(i + 1, 5):
            assert close(D[i, j], dg[i], dg[j], 50)
    assert np.array_equal(pkg.sliced_wasserstein_matrix(dg[:2], other=dg[2:]), D[:2, 2:])


def test_sweep_layers_end_to_end(pkg, ref_clouds):
    """ripser_batch on 4 layers of the reference's 48-point clouds, then the
    layer-against-layer matrix of the H1 diagrams from the batch's shared arrays."""
    results = pkg.ripser_batch(ref_clouds[:4], maxdim=1)
    D = pkg.layer_distance_matrix(results, dim=1)
    h1 = [r.dgms[1] for r in results]
    assert D.shape == (4, 4) and np.array_equal(D, pkg.sliced_wasserstein_matrix(h1))
    assert np.array_equal(D, pkg.sliced_wasserstein_matrix(results[::-1], dim=1)[::-1, ::-1])
    for i in range(4):
        for j in range(i + 1, 4):
            assert close(D[i, j], h1[i], h1[j], 50)
    # H0 holds one essential class per layer: dropped, with a warning
    with pytest.warns(UserWarning, match="non-finite"):
        D0 = pkg.layer_distance_matrix(results, dim=0, M=7)
    assert close(D0[0, 1], results[0].dgms[0], results[1].dgms[0], 7)


def test_unsupported_size_through_the_abi(pkg):
    """n1 + n2 = 4097 returns TDA_E_UNSUPPORTED (before any device work: the
    same call is refused on a machine without a device), 4096 is computed."""
    L, lb = pkg.lib(), pkg._lib
    A, B = case(2048, 2048)[:2]
    pts = np.ascontiguousarray(np.concatenate([A, B, [[1.0, 2.0]]]))
    res = ctypes.POINTER(lb.SwResult)()
    a = lb.SwArgs()
    a.points, a.S, a.M, a.device = pts.ctypes.data, 2, 7, 0
    off = np.array([0, 2048, 4097], np.int64)
    a.offsets = off.ctypes.data
    assert L.tda_sliced_wasserstein(ctypes.byref(a), ctypes.byref(res)) == -2 and not res
    assert b"4096" in L.tda_last_error()
    off = np.array([0, 2048, 4096], np.int64)
    a.offsets = off.ctypes.data
    assert L.tda_sliced_wasserstein(ctypes.byref(a), ctypes.byref(res)) == 0 and res
    try:
        assert res.contents.P == 1 and res.contents.device_ms > 0
        assert res.contents.dist[0] == pkg.sliced_wasserstein(A, B, M=7)
    finally:
        L.tda_sw_free(res)
