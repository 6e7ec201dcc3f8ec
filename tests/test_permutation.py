"""GPU tests of the permutation test between groups of diagrams (tda_permutation_test), on arrays
only: every value equals the numpy restatement perm_ref bit for bit on both kernels, labellings of
one partition tie exactly, a row's value does not depend on the call that holds it, a decidable case
is decided, the diagram entry is the matrix entry followed by the test, and two orders of the same
diagrams stay within the documented bound."""
import numpy as np
import pytest

import perm_ref as pr

pytestmark = pytest.mark.gpu

LDS_S = 128  # kPermLdsS (asserted against the sources in test_permutation_cpu.py and below)


def _bits(x):
    return np.float64(x).tobytes()


def _w_points(S, seed):
    """Euclidean distances of random points: symmetric bit for bit ((a - b)^2 == (b - a)^2), +0.0 diagonal."""
    P = np.random.default_rng(seed).standard_normal((S, 3))
    d2 = np.zeros((S, S))
    for k in range(3):
        d2 = d2 + (P[:, None, k] - P[None, :, k]) ** 2
    return np.sqrt(d2)


def _w_int(S, seed):
    """Integer-valued distances: every sum in the statistic but the weights' products is exact."""
    A = np.triu(np.random.default_rng(seed).integers(1, 50, size=(S, S)), 1).astype(np.float64)
    return A + A.T


def _obs(sizes, seed):
    return np.random.default_rng(seed).permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.uint8)


def _table(obs, B, seed):
    return np.random.default_rng(seed).permuted(np.tile(obs, (B, 1)), axis=1)


def _run(pkg, W, obs, lab):
    return pkg.permutation_test(W, obs, permutations=lab, return_null=True)


def _check_exact(r, W, obs, lab, G):
    t, null, count, pvalue = pr.permutation_test(W, obs, lab, G)
    assert _bits(r.statistic) == _bits(t)
    assert r.null.dtype == np.float64 and r.null.tobytes() == null.tobytes()
    assert r.count == count and _bits(r.pvalue) == _bits(pvalue) and r.B == len(lab)


# S, group sizes, B, kind of W: both kernels (S <= 128: resident), S around the wave (64) and the
# slab (256) sizes, equal and unequal groups, a group of exactly 2, G = 2 and 3
CASES = [
    (4, (2, 2), 17, "pts"),
    (5, (2, 3), 1000, "int"),
    (63, (21, 21, 21), 17, "pts"),
    (63, (2, 61), 1, "int"),
    (64, (32, 32), 1000, "pts"),
    (64, (2, 40, 22), 17, "int"),
    (65, (30, 35), 17, "int"),
    (65, (21, 22, 22), 1000, "pts"),
    (127, (2, 125), 1000, "pts"),
    (127, (42, 42, 43), 1, "int"),
    (LDS_S, (64, 64), 1000, "int"),
    (LDS_S, (50, 2, 76), 17, "pts"),
    (LDS_S + 1, (64, 65), 17, "pts"),
    (LDS_S + 1, (43, 43, 43), 1000, "int"),
    (200, (100, 100), 1000, "pts"),
    (200, (2, 120, 78), 17, "int"),
    (2048, (1024, 1024), 8, "int"),
    (2048, (2, 1000, 1046), 8, "pts"),
]


def test_lds_threshold_is_the_sources(pkg):
    assert pkg._lib.TDA_PERM_LDS_S == LDS_S


@pytest.mark.parametrize("S,sizes,B,kind", CASES, ids=[f"S{c[0]}-G{len(c[1])}-B{c[2]}-{c[3]}" for c in CASES])
def test_equals_the_restatement_bit_for_bit(pkg, S, sizes, B, kind):
    assert sum(sizes) == S
    W = (_w_points if kind == "pts" else _w_int)(S, seed=S)
    obs = _obs(sizes, seed=S + 1)
    lab = _table(obs, B, seed=S + 2)
    r = _run(pkg, W, obs, lab)
    _check_exact(r, W, obs, lab, len(sizes))


@pytest.mark.parametrize("S,sizes", [(60, (20, 20, 20)), (LDS_S, (64, 64)), (150, (50, 50, 50)), (150, (40, 70, 40))],
                         ids=["resident-3", "resident-2", "tiled-3", "tiled-2of3"])
def test_labellings_of_one_partition_tie_exactly(pkg, S, sizes):
    """Rows 0 .. k are the observed split under every renaming of the codes that keeps the sizes
    (swapping groups of equal size): each equals T_obs in bits and counts as <= T_obs."""
    import itertools

    W = _w_points(S, seed=7)
    obs = _obs(sizes, seed=8)
    G = len(sizes)
    renamings = [np.array(p, np.uint8) for p in itertools.permutations(range(G)) if all(sizes[p[g]] == sizes[g] for g in range(G))]
    assert len(renamings) == (6 if len(set(sizes)) == 1 and G == 3 else 2)
    same = np.stack([p[obs] for p in renamings])
    lab = np.vstack([same, _table(obs, 40, seed=9)])
    assert pr.same_partition(lab[:len(same)], obs).all()
    r = _run(pkg, W, obs, lab)
    for b in range(len(same)):
        assert _bits(r.null[b]) == _bits(r.statistic), b
    n_same = int(pr.same_partition(lab, obs).sum())
    assert r.count >= n_same >= len(same)
    assert all(_bits(r.null[b]) == _bits(r.statistic) for b in np.flatnonzero(pr.same_partition(lab, obs)))
    _check_exact(r, W, obs, lab, G)


@pytest.mark.parametrize("S,sizes", [(100, (30, 70)), (LDS_S + 72, (60, 70, 70))], ids=["resident", "tiled"])
def test_a_row_does_not_depend_on_the_call(pkg, monkeypatch, S, sizes):
    """The first 17 rows of a B = 1000 call against a B = 17 call of those rows, whole and with the
    launches' row chunk (TDA_PERM_CHUNK, the host file's kPermChunkRows) cut to 5 and to 8 rows, so
    that chunk boundaries fall inside the table and before the observed row."""
    W = _w_points(S, seed=3)
    obs = _obs(sizes, seed=4)
    lab = _table(obs, 1000, seed=5)
    big = _run(pkg, W, obs, lab)
    small = _run(pkg, W, obs, lab[:17].copy())
    assert small.null.tobytes() == big.null[:17].tobytes() and _bits(small.statistic) == _bits(big.statistic)
    for chunk in ("5", "8", "17", "18"):
        monkeypatch.setenv("TDA_PERM_CHUNK", chunk)
        c = _run(pkg, W, obs, lab[:17].copy())
        assert c.null.tobytes() == small.null.tobytes() and _bits(c.statistic) == _bits(small.statistic), chunk
    monkeypatch.setenv("TDA_PERM_CHUNK", "300")
    c = _run(pkg, W, obs, lab)
    assert c.null.tobytes() == big.null.tobytes() and (c.count, c.pvalue) == (big.count, big.pvalue)
    monkeypatch.delenv("TDA_PERM_CHUNK")
    rev = _run(pkg, W, obs, lab[16::-1].copy())  # the row's position
    assert rev.null[::-1].tobytes() == small.null.tobytes()


@pytest.mark.parametrize("S,sizes", [(5, (2, 3)), (64, (32, 32)), (100, (2, 58, 40)), (LDS_S, (64, 64))])
def test_both_kernels_give_the_same_bits(pkg, monkeypatch, S, sizes):
    """Which kernel ran does not enter the bits: the tiled kernel forced (TDA_PERM_TILED=1) at sizes
    the resident kernel serves."""
    W = _w_points(S, seed=11)
    obs = _obs(sizes, seed=12)
    lab = _table(obs, 50, seed=13)
    a = _run(pkg, W, obs, lab)
    monkeypatch.setenv("TDA_PERM_TILED", "1")
    b = _run(pkg, W, obs, lab)
    assert a.null.tobytes() == b.null.tobytes() and _bits(a.statistic) == _bits(b.statistic)
    assert (a.count, a.pvalue) == (b.count, b.pvalue)
    _check_exact(b, W, obs, lab, len(sizes))


@pytest.mark.parametrize("n1,n2", [(5, 7), (60, 90)], ids=["resident", "tiled"])
def test_a_decidable_outcome(pkg, n1, n2):
    """Two clusters: within-distances at most delta = 2, between-distances at least Delta = 1000 - 2,
    unequal groups.  T_obs <= delta (each group's weighted sum is half its mean distance).  A row of
    another partition has a group g that mixes the clusters, with at least 2 (n_g - 1) ordered
    between-pairs, so T >= Delta / n_g >= Delta / S > delta: it is never <= T_obs, whatever the
    rounding (the margin is a factor of 3 at least, the rounding 1e-13).  With unequal groups only
    the observed labelling itself describes the observed partition.  So count is the number of such
    rows, counted from the table."""
    S = n1 + n2
    rng = np.random.default_rng(n1)
    x = np.concatenate([rng.random(n1), 1000.0 + rng.random(n2)])
    W = np.abs(x[:, None] - x[None, :])
    obs = np.repeat([0, 1], [n1, n2]).astype(np.uint8)
    lab = _table(obs, 400, seed=1)
    lab = lab[~pr.same_partition(lab, obs)]  # no row of the observed partition
    assert len(lab) > 300
    r = _run(pkg, W, obs, lab)
    assert r.count == 0 and r.pvalue == 1.0 / (len(lab) + 1)
    assert r.statistic <= 2.0 and r.null.min() >= 998.0 / S > 2.0
    with_obs = lab.copy()
    with_obs[[0, 17, 99]] = obs
    r = _run(pkg, W, obs, with_obs)
    assert r.count == int(pr.same_partition(with_obs, obs).sum()) == 3
    assert r.pvalue == np.float64(4) / np.float64(len(lab) + 1)
    _check_exact(r, W, obs, with_obs, 2)


def _families(n_each, seed):
    """Two families of synthetic diagrams: a few long bars near (0.2, 1.2) against many short ones."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(2 * n_each):
        n = int(rng.integers(3, 9))
        b = rng.random(n) * 0.3
        pers = (1.0 + 0.2 * rng.random(n)) if k < n_each else 0.1 + 0.1 * rng.random(n)
        out.append(np.stack([b, b + pers], 1))
    return out


@pytest.mark.parametrize("metric,kw,entry", [("sliced_wasserstein", dict(M=20), "sliced_wasserstein_matrix"), ("heat", dict(sigma=0.3), "heat_matrix")])
def test_diagram_entry_end_to_end(pkg, metric, kw, entry):
    """diagram_permutation_test = the metric's matrix entry, then the test on what it returned."""
    dgms = _families(6, seed=2)
    labels = ["long"] * 6 + ["short"] * 6
    D = getattr(pkg, entry)(dgms, **kw)
    lab = pkg.label_permutations(labels, 200, seed=9)
    r = pkg.diagram_permutation_test(dgms, labels, metric=metric, B=200, seed=9, return_null=True, **kw)
    assert list(r.groups) == ["long", "short"]
    obs = np.repeat([0, 1], 6).astype(np.uint8)
    _check_exact(r, D, obs, lab, 2)
    assert r.pvalue < 0.05  # the families differ
    r2 = pkg.diagram_permutation_test(dgms, labels, metric=metric, B=200, seed=9, q=2.0, return_null=True, **kw)
    _check_exact(r2, np.power(D, 2.0), obs, lab, 2)


@pytest.mark.parametrize("S,sizes", [(100, (30, 70)), (200, (120, 76, 4))], ids=["resident", "tiled"])
def test_order_of_the_diagrams_within_the_documented_bound(pkg, S, sizes):
    """Rows and columns of W and the labels permuted together: the additions are permuted, the bits
    may differ, and each order stays within S u T + 7 u T of the exact value (perm_ref.plain, whose
    own error of at most 3 u T the derivation's (n_max + 3 + ceil(S / 64)) u T leaves room for:
    tda_rips.h), the two orders within twice that of each other."""
    W = _w_points(S, seed=21)
    obs = _obs(sizes, seed=22)
    lab = _table(obs, 30, seed=23)
    p = np.random.default_rng(24).permutation(S)
    a = _run(pkg, W, obs, lab)
    b = _run(pkg, np.ascontiguousarray(W[np.ix_(p, p)]), obs[p].copy(), np.ascontiguousarray(lab[:, p]))
    for row, ta, tb in zip(np.vstack([obs[None], lab]), np.append(a.statistic, a.null), np.append(b.statistic, b.null)):
        exact = pr.plain(W, row)
        assert abs(ta - exact) <= pr.bound(S, exact) and abs(tb - exact) <= pr.bound(S, exact)
        assert abs(ta - tb) <= 2 * pr.bound(S, exact)
