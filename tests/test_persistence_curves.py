"""GPU tests of the persistence curves (include/tda_dgm.h tda_persistence_curve, diagrams.py)
against the CPU reference tests/pc_ref.py.

Every comparison is ``np.array_equal`` with the numpy restatement, and no value is -0.0.  The
bitwise promises (a diagram alone / among others of both launches / at any position / on a permuted
grid / run to run) are ``==``.

Sizes: empty, one and two points, one wave and two (63 / 64 / 65: the packed launch serves n <= 64,
the chunked one everything above), the plan's classes (256, 1024) and the chunks of 1024 rows
(1024 / 2048 / 3072, each -1, +0, +1) up to the limit; grids below, at and above the packed
launch's tile of 64 values and the chunked launch's of 256.  The grid recipe is
test_vectorize.pl_grid's with a larger pool: births, deaths, midpoints, values outside every bar
and -0.0.  No test here calls the persistence pipeline (known limits)."""
import ctypes
import functools

import numpy as np
import pytest

import pc_ref
from test_wasserstein import diagram

pytestmark = pytest.mark.gpu

E = np.zeros((0, 2))
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 3073, 4095, 4096]
REPEATED = np.tile(np.array([[1.0, 4.0]]), (70, 1))  # one bar 70 times
FLAT = np.stack([np.arange(5.0), np.arange(5.0)], 1)  # d == b rows: an empty support
KERNELS = ("indicator", "tent")
COEFS = ("none", "positive", "mixed")
G_MIXED = 257  # two tiles of the chunked launch, five of the packed one


@functools.lru_cache(maxsize=None)
def mixed():
    return tuple([diagram(n, 600 + n) for n in SIZES] + [REPEATED, FLAT, np.concatenate([REPEATED[:3], diagram(40, 9), REPEATED[:2]])])


def small():
    return [d for d in mixed() if len(d) <= 70] + [diagram(257, 857)]


def coefs(dgms, kind: str):
    if kind == "none":
        return None
    rng = np.random.default_rng(len(dgms))
    return [rng.uniform(0.1, 2.0, len(d)) if kind == "positive" else rng.normal(0.0, 1.0, len(d)) for d in dgms]


def pc_grid(G: int, seed: int = 0) -> np.ndarray:
    """G values out of births, deaths and midpoints of seeded diagrams, values outside every bar, and -0.0; shuffled."""
    D = np.concatenate([diagram(1400, 1500), diagram(65, 665)[:10], REPEATED[:1]])
    pool = np.concatenate([[-0.0, -1.0, 11.5, 2.5], D[:, 0], D[:, 1], 0.5 * (D[:, 0] + D[:, 1])])
    assert G <= len(pool)
    rng = np.random.default_rng(seed)
    head, rest = pool[:4], pool[4:]
    g = np.concatenate([head, rest[rng.permutation(len(rest))]])[:max(G, 1)]
    return g[rng.permutation(len(g))][:G]


@functools.lru_cache(maxsize=None)
def mixed_ref(kernel: str, kind: str):
    """(acc (S, G), W (S,)) of the mixed list on its grid: computed once, shared and left unchanged."""
    dgms, grid, c = mixed(), pc_grid(G_MIXED, 1), coefs(mixed(), kind)
    pairs = [pc_ref.accumulate(D, grid, None if c is None else c[s], kernel) for s, D in enumerate(dgms)]
    acc, W = np.stack([a for a, _ in pairs]), np.array([w for _, w in pairs])
    acc.setflags(write=False)
    return acc, W


def expected(kernel: str, kind: str, normalize: bool) -> np.ndarray:
    acc, W = mixed_ref(kernel, kind)
    return np.stack([pc_ref.normalized(a, w) for a, w in zip(acc, W)]) if normalize else acc


def run(pkg, dgms, grid, coef=None, kernel="indicator", normalize=False, essential=False):
    out, ms = pkg.persistence_curves(list(dgms), grid, coef, kernel, normalize, essential, return_time=True)
    assert ms > 0 and out.shape == (len(dgms), len(grid)) and out.dtype == np.float64
    return out


@pytest.mark.parametrize("normalize", (False, True))
@pytest.mark.parametrize("kind", COEFS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_curves_equal_the_restatement(pkg, kernel, kind, normalize):
    dgms, grid = mixed(), pc_grid(G_MIXED, 1)
    out = run(pkg, dgms, grid, coefs(dgms, kind), kernel, normalize)
    ref = expected(kernel, kind, normalize)
    for s, D in enumerate(dgms):
        assert np.array_equal(out[s], ref[s]), (len(D), kernel, kind, normalize)
    assert not np.signbit(out[ref == 0]).any()  # +0.0 where the reference has it
    assert not out[0].any() and not out[len(SIZES) + 1].any()  # the empty diagram, the d == b rows
    if kind != "mixed":
        assert out[len(SIZES)].max() > 0 and not np.signbit(out).any()


@pytest.mark.parametrize("G", (1, 7, 63, 64, 65, 255, 256, 257))
def test_grid_sizes_on_both_sides_of_the_tiles(pkg, G):
    dgms, grid = small(), pc_grid(G, G)
    for kernel in KERNELS:
        for kind in COEFS:
            c = coefs(dgms, kind)
            out = run(pkg, dgms, grid, c, kernel, kind == "positive")
            assert np.array_equal(out, pc_ref.curves(dgms, grid, c, kernel=kernel, normalize=kind == "positive")), (kernel, kind)


@pytest.mark.parametrize("kernel", KERNELS)
def test_bitwise_invariants(pkg, kernel):
    """A diagram alone == among the others == at another position == in a second run, and a permuted grid
    gives permuted columns, for diagrams of both launches and with several chunks."""
    dgms, grid = mixed(), pc_grid(G_MIXED, 1)
    c = coefs(dgms, "mixed")
    among = run(pkg, dgms, grid, c, kernel, True)
    assert np.array_equal(among, expected(kernel, "mixed", True))
    assert np.array_equal(run(pkg, dgms, grid, c, kernel, True), among)  # two runs
    back = run(pkg, dgms[::-1], grid, c[::-1], kernel, True)  # every diagram at another position
    assert np.array_equal(back[::-1], among)
    for s in (2, 4, 5, 11, 19, len(SIZES)):
        alone = run(pkg, [dgms[s]], grid, [c[s]], kernel, True)
        assert np.array_equal(alone[0], among[s]), len(dgms[s])
        twice = run(pkg, [dgms[s], E, dgms[s]], grid, [c[s], [], c[s]], kernel, True)
        assert np.array_equal(twice[0], among[s]) and np.array_equal(twice[2], among[s]) and not twice[1].any()
    perm = np.random.default_rng(4).permutation(G_MIXED)
    assert np.array_equal(run(pkg, dgms, grid[perm], c, kernel, True), among[:, perm])
    assert np.array_equal(run(pkg, dgms, np.sort(grid)[:100], c, kernel, True), among[:, np.argsort(grid, kind="stable")[:100]])


def test_output_limit_with_tiny_diagrams(pkg):
    """S * G == TDA_VEC_MAX_OUT is computed, one diagram more is refused before any device work."""
    rng = np.random.default_rng(11)
    G = S = 4096
    assert S * G == pkg._lib.TDA_VEC_MAX_OUT
    pool = diagram(64, 664)
    dgms = [pool[rng.integers(0, 64, int(n))] for n in rng.integers(0, 3, S)]
    grid = pc_grid(G, 2)
    out = run(pkg, dgms, grid, kernel="tent")
    for s in (0, 1, 2, 1000, 2047, 2048, 4094, 4095):
        assert np.array_equal(out[s], pc_ref.curve(dgms[s], grid, kernel="tent")), s
    empty = [s for s, d in enumerate(dgms) if not len(d)]
    assert len(empty) > 1000 and not out[empty].any() and not np.signbit(out).any()
    one = [s for s, d in enumerate(dgms) if len(d) == 1]
    D1 = np.concatenate([dgms[s] for s in one])  # every one-point diagram at once: a tent each
    t = np.minimum(grid[None, :] - D1[:, :1], D1[:, 1:] - grid[None, :])
    assert np.array_equal(out[one], np.where(t > 0, t, 0.0))
    L, lb = pkg.lib(), pkg._lib
    off = np.zeros(S + 2, np.int64)
    res = ctypes.POINTER(lb.PcResult)()
    a = lb.PcArgs()
    a.offsets, a.grid, a.G, a.S, a.device = off.ctypes.data, grid.ctypes.data, G, S + 1, 0
    assert L.tda_persistence_curve(ctypes.byref(a), ctypes.byref(res)) == -2 and not res and b"2^24" in L.tda_last_error()


def test_largest_diagram_on_the_longest_grid(pkg):
    D, grid = diagram(4096, 4696), pc_grid(4096, 3)
    c = np.random.default_rng(6).normal(0.0, 1.0, 4096)
    out = run(pkg, [D, REPEATED], grid, [c, np.ones(70)], "tent", True)
    assert np.array_equal(out[0], pc_ref.curve(D, grid, c, "tent", True)) and np.array_equal(out[1], pc_ref.curve(REPEATED, grid, None, "tent", True))


def test_betti_curve_counts_classes(pkg):
    D = np.concatenate([diagram(300, 900), [[0.5, np.inf], [2.0, np.inf], [np.nan, 1.0], [-np.inf, 3.0]]])
    fin = D[:300]
    grid = np.concatenate([fin[:40, 0], fin[:40, 1], [-1.0, 0.5, 2.0, 1e300, -0.0]])  # values equal to births and to deaths
    with pytest.warns(UserWarning, match="2 points with a non-finite"):
        with_ess = run(pkg, [D, fin], grid, essential=True)
    with pytest.warns(UserWarning, match="4 points with a non-finite"):
        without = run(pkg, [D, fin], grid)
    count = np.searchsorted(np.sort(fin[:, 0]), grid, "right") - np.searchsorted(np.sort(fin[:, 1]), grid, "right")
    assert np.array_equal(without[0], count) and np.array_equal(without[1], count) and np.array_equal(with_ess[1], count)
    assert np.array_equal(with_ess[0], count + (grid >= 0.5) + (grid >= 2.0))  # an essential class counts from its birth on
    assert np.array_equal(with_ess, np.floor(with_ess)) and with_ess[0, -2] == 2.0 and with_ess.min() == 0.0
    assert np.array_equal(with_ess[0], pc_ref.betti(D, grid)) and np.array_equal(without[0], pc_ref.betti(D, grid, essential=False))
    bar = np.array([[1.0, 2.0]])
    ends = np.array([np.nextafter(1.0, 0.0), 1.0, np.nextafter(2.0, 0.0), 2.0])
    assert run(pkg, [bar], ends)[0].tolist() == [0.0, 1.0, 1.0, 0.0]  # closed at b, open at d
    with pytest.warns(UserWarning):
        assert run(pkg, [np.array([[1.0, np.inf]])], ends, essential=True)[0].tolist() == [0.0, 1.0, 1.0, 1.0] and not run(pkg, [np.array([[1.0, np.inf]])], ends).any()


def test_normalised_zero_weights_give_positive_zeros(pkg):
    grid = pc_grid(70, 5)
    D, big = diagram(40, 940), diagram(1100, 2000)
    cancel = np.tile([1.5, -1.5], 20)
    for kernel in KERNELS:
        out = run(pkg, [D, D, E, big, D, D], grid, [np.zeros(40), cancel, [], np.zeros(1100), -np.ones(40), np.full(40, -0.0)], kernel, True)
        assert not out[[0, 1, 2, 3, 5]].any() and not np.signbit(out).any()  # W == 0; and under W < 0 a zero sum is +0.0, not -0.0
        assert np.array_equal(out[4], pc_ref.curve(D, grid, -np.ones(40), kernel, True)) and out[4].max() > 0
        plain = run(pkg, [D, D], grid, [np.zeros(40), cancel], kernel)
        assert not plain[0].any() and not np.signbit(plain[0]).any() and np.array_equal(plain[1], pc_ref.curve(D, grid, cancel, kernel))


def test_one_point_tents_are_the_first_landscape(pkg):
    dg = __import__("importlib").import_module(pkg.__name__ + ".diagrams")
    bars = diagram(90, 990)
    dgms = [bars[i:i + 1] for i in range(90)] + [E]
    grid = pc_grid(130, 7)
    pts, off, _ = dg._vec_inputs(dgms, 1)
    lam, _ = dg._call_pl(pts, off, grid, 1, 0)
    assert np.array_equal(run(pkg, dgms, grid, kernel="tent"), lam[:, 0, :])
    assert np.array_equal(run(pkg, dgms, grid, kernel="tent", normalize=True), lam[:, 0, :])  # n = 1


def test_named_entries_equal_the_reference_formulas(pkg):
    dgms = [diagram(n, 700 + n) for n in (5, 40, 65, 300, 1030)] + [E]
    allp = np.concatenate(dgms)
    grid = np.linspace(allp[:, 0].min(), allp[:, 1].max(), 100)
    for name, ref in (("betti_curves", pc_ref.betti), ("lifespan_curves", pc_ref.lifespan), ("entropy_curves", pc_ref.entropy),
                      ("persistence_silhouettes", pc_ref.silhouette)):
        out, g, ms = getattr(pkg, name)(dgms, return_grid=True, return_time=True)
        assert np.array_equal(g, grid) and ms > 0 and out.shape == (6, 100)
        assert np.array_equal(out, np.stack([ref(D, grid) for D in dgms])), name
        single = getattr(pkg, name[:-1])
        assert np.array_equal(single(dgms[2], grid[0], grid[-1], 100), out[2])
    for power in (0.0, 0.5, 2.0):
        out = pkg.persistence_silhouettes(dgms, grid[0], grid[-1], 100, power=power)
        assert np.array_equal(out, np.stack([pc_ref.silhouette(D, grid, power) for D in dgms])), power
    withinf = np.concatenate([dgms[1][:7], [[0.25, np.inf]], dgms[1][7:]])
    assert np.array_equal(pkg.betti_curve(withinf, grid[0], grid[-1], 100), pc_ref.betti(withinf, grid))
    assert pkg.betti_curve(withinf, grid[0], grid[-1], 100)[-1] == 1.0
    with pytest.warns(UserWarning, match="non-finite"):
        assert np.array_equal(pkg.lifespan_curve(withinf, grid[0], grid[-1], 100), pkg.lifespan_curve(dgms[1], grid[0], grid[-1], 100))
    F = pkg.layer_features(dgms, "silhouette", start=grid[0], stop=grid[-1])
    assert F.shape == (6, 100) and np.array_equal(F, np.stack([pc_ref.silhouette(D, grid) for D in dgms]))
