"""GPU tests of the persistence landscapes and persistence images
(include/tda_dgm.h, diagrams.py) against the CPU references tests/pl_ref.py and
tests/pi_ref.py.

Landscapes are exact: every comparison is ``np.array_equal`` with the numpy
restatement, and no value is -0.0.  Images are compared pixel by pixel with the
40-digit reference under the bound the header derives, C(n) u sum(w) with
C(n) = 2 * 16 + 9 + n (pi_ref.bound).  The bitwise promises (a diagram alone /
among others of every size class / at any position / run to run) are ``==``.

Sizes: empty, one and two points, one wave and two (63 / 64 / 65), both sides of
the landscape kernel's size classes (n <= 64 / 256 / 1024 / 4096) and the limit;
image shapes below, at and above the 32 x 32 pixel tile, with points in chunks of
32.  No test but the last calls the persistence pipeline."""
import ctypes
import warnings

import numpy as np
import pytest

import pi_ref
import pl_ref
from test_wasserstein import diagram

pytestmark = pytest.mark.gpu

E = np.zeros((0, 2))
PL_SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 1024, 1025, 4095, 4096]
REPEATED = np.tile(np.array([[1.0, 4.0]]), (70, 1))  # one bar 70 times: the tie crosses K and a wave
FLAT = np.stack([np.arange(5.0), np.arange(5.0)], 1)  # d == b rows


def pl_diagrams():
    return [diagram(n, 500 + n) for n in PL_SIZES] + [REPEATED, FLAT, np.concatenate([REPEATED[:3], diagram(40, 9), REPEATED[:2]])]


def pl_grid(G: int, seed: int = 0) -> np.ndarray:
    """G values out of births, deaths and midpoints of the test diagrams, values outside every bar, and
    -0.0; shuffled."""
    D = np.concatenate([diagram(1000, 1500)[:40], diagram(65, 565)[:10], REPEATED[:1]])
    pool = np.concatenate([[-0.0, -1.0, 11.5, 2.5], D[:, 0], D[:, 1], 0.5 * (D[:, 0] + D[:, 1])])
    rng = np.random.default_rng(seed)
    head, rest = pool[:4], pool[4:]
    g = np.concatenate([head, rest[rng.permutation(len(rest))]])[:max(G, 1)]
    return g[rng.permutation(len(g))][:G]


def call_pl(pkg, dgms, grid, K):
    """One library call on a given grid (the Python entry forms its grid with linspace)."""
    dg = __import__("importlib").import_module(pkg.__name__ + ".diagrams")
    pts, off, _ = dg._vec_inputs(dgms, 1)
    out, ms = dg._call_pl(pts, off, np.ascontiguousarray(grid, np.float64), K, 0)
    assert ms > 0 and out.shape == (len(dgms), K, len(grid)) and out.dtype == np.float64
    return out


@pytest.mark.parametrize("G", (1, 7, 70))
@pytest.mark.parametrize("K", (1, 3, 9))
def test_landscapes_equal_the_restatement(pkg, K, G):
    dgms, grid = pl_diagrams(), pl_grid(G, 10 * K + G)
    out = call_pl(pkg, dgms, grid, K)
    ref = pl_ref.landscapes(dgms, grid, K)
    for s, D in enumerate(dgms):
        assert np.array_equal(out[s], ref[s]), (len(D), K, G)
    assert not np.signbit(out).any()
    assert not out[0].any() and not out[len(PL_SIZES) + 1].any()  # the empty diagram, the d == b rows
    # the same values on the sorted grid: a grid value's column does not depend on its place
    order = np.argsort(grid, kind="stable")
    assert np.array_equal(call_pl(pkg, dgms, grid[order], K), out[:, :, order])


@pytest.mark.parametrize("n", PL_SIZES)
def test_landscape_of_one_diagram_alone(pkg, n):
    D, grid = diagram(n, 500 + n), pl_grid(70, n)
    out = call_pl(pkg, [D], grid, 9)
    assert np.array_equal(out[0], pl_ref.landscape(D, grid, 9)) and not np.signbit(out).any()


def test_landscape_at_the_limits(pkg):
    D, grid = diagram(4096, 4596), pl_grid(64, 5)
    out = call_pl(pkg, [D, REPEATED], grid, 64)
    assert np.array_equal(out, pl_ref.landscapes([D, REPEATED], grid, 64)) and not np.signbit(out).any()
    inside = (grid > 1.0) & (grid < 4.0)
    assert inside.any() and (out[1][:, inside] > 0).all() and (out[1] == out[1][:1]).all()  # 70 equal tents fill all 64 depths


def test_landscape_python_entry(pkg):
    dgms = [diagram(n, 500 + n) for n in (5, 65, 300)] + [E]
    out, grid, ms = pkg.persistence_landscapes(dgms, num_steps=33, depth=4, return_grid=True, return_time=True)
    allp = np.concatenate(dgms)
    assert np.array_equal(grid, np.linspace(allp[:, 0].min(), allp[:, 1].max(), 33)) and ms > 0
    assert np.array_equal(out, pl_ref.landscapes(dgms, grid, 4))
    assert np.array_equal(pkg.persistence_landscape(dgms[1], grid[0], grid[-1], 33, 4), out[1])
    withinf = np.concatenate([dgms[1][:7], [[0.0, np.inf]], dgms[1][7:]])
    with pytest.warns(UserWarning, match="non-finite"):
        assert np.array_equal(pkg.persistence_landscape(withinf, grid[0], grid[-1], 33, 4), out[1])


# ---------------------------------------------------------------- images
XR = YR = (-1.0, 6.0)  # a range of 7: sigma 0.01 saturates a pixel, 0.5 is ordinary, 5 is flat


def check_image(pkg, D, birth_range, pers_range, shape, sigma, power=1.0):
    out = pkg.persistence_image(D, birth_range, pers_range, shape, sigma, power)
    xe, ye = np.linspace(*birth_range, shape[0] + 1), np.linspace(*pers_range, shape[1] + 1)
    assert out.shape == shape and out.dtype == np.float64
    err, tol = pi_ref.errors(out, pi_ref.image(D, xe, ye, sigma, power)), pi_ref.bound(D, weight_power=power)
    print(f"n={len(D)} shape={shape} sigma={sigma} power={power}: max error {err.max():.3e}, bound {tol:.3e}")
    assert (err <= tol).all(), (err.max(), tol)
    return out


@pytest.mark.parametrize("n", (0, 1, 5, 64, 65, 257))
def test_image_sizes(pkg, n):
    D = diagram(n, 700 + n)
    check_image(pkg, D, XR, YR, (4, 3), 0.5)
    out = check_image(pkg, D, XR, YR, (17, 33), 0.5)
    if n == 0:
        assert not out.any() and not np.signbit(out).any()
    else:
        assert out.sum() > 0


def test_image_1000_points(pkg):
    check_image(pkg, diagram(1000, 1700), XR, YR, (16, 16), 0.5)


def test_image_4096_points(pkg):
    check_image(pkg, diagram(4096, 4796), XR, YR, (4, 3), 0.5)


@pytest.mark.parametrize("shape", ((1, 1), (4, 3), (16, 16), (17, 33)))
def test_image_shapes_sigmas_and_weights(pkg, shape):
    D = diagram(65, 765)
    for sigma in (0.01, 0.5, 5.0):
        for power in (0.0, 1.0, 2.0):
            check_image(pkg, D, XR, YR, shape, sigma, power)


def test_image_with_points_outside_on_every_side(pkg):
    D = diagram(64, 764)
    b, p = D[:, 0], D[:, 1] - D[:, 0]
    assert b.min() < 1.5 < 3.5 < b.max() and p.min() < 1.0 < 3.0 < p.max()
    for sigma in (0.01, 0.5):
        check_image(pkg, D, (1.5, 3.5), (1.0, 3.0), (17, 33), sigma)
    flat = np.concatenate([D[:5], [[1.0, 1.0], [3.0, 2.0]]])  # d <= b adds nothing
    assert np.array_equal(pkg.persistence_image(flat, XR, YR, (4, 3), 0.5), pkg.persistence_image(D[:5], XR, YR, (4, 3), 0.5))


# ---------------------------------------------------------------- the bitwise promises
OTHERS = [0, 1, 3, 5, 8, 13, 20, 31, 40, 63, 64, 64, 65, 70, 100, 128, 200, 255, 256, 257, 300, 500, 700, 1024, 1025, 1500, 2048, 3000, 4095,
          4096]


@pytest.mark.parametrize("entry", ("landscape", "image"))
def test_bitwise_invariants(pkg, entry):
    """The same diagram alone == first, last and in the middle of 30 others that span every size class
    == in a second call == with the others permuted."""
    grid = pl_grid(70, 3)
    if entry == "landscape":
        run = lambda dgms: call_pl(pkg, dgms, grid, 9)  # noqa: E731
    else:
        run = lambda dgms: pkg.persistence_images(dgms, XR, YR, (17, 33), 0.5)  # noqa: E731
    others = [diagram(n, 900 + i) for i, n in enumerate(OTHERS)]
    assert len(others) == 30
    rng = np.random.default_rng(8)
    for n in (70, 300, 1100, 4096, 0):
        D = diagram(n, 800 + n)
        alone = run([D])[0]
        assert np.array_equal(run([D])[0], alone)  # a second call
        first, last = run([D] + others), run(others + [D])
        mid = run(others[:15] + [D] + others[15:])
        assert np.array_equal(first[0], alone) and np.array_equal(last[-1], alone) and np.array_equal(mid[15], alone)
        assert np.array_equal(first[1:], last[:-1]) and np.array_equal(first[1:16], mid[:15]) and np.array_equal(first[16:], mid[16:])
        perm = rng.permutation(30)
        shuffled = run([others[i] for i in perm[:11]] + [D] + [others[i] for i in perm[11:]])
        assert np.array_equal(shuffled[11], alone)
        assert np.array_equal(np.delete(shuffled, 11, axis=0), first[1:][perm])
        assert np.array_equal(run([D, D])[1], alone)


# ---------------------------------------------------------------- other
def test_output_limit_through_the_abi(pkg):
    """S * F above TDA_VEC_MAX_OUT returns TDA_E_UNSUPPORTED with no result (and no device work: the
    plan refuses it), the largest call below it is computed."""
    L, lb = pkg.lib(), pkg._lib
    off = np.zeros(258, np.int64)
    grid = np.linspace(0.0, 1.0, 4096)
    res = ctypes.POINTER(lb.PlResult)()
    a = lb.PlArgs()
    a.offsets, a.grid, a.G, a.K, a.device = off.ctypes.data, grid.ctypes.data, 4096, 64, 0
    a.S = 65
    assert L.tda_landscape(ctypes.byref(a), ctypes.byref(res)) == -2 and not res and b"2^24" in L.tda_last_error()
    a.S = 64
    assert L.tda_landscape(ctypes.byref(a), ctypes.byref(res)) == 0 and res
    try:
        r = res.contents
        assert (r.S, r.F) == (64, 64 * 4096) and r.device_ms > 0
        v = np.ctypeslib.as_array(r.values, shape=(r.S * r.F,))
        assert not v.any() and not np.signbit(v).any()
    finally:
        L.tda_pl_free(res)
    e = np.arange(257.0)
    res = ctypes.POINTER(lb.PiResult)()
    a = lb.PiArgs()
    a.offsets, a.x_edges, a.y_edges, a.W, a.H, a.sigma, a.weight_power, a.device = off.ctypes.data, e.ctypes.data, e.ctypes.data, 256, 256, 1.0, 1.0, 0
    a.S = 257
    assert L.tda_persistence_image(ctypes.byref(a), ctypes.byref(res)) == -2 and not res and b"2^24" in L.tda_last_error()
    a.S = 2
    assert L.tda_persistence_image(ctypes.byref(a), ctypes.byref(res)) == 0 and res
    try:
        r = res.contents
        assert (r.S, r.F) == (2, 65536) and not np.ctypeslib.as_array(r.values, shape=(r.S * r.F,)).any()
    finally:
        L.tda_pi_free(res)


@pytest.mark.parametrize("dim", (0, 1))
def test_layer_results_give_the_bits_of_their_arrays(pkg, dim):
    res = pkg.ripser_batch(pkg.synthetic.sweep48(4), maxdim=1, device=0)
    arrays = [r.dgms[dim] for r in res]
    assert len(res) == 4
    fin = pl_ref.finite_points(np.concatenate(arrays))
    lo, hi = (float(fin.min()), float(fin.max())) if len(fin) else (0.0, 1.0)  # the sweep's own scale
    assert dim == 1 or (len(fin) == 4 * 47 and hi > lo)
    pl = dict(start=lo, stop=hi, num_steps=50, depth=5)
    im = dict(birth_range=(lo - 0.25 * (hi - lo), hi), pers_range=(0.0, hi - lo), resolution=(17, 9), sigma=0.05 * (hi - lo))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # H0 holds one essential class per layer
        a, b = pkg.persistence_landscapes(res, dim=dim, **pl), pkg.persistence_landscapes(arrays, **pl)
        c, d = pkg.persistence_images(res, dim=dim, **im), pkg.persistence_images(arrays, **im)
        assert np.array_equal(a, b) and np.array_equal(c, d) and c.any() == bool(len(fin)) and (dim == 1 or a.any())
        assert np.array_equal(a, pl_ref.landscapes(arrays, np.linspace(lo, hi, 50), 5))
        assert np.array_equal(pkg.layer_features(res, "landscape", dim=dim, **pl), a.reshape(4, -1))
        assert np.array_equal(pkg.layer_features(res, "image", dim=dim, **im), c.reshape(4, -1))
        assert np.array_equal(pkg.layer_features(res[::-1], "image", dim=dim, **im), c[::-1].reshape(4, -1))
