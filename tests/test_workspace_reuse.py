"""GPU tests of the per-device workspaces of the entries beside the persistence pipeline
(csrc/aux_ws.h): sliced Wasserstein, bottleneck, the spectral metrics, greedy landmarks and UMAP.

Each test runs a small call, a call large enough to make the entry's workspace grow (and, for the
diagram distances, to reach another launch class), and the small call again.  The first and the
third result are equal with ``==``: the buffer moved, every offset into it is carved anew, and the
small call's values may depend on neither.  The small result also matches the entry's own reference
with the helpers and at the tolerance of the entry's own test file.

The file's name sorts after every other test file, so it runs last and shifts nothing ahead of
the parity tests; no test here calls the persistence pipeline (known limits)."""
import numpy as np
import pytest

import bn_ref
import spectral_ref
import test_bottleneck as tb
import test_greedy_perm as tg
import test_sliced_wasserstein as tsw
import test_umap as tu
from oracle import umap_ref

pytestmark = pytest.mark.gpu

ED_TOL = 1e-5  # test_spectral_metrics.py, test_gpu_parity.py


def test_sliced_wasserstein_workspace(pkg, built_lib):
    small = [tsw.diagram(5, 70 + i) for i in range(3)]
    big = [tsw.diagram(600, 80 + i) for i in range(4)]  # pairs of 1,200 points: the 1,024-thread class, a larger (P, M) buffer
    first = pkg.sliced_wasserstein_matrix(small, M=8)
    grown = pkg.sliced_wasserstein_matrix(big, M=16)
    again = pkg.sliced_wasserstein_matrix(small, M=8)
    assert np.array_equal(first, again)
    for D, dg, M in ((first, small, 8), (grown, big, 16)):
        assert np.array_equal(D, D.T) and not np.diag(D).any()
        for i in range(len(dg)):
            for j in range(i + 1, len(dg)):
                assert tsw.close(D[i, j], dg[i], dg[j], M)


def test_bottleneck_workspace(pkg, built_lib):
    small = [tb.diagram(5, 70 + i) for i in range(3)]
    big = [tb.diagram(300, 80 + i) for i in range(3)]  # the 512-thread class
    first = pkg.bottleneck_matrix(small)
    grown = pkg.bottleneck_matrix(big)
    again = pkg.bottleneck_matrix(small)
    assert np.array_equal(first, again)
    assert np.array_equal(grown, grown.T) and np.all(grown[~np.eye(3, dtype=bool)] > 0.0)
    for i in range(3):
        for j in range(i + 1, 3):
            assert first[i, j] == first[j, i] == bn_ref.bottleneck(small[i], small[j])


def test_spectral_workspace(pkg, built_lib):
    rng = np.random.default_rng(11)
    small = rng.standard_normal((2, 8, 4)).astype(np.float32)
    big = rng.standard_normal((4, 40, 64)).astype(np.float32)  # N <= D, D >= 32: the Gram matrices on the matrix cores
    alphas = [0.5, 2.0]  # 8 results after 2: the pinned buffer grows too
    first = pkg.compute_effective_dimensionality(small)
    grown = pkg.matrix_entropy_profile(big, alphas)
    again = pkg.compute_effective_dimensionality(small)
    assert first.dtype == np.float32 and first.shape == (2,) and np.array_equal(first, again)
    for g, w in zip(first, spectral_ref.effective_dimensionality(small)):
        assert spectral_ref.rel_gap(g, w, 0.0) <= ED_TOL, (float(g), float(w))
    assert grown.shape == (4, 2)
    for k, al in enumerate(alphas):
        for g, w in zip(grown[:, k], spectral_ref.matrix_entropy(big, al)):
            assert spectral_ref.rel_gap(g, w, spectral_ref.F32_ULP) <= ED_TOL, (al, float(g), float(w))


def test_greedy_workspace(pkg, built_lib, oracle):
    small, big = tg.cloud(16, seed=5)[None], np.stack([tg.cloud(300, seed=6 + l) for l in range(3)])
    first = pkg.greedy_perm_batch(small, 4, want_dperm2all=False)
    grown = pkg.greedy_perm_batch(big, 32)
    again = pkg.greedy_perm_batch(small, 4, want_dperm2all=False)
    assert np.array_equal(first.idx_perm, again.idx_perm) and np.array_equal(first.lambdas, again.lambdas)
    tg.check_layer(first, 0, oracle.distances(small[0]), 4)
    for l in range(3):
        tg.check_layer(grown, l, oracle.distances(big[l]), 32, l)


def test_umap_workspace(pkg, built_lib):
    """The fit and the transform share one workspace and carve it differently."""
    rng = np.random.default_rng(32)
    small = rng.standard_normal((1, 32, 3)).astype(np.float32)
    big = rng.standard_normal((2, 96, 8)).astype(np.float32)
    new = rng.standard_normal((1, 8, 3)).astype(np.float32)
    a, b = tu.ab_params()
    lr = 0.1  # the restatement's own sensitivity stays far below the 1e-3 cap of sgd_tolerance at this rate
    kw = dict(n_neighbors=5, n_components=2, metric="euclidean", random_state=tu.SEED, n_epochs=20, init="random", a=a, b=b)
    first = pkg.umap.umap_batch(small, learning_rate=lr, **kw)
    grown = pkg.umap.umap_batch(big, learning_rate=lr, **kw)
    moved = pkg.umap.umap_transform_batch(small[0], first[0], new, n_neighbors=5, n_epochs=20, a=a, b=b, seed=tu.SEED)
    again = pkg.umap.umap_batch(small, learning_rate=lr, **kw)
    assert np.array_equal(first, again)
    assert grown.shape == (2, 96, 2) and np.all(np.isfinite(grown)) and moved.shape == (1, 8, 2) and np.all(np.isfinite(moved))
    # the small fit against the restatement, from the GPU's own graph and start (test_umap.py: test_fuzzy_graph_vs_restatement,
    # test_fit_sgd_vs_restatement)
    E0, G = pkg.umap.umap_batch(small, learning_rate=0.0, return_graph=True, **kw)
    ref = umap_ref.fuzzy_graph(small[0], 5, "euclidean", n_epochs=20)
    assert np.array_equal(G[0] > 0, ref > 0) and np.max(np.abs(G[0] - ref)) < 2e-5

    def run(E):
        return umap_ref.sgd_fit(G[0], E, 20, a, b, lr=lr, gamma=1.0, neg_rate=5, seed=tu.SEED)

    want = run(E0[0])
    sens, tol = tu.sgd_tolerance(run, E0[0], want)
    diff = float(np.max(np.abs(first[0] - want)))
    msg = f"small fit: sens {sens:.3g} tol {tol:.3g} max diff {diff:.3g} moved {float(np.max(np.abs(want - E0[0]))):.3g}"
    print(msg)
    assert tol <= 1e-3, msg
    assert diff <= tol, msg
