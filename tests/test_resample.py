"""GPU tests of the resampling stage and the Hausdorff confidence bands: k_resample_hausdorff through
tda_resample, hausdorff_resamples and confidence_bands.

Every output is an f32 distance that is copied or compared, never computed, so every check is exact
equality against the numpy restatement (resample_ref.py) over ``dm``, the ``dist`` that
``ripser_batch(X, want_dist=True)`` returns.  No test here calls the bottleneck entry, and none
hands a device buffer of this entry to the persistence pipeline (known limits).
"""
import numpy as np
import pytest

import resample_ref as rr
import side_plan_ref as spr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pkg, built_lib):
    import torch  # a process that hands torch CUDA tensors to the library initialises torch's device first

    torch.cuda.init()
    assert pkg.lib().tda_device_ok(0) == 1, "no gfx950 device visible"
    return pkg


def cloud(n, d=3, seed=0):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def clouds(L, n, d=3, seed=0):
    return np.stack([cloud(n, d, seed + 100 * l) for l in range(L)])


_DM = {}


def dist_of(gpu, X, key=None):
    """The library's own (L, N, N) f32 matrices of X, computed once per key and left unchanged."""
    if key is None or key not in _DM:
        dm = np.stack([r.dist for r in gpu.ripser_batch(X, maxdim=0, want_dist=True)])
        dm.setflags(write=False)
        if key is None:
            return dm
        _DM[key] = dm
    return _DM[key]


def dgms_equal(a, b, maxdim, tag=""):
    for d in range(maxdim + 1):
        x, y = np.asarray(a[d], np.float64).reshape(-1, 2), np.asarray(b[d], np.float64).reshape(-1, 2)
        assert x.shape == y.shape and np.array_equal(x, y), (tag, d)


def size(gpu, nn):
    """A point count: a number, or "lds" / "lds+1" for the largest N of the LDS path and the first above it."""
    return {"lds": gpu._lib.TDA_RS_LDS_N, "lds+1": gpu._lib.TDA_RS_LDS_N + 1}.get(nn, nn)


# ---------------------------------------------------------------- 1. Hausdorff, bit for bit
@pytest.mark.parametrize("nn", [1, 2, 36, 64, 65, "lds", "lds+1", 1025])
def test_hausdorff_equals_numpy(gpu, nn):
    """Around one wave (64, 65), around the LDS tile (TDA_RS_LDS_N, + 1), several columns per
    thread on the global path (1025), and the degenerate N = 1, 2; B around kRsPerBlock and one
    wave's share of it; m = 1, N // 2, N."""
    n = size(gpu, nn)
    X = clouds(3, n, seed=n)
    dm = dist_of(gpu, X, ("h", n))
    rng = np.random.default_rng(n)
    for B in (1, 7, 65):
        for m in sorted({1, max(1, n // 2), n}):
            idx = rng.integers(0, n, size=(B, m), dtype=np.int32)
            H = gpu.hausdorff_resamples(X, idx)
            assert H.dtype == np.float64 and H.shape == (3, B)
            assert np.array_equal(H, rr.hausdorff(dm, idx)), (n, B, m)


@pytest.mark.parametrize("nn", [36, "lds+1"])
def test_hausdorff_special_tables(gpu, nn):
    n = size(gpu, nn)
    X = clouds(3, n, seed=n)  # the clouds of test_hausdorff_equals_numpy: one dm for both
    dm = dist_of(gpu, X, ("h", n))
    # the identity sample (and a permutation of it): every point is in the sample, H is exactly 0
    ident = np.stack([np.arange(n), np.arange(n)[::-1], np.random.default_rng(1).permutation(n)]).astype(np.int32)
    assert not gpu.hausdorff_resamples(X, ident).any()
    # one index repeated m times: H is that row's maximum
    rep = np.stack([np.full(n, j) for j in (0, n // 3, n - 1)]).astype(np.int32)
    H = gpu.hausdorff_resamples(X, rep)
    for l in range(3):
        assert H[l].tolist() == [float(dm[l][j].max()) for j in (0, n // 3, n - 1)]
    assert np.array_equal(H, rr.hausdorff(dm, rep))
    # a table per layer
    per = np.random.default_rng(2).integers(0, n, size=(3, 7, n // 2), dtype=np.int32)
    H = gpu.hausdorff_resamples(X, per)
    assert np.array_equal(H, rr.hausdorff(dm, per))
    assert not np.array_equal(H, rr.hausdorff(dm, per[0]))  # the layers' tables do differ
    assert np.array_equal(gpu.hausdorff_resamples(X, per.astype(np.int64)), H)  # any integer dtype


def test_hausdorff_ties_and_duplicates(gpu):
    """The unnoised 12 x 12 integer grid (most distances tied: the maximum and the minima are
    reached many times over) and a cloud with 20 exact duplicates (zero distances off the diagonal)."""
    i, j = np.meshgrid(np.arange(12), np.arange(12), indexing="ij")
    G = np.stack([i.ravel(), j.ravel()], 1).astype(np.float32)
    X = np.stack([G, G[::-1].copy(), G * 2.0])
    dm = dist_of(gpu, X)
    assert len(np.unique(dm[0])) < 80  # 144^2 entries, few distinct values
    idx = np.random.default_rng(3).integers(0, 144, size=(9, 40), dtype=np.int32)
    H = gpu.hausdorff_resamples(X, idx)
    assert np.array_equal(H, rr.hausdorff(dm, idx)) and np.array_equal(H[2], 2.0 * H[0])
    base = cloud(40, seed=1)
    Y = np.concatenate([base, base[:20]])[None]  # 60 points, 20 exact duplicates
    dmy = dist_of(gpu, Y)
    idy = np.concatenate([np.random.default_rng(4).integers(0, 60, size=(6, 30), dtype=np.int32),
                          np.arange(40, dtype=np.int32)[None, :30], np.arange(30, 60, dtype=np.int32)[None]])
    H = gpu.hausdorff_resamples(Y, idy)
    assert np.array_equal(H, rr.hausdorff(dmy, idy))
    both = np.arange(40, dtype=np.int32)[None]  # every distinct point: the duplicates are at distance 0
    assert gpu.hausdorff_resamples(Y, both).tolist() == [[0.0]]


# ---------------------------------------------------------------- 3. layers and resamples do not bleed
def test_layers_and_resamples_do_not_bleed(gpu):
    n, L, B = 65, 4, 9
    X = clouds(L, n, seed=33)
    idx = gpu.resample_indices(n, B, seed=5)
    H = gpu.hausdorff_resamples(X, idx)
    H_l, H_b = gpu.hausdorff_resamples(X[::-1].copy(), idx), gpu.hausdorff_resamples(X, idx[::-1].copy())
    assert len({H.tobytes(), H_l.tobytes(), H_b.tobytes()}) == 3
    assert np.array_equal(H_l, H[::-1]) and np.array_equal(H_b, H[:, ::-1])
    # a table per layer, its layers reversed with the clouds
    per = np.random.default_rng(6).integers(0, n, size=(L, B, 30), dtype=np.int32)
    H_p, H_q = gpu.hausdorff_resamples(X, per), gpu.hausdorff_resamples(X[::-1].copy(), per[::-1].copy())
    assert np.array_equal(H_q, H_p[::-1]) and np.array_equal(H_p, rr.hausdorff(dist_of(gpu, X), per))


# ---------------------------------------------------------------- 3b. chunks of layers
_CHUNK = {}


def chunk_case(oracle, n, d):
    """Five clouds, their oracle matrices (no pipeline call), a shared and a per-layer table: once per shape."""
    if (n, d) not in _CHUNK:
        X = clouds(5, n, d, seed=80 + d)
        dm = np.stack([oracle.distances(X[l]) for l in range(5)])
        dm.setflags(write=False)
        rng = np.random.default_rng(n)
        _CHUNK[n, d] = X, dm, {"shared": rng.integers(0, n, size=(9, 30), dtype=np.int32), "per_layer": rng.integers(0, n, size=(5, 9, 30), dtype=np.int32)}
    return _CHUNK[n, d]


@pytest.mark.parametrize("n,d,table,Lc", [(65, 3, "shared", 2), (65, 3, "shared", 1), (65, 3, "per_layer", 2), (65, 3, "per_layer", 1),
                                          (150, 64, "per_layer", 2)])
def test_layer_chunks_equal_the_whole_call(gpu, oracle, monkeypatch, n, d, table, Lc):
    """L = 5 under a cap of TDA_SIDE_WS_BYTES that serves Lc layers per chunk (2, 2, 1, or one by one): the
    chunk buffers reused, the results at l0 * B, a per-layer table uploaded chunk by chunk.  Byte for byte
    the uncapped call and the restatement over the oracle's matrices."""
    X, dm, tables = chunk_case(oracle, n, d)
    idx = tables[table]
    plan = dict(L=5, N=n, D=d, dtype=spr.F32, is_dist=False, host_in=True, B=9, m=30, per_layer_idx=table == "per_layer")
    whole = gpu.hausdorff_resamples(X, idx)
    cap = spr.cap_for(spr.resample, Lc, **plan)
    assert spr.resample(cap=cap, **plan)["Lc"] == Lc and spr.resample(**plan)["Lc"] == 5
    monkeypatch.setenv("TDA_SIDE_WS_BYTES", str(cap))
    H = gpu.hausdorff_resamples(X, idx)
    assert H.shape == (5, 9) and H.tobytes() == whole.tobytes()
    assert np.array_equal(H, rr.hausdorff(dm, idx))


# ---------------------------------------------------------------- 4. input forms
@pytest.mark.parametrize("n,d", [(40, 3), (40, 64), (150, 64)])
def test_input_forms_agree(gpu, n, d):
    """f32 points (D = 3: the scalar distance kernel; D = 64: the matrix-core ones, whole-layer at
    N = 40 and tiled at N = 150), f32 and f64 distance matrices and torch device tensors: the bits
    that the f32 host points give through the returned dm."""
    import torch

    L, B = 2, 6
    X = clouds(L, n, d, seed=40 + d)
    dm = dist_of(gpu, X)
    idx = gpu.resample_indices(n, B, seed=8)
    want = rr.hausdorff(dm, idx)
    Xd, Md = torch.from_numpy(X).cuda(), torch.from_numpy(np.array(dm)).cuda()
    forms = [("f32 points", X, False), ("device points", Xd, False), ("f32 matrices", np.array(dm), True),
             ("f64 matrices", dm.astype(np.float64), True), ("device matrices", Md, True)]
    for tag, Y, is_dm in forms:
        assert np.array_equal(gpu.hausdorff_resamples(Y, idx, distance_matrix=is_dm), want), tag


# ---------------------------------------------------------------- 5. confidence_bands end to end
@pytest.fixture(scope="module")
def bands_ref(ref_clouds, oracle):
    """The CPU restatement at L = 2, N = 36, B = 16 on the committed layers: oracle.rips for the
    full clouds' diagrams, oracle.distances and numpy for the rest."""
    X = np.ascontiguousarray(ref_clouds[:2], dtype=np.float32)
    L, N, B = 2, X.shape[1], 16
    idx = np.random.default_rng(11).integers(0, N, size=(B, N), dtype=np.int32)
    dm = np.stack([oracle.distances(X[l]) for l in range(L)])
    full = [oracle.rips(X[l], maxdim=1)["dgms"] for l in range(L)]
    return X, idx, full, np.broadcast_to(2.0 * rr.hausdorff(dm, idx), (2, L, B)).copy()


def assert_bands(cb, full, stat, alpha, dims, idx):
    q, sig, n = rr.bands(full, stat, alpha, dims)
    assert cb.method == "hausdorff" and np.array_equal(cb.idx, idx) and cb.idx.dtype == np.int32
    assert cb.stat.dtype == np.float64 and cb.stat.shape == stat.shape and np.array_equal(cb.stat, stat)
    assert np.array_equal(cb.quantile, q) and np.array_equal(cb.radius, q)
    assert cb.n_significant.dtype == np.int64 and np.array_equal(cb.n_significant, n)
    for l in range(len(full)):
        dgms_equal(cb.results[l].dgms, full[l], max(dims))
        for k in range(len(dims)):
            assert cb.significant[l][k].dtype == bool and cb.significant[l][k].tolist() == sig[l][k].tolist(), (l, k)


def test_confidence_bands_end_to_end(gpu, bands_ref):
    X, idx, full, stat = bands_ref
    for alpha in (0.05, 0.5):  # ranks 16 (the maximum) and 8
        cb = gpu.confidence_bands(X, alpha=alpha, method="hausdorff", maxdim=1, idx=idx)
        assert_bands(cb, full, stat, alpha, [0, 1], idx)
    # every H0 bar of a full cloud but the essential one is finite; that one is always significant
    assert all(cb.significant[l][0][-1] and cb.n_significant[0, l] >= 1 for l in range(2))
    one = gpu.confidence_bands(X, alpha=0.5, maxdim=1, dims=[1], idx=idx)  # one dimension only; the default method
    assert_bands(one, full, stat[1:], 0.5, [1], idx)
    # the table of the defaults is resample_indices', and the call is reproducible
    a, b = gpu.confidence_bands(X, B=8, seed=3), gpu.confidence_bands(X, B=8, seed=3)
    assert np.array_equal(a.idx, gpu.resample_indices(36, 8, seed=3)) and a.stat.tobytes() == b.stat.tobytes()
    assert a.stat.shape == (2, 2, 8)


# ---------------------------------------------------------------- 7. workspace
def test_resample_workspace(gpu):
    """A small call, one large enough to make the workspace grow and to take the global-memory
    path, a smaller one, and the small call again: the same bits, those of the restatement (which
    is what a fresh process gives: no value depends on the buffer or on the offsets carved into it)."""
    small, big = clouds(2, 16, seed=50), clouds(3, 300, seed=60)
    tiny = small[:1, :5].copy()
    i_small, i_big, i_tiny = gpu.resample_indices(16, 5, seed=1), gpu.resample_indices(300, 12, m=100, seed=2), gpu.resample_indices(5, 2, seed=3)
    H1 = gpu.hausdorff_resamples(small, i_small)
    H2 = gpu.hausdorff_resamples(big, i_big)
    Ht = gpu.hausdorff_resamples(tiny, i_tiny)
    H3 = gpu.hausdorff_resamples(small, i_small)
    assert H1.tobytes() == H3.tobytes() and np.array_equal(H1, rr.hausdorff(dist_of(gpu, small), i_small))
    assert np.array_equal(H2, rr.hausdorff(dist_of(gpu, big), i_big))
    assert np.array_equal(Ht, rr.hausdorff(dist_of(gpu, tiny), i_tiny))
