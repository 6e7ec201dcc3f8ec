"""GPU tests of greedy landmark subsampling (ripser.py's n_perm): k_greedy_perm /
k_gather_landmarks through tda_greedy_perm, and ripser_batch(n_perm=k).

Every output is an index or an f32 distance that is copied or compared, never
computed, so every check is exact equality against a numpy restatement of
upstream's get_greedy_perm over the oracle's distance matrix (for
distance-matrix input: over the matrix itself).
"""
import numpy as np
import pytest

import side_plan_ref as spr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pkg, built_lib):
    import torch  # a process that hands torch CUDA tensors to the library initialises torch's device first

    torch.cuda.init()
    assert pkg.lib().tda_device_ok(0) == 1, "no gfx950 device visible"
    return pkg


def greedy_ref(dm, k):
    """ripser.py get_greedy_perm, restated: (idx_perm, lambdas, number of steps with a tied maximum)."""
    dm = np.asarray(dm)
    idx = np.zeros(k, np.int64)
    lam = np.zeros(k, np.float64)
    ds = dm[0].copy()
    ties = 0
    for i in range(1, k):
        j = int(np.argmax(ds))  # first occurrence: the lowest index among equal maxima
        ties += int(np.count_nonzero(ds == ds[j]) > 1)
        idx[i] = j
        lam[i - 1] = ds[j]
        ds = np.minimum(ds, dm[j])
    lam[k - 1] = ds.max()
    return idx, lam, ties


def cloud(n, d=3, seed=0):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def check_layer(g, l, dm, k, tag=""):
    idx, lam, _ = greedy_ref(dm, k)
    assert g.idx_perm[l].tolist() == idx.tolist(), tag
    assert g.lambdas[l].tolist() == lam.tolist(), tag
    assert g.r_cover[l] == lam[-1], tag
    if g.dperm2all is not None:
        assert np.array_equal(g.dperm2all[l], np.asarray(dm, np.float32)[idx]), tag
    return idx


def test_ties_on_the_integer_grid(gpu, oracle):
    """The unnoised 12 x 12 integer grid: 32 of the 39 selection steps have a
    tied maximum, so a wrong tie rule or reduction order changes idx_perm."""
    i, j = np.meshgrid(np.arange(12), np.arange(12), indexing="ij")
    X = np.stack([i.ravel(), j.ravel()], 1).astype(np.float32)
    dm = oracle.distances(X)
    assert greedy_ref(dm, 40)[2] == 32
    g = gpu.greedy_perm_batch(X[None], 40)
    assert g.idx_perm.dtype == np.int64 and g.idx_perm.shape == (1, 40)
    assert g.lambdas.dtype == np.float64 and g.lambdas.shape == (1, 40) and g.dperm2all.shape == (1, 40, 144)
    check_layer(g, 0, dm, 40)
    # the single-cloud form returns upstream's triple
    ip, lam, dp = gpu.greedy_perm(X, 40)
    assert np.array_equal(ip, g.idx_perm[0]) and np.array_equal(lam, g.lambdas[0]) and np.array_equal(dp, g.dperm2all[0])


def test_duplicates_and_edges(gpu, oracle):
    base = cloud(40, seed=1)
    X = np.concatenate([base, base[:20]])  # 60 points, 20 exact duplicates
    dm = oracle.distances(X)
    # more landmarks than distinct points: once ds is all zero argmax returns index 0 again, as upstream
    for k in (1, 30, 50, 60):
        idx = check_layer(gpu.greedy_perm_batch(X[None], k), 0, dm, k, k)
    assert len(set(idx.tolist())) == 40
    Y = cloud(50, seed=2)
    g = gpu.greedy_perm_batch(Y[None], 50)  # n_perm = N: a permutation, nothing left uncovered
    check_layer(g, 0, oracle.distances(Y), 50)
    assert sorted(g.idx_perm[0].tolist()) == list(range(50)) and g.r_cover[0] == 0.0
    g = gpu.greedy_perm_batch(cloud(1, seed=3)[None], 1)  # N = 1
    assert g.idx_perm.tolist() == [[0]] and g.lambdas.tolist() == [[0.0]] and g.dperm2all.tolist() == [[[0.0]]]


@pytest.mark.parametrize("n,k", [(63, 16), (64, 16), (65, 16), (1023, 16), (1025, 16), (1025, 64), (4099, 16)])
def test_thread_layout_borders(gpu, oracle, n, k):
    """Around one wave, around one entry per thread, and several entries per
    thread at an N that is a multiple of nothing."""
    X = cloud(n, seed=n)
    check_layer(gpu.greedy_perm_batch(X[None], k), 0, oracle.distances(X), k)


@pytest.mark.parametrize("n,d", [(130, 4096), (200, 64)])
def test_distance_paths_match_sklearn_columns(gpu, n, d):
    """D >= 32: the matrix comes from the MFMA kernels (N <= 144: the D-split
    whole-layer Gram + combine).  sklearn's pairwise_distances(X, X[i][None])
    is column i of its full matrix bit for bit off the diagonal."""
    from sklearn.metrics import pairwise_distances

    X = cloud(n, d, seed=d)
    g = gpu.greedy_perm_batch(X[None], 32)
    idx = g.idx_perm[0]
    cols = pairwise_distances(X, X[idx])  # (n, 32)
    assert cols.dtype == np.float32
    want = cols.T.copy()
    got = g.dperm2all[0]
    own = (np.arange(32), idx)
    assert np.all(got[own] == 0.0)  # a landmark's distance to itself is 0 here (upstream: up to 6e-6)
    want[own] = 0.0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # and the selection is the restatement's over the library's own matrix of this cloud
    dm = gpu.ripser_batch(X[None], maxdim=0, want_dist=True)[0].dist
    check_layer(g, 0, dm, 32)


def test_batch_layers_do_not_bleed(gpu, oracle):
    X = gpu.synthetic.sweep144(8)
    g = gpu.greedy_perm_batch(X, 48)
    for l in range(8):
        check_layer(g, l, oracle.distances(X[l]), 48, l)
    # (4, 100, 100) float64 distance matrices (f32-representable values: the library reads them as f32)
    M = np.stack([oracle.distances(cloud(100, seed=10 + l)) for l in range(4)]).astype(np.float64)
    g = gpu.greedy_perm_batch(M, 25, distance_matrix=True)
    for l in range(4):
        check_layer(g, l, M[l], 25, l)
    g32 = gpu.greedy_perm_batch(M.astype(np.float32), 25, distance_matrix=True, want_dperm2all=False)
    assert g32.dperm2all is None and np.array_equal(g32.idx_perm, g.idx_perm) and np.array_equal(g32.lambdas, g.lambdas)


# ---- chunks of layers: TDA_SIDE_WS_BYTES caps a chunk's bytes, so that a call of 5 layers runs the chunk loop
_CHUNK = {}


def chunk_case(oracle, form):
    """(X as the call takes it, its keywords, the plan's keywords, the layers' oracle matrices), once per form."""
    if form not in _CHUNK:
        n, d = {"n40_d64": (40, 64), "n150_d64": (150, 64)}.get(form, (65, 3))
        X = np.stack([cloud(n, d, seed=70 + l) for l in range(5)])
        dm = np.stack([oracle.distances(X[l]) for l in range(5)])
        dm.setflags(write=False)
        plan = dict(L=5, N=n, D=d, dtype=spr.F32, is_dist=False, host_in=True, k=16, want_dp=True)
        if form == "f64_matrices":
            _CHUNK[form] = dm.astype(np.float64), dict(distance_matrix=True), dict(plan, D=n, dtype=spr.F64, is_dist=True), dm
        else:
            _CHUNK[form] = X, {}, dict(plan, host_in=form != "device_points"), dm
    return _CHUNK[form]


@pytest.mark.parametrize("Lc", [2, 1])
@pytest.mark.parametrize("form", ["n65_d3", "n40_d64", "n150_d64", "f64_matrices", "device_points"])
def test_layer_chunks_equal_the_whole_call(gpu, oracle, monkeypatch, form, Lc):
    """L = 5 in chunks of 2, 2, 1 and of one layer: the chunk buffers and the two kernel events reused,
    the results at l0 * k, dperm2all copied down per chunk.  D = 64: the partial Grams of a chunk on the
    whole-layer path (N = 40) and on the tiled path (N = 150); f64 matrices and a device tensor: the chunk's
    pointer into the caller's memory.  Byte for byte the uncapped call and the host loop on the oracle's matrix."""
    import torch

    X, kw, plan, dm = chunk_case(oracle, form)
    Y = torch.from_numpy(X).cuda() if form == "device_points" else X
    whole = gpu.greedy_perm_batch(Y, 16, **kw)
    cap = spr.cap_for(spr.greedy, Lc, **plan)
    assert spr.greedy(cap=cap, **plan)["Lc"] == Lc and spr.greedy(**plan)["Lc"] == 5
    monkeypatch.setenv("TDA_SIDE_WS_BYTES", str(cap))
    g = gpu.greedy_perm_batch(Y, 16, **kw)
    for name in ("idx_perm", "lambdas", "dperm2all"):
        assert getattr(g, name).tobytes() == getattr(whole, name).tobytes(), name
    for l in range(5):
        check_layer(g, l, dm[l], 16, l)
    print(f"{form} Lc={Lc}: select_ms {g.select_ms:.4f} device_ms {g.device_ms:.4f}")
    assert 0 < g.select_ms <= g.device_ms


def _pairs(res, d):
    return [(float(b), float(e), int(bi), int(di)) for (b, e), bi, di in zip(res.dgms[d], res.birth_idx[d], res.death_idx[d])]


def _opairs(o, d):
    return [(float(b), float(e), int(bi), int(di)) for (b, e), bi, di in zip(o["dgms"][d], o["birth_idx"][d], o["death_idx"][d])]


def assert_landmark_persistence(res, dm, k, maxdim, oracle, tag=""):
    idx, lam, _ = greedy_ref(dm, k)
    sub = dm[np.ix_(idx, idx)]
    o = oracle.rips(sub, maxdim=maxdim, distance_matrix=True)
    assert res.idx_perm.tolist() == idx.tolist() and res.r_cover == lam[-1], tag
    assert np.float32(res.thresh) == np.float32(o["thresh"]) and res.num_edges == o["num_edges"], tag
    for d in range(maxdim + 1):
        assert _pairs(res, d) == _opairs(o, d), (tag, d)
        assert res.checksum[d] == o["checksum"][d], (tag, d)
    return sub


def test_persistence_on_landmarks(gpu, oracle):
    X = gpu.synthetic.sweep144(4)
    res = gpu.ripser_batch(X, maxdim=2, n_perm=48, want_dist=True)
    for l in range(4):
        sub = assert_landmark_persistence(res[l], oracle.distances(X[l]), 48, 2, oracle, l)
        assert np.array_equal(res[l].dist, sub)  # dist describes the landmark matrix
    # without subsampling: every point, nothing uncovered
    plain = gpu.ripser_batch(X[:1], maxdim=0)[0]
    assert plain.idx_perm.tolist() == list(range(144)) and plain.r_cover == 0.0


def test_circle_4096_runs_through_landmarks(gpu, oracle):
    """The capability: N = 4096 is above the H1 limit (2,900), 256 landmarks are
    not; the circle's one long class survives, every other bar is within the
    2 * r_cover bottleneck bound of the diagonal."""
    X = gpu.synthetic.circle(4096)
    with pytest.raises(NotImplementedError):
        gpu.ripser_batch(X[None], maxdim=1)
    res = gpu.ripser_batch(X[None], maxdim=1, n_perm=256)[0]
    assert_landmark_persistence(res, oracle.distances(X), 256, 1, oracle)
    h1 = res.dgms[1]
    assert res.r_cover > 0.0 and int(np.count_nonzero(h1[:, 1] - h1[:, 0] > 2 * res.r_cover)) == 1


def test_device_input_equals_host_input(gpu):
    import torch

    X = np.stack([cloud(300, seed=20), cloud(300, seed=21)])
    Xd = torch.from_numpy(X).cuda()
    gh, gd = gpu.greedy_perm_batch(X, 32), gpu.greedy_perm_batch(Xd, 32)
    assert np.array_equal(gh.idx_perm, gd.idx_perm) and np.array_equal(gh.lambdas, gd.lambdas)
    assert np.array_equal(gh.dperm2all, gd.dperm2all)
    rh, rd = gpu.ripser_batch(X, maxdim=1, n_perm=32), gpu.ripser_batch(Xd, maxdim=1, n_perm=32)
    for l in range(2):
        assert rh[l].idx_perm.tolist() == rd[l].idx_perm.tolist() and rh[l].r_cover == rd[l].r_cover
        assert rh[l].checksum == rd[l].checksum and all(_pairs(rh[l], d) == _pairs(rd[l], d) for d in range(2))
