"""GPU tests of the geodesic-distance entry: the graph kernels and both closures through tda_geodesic
and geodesic_distances.

Most cases hand the library a host f32 distance matrix, which it uses as it is (upper triangle, zero
diagonal), so ``dm`` is known on the host; for point input ``dm`` is read back through the entry
itself (``radius=inf, graph_only=True`` returns it).  The graph is a copy of ``dm`` or ``inf``, so it
is compared bit for bit with the numpy restatement (geo_ref.py); the closure is compared bit for bit
where every sum is exact and within the header's bound elsewhere.  Inputs are arrays only: no test
here calls a pipeline entry (known limits).
"""
import numpy as np
import pytest

import geo_ref
from test_shortest_paths_cpu import F32, cloud, distances, two_clusters

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def gpu(pkg, built_lib):
    import torch  # a process that hands torch CUDA tensors to the library initialises torch's device first

    torch.cuda.init()
    assert pkg.lib().tda_device_ok(0) == 1, "no gfx950 device visible"
    return pkg


def lattice(side):
    i, j = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    return np.stack([i.ravel(), j.ravel()], 1).astype(np.float32)


def duplicated(n, seed):
    """n points, the first half repeated: zero distances off the diagonal, and every distance twice."""
    base = cloud((n + 1) // 2, 3, seed)
    return np.concatenate([base, base])[:n]


_REF = {}


def ref(tag, dm, k=None, radius=None, graph_only=False):
    """geo_ref.geodesic (or, graph_only, geo_ref.graph: W and the edge count) of one layer, computed once
    per (tag, graph) and left unchanged; the row order once per tag."""
    key = (tag, k, radius, graph_only)
    if key not in _REF:
        if k is not None and ("order", tag) not in _REF:
            _REF[("order", tag)] = geo_ref.row_order(dm)
        order = _REF.get(("order", tag))
        out = geo_ref.graph(dm, k, radius, order=order) if graph_only else geo_ref.geodesic(dm, k, radius, order=order)
        for a in out[:1 if graph_only else 2]:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def int_matrix(n, seed):
    """A symmetric matrix of integers 1 .. 1023, zero diagonal: every path sum below 2^24 is exact in f32."""
    m = np.random.default_rng(seed).integers(1, 1024, size=(n, n)).astype(np.float32)
    m = np.triu(m, 1)
    return m + m.T


def check_contract(g, l, W):
    G = g.dist[l]
    assert G.tobytes() == G.T.copy().tobytes() and not G.diagonal().any()
    assert (G <= W).all()


# ---------------------------------------------------------------- 1. the graph, bit for bit
@pytest.mark.parametrize("n", [1, 2, 3, 36, 64, 65, 129, 324, 1025])
def test_graph_only_equals_the_restatement(gpu, n):
    """Gaussian clouds, a cloud with duplicated points (ties decide membership) and, at N = 36, the
    6 x 6 lattice (every distance ties); k = 1, 2, 6, N - 1 and N + 5 (clipped), radius = 0, a median
    distance and inf.  Every value is a copy of dm or inf; n_edges is equal."""
    clouds = [cloud(n, 3, n), duplicated(n, n + 1)] + ([lattice(6)] if n == 36 else [])
    dm = np.stack([distances(X) for X in clouds])
    med = float(np.median(dm[0])) if n > 1 else 0.0
    modes = [(k, None) for k in sorted({1, 2, 6, n - 1, n + 5}) if k >= 1] + [(None, 0.0), (None, med), (None, INF)]
    for k, radius in modes:
        g = gpu.geodesic_distances(dm, n_neighbors=k, radius=radius, distance_matrix=True, graph_only=True)
        assert g.dist.dtype == np.float32 and g.dist.shape == dm.shape and g.connected is None and (g.n_components == -1).all()
        for l in range(len(clouds)):
            W, ne = ref(("graph", n, l), dm[l], k, radius, graph_only=True)
            assert g.dist[l].tobytes() == W.tobytes(), (n, l, k, radius)
            assert g.n_edges[l] == ne, (n, l, k, radius)


# ---------------------------------------------------------------- 2. integer weights: every schedule, bit for bit
@pytest.mark.parametrize("n,lds_n", [(2, None), (63, None), (64, None), (65, None), (128, None), (129, None), (200, None), (1025, None),
                                     (2, 1), (64, 1), (65, 1), (129, 1)])
def test_integer_weights_are_exact(gpu, monkeypatch, n, lds_n):
    """Symmetric integer matrices with entries 1 .. 1023: every path sum is exact in f32, so G == G* bit
    for bit under any schedule.  The resident closure up to its limit, the blocked one above it, and
    with TDA_GEO_LDS_N = 1 the blocked one at one tile, one tile exactly, two tiles, and three with
    padding."""
    if lds_n is not None:
        monkeypatch.setenv("TDA_GEO_LDS_N", str(lds_n))
    p = geo_ref.plan(L=2, N=n, D=n, dtype=F32, is_dist=True, host_in=True, n_neighbors=3, lds_n=lds_n)[1]
    assert p["resident"] == int(lds_n is None and n <= 128) and (p["resident"] or p["tiles"] == -(-n // 64))
    dm = np.stack([int_matrix(n, 7 * n + l) for l in range(2)])
    for k in (3, 6):
        g = gpu.geodesic_distances(dm, n_neighbors=k, distance_matrix=True)
        for l in range(2):
            W, G, nc, ne = ref(("int", n, l), dm[l], k)
            assert G[np.isfinite(G)].max() < 2 ** 24
            assert g.dist[l].tobytes() == G.astype(np.float32).tobytes(), (n, lds_n, k, l)
            assert g.n_components[l] == nc and g.n_edges[l] == ne and g.connected[l] == (nc == 1)
            check_contract(g, l, W)


# ---------------------------------------------------------------- 3. the complete graph
@pytest.mark.parametrize("n", [36, 200])
def test_complete_graph_is_the_metric(gpu, n):
    """radius = inf on a Gaussian 3-D cloud: G == dm bit for bit, because no detour is shorter.  Checked
    on the host first: every dm[i][k] + dm[k][j] exceeds dm[i][j] by more than 2 ulp (2^-22 relative),
    so its rounded f32 sum (at most 2^-24 relative below) is still above dm[i][j], and by induction no
    step of any schedule lowers a value.  Seed 3 has this property at both sizes."""
    dm = distances(cloud(n, 3, 3))
    d64 = dm.astype(np.float64)
    off = ~np.eye(n, dtype=bool)
    for k in range(n):
        detour = d64[:, k][:, None] + d64[k, :][None, :]
        ok = off.copy()
        ok[k, :] = ok[:, k] = False
        assert (detour[ok] > d64[ok] * (1 + 2.0 ** -22)).all(), k
    g = gpu.geodesic_distances(dm[None], radius=INF, distance_matrix=True)
    assert g.dist[0].tobytes() == dm.tobytes() and g.n_components[0] == 1 and g.n_edges[0] == n * (n - 1) // 2


# ---------------------------------------------------------------- 4. float clouds within the header's bound
@pytest.mark.parametrize("n,d", [(36, 3), (180, 3), (324, 3), (1025, 3), (36, 64), (180, 64), (324, 64), (1025, 64)])
def test_float_clouds_within_the_bound(gpu, n, d):
    """The reference's sizes and one above 1024, k = 6, point input in 3 and 64 dimensions (the scalar and
    the matrix-core distance kernels): |G - G*| <= ((1 + 2^-24)^c - 1) G* with the header's c for the
    schedule that ran, bitwise symmetry, zero diagonal, the inf pattern and the components."""
    X = np.stack([cloud(n, d, 11 * n + d), cloud(n, d, 11 * n + d + 1)])
    dm = gpu.geodesic_distances(X, radius=INF, graph_only=True).dist  # the library's own distances of these points
    assert dm.tobytes() == dm.transpose(0, 2, 1).copy().tobytes() and (dm >= 0).all()
    g = gpu.geodesic_distances(X, n_neighbors=6)
    worst = 0.0
    for l in range(2):
        W, G, nc, ne = ref(("float", n, d, l), dm[l], 6)
        check_contract(g, l, W)
        got = g.dist[l].astype(np.float64)
        assert np.array_equal(np.isinf(got), np.isinf(G)) and g.n_components[l] == nc and g.n_edges[l] == ne
        fin = np.isfinite(G) & (G > 0)
        gap = np.abs(got[fin] - G[fin]) / G[fin]
        worst = max(worst, float(gap.max()) if gap.size else 0.0)
        assert (gap <= geo_ref.bound(n)).all(), (n, d, l, gap.max() / geo_ref.U, geo_ref.depth(n))
        assert np.array_equal(got[G == 0], G[G == 0])
    print(f"[geodesic] N = {n}, D = {d}: largest gap {worst / geo_ref.U:.3f} x 2^-24 G* (c = {geo_ref.depth(n)})")  # shown with -s or on failure


# ---------------------------------------------------------------- 4b. which schedule ran
@pytest.mark.parametrize("n", [65, 100])
def test_each_schedule_equals_its_own_restatement(gpu, monkeypatch, n):
    """A float cloud on which the two schedules round differently (asserted on the host first): the
    default call equals the resident schedule restated step for step in numpy f32, and the call under
    TDA_GEO_LDS_N = 1 equals the blocked one, bit for bit.  So the override reaches the library and the
    blocked cases of this file do run the blocked kernels; were it ignored, the second half would fail."""
    dm = distances(cloud(n, 3, 500))
    W = geo_ref.graph(dm, 6)[0]
    res, blk = geo_ref.closure_resident(W), geo_ref.closure_blocked(W)
    assert np.count_nonzero(res != blk) > 0
    got = gpu.geodesic_distances(dm[None], n_neighbors=6, distance_matrix=True).dist[0]
    assert got.tobytes() == res.tobytes()
    monkeypatch.setenv("TDA_GEO_LDS_N", "1")
    got = gpu.geodesic_distances(dm[None], n_neighbors=6, distance_matrix=True).dist[0]
    assert got.tobytes() == blk.tobytes()


# ---------------------------------------------------------------- 5. disconnection
def test_two_clusters(gpu):
    X = two_clusters()
    dm = distances(X)[None]
    g = gpu.geodesic_distances(dm, n_neighbors=3, distance_matrix=True)
    G = g.dist[0]
    assert g.n_components[0] == 2 and not g.connected[0]
    assert np.isinf(G[:6, 6:]).all() and np.isinf(G[6:, :6]).all() and np.isfinite(G[:6, :6]).all() and np.isfinite(G[6:, 6:]).all()
    f = g.filled(1000.0)
    assert (f[0][:6, 6:] == 1000.0).all() and np.array_equal(f[0][:6, :6], G[:6, :6])
    one = gpu.geodesic_distances(dm, radius=float(dm.max()), distance_matrix=True)
    assert one.n_components[0] == 1 and one.connected[0] and np.isfinite(one.dist).all()


# ---------------------------------------------------------------- 6. layers do not bleed
@pytest.mark.parametrize("lds_n", [None, 1])
def test_mixed_layers_equal_single_calls(gpu, monkeypatch, lds_n):
    """Five different layers of N = 36 in one call equal five calls of one layer, bit for bit, under
    both closures."""
    if lds_n is not None:
        monkeypatch.setenv("TDA_GEO_LDS_N", str(lds_n))
    ang = 2 * np.pi * np.arange(36) / 36
    ring = np.stack([np.cos(ang), np.sin(ang), 0 * ang], 1).astype(np.float32)
    clusters = np.concatenate([cloud(18, 3, 1), cloud(18, 3, 2) + np.float32(100.0)])
    lat = np.concatenate([lattice(6), np.zeros((36, 1), np.float32)], 1)
    X = np.stack([cloud(36, 3, 5), duplicated(36, 6), lat, clusters, ring])
    for kw in (dict(n_neighbors=3), dict(radius=1.0)):
        whole = gpu.geodesic_distances(X, **kw)
        assert len(set(whole.n_components.tolist())) > 1
        for l in range(5):
            alone = gpu.geodesic_distances(X[l:l + 1], **kw)
            assert alone.dist[0].tobytes() == whole.dist[l].tobytes(), (kw, l)
            assert alone.n_components[0] == whole.n_components[l] and alone.n_edges[0] == whole.n_edges[l]
        rev = gpu.geodesic_distances(X[::-1].copy(), **kw)
        assert rev.dist[::-1].tobytes() == whole.dist.tobytes()


# ---------------------------------------------------------------- 7. chunks of layers
@pytest.mark.parametrize("n,Lc", [(65, 1), (65, 2), (130, 1), (130, 2)])
def test_layer_chunks_equal_the_whole_call(gpu, monkeypatch, n, Lc):
    """L = 3 under a cap of TDA_SIDE_WS_BYTES that serves Lc layers per chunk: the chunk's buffers reused,
    the counts at l0, the matrices read back chunk by chunk.  Byte for byte the uncapped call."""
    dm = np.stack([int_matrix(n, 3 * n + l) for l in range(3)])
    plan = dict(L=3, N=n, D=n, dtype=F32, is_dist=True, host_in=True, n_neighbors=4)
    whole = gpu.geodesic_distances(dm, n_neighbors=4, distance_matrix=True)
    cap = geo_ref.cap_for(Lc, **plan)
    assert geo_ref.plan(cap=cap, **plan)[1]["Lc"] == Lc and geo_ref.plan(**plan)[1]["Lc"] == 3
    monkeypatch.setenv("TDA_SIDE_WS_BYTES", str(cap))
    parts = gpu.geodesic_distances(dm, n_neighbors=4, distance_matrix=True)
    assert parts.dist.tobytes() == whole.dist.tobytes()
    assert parts.n_components.tolist() == whole.n_components.tolist() and parts.n_edges.tolist() == whole.n_edges.tolist()
    for l in range(3):
        assert whole.dist[l].tobytes() == ref(("chunk", n, l), dm[l], 4)[1].astype(np.float32).tobytes()


# ---------------------------------------------------------------- 8. input forms
@pytest.mark.parametrize("n,d", [(40, 3), (150, 64)])
def test_input_forms_agree(gpu, n, d):
    """Host f32 points, a torch CUDA tensor of points, the library's own matrix on the host (f32 and
    f64) and on the device: the same bytes."""
    import torch

    X = np.stack([cloud(n, d, 40 + d), cloud(n, d, 41 + d)])
    dm = gpu.geodesic_distances(X, radius=INF, graph_only=True).dist
    want = gpu.geodesic_distances(X, n_neighbors=5)
    Xd, Md = torch.from_numpy(X).cuda(), torch.from_numpy(dm).cuda()
    for tag, Y, is_dm in (("device points", Xd, False), ("f32 matrices", dm, True), ("device matrices", Md, True), ("f64 matrices", dm.astype(np.float64), True)):
        g = gpu.geodesic_distances(Y, n_neighbors=5, distance_matrix=is_dm)
        assert g.dist.tobytes() == want.dist.tobytes(), tag
        assert g.n_edges.tolist() == want.n_edges.tolist() and g.n_components.tolist() == want.n_components.tolist(), tag
    for l in range(2):
        assert want.n_edges[l] == ref(("forms", n, d, l), dm[l], 5)[3]


# ---------------------------------------------------------------- 9. workspace
def test_workspace_grows_and_is_reused(gpu):
    """A large call (the workspace grows; the blocked closure), a small one (the resident closure, in the
    grown buffer), the large one again: the same bytes, those of the restatement.  The workspace is
    tda_resample's: a Hausdorff call between them changes nothing.  Every result is freed by the
    binding on return (the entry's context manager)."""
    big, small = np.stack([int_matrix(300, 60 + l) for l in range(2)]), np.stack([int_matrix(16, 50 + l) for l in range(3)])
    g1 = gpu.geodesic_distances(big, n_neighbors=4, distance_matrix=True)
    g2 = gpu.geodesic_distances(small, n_neighbors=4, distance_matrix=True)
    H = gpu.hausdorff_resamples(small, np.arange(8, dtype=np.int32).reshape(2, 4), distance_matrix=True)
    g3 = gpu.geodesic_distances(big, n_neighbors=4, distance_matrix=True)
    assert g1.dist.tobytes() == g3.dist.tobytes() and g1.n_edges.tolist() == g3.n_edges.tolist()
    for l in range(2):
        assert g1.dist[l].tobytes() == ref(("big", l), big[l], 4)[1].astype(np.float32).tobytes()
    for l in range(3):
        assert g2.dist[l].tobytes() == ref(("small", l), small[l], 4)[1].astype(np.float32).tobytes()
    assert H.shape == (3, 2)
