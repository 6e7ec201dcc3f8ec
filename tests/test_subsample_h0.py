"""GPU tests of the subsample H0 entry and the persistent-homology dimension: k_subsample_h0 through
tda_subsample_h0, h0_subsamples and ph_dimension.

A death is an f32 distance that is copied or compared, never computed, and E at alpha 1 and 2 is a
float64 sum of exact terms in a fixed order, so those checks are exact equality against the numpy
restatement (sh0_ref.py).  Most cases hand the library a host f32 distance matrix, which it uses as
it is (upper triangle, zero diagonal), so ``dm`` is known on the host.  The only pipeline calls are
``ripser_batch(host array, maxdim=0, want_dist=True)``; no test makes a diagram-entry call or hands a
device buffer of its own to the pipeline (known limits).
"""
import numpy as np
import pytest

import sh0_ref
from test_subsample_h0_cpu import F32, cap_for, duplicated, lattice, plan_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pkg, built_lib):
    import torch  # a process that hands torch CUDA tensors to the library initialises torch's device first

    torch.cuda.init()
    assert pkg.lib().tda_device_ok(0) == 1, "no gfx950 device visible"
    return pkg


def cloud(n, d=3, seed=0):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


_DM = {}


def matrices(L, n, seed=0, d=3):
    """(L, n, n) f32 matrices, symmetric with a zero diagonal: computed once per key and left unchanged."""
    key = (L, n, seed, d)
    if key not in _DM:
        dm = np.stack([sh0_ref.distances(cloud(n, d, seed + 100 * l)) for l in range(L)])
        dm.setflags(write=False)
        _DM[key] = dm
    return _DM[key]


def mixed_table(n, B, m, seed):
    """B rows of length m over n points (with repetition when m > n), sizes cycling 1, 2, n // 2, m."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n, size=(B, m), dtype=np.int32)
    if m <= n:
        for b in range(B):
            idx[b] = rng.permutation(n)[:m]
    sizes = np.array([min(m, max(1, s)) for s in (1, 2, n // 2, m)] * B, dtype=np.int32)[:B]
    if B == 1:
        sizes[0] = m
    return idx, sizes


def check_against_ref(gpu, dm, idx, sizes, alphas=(1.0, 2.0), tag=None):
    for alpha in alphas:
        E, D = gpu.h0_subsamples(np.array(dm), idx, sizes, alpha=alpha, deaths=True, distance_matrix=True)
        Er, Dr = sh0_ref.h0_subsamples(dm, idx, sizes, alpha)
        assert E.dtype == np.float64 and E.shape == Er.shape
        assert E.tobytes() == Er.tobytes(), (tag, alpha)
        for l in range(len(Dr)):
            for b in range(len(Dr[l])):
                assert D[l][b].dtype == np.float64 and D[l][b].astype(np.float32).tobytes() == Dr[l][b].tobytes(), (tag, l, b)
        assert np.array_equal(gpu.h0_subsamples(np.array(dm), idx, sizes, alpha=alpha, distance_matrix=True), E)  # without the deaths: the same E


# ---------------------------------------------------------------- 1. bit equality with the restatement
@pytest.mark.parametrize("n", [1, 2, 36, 64, 65, 128, 129, 257, 1025])
def test_equals_the_restatement(gpu, n):
    """Around one wave (64, 65), around the resident path's border (128, 129), several positions per
    thread on the global path (257, 1025) and the degenerate N = 1, 2; sizes 1, 2, N // 2 and N mixed
    in one call; B around kSh0PerBlock and one wave's share of it."""
    dm = matrices(3, n, seed=n)
    for B in (1, 7, 65):
        if n == 1025 and B == 65:
            B = 9  # the restatement's time
        idx, sizes = mixed_table(n, B, n, seed=n + B)
        check_against_ref(gpu, dm, idx, sizes, tag=(n, B))


@pytest.mark.parametrize("n,m", [(128, 127), (128, 128), (128, 129), (129, 128), (36, 200)])
def test_path_choice_borders(gpu, n, m):
    """Both sides of the path choice in both of its conditions (N at 128 / 129, m at 128 / 129), and a
    row longer than the cloud (repeats) that puts the global path at a small N."""
    p = plan_ref(L=3, N=n, D=n, dtype=F32, is_dist=True, host_in=True, B=7, m=m, per_layer_idx=0, want_deaths=1)[1]
    assert p["resident"] == int(n <= 128 and m <= 128)
    dm = matrices(3, n, seed=n)
    idx, sizes = mixed_table(n, 7, m, seed=m)
    sizes[3] = m
    check_against_ref(gpu, dm, idx, sizes, tag=(n, m))


# ---------------------------------------------------------------- 2. ties and duplicates
def test_ties_and_duplicates(gpu):
    from oracle import oracle

    for X, n_zero in ((lattice(), 0), (duplicated(), 20)):
        n = len(X)
        dm = oracle.distances(X)[None]
        fwd, rev = np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32)[::-1].copy()
        idx = np.stack([fwd, rev, np.full(n, n // 2, dtype=np.int32), np.random.default_rng(1).permutation(n).astype(np.int32)])
        for alpha in (1.0, 2.0):
            E, D = gpu.h0_subsamples(dm, idx, alpha=alpha, deaths=True, distance_matrix=True)
            Er, Dr = sh0_ref.h0_subsamples(dm, idx, None, alpha)  # each table in its own order
            assert E.tobytes() == Er.tobytes()
            assert all(D[0][b].astype(np.float32).tobytes() == Dr[0][b].tobytes() for b in range(4))
            assert E[0, 2] == 0.0 and not D[0][2].any() and len(D[0][2]) == n - 1  # one index repeated
            assert np.array_equal(np.sort(D[0][0]), np.sort(D[0][1])) and np.array_equal(np.sort(D[0][0]), np.sort(D[0][3]))
            assert np.count_nonzero(D[0][0] == 0.0) == n_zero
    E, D = gpu.h0_subsamples(oracle.distances(lattice())[None], np.arange(36, dtype=np.int32)[None], deaths=True, distance_matrix=True)
    assert E[0, 0] == 35.0 and set(D[0][0].tolist()) == {1.0}
    # a global-path call on the same clouds (m > 128, repeats)
    dm = oracle.distances(lattice())[None]
    idx = np.random.default_rng(2).integers(0, 36, size=(5, 150), dtype=np.int32)
    check_against_ref(gpu, dm, idx, np.array([150, 1, 149, 75, 2], np.int32), tag="lattice, global")


# ---------------------------------------------------------------- 3. other alpha
@pytest.mark.parametrize("alpha", [0.5, 3.7])
def test_other_alpha_within_the_bound(gpu, alpha, capsys):
    """|E - ref| <= (s + 16) * 2^-52 * ref: a term differs from numpy's pow by the two libraries'
    roundings, all terms are non-negative, the sum adds s roundings."""
    worst = 0.0
    for n, m in ((36, 36), (129, 129), (36, 200)):
        dm = matrices(3, n, seed=n)
        idx, sizes = mixed_table(n, 7, m, seed=m + 1)
        E, D = gpu.h0_subsamples(np.array(dm), idx, sizes, alpha=alpha, deaths=True, distance_matrix=True)
        Er, Dr = sh0_ref.h0_subsamples(dm, idx, sizes, alpha)
        for l in range(3):
            for b in range(7):
                assert D[l][b].astype(np.float32).tobytes() == Dr[l][b].tobytes()
                s = int(sizes[b])
                gap = abs(E[l, b] - Er[l, b])
                if Er[l, b] > 0:
                    worst = max(worst, gap / Er[l, b] * 2.0 ** 52)
                assert gap <= (s + 16) * 2.0 ** -52 * Er[l, b], (n, m, l, b, E[l, b], Er[l, b])
    with capsys.disabled():
        print(f"\n[sh0] alpha = {alpha}: largest gap {worst:.3f} x 2^-52")


# ---------------------------------------------------------------- 4. no bleeding between subsamples
@pytest.mark.parametrize("n,m", [(65, 40), (65, 140)])
def test_subsamples_and_layers_do_not_bleed(gpu, n, m):
    L, B = 3, 9
    dm = matrices(L, n, seed=33)
    rng = np.random.default_rng(6)
    idx = rng.integers(0, n, size=(B, m), dtype=np.int32)
    sizes = np.array([1, 2, m // 2, m - 1, m, 3, m // 3, 2, m - 2], np.int32)
    past = np.arange(m)[None, :] >= sizes[:, None]
    hi, lo = np.where(past, n - 1, idx).astype(np.int32), np.where(past, 0, idx).astype(np.int32)
    E_hi, D_hi = gpu.h0_subsamples(np.array(dm), hi, sizes, deaths=True, distance_matrix=True)
    E_lo, D_lo = gpu.h0_subsamples(np.array(dm), lo, sizes, deaths=True, distance_matrix=True)
    assert E_hi.tobytes() == E_lo.tobytes()  # entries past sizes[b] are never read
    assert all(D_hi[l][b].tobytes() == D_lo[l][b].tobytes() for l in range(L) for b in range(B))
    Er, _ = sh0_ref.h0_subsamples(dm, idx, sizes)
    assert E_hi.tobytes() == Er.tobytes()
    # a table per layer differs from the shared one where it should
    per = np.stack([idx, rng.integers(0, n, size=(B, m), dtype=np.int32), idx])
    E_p = gpu.h0_subsamples(np.array(dm), per, sizes, distance_matrix=True)
    assert E_p.tobytes() == sh0_ref.h0_subsamples(dm, per, sizes)[0].tobytes()
    assert np.array_equal(E_p[0], E_hi[0]) and np.array_equal(E_p[2], E_hi[2]) and not np.array_equal(E_p[1, 2:], E_hi[1, 2:])
    # a layer's result does not depend on its neighbours in the call
    alone = gpu.h0_subsamples(np.array(dm[1:2]), idx, sizes, distance_matrix=True)
    rev = gpu.h0_subsamples(np.array(dm[::-1]), idx, sizes, distance_matrix=True)
    assert np.array_equal(alone[0], E_hi[1]) and np.array_equal(rev, E_hi[::-1])


# ---------------------------------------------------------------- 5. chunks of layers and of subsamples
@pytest.mark.parametrize("table,Lc", [("shared", 1), ("shared", 2), ("per_layer", 1), ("per_layer", 2)])
def test_layer_chunks_equal_the_whole_call(gpu, monkeypatch, table, Lc):
    """L = 3, N = 65 under a cap of TDA_SIDE_WS_BYTES that serves Lc layers per chunk: the chunk's buffers
    reused, E at l0 * B, a per-layer table uploaded and the deaths read back chunk by chunk.  Byte for
    byte the uncapped call and the restatement."""
    n, B, m = 65, 9, 30
    dm = matrices(3, n, seed=33)
    rng = np.random.default_rng(n)
    idx = rng.integers(0, n, size=(B, m) if table == "shared" else (3, B, m), dtype=np.int32)
    sizes = np.array([30, 1, 15, 2, 29, 30, 7, 3, 30], np.int32)
    plan = dict(L=3, N=n, D=n, dtype=F32, is_dist=True, host_in=True, B=B, m=m, per_layer_idx=int(table == "per_layer"), want_deaths=1)
    E, D = gpu.h0_subsamples(np.array(dm), idx, sizes, deaths=True, distance_matrix=True)
    cap = cap_for(Lc, **plan)
    assert plan_ref(cap=cap, **plan)[1]["Lc"] == Lc and plan_ref(**plan)[1]["Lc"] == 3
    monkeypatch.setenv("TDA_SIDE_WS_BYTES", str(cap))
    E_c, D_c = gpu.h0_subsamples(np.array(dm), idx, sizes, deaths=True, distance_matrix=True)
    assert E_c.tobytes() == E.tobytes() and all(D_c[l][b].tobytes() == D[l][b].tobytes() for l in range(3) for b in range(B))
    Er, Dr = sh0_ref.h0_subsamples(dm, idx, sizes)
    assert E_c.tobytes() == Er.tobytes() and all(D_c[l][b].astype(np.float32).tobytes() == Dr[l][b].tobytes() for l in range(3) for b in range(B))


def test_subsample_chunks(gpu):
    """B = 65537: two launches of the subsample loop (65535 + 2).  Every row against the restatement,
    computed once per distinct (row, size)."""
    n, B, m = 4, 65537, 4
    dm = matrices(2, n, seed=4)
    rng = np.random.default_rng(9)
    idx = rng.integers(0, n, size=(B, m), dtype=np.int32)
    sizes = rng.integers(1, m + 1, size=B, dtype=np.int32)
    E, D = gpu.h0_subsamples(np.array(dm), idx, sizes, deaths=True, distance_matrix=True)
    assert E.shape == (2, B)
    memo = {}
    for b in range(B):
        key = (int(sizes[b]), *idx[b, :sizes[b]].tolist())
        if key not in memo:
            memo[key] = [sh0_ref.prim(dm[l], key[1:]) for l in range(2)]
        for l in range(2):
            Er, dr = memo[key][l]
            assert E[l, b] == Er and D[l][b].astype(np.float32).tobytes() == dr.tobytes(), (l, b)


# ---------------------------------------------------------------- 6. input forms
@pytest.mark.parametrize("n,d", [(40, 3), (150, 64)])
def test_input_forms_agree(gpu, n, d):
    """Host f32 points, a torch CUDA tensor of points, the library's own matrix (want_dist) on the host
    and on the device: the same bytes, those of the restatement over that matrix."""
    import torch

    L = 2
    X = np.stack([cloud(n, d, 40 + d + 100 * l) for l in range(L)])
    dm = np.stack([r.dist for r in gpu.ripser_batch(X, maxdim=0, want_dist=True)])
    idx, sizes = gpu.subsample_indices(n, [n // 4, n // 2, n], 2, seed=8)
    Er, Dr = sh0_ref.h0_subsamples(dm, idx, sizes)
    Xd, Md = torch.from_numpy(X).cuda(), torch.from_numpy(dm).cuda()
    for tag, Y, is_dm in (("f32 points", X, False), ("device points", Xd, False), ("f32 matrices", dm, True), ("device matrices", Md, True),
                          ("f64 matrices", dm.astype(np.float64), True)):
        E, D = gpu.h0_subsamples(Y, idx, sizes, deaths=True, distance_matrix=is_dm)
        assert E.tobytes() == Er.tobytes(), tag
        assert all(D[l][b].astype(np.float32).tobytes() == Dr[l][b].tobytes() for l in range(L) for b in range(len(sizes))), tag


# ---------------------------------------------------------------- 7. ph_dimension end to end
def test_ph_dimension_end_to_end(gpu):
    """The four N = 256 clouds of the unit square of the CPU test, as one call of four layers."""
    X = np.stack([np.random.default_rng(s).random((256, 2)).astype(np.float32) for s in range(4)])
    dm = np.stack([r.dist for r in gpu.ripser_batch(X, maxdim=0, want_dist=True)])
    ph = gpu.ph_dimension(X)
    idx, sz = sh0_ref.subsample_indices(256, sh0_ref.default_sizes(256), 8, 0)
    assert ph.idx.tobytes() == idx.tobytes() and ph.sizes.tobytes() == sz.tobytes() and ph.alpha == 1.0
    Er, _ = sh0_ref.h0_subsamples(dm, idx, sz)
    assert ph.E.tobytes() == Er.tobytes()
    for l in range(4):
        dim, slope, icpt = sh0_ref.regression(Er[l], sz)
        assert abs(ph.dimension[l] - dim) <= 1e-12 * abs(dim) and abs(ph.slope[l] - slope) <= 1e-12 and abs(ph.intercept[l] - icpt) <= 1e-11
        assert 1.7 <= ph.dimension[l] <= 2.3
    again = gpu.ph_dimension(X)
    assert again.E.tobytes() == ph.E.tobytes() and again.dimension.tobytes() == ph.dimension.tobytes()
    assert gpu.ph_dimension(X, seed=1).E.tobytes() != ph.E.tobytes()
    # a layer of coincident points (an all-zero matrix): E = 0, nan, and the other layers unchanged
    Z = dm.copy()
    Z[1] = 0.0
    z = gpu.ph_dimension(Z, distance_matrix=True)
    assert np.isnan(z.dimension[1]) and not z.E[1].any() and np.array_equal(z.dimension[[0, 2, 3]], ph.dimension[[0, 2, 3]])
    # alpha = 2 through the distance matrices
    ph2 = gpu.ph_dimension(dm, alpha=2.0, distance_matrix=True)
    assert ph2.E.tobytes() == sh0_ref.h0_subsamples(dm, idx, sz, 2.0)[0].tobytes()


# ---------------------------------------------------------------- 8. workspace
def test_workspace_grows_and_is_reused(gpu):
    """A large call (the workspace grows; the global path), a small one (the resident path, in the grown
    buffer), the large one again: the same bytes, those of the restatement.  The workspace is
    tda_resample's: a Hausdorff call between them changes nothing."""
    big, small = matrices(3, 300, seed=60), matrices(2, 16, seed=50)
    i_big, s_big = gpu.subsample_indices(300, [75, 150, 300], 3, seed=2)
    i_small, s_small = gpu.subsample_indices(16, [4, 8, 16], 2, seed=1)
    E1, D1 = gpu.h0_subsamples(np.array(big), i_big, s_big, deaths=True, distance_matrix=True)
    E2 = gpu.h0_subsamples(np.array(small), i_small, s_small, distance_matrix=True)
    H = gpu.hausdorff_resamples(np.array(small), i_small, distance_matrix=True)
    E3, D3 = gpu.h0_subsamples(np.array(big), i_big, s_big, deaths=True, distance_matrix=True)
    assert E1.tobytes() == E3.tobytes() and all(D1[l][b].tobytes() == D3[l][b].tobytes() for l in range(3) for b in range(9))
    assert E1.tobytes() == sh0_ref.h0_subsamples(big, i_big, s_big)[0].tobytes()
    assert E2.tobytes() == sh0_ref.h0_subsamples(small, i_small, s_small)[0].tobytes()
    assert H.shape == (2, 6)
