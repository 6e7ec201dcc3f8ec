"""The pipeline above N = 2048 on the GPU: H0 to the limit of 8192, TwoNN, silhouette, H1 to 2900.

tda_rips_batch takes N <= 8192 for H0, <= 2900 for H1 and <= 2048 for H2; the n_perm path,
compute_intrinsic_dimensionality and silhouette_score send clouds of that size into it.  Here the
kernels whose loops, LDS carve or merge passes first take another trip at those sizes run against
the project's CPU references; tests/large_n.py holds the sizes (tests/test_rips_plan_cpu.py pins
them to h0_shape), the clouds and the thresholds.

* H0 (maxdim 0, two layers: a normal cloud and a lattice cloud with equal points and hundreds of
  groups of equal deaths): both sides of every sort-chunk border of k_h0 (2026/2027, 6122/6123,
  8170/8171), of the elder-rule switch (1024/1025), 4096/4097/4098 and 8191/8192.  block_sort merges
  in HBM from N = 6123 (two chunks, copy back) and with four chunks and an uneven tail from 8171; one
  size on each side of 6122/6123 runs again with a finite threshold that leaves both forests in
  pieces.  == with the oracle (assert_same), from N = 4096 with its committed result
  (tests/golden/large_n_h0_*.npz, tests/golden/make_golden_large_n.py).
* TwoNN (persistence=False: distances and k_twonn alone) at n = 1023 .. 8192: a normal cloud, a cloud
  of which a third are twins (fewer finite ratios than points: INFINITY padding inside pw2), at 1025
  and 8192 a cloud of twins only (NaN); discard 0.1, 0.0 and 0.999; 1e-5 relative against
  oracle/twonn.py on oracle.distances.
* Silhouette at n = 255 .. 513 and 8192: K = 2, 32 (shuffled codes), 31 (three singletons) in one call
  -- the launch runs with K = 32, so the K = 2 set has thirty empty clusters whose 0 / 0 the minimum
  must skip --; 1e-9 against oracle.silhouette; the H0 pairs of the call equal those without labels.
* H1 (one torus layer, finite threshold) at N = 2049 and 2900, where triangle indices pass 2^31.
* The refusals one past each limit, next to the accepted call at the limit.

Every persistence call is one clean first attempt (tda_debug_attempts).  Host numpy inputs, slot 0.
The file's name sorts behind tests/test_gpu_parity.py, and the N = 8192 cases, which grow slot 0's
workspace most, come last in it (known limits).
"""
import functools
import importlib
import os

import numpy as np
import pytest

import large_n as ln
from conftest import GOLDEN
from test_gpu_parity import _pairs, assert_same
from test_retry_paths import FIRST, attempts, clean

pytestmark = pytest.mark.gpu

SLOT = 0


@pytest.fixture(scope="module")
def gpu(pkg, built_lib):
    # torch ships its own HIP runtime: the process initialises torch's device first, as the other GPU
    # files do ("torch and the HIP runtime")
    import torch

    torch.cuda.init()
    assert pkg.lib().tda_device_ok(0) == 1, "no gfx950 device visible"
    return pkg


@pytest.fixture(autouse=True)
def memo_off(monkeypatch):
    # no earlier test's retry memo moves a call's first attempt
    monkeypatch.setenv("TDA_RETRY_MEMO", "0")


def one_clean_attempt(gpu, tag):
    at = attempts(gpu, SLOT)
    assert len(at) == 1 and clean(at[0], FIRST), (tag, at)


# ---------------------------------------------------------------- H0
def golden_h0(name, X):
    """The oracle's H0 of a two-layer case from its fixture, as oracle.rips returns it."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert str(z["sha"]) == ln.sha(X), name  # the clouds the fixture was recorded on
    out = []
    for l in range(X.shape[0]):
        death, ess = z[f"l{l}__death"].astype(np.float64), z[f"l{l}__ess"]
        dg = np.zeros((len(death) + len(ess), 2))
        dg[:, 1] = np.concatenate([death, np.full(len(ess), np.inf)])
        out.append({"dgms": [dg], "birth_idx": [np.concatenate([z[f"l{l}__bidx"], ess]).astype(np.int64)],
                    "death_idx": [np.concatenate([z[f"l{l}__didx"], np.full(len(ess), -1)]).astype(np.int64)],
                    "thresh": float(z["thresh"][l]), "num_edges": int(z["num_edges"][l]), "n_all_pairs": [int(z["n_all_pairs"][l])],
                    "checksum": [int(z["checksum"][l])]})
    return out


def h0_refs(n, X, scale=1.0, thresh=np.inf):
    if n >= ln.H0_GOLDEN_MIN_N or np.isfinite(thresh):
        return golden_h0("large_n_h0_%d" % n + ("_t" if np.isfinite(thresh) else ""), X)
    from oracle import oracle

    return [oracle.rips(X[l], maxdim=0, thresh=thresh) for l in range(X.shape[0])]


def h0_counts(o):
    d = o["dgms"][0][:, 1]
    fin = int(np.isfinite(d).sum())
    return fin, len(d) - fin, o["n_all_pairs"][0] - fin  # finite pairs, essential classes, zero-length forest edges


def run_h0(gpu, n, scale=1.0, thresh=np.inf):
    X = ln.h0_layers(n, scale)
    assert X.shape == (ln.H0_L, n, 3)
    refs = h0_refs(n, X, scale, thresh)
    # the inputs test something: equal points in the lattice layer's forest and, on a spanning forest, a hundred
    # groups of equal deaths; under a threshold both forests are in pieces and still have a thousand deaths
    fin, ess, zero = zip(*(h0_counts(o) for o in refs))
    assert zero[1] >= 1, (n, zero)
    if np.isfinite(thresh):
        assert min(ess) > 1 and min(fin) >= ln.H0_THRESH_MIN_FINITE, (n, thresh, fin, ess)
    else:
        assert ess == (1, 1) and refs[0]["n_all_pairs"][0] == refs[1]["n_all_pairs"][0] == n - 1, (n, ess)
        assert ln.equal_death_groups(refs[1]["dgms"][0][:, 1]) >= ln.LATTICE_MIN_GROUPS, n
    res = gpu.ripser_batch(X, maxdim=0, thresh=thresh, slot=SLOT)
    one_clean_attempt(gpu, ("h0", n, thresh))
    assert len(res) == ln.H0_L
    for l, o in enumerate(refs):
        assert_same(res[l], o, 0, ("h0", n, thresh, l))
    return res


H0_LAST = tuple(n for n in ln.H0_NS if n >= 8170)  # the largest workspaces: at the end of the file


@pytest.mark.parametrize("n", [n for n in ln.H0_NS if n not in H0_LAST])
def test_h0_sort_chunk_and_elder_borders(gpu, n):
    run_h0(gpu, n)


@pytest.mark.parametrize("n,scale,thresh", ln.H0_THRESH_CASES)
def test_h0_forest_in_pieces(gpu, n, scale, thresh):
    """A finite threshold: fewer than N - 1 keys reach block_sort (6,025 and 4,266 at N = 6122, one chunk
    of 8192; 6,029 and 4,241 at 6123, two chunks of 4096 of which the second holds 1,933 and 145)."""
    run_h0(gpu, n, scale, thresh)


# ---------------------------------------------------------------- TwoNN
@functools.lru_cache(maxsize=2)
def twonn_dist(n, all_twin, l):
    from oracle import oracle

    D = oracle.distances(ln.twonn_layers(n, all_twin)[l])
    D.setflags(write=False)
    return D


def finite_ratios(D, eps=1e-10):
    """How many points have a finite r2 / r1 (oracle/twonn.py's `valid` and isfinite steps)."""
    D = np.array(D, dtype=np.float32)
    np.fill_diagonal(D, np.inf)
    r = np.partition(D, 1, axis=1)[:, :2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mu = np.where((r[:, 0] > np.float32(eps)) & (r[:, 1] > np.float32(eps)), r[:, 1] / r[:, 0], np.float32(np.inf))
    return int(np.isfinite(mu).sum())


def run_twonn(gpu, n, all_twin):
    from oracle.twonn import twonn_from_dist

    X = ln.twonn_layers(n, all_twin)
    # layer -> (same cloud's distances, however the call orders its layers)
    key = [(n, True, 0), (n, False, 0)] if all_twin else [(n, False, 0), (n, False, 1)]
    v = [finite_ratios(twonn_dist(*k)) for k in key]
    if all_twin:
        assert v[0] == 0 and v[1] == n, (n, v)  # no finite ratio at all: NaN
    else:
        assert v[0] == n and 5 < v[1] < n - n // 4, (n, v)  # the twins and their originals drop out: padding inside pw2
    for discard in ln.TWONN_DISCARDS:
        res = gpu.ripser_batch(X, maxdim=0, persistence=False, twonn=True, discard_fraction=discard, slot=SLOT)
        assert len(res) == 2
        for l, k in enumerate(key):
            want, got = twonn_from_dist(twonn_dist(*k), discard), res[l].twonn
            print("twonn n=%d all_twin=%d layer %d discard %g: gpu %.9g ref %.9g rel %.3g" % (
                n, all_twin, l, discard, got, want, abs(got - want) / abs(want) if want == want and want else float("nan")))
            assert np.isnan(got) == np.isnan(want), (n, all_twin, l, discard, got, want)
            if all_twin and l == 0:
                assert np.isnan(want), (n, want)
            elif not np.isnan(want):
                assert abs(got - want) <= ln.TWONN_RTOL * abs(want), (n, all_twin, l, discard, got, want)
            if discard == 0.999 and n == ln.MAX_N and v[l] == n:
                assert max(int(v[l] * (1.0 - discard)), 5) > 5, (n, v[l])  # far from the clamp at 5
            assert len(res[l].dgms[0]) == 0  # no persistence in this call


TWONN_CASES = [(n, False) for n in ln.TWONN_NS] + [(n, True) for n in ln.TWONN_ALL_TWIN_NS]


@pytest.mark.parametrize("n,all_twin", [c for c in TWONN_CASES if c[0] < ln.MAX_N])
def test_twonn_more_than_one_trip(gpu, n, all_twin):
    """k_twonn's padding loop, bitonic sort and regression sums stride by its 1024 threads: one trip up to
    n = 1024, two from 1025, four from 2049, eight from 4097."""
    run_twonn(gpu, n, all_twin)


# ---------------------------------------------------------------- silhouette
def intra_inter(D, labels):
    """sklearn's mean intra-cluster and nearest mean inter-cluster distance of every sample (oracle.silhouette's steps)."""
    _, lab = np.unique(np.asarray(labels), return_inverse=True)
    n, freq = D.shape[0], np.bincount(lab)
    sums = np.stack([np.bincount(lab, weights=D[i], minlength=len(freq)) for i in range(n)])
    intra = sums[np.arange(n), lab]
    sums[np.arange(n), lab] = np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        return intra / (freq - 1)[lab], (sums / freq).min(axis=1)


def run_silhouette(gpu, n):
    from oracle import oracle

    X = ln.sil_layers(n)
    sets = ln.sil_label_sets(n, 7600000 + n)
    D = [oracle.distances(X[l]) for l in range(X.shape[0])]
    assert [len(np.unique(s)) for s in sets[:3]] == [2, 32, 31]
    assert sum((np.bincount(np.unique(sets[2], return_inverse=True)[1]) == 1)) == 3
    if n == 257:
        # a set whose only member in the second pass of 256 points is a cluster of its own
        assert len(sets) == 4 and (sets[3] == sets[3][256]).sum() == 1
        # and, on the box cloud, a sample with a = b = 0: its cluster and its nearest cluster lie on its own site
        sets.append(ln.zero_zero_labels(X[1], 7700000 + n))
        a, b = intra_inter(D[1], sets[4])
        assert ((a == 0) & (b == 0)).any()
    res = gpu.ripser_batch(X, maxdim=0, labels=sets, slot=SLOT)
    one_clean_attempt(gpu, ("silhouette", n))
    for l in range(X.shape[0]):
        assert len(res[l].silhouette) == len(sets)
        for s, lab in enumerate(sets):
            want, got = oracle.silhouette(D[l], lab), res[l].silhouette[s]
            print("silhouette n=%d layer %d set %d: gpu %.12g ref %.12g diff %.3g" % (n, l, s, got, want, abs(got - want)))
            assert abs(got - want) <= ln.SIL_ATOL, (n, l, s, got, want)
    plain = gpu.ripser_batch(X, maxdim=0, slot=SLOT)
    one_clean_attempt(gpu, ("no labels", n))
    for l in range(X.shape[0]):
        assert _pairs(res[l], 0) == _pairs(plain[l], 0) and len(_pairs(plain[l], 0)) > 1, (n, l)
        assert res[l].checksum == plain[l].checksum and res[l].num_edges == plain[l].num_edges, (n, l)
    return res


@pytest.mark.parametrize("n", ln.SIL_NS)
def test_silhouette_pass_border_and_mixed_k(gpu, n):
    """k_silhouette takes 256 points a pass: one pass at 255 and 256, a second of one point at 257, three at 513."""
    assert ln.sil_layers(n).shape[0] == ln.SIL_L
    run_silhouette(gpu, n)


# ---------------------------------------------------------------- H1 above 2048, and the refusals
def refused(gpu, n, maxdim, limit):
    with pytest.raises(NotImplementedError, match=str(limit)):
        gpu.ripser_batch(np.zeros((1, n, 3), np.float32), maxdim=maxdim, slot=SLOT)


@pytest.mark.parametrize("n,thresh", ln.H1_CASES)
def test_h1_above_2048(gpu, n, thresh):
    """H1 keys hold a 32-bit row-simplex index: at N = 2900 triangle indices reach 4.06e9, and 317 death
    triangles of the oracle's pairs lie at or above 2^31 -- a signed intermediate would lose them."""
    from oracle import oracle

    X = gpu.synthetic.torus(n, seed=0)
    o = oracle.rips(X, maxdim=1, thresh=thresh)
    assert o["n_all_pairs"][1] > 0 and o["n_adds"][1] > 0, (n, o["n_adds"])
    assert o["num_edges"] * 3 < n * (n - 1) // 2  # sparse: the threshold is what keeps the oracle at a second
    if n == ln.H1_LIMIT_N:
        assert (o["death_idx"][1] >= 2 ** 31).any(), int(o["death_idx"][1].max())
    res = gpu.ripser_batch(X[None], maxdim=1, thresh=thresh, slot=SLOT)
    one_clean_attempt(gpu, ("h1", n, thresh))
    assert_same(res[0], o, 1, ("h1", n, thresh))
    if n == ln.H1_LIMIT_N:
        refused(gpu, ln.H1_LIMIT_N + 1, 1, ln.H1_LIMIT_N)
    else:
        refused(gpu, ln.H2_LIMIT_N + 1, 2, ln.H2_LIMIT_N)


# ---------------------------------------------------------------- the cases at and next to N = 8192, last
@pytest.mark.parametrize("n,all_twin", [c for c in TWONN_CASES if c[0] == ln.MAX_N])
def test_twonn_at_the_limit(gpu, n, all_twin):
    """pw2 = 8192: the whole 32 KB of k_twonn's LDS attribute, eight trips; no padding on the normal layer."""
    run_twonn(gpu, n, all_twin)


def test_silhouette_at_the_limit(gpu):
    """K = 32 at n = 8192: 98,304 bytes of LDS, thirty-two passes.  The cloud is layer 0 of the H0 case."""
    res = run_silhouette(gpu, ln.SIL_BIG_N)
    X = ln.h0_layers(ln.SIL_BIG_N)
    assert np.array_equal(ln.sil_layers(ln.SIL_BIG_N)[0], X[0])
    assert_same(res[0], h0_refs(ln.SIL_BIG_N, X)[0], 0, "silhouette call's H0")


@pytest.mark.parametrize("n", H0_LAST)
def test_h0_four_chunks_to_the_limit(gpu, n):
    """8170: the last N with a chunk of 4096 keys (two chunks); 8171 .. 8192: four chunks of 2048, the last one short."""
    run_h0(gpu, n)
    if n == ln.MAX_N:
        for maxdim in (0, 1, 2):
            refused(gpu, ln.MAX_N + 1, maxdim, ln.MAX_N)
