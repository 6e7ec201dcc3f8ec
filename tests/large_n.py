"""The sizes above N = 2048 at which the pipeline's H0 and side-metric kernels change shape, and the
clouds, label sets and thresholds run there.

HIP-free (numpy only).  Three files import it:

* tests/test_rips_plan_cpu.py checks H0_BORDERS against the host plan program (h0_shape,
  csrc/rips_plan.h): the H0 shape of N = 65 .. 8192 changes in the fields below at exactly these N and
  takes these values at N - 1 and at N;
* tests/test_large_n.py runs the kernels at the sizes that follow from it and compares with the
  project's CPU references;
* tests/golden/make_golden_large_n.py records the oracle where it is too slow to run in a test.

So a constant that moves (kLdsMax, kH0BorWQ, kH0WaveMaxN, the pieces of k_h0's LDS carve) fails the
CPU test, which prints where the shape changes now: move H0_BORDERS there, and the GPU cases follow.
"""
import hashlib

import numpy as np

K_LDS_MAX = 160 * 1024         # csrc/rips_shapes.h kLdsMax: k_h0
BOR_HOOK_LDS_MAX = 150 * 1024  # k_bor_hook's dynamic LDS attribute
TWONN_LDS_MAX = 8192 * 4       # k_twonn's
SIL_LDS_MAX = 128 * 1024       # k_silhouette's
SIL_MAX_K, SIL_T, TWONN_T = 32, 256, 1024
ELDER_LDS, ELDER_WAVE, ELDER_SERIAL = 0, 1, 2  # csrc/rips_plan.h: which k_h0 instantiation runs the elder rule

# the fields of an H0 shape the borders are read from (tests/rips_plan_main.cpp prints them by these names):
# block size, the matrix staged in LDS, keys of the LDS sort chunk, the elder-rule variant
H0_FIELDS = ("T", "dlds", "ch", "elder")
H0_SCAN = (65, 8192)
# (first N of the new shape, {field: (value at N - 1, value at N)}): every N in 66 .. 8192 at which one of
# H0_FIELDS changes -- and k_h0's dynamic LDS on both sides (lds: bytes, not part of the scan)
H0_BORDERS = (
    (129, {"ch": (128, 256), "lds": (68944, 71028)}),  # the LDS path: the chunk just covers the forest (next_pow2(N))
    # off the LDS-staged matrix: the sort chunk is whatever fits beside the base, 16384 keys at most
    (191, {"T": (1024, 256), "dlds": (1, 0), "ch": (256, 16384), "elder": (ELDER_LDS, ELDER_WAVE), "lds": (149824, 134480)}),
    (257, {"T": (256, 1024), "lds": (135504, 135536)}),
    (1025, {"elder": (ELDER_WAVE, ELDER_SERIAL), "lds": (147792, 147824)}),  # 64 * kH0BorWQ: thread 0 runs the elder rule
    # the chunk halves where base + 8 ch passes kLdsMax; the last N of each chunk is 16 bytes below the limit
    (2027, {"ch": (16384, 8192), "lds": (163824, 98320)}),
    (6123, {"ch": (8192, 4096), "lds": (163824, 131088)}),
    (8171, {"ch": (4096, 2048), "lds": (163824, 147472)}),
)
# The forest has at most N - 1 keys, and block_sort merges in HBM only when they outgrow the chunk: never up to
# N = 6122 (the chunk is at least 8192 keys there), two chunks (one merge pass, then the copy back from the
# temporary buffer) for 6123 <= N <= 8170, four chunks with an uneven tail (two passes, the result lands in
# place) for 8171 <= N <= 8192.
H0_LDS_AT_8192, BOR_HOOK_LDS_AT_8192, SIL_LDS_AT_8192 = 147792, 131072, 98304


def h0_below(border):
    """The H0_FIELDS values of the shape at N = border - 1, read off H0_BORDERS."""
    state = {"T": 1024, "dlds": 1, "ch": 128, "elder": ELDER_LDS}  # N = 65
    for n, f in H0_BORDERS:
        if n >= border:
            break
        state.update({k: v[1] for k, v in f.items() if k in H0_FIELDS})
    return state


_ch = tuple(n for n, f in H0_BORDERS if "ch" in f and n > 191)  # 190 / 191 runs in tests/test_size_borders.py
_elder = tuple(n for n, f in H0_BORDERS if f.get("elder") == (ELDER_WAVE, ELDER_SERIAL))
# both sides of every chunk border and of the elder-rule switch; 4096 / 4097 / 4098 (the Borůvka rounds and
# k_twonn's pw2 step at 4097, 4097 keys at 4098); the limit and the size below it
H0_NS = tuple(sorted({m for n in _ch + _elder for m in (n - 1, n)} | {4096, 4097, 4098, 8191, 8192}))
H0_L = 2  # layer 0 a normal cloud, layer 1 a lattice cloud
# the oracle (one core) takes more than 5 s on two layers from here on: tests/golden/large_n_h0_<N>.npz
H0_GOLDEN_MIN_N = 4096
# The oracle on the two layers of each size (one core; edges at the enclosing radius; the lattice layer's finite
# pairs, zero-length forest edges and groups of equal deaths; the normal layer has N - 1 finite pairs):
#   1024  0.3 s    824 / 199 / 127        4098  6.7 s  8.2 M + 8.3 M edges  2,665 / 1,432 / 188
#   1025  0.3 s    825 / 199 / 125        6122  15.8 s  18.0 M + 18.6 M     3,807 / 2,314 / 204
#   2026  1.4 s  1,459 / 566 / 166        6123  17.8 s  18.4 M + 18.5 M     3,795 / 2,327 / 202
#   2027  1.4 s  1,463 / 563 / 170        8170  29.5 s  32.8 M + 33.0 M     4,895 / 3,274 / 200
#   4096  8.2 s  2,692 / 1,403 / 198      8171  about 28 s                  4,884 / 3,286 / 195
#   4097  7.7 s  2,676 / 1,420 / 194      8191  27.3 s  32.3 M + 33.4 M     4,905 / 3,285 / 197
#                                         8192  33.9 s  32.7 M + 33.2 M     4,914 / 3,277 / 206


def h0_seeds(n):
    return (7000000 + n, 7100000 + n)  # (normal, lattice)


# ---- clouds
def normal_cloud(n, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal((n, 3)) * scale).astype(np.float32)


def lattice_cloud(n, seed):
    """Integer coordinates: every other point in a box a few units wide (equal points and unit edges in
    plenty), the others spread forty units wide (integer squared lengths, each value many times over).
    The spanning forest has zero-length edges and hundreds of groups of equal deaths: the order
    (diameter ascending, index descending) within a group is what a merge gets wrong."""
    X = np.random.default_rng(seed).standard_normal((n, 3))
    return np.round(X * np.where(np.arange(n)[:, None] % 2 == 0, 2.0, 40.0)).astype(np.float32)


def box_cloud(n, seed, side=4):
    """Integer coordinates in a box of side^3 sites: at n > 2 side^3 some site holds three points or more."""
    return np.random.default_rng(seed).integers(0, side, (n, 3)).astype(np.float32)


def twin_cloud(n, seed, frac):
    """A normal cloud in which the last n // frac points are exact copies of the first: their nearest
    neighbour is at distance 0, so TwoNN has no finite ratio for them (nor for their originals).
    frac = 2: every point has a twin (at odd n the last point copies point 0 as well)."""
    X = normal_cloud(n, seed)
    k = n // frac
    X[n - k:] = X[:k]
    if frac == 2 and n % 2:
        X[k] = X[0]
    return X


def sha(X):
    return hashlib.sha256(np.ascontiguousarray(X).tobytes()).hexdigest()


def h0_layers(n, scale=1.0):
    s0, s1 = h0_seeds(n)
    return np.stack([normal_cloud(n, s0, scale), lattice_cloud(n, s1)])


def equal_death_groups(deaths):
    """Groups of two or more equal finite deaths in an H0 diagram."""
    d = np.asarray(deaths, dtype=np.float64)
    _, c = np.unique(d[np.isfinite(d)], return_counts=True)
    return int((c >= 2).sum())


LATTICE_MIN_GROUPS = 100

# ---- H0 with a finite threshold: the forest does not span, fewer than N - 1 keys are sorted.  One size on
# each side of the 6122 / 6123 chunk border (no merge / a merge of two chunks whose second is short).  The
# normal layer is scaled so that one threshold leaves both layers in pieces.
# (N, scale of the normal layer, thresh)
H0_THRESH_CASES = (
    # oracle, two layers (normal, lattice): 1.4 s each case
    (6122, 12.0, 6.0),  # edges 213,169 / 3,636,388; forest keys 6,025 / 4,266; finite pairs 6,025 / 1,952; essential 97 / 1,856
    (6123, 12.0, 6.0),  # edges 207,056 / 3,640,657; forest keys 6,029 / 4,241; finite pairs 6,029 / 1,914; essential 94 / 1,882
)
H0_THRESH_MIN_FINITE = 1000

# ---- TwoNN (persistence=False: distances and k_twonn alone), two layers a call
TWONN_NS = (1023, 1024, 1025, 2048, 2049, 4097, 8192)
TWONN_ALL_TWIN_NS = (1025, 8192)
TWONN_DISCARDS = (0.1, 0.0, 0.999)
TWONN_RTOL = 1e-5


def twonn_layers(n, all_twin=False):
    """(a normal cloud, one in which a third of the points are twins); all_twin: (every point has a
    twin -- NaN --, a normal cloud)."""
    if all_twin:
        return np.stack([twin_cloud(n, 7300000 + n, 2), normal_cloud(n, 7200000 + n)])
    return np.stack([normal_cloud(n, 7200000 + n), twin_cloud(n, 7300000 + n, 3)])


# ---- silhouette: several label sets a call
SIL_NS, SIL_L = (255, 256, 257, 513), 2
SIL_BIG_N = 8192  # one layer
SIL_ATOL = 1e-9


def sil_layers(n):
    """(a normal cloud, a box cloud: 64 sites, so equal points in every cluster); one normal layer at SIL_BIG_N,
    the H0 case's, whose oracle result is on file."""
    if n == SIL_BIG_N:
        return normal_cloud(n, h0_seeds(n)[0])[None]
    return np.stack([normal_cloud(n, 7400000 + n), box_cloud(n, 7500000 + n)])


def sil_label_sets(n, seed):
    """K = 2; K = 32 with shuffled codes; K = 31 of which three clusters are singletons; at n = 257 a
    fourth set whose only member past the first 256 points is a singleton cluster."""
    rng = np.random.default_rng(seed)
    two = rng.integers(0, 2, n)
    two[:2] = (0, 1)
    k32 = rng.permutation(np.arange(n) % 32)  # every code present
    k32 = rng.permutation(32)[k32] * 3 + 5    # labels are any sortable values: the encoder sorts them
    k31 = np.arange(n) % 28
    k31[rng.permutation(n)] = k31.copy()
    single = rng.choice(n, 3, replace=False)
    k31[single] = (28, 29, 30)
    assert len(np.unique(k31)) == 31 and all((k31 == c).sum() == 1 for c in (28, 29, 30))
    sets = [two, k32, k31]
    if n == 257:
        last = np.arange(n) % 7
        last[256] = 7
        sets.append(last)
    return sets


def zero_zero_labels(X, seed):
    """Labels on a cloud with at least three equal points p, q, r: {p, q} are one cluster and {r}
    another, so p's mean intra and its nearest mean inter distance are both 0 (sklearn: 0 / 0 -> 0)."""
    _, inv, cnt = np.unique(X, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    site = int(np.argmax(cnt >= 3))
    assert cnt[site] >= 3
    p, q, r = np.flatnonzero(inv == site)[:3]
    lab = 2 + np.random.default_rng(seed).integers(0, 5, X.shape[0])
    lab[[p, q]] = 0
    lab[r] = 1
    lab[np.flatnonzero(inv == site)[3:]] = 2
    return lab


# ---- H1 above N = 2048: (N, thresh) on synthetic.torus(N, seed 0), one layer; the row-simplex index of a
# key is 32 bits wide and C(2900, 3) = 4,061,193,700 < 2^32
# chosen like BIG_CASES of tests/size_borders.py: the oracle (one core) takes about a second and adds columns in H1
H1_CASES = (
    (2049, 1.2),  # 1.12 s; 151,514 of 2,098,176 edges; pairs 2,048 / 149,464 (574 emitted); column additions 20,898
    # 317 of the emitted pairs die at a triangle index >= 2^31 (the largest 4,059,955,638)
    (2900, 0.7),  # 1.02 s; 95,636 of 4,203,550 edges; pairs 2,899 / 92,735 (821 emitted); column additions 11,030
)
H1_LIMIT_N, H2_LIMIT_N, MAX_N = 2900, 2048, 8192
