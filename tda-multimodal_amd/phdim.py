"""The persistent-homology dimension on the GPU (include/tda_rips.h tda_subsample_h0).

A topological estimate of intrinsic dimension beside TwoNN and the effective dimensionality (Adams
et al. 2020, "A fractal dimension for measures via persistent homology"; Birdal et al. 2021,
"Intrinsic dimension, persistent homology and generalization in neural networks").  For a subsample
of n points of a cloud, the H0 deaths are the edge weights of its minimum spanning tree and
``E_alpha(n)`` is the sum of their alpha-th powers.  For a d-dimensional measure ``E_alpha(n)``
grows like ``n^((d - alpha) / d)``, so with ``s`` the slope of ``log E_alpha(n)`` against ``log n``
the dimension is ``alpha / (1 - s)``.

The H0 persistence of every subsample of every layer is one ``tda_subsample_h0`` call: the layers'
distance matrices on the device (the kernels of ``ripser_batch``), then Prim's algorithm over the
index table where the distances lie.  A death is an f32 distance, copied and compared, never
computed; ``E`` is a float64 sum in step order, for alpha 1 and 2 bit for bit a sequential loop.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .bootstrap import _check_count, _Input
from .ripser import _arr, _data_ptrs


def subsample_indices(N: int, sizes, n_trials: int, seed: int = 0):
    """Subsamples without repetition of N points: for every size n in ``sizes`` in the given order,
    then for each of ``n_trials`` trials, ``rng.permutation(N)[:n]`` from one
    ``rng = numpy.random.default_rng(seed)`` (this draw order is part of the contract).  Returns
    ``(idx, sz)``: the int32 (B, max(sizes)) table, rows padded with 0, and the int32 (B,) sizes,
    B = len(sizes) * n_trials."""
    N, n_trials = _check_count("N", N), _check_count("n_trials", n_trials)
    sizes = [_check_count("a size", n) for n in np.asarray(sizes).reshape(-1).tolist()]
    if not sizes or max(sizes) > N:
        raise ValueError(f"sizes must be a non-empty list of sizes in 1 .. N = {N}, got {sizes}")
    rng = np.random.default_rng(seed)
    idx = np.zeros((len(sizes) * n_trials, max(sizes)), dtype=np.int32)
    sz = np.repeat(np.asarray(sizes, dtype=np.int32), n_trials)
    for b, n in enumerate(sz.tolist()):
        idx[b, :n] = rng.permutation(N)[:n]
    return idx, sz


def _check_table(idx, sizes, L: int, N: int):
    """idx as a contiguous int32 (B, m) or (L, B, m) table and sizes as int32 (B,): 1 <= sizes[b] <= m
    and the first sizes[b] entries of every row are indices into 0 .. N-1 (the rest is never read)."""
    idx = np.asarray(idx)
    if idx.dtype.kind not in "iu":
        raise ValueError(f"idx must hold integers, got dtype {idx.dtype}")
    if idx.ndim not in (2, 3) or idx.size == 0:
        raise ValueError(f"idx must be a non-empty (B, m) or (L, B, m) table, got shape {idx.shape}")
    if idx.ndim == 3 and idx.shape[0] != L:
        raise ValueError(f"a per-layer idx must be (L = {L}, B, m), got shape {idx.shape}")
    B, m = int(idx.shape[-2]), int(idx.shape[-1])
    sizes = np.full(B, m, dtype=np.int32) if sizes is None else np.asarray(sizes)
    if sizes.dtype.kind not in "iu" or sizes.shape != (B,):
        raise ValueError(f"sizes must hold B = {B} integers, got dtype {sizes.dtype}, shape {sizes.shape}")
    if sizes.min() < 1 or sizes.max() > m:
        raise ValueError(f"sizes must lie in 1 .. m = {m}, got {int(sizes.min())} .. {int(sizes.max())}")
    used = idx[..., np.arange(m)[None, :] < sizes[:, None]]
    if used.min() < 0 or used.max() >= N:
        raise ValueError(f"idx must hold indices into 0 .. N-1 = {N - 1}, got {int(used.min())} .. {int(used.max())}")
    unused = np.arange(m)[None, :] >= sizes[:, None]
    if idx.dtype != np.int32 and unused.any():  # what is never read need not fit int32
        idx = np.where(unused, 0, idx)
    return np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(sizes, dtype=np.int32)


def _check_alpha(alpha) -> float:
    alpha = float(alpha)
    if not np.isfinite(alpha) or alpha <= 0.0:
        raise ValueError(f"alpha must be finite and > 0, got {alpha}")
    return alpha


def _subsample_h0(inp: _Input, idx: np.ndarray, sizes: np.ndarray, alpha: float, want_deaths: bool):
    """One tda_subsample_h0 call: ((L, B) float64, (L, B, m - 1) float32 or None, device ms)."""
    a = _lib.SubsampleH0Args()
    a.x = _data_ptrs([inp.keep], inp.on_dev)[0]
    a.dtype = _lib.TDA_F64 if inp.is64 else _lib.TDA_F32
    a.x_on_device = 1 if inp.on_dev else 0
    a.L, a.N, a.D = inp.L, inp.N, inp.D
    a.is_dist = 1 if inp.is_dist else 0
    a.device = inp.device
    a.stream = (inp.stream or None) if inp.on_dev else None
    a.B, a.m = int(idx.shape[-2]), int(idx.shape[-1])
    a.idx_per_layer = 1 if idx.ndim == 3 else 0
    a.idx, a.sizes = idx.ctypes.data, sizes.ctypes.data
    a.alpha = alpha
    a.want_deaths = 1 if want_deaths else 0
    L = _lib.lib()
    res = ctypes.POINTER(_lib.SubsampleH0Result)()
    _lib.check(L.tda_subsample_h0(ctypes.byref(a), ctypes.byref(res)))
    try:
        r = res.contents
        B, m = int(a.B), int(a.m)
        E = _arr(r.E, inp.L * B, np.float64).reshape(inp.L, B).copy()
        d = _arr(r.deaths, inp.L * B * (m - 1), np.float32).reshape(inp.L, B, m - 1) if want_deaths else None
        return E, d, float(r.device_ms)
    finally:
        L.tda_subsample_h0_free(res)


def h0_subsamples(X, idx, sizes=None, alpha: float = 1.0, deaths: bool = False, distance_matrix: bool = False, device: int = 0):
    """H0 persistence of subsamples of every layer, one library call.

    X: (L, N, D) float32 point clouds or (L, N, N) distance matrices (distance_matrix=True; upper
    triangle used, diagonal taken as 0; host matrices must be finite), numpy or a torch CUDA
    tensor; N <= 8192.  idx: a (B, m) integer table shared by every layer
    (:func:`subsample_indices`), or (L, B, m) for a table per layer; sizes: (B,) integers, subsample
    b is the first ``sizes[b]`` entries of row b (default: every row whole; the rest of a row is
    never read); m <= 8192 and L * B <= 2^27.  Returns ``E``, (L, B) float64: ``E[l, b]`` is the sum
    over the subsample's H0 deaths ``w`` (the edge weights of its minimum spanning tree on the
    library's own f32 distances) of ``w ** alpha``, added in float64 in the order Prim's algorithm
    from position 0 finds them (the lowest position wins ties): for alpha 1 and 2 bit for bit a
    sequential loop.  With ``deaths=True`` returns ``(E, D)``, ``D[l][b]`` the float64 array
    (holding f32 values) of the ``sizes[b] - 1`` deaths in that order; sorted, they are the finite
    H0 deaths of ripser on the subsample."""
    alpha = _check_alpha(alpha)
    inp = _Input(X, distance_matrix, device)
    idx, sizes = _check_table(idx, sizes, inp.L, inp.N)
    E, d, _ = _subsample_h0(inp, idx, sizes, alpha, bool(deaths))
    if not deaths:
        return E
    return E, [[d[l, b, :n - 1].astype(np.float64) for b, n in enumerate(sizes.tolist())] for l in range(inp.L)]


class PHDimension:
    """The persistent-homology dimension of L layers (:func:`ph_dimension`).

    ``dimension`` (L,) float64: ``alpha / (1 - slope)``, nan for a layer with any ``E <= 0``;
    ``slope`` and ``intercept`` (L,): the least-squares line of ``log E`` against ``log sizes``
    over all B subsamples; ``E`` (L, B) float64; ``sizes`` (B,) int32; ``idx``: the int32 index
    table used; ``alpha``: as given; ``device_ms``: the device time of the library call."""

    __slots__ = ("dimension", "slope", "intercept", "E", "sizes", "idx", "alpha", "device_ms")


def default_sizes(N: int) -> np.ndarray:
    """The default subsample sizes of :func:`ph_dimension`: ten sizes from N / 4 to N, rounded,
    distinct, at least 2."""
    s = np.unique(np.round(np.linspace(N / 4, N, 10)).astype(int))
    return s[s >= 2]


def ph_dimension(X, alpha: float = 1.0, sizes=None, n_trials: int = 8, seed: int = 0, idx=None, distance_matrix: bool = False,
                 device: int = 0) -> PHDimension:
    """The persistent-homology dimension of every layer.

    X as for :func:`h0_subsamples`.  The subsamples are ``subsample_indices(N, sizes, n_trials,
    seed)``, shared by every layer (default ``sizes``: :func:`default_sizes`; fewer than two
    distinct sizes raise ValueError), or the given ``idx`` ((B, m) or (L, B, m)) with ``sizes``
    then the (B,) sizes of its rows.  ``log E_alpha`` is fitted against ``log n`` by ordinary
    least squares in float64 over all B subsamples of a layer, trials not averaged, and
    ``dimension = alpha / (1 - slope)``; a layer with any ``E <= 0`` (a subsample of one point, or
    of coincident points) gets nan.  One ``tda_subsample_h0`` call.  Returns a :class:`PHDimension`."""
    alpha = _check_alpha(alpha)
    if idx is None:
        n_trials = _check_count("n_trials", n_trials)
    inp = _Input(X, distance_matrix, device)
    if idx is None:
        sizes = default_sizes(inp.N) if sizes is None else np.asarray(sizes).reshape(-1)
        if len(np.unique(sizes)) < 2:
            raise ValueError(f"the regression needs at least two distinct subsample sizes, got {np.asarray(sizes).tolist()} (N = {inp.N})")
        idx, sz = subsample_indices(inp.N, sizes, n_trials, seed)
    else:
        idx, sz = _check_table(idx, sizes, inp.L, inp.N)
        if len(np.unique(sz)) < 2:
            raise ValueError(f"the regression needs at least two distinct subsample sizes, got {np.unique(sz).tolist()}")
    E, _, ms = _subsample_h0(inp, idx, sz, alpha, False)

    x = np.log(sz.astype(np.float64))
    xc = x - x.mean()
    ph = PHDimension()
    ph.E, ph.sizes, ph.idx, ph.alpha, ph.device_ms = E, sz, idx, alpha, ms
    ph.slope = np.full(inp.L, np.nan)
    ph.intercept = np.full(inp.L, np.nan)
    for l in range(inp.L):
        if (E[l] > 0.0).all():
            y = np.log(E[l])
            ph.slope[l] = float((xc * (y - y.mean())).sum() / (xc * xc).sum())
            ph.intercept[l] = float(y.mean() - ph.slope[l] * x.mean())
    with np.errstate(divide="ignore", invalid="ignore"):
        ph.dimension = alpha / (1.0 - ph.slope)
    return ph
