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

import numpy as np

from . import _cloud, _lib
from ._cloud import check_count as _check_count, check_table as _check_table
from .ripser import _arr


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


def _check_alpha(alpha) -> float:
    alpha = float(alpha)
    if not np.isfinite(alpha) or alpha <= 0.0:
        raise ValueError(f"alpha must be finite and > 0, got {alpha}")
    return alpha


def _subsample_h0(inp: _cloud.CloudInput, idx: np.ndarray, sizes: np.ndarray, alpha: float, want_deaths: bool):
    """One tda_subsample_h0 call: ((L, B) float64, (L, B, m - 1) float32 or None, device ms)."""
    a = _lib.SubsampleH0Args()
    _cloud.fill_table_head(a, inp, idx)
    a.sizes = sizes.ctypes.data
    a.alpha = alpha
    a.want_deaths = 1 if want_deaths else 0
    with _lib.result("sh0", a) as r:
        B, m = int(a.B), int(a.m)
        E = _arr(r.E, inp.L * B, np.float64).reshape(inp.L, B).copy()
        d = _arr(r.deaths, inp.L * B * (m - 1), np.float32).reshape(inp.L, B, m - 1) if want_deaths else None
        return E, d, float(r.device_ms)


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
    inp = _cloud.table_input(X, distance_matrix, device)
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
    inp = _cloud.table_input(X, distance_matrix, device)
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
