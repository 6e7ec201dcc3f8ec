"""Bootstrap confidence bands for persistence diagrams on the GPU (include/tda_rips.h tda_resample).

Which bars of a diagram are signal?  The bootstrap answer (Fasy et al. 2014, Chazal et al. 2014):
resample the cloud B times, take the (1 - alpha) quantile of a statistic that bounds how far a
diagram moves under resampling, and call a bar significant when its persistence exceeds twice that
radius -- the bars that no diagram within the radius could have at the diagonal.

The statistic here is ``2 * H(X, X*)``, H the Hausdorff distance between the cloud and the
resample.  For the Rips filtration parameterised by the diameter (as here and in ripser),
``d_B(dgm(X), dgm(X*)) <= 2 d_GH(X, X*) <= 2 H(X, X*)`` (Chazal, de Silva and Oudot 2014), in every
dimension: the band is never narrower than the one the bottleneck distances themselves would give
on the same resamples, and it needs no persistence of the resamples at all.

The resampling stage runs where the distances already lie.  One ``tda_resample`` call computes the
layers' distance matrices on the device (the kernels of ``ripser_batch``) and every resample's
Hausdorff distance from them.  The kernel copies and compares f32 distances, never computes one:
every value here is exact and bit-reproducible.

Not here yet: the bottleneck statistic itself (persistence of every resample, then the bottleneck
entry), which would drive the persistence pipeline and the bottleneck entry in one process
(known limits).
"""
from __future__ import annotations

import math

import numpy as np

from . import _cloud, _lib
from ._cloud import check_count as _check_count
from .ripser import _arr, _check_common, ripser_batch

METHODS = ("hausdorff",)


def resample_indices(N: int, B: int, m=None, replace: bool = True, seed: int = 0) -> np.ndarray:
    """B resamples of m of N points: a (B, m) int32 table of indices into 0 .. N-1, drawn with
    ``numpy.random.default_rng(seed)`` (the same seed gives the same table).  ``m`` defaults to N;
    ``replace=False`` draws every row without repetition and needs m <= N."""
    N, B = _check_count("N", N), _check_count("B", B)
    m = N if m is None else _check_count("m", m)
    rng = np.random.default_rng(seed)
    if replace:
        return rng.integers(0, N, size=(B, m), dtype=np.int32)
    if m > N:
        raise ValueError(f"replace=False needs m <= N, got m = {m}, N = {N}")
    return np.ascontiguousarray(rng.permuted(np.tile(np.arange(N, dtype=np.int32), (B, 1)), axis=1)[:, :m])


def _check_idx(idx, L: int, N: int) -> np.ndarray:
    """idx as a contiguous int32 (B, m) or (L, B, m) table of indices into 0 .. N-1."""
    return _cloud.check_table(idx, None, L, N)[0]


def _hausdorff(inp: _cloud.CloudInput, idx: np.ndarray):
    """One tda_resample call: ((L, B) float64 holding f32 values, device ms)."""
    a = _lib.ResampleArgs()
    _cloud.fill_table_head(a, inp, idx)
    with _lib.result("resample", a) as r:
        return _arr(r.hausdorff, inp.L * int(a.B), np.float32).reshape(inp.L, int(a.B)).astype(np.float64), float(r.device_ms)


def hausdorff_resamples(X, idx, distance_matrix: bool = False, device: int = 0) -> np.ndarray:
    """Hausdorff distance between each layer's cloud and each of its resamples, one library call.

    X: (L, N, D) float32 point clouds or (L, N, N) distance matrices (distance_matrix=True; upper
    triangle used, diagonal taken as 0), numpy or a torch CUDA tensor; N <= 8192.  idx: a (B, m)
    integer table of indices into 0 .. N-1 shared by every layer (:func:`resample_indices`), or
    (L, B, m) for a table per layer; m <= 8192 and L * B <= 2^27.  Returns the (L, B) float64 array
    (holding f32 values) ``H[l, b] = max_i min_j dm[l][idx[b][j]][i]`` on the library's own f32
    distance matrix ``dm`` (what ``ripser_batch(X, want_dist=True)`` returns as ``dist``): every
    value is copied from it, so it equals ``dm[l][idx[b]].min(0).max()`` exactly."""
    inp = _cloud.table_input(X, distance_matrix, device)
    return _hausdorff(inp, _check_idx(idx, inp.L, inp.N))[0]


def quantile_rank(B: int, alpha: float) -> int:
    """The rank k = ceil((1 - alpha) * B), evaluated in float64 and kept within 1 .. B: the
    (1 - alpha) quantile of B statistics is their k-th smallest."""
    return min(max(math.ceil((1.0 - float(alpha)) * int(B)), 1), int(B))


def order_quantile(stat, alpha: float) -> np.ndarray:
    """The (1 - alpha) quantile along the last axis as an order statistic: the
    :func:`quantile_rank`-th smallest value, one of the inputs, never interpolated."""
    stat = np.asarray(stat, dtype=np.float64)
    return np.sort(stat, axis=-1)[..., quantile_rank(stat.shape[-1], alpha) - 1]


class ConfidenceBands:
    """Bootstrap confidence bands of L layers (:func:`confidence_bands`).

    ``results``: the L :class:`LayerResult` of the full clouds.  ``stat`` (len(dims), L, B)
    float64: the statistic of every resample; ``quantile`` (len(dims), L): its (1 - alpha) order
    statistic; ``radius`` = ``quantile``: the band's half-width in bottleneck distance.
    ``significant[l][k]``: a bool mask over ``results[l].dgms[dims[k]]``, True where the
    persistence exceeds ``2 * radius[k, l]`` (essential bars always); ``n_significant``
    (len(dims), L) int64 counts them.  ``idx``: the int32 index table used; ``method``: as given."""

    __slots__ = ("results", "stat", "quantile", "radius", "significant", "n_significant", "idx", "method")


def confidence_bands(X, B: int = 1000, alpha: float = 0.05, method: str = "hausdorff", maxdim: int = 1, dims=None, m=None,
                     replace: bool = True, seed: int = 0, idx=None, thresh: float = np.inf, distance_matrix: bool = False,
                     device: int = 0) -> ConfidenceBands:
    """Bootstrap confidence bands for the persistence diagrams of L layers.

    X: (L, N, D) float32 point clouds or (L, N, N) distance matrices, numpy or a torch CUDA
    tensor.  The B resamples of m points (default N) are ``resample_indices(N, B, m, replace,
    seed)``, shared by every layer, or the given ``idx`` ((B, m) or (L, B, m); B and m are then
    its).  ``dims`` (default 0 .. maxdim) are the diagram dimensions to band.

    method="hausdorff" (the one implemented; "bottleneck" raises NotImplementedError):
    ``stat[k, l, b] = 2 * H(X_l, X_l*)`` for every k, H the Hausdorff distance between the cloud
    and the resample; no persistence of the resamples.  By ``d_B <= 2 d_GH <= 2 H`` for the
    diameter-parameterised Rips filtration (Chazal, de Silva and Oudot 2014) every diagram of a
    resample lies within ``stat`` of the full cloud's in bottleneck distance, so this band is never
    narrower than the one of the bottleneck distances on the same ``idx``.
    ``quantile`` is the ceil((1 - alpha) * B)-th smallest statistic (:func:`order_quantile`: an
    order statistic, no interpolation), ``radius = quantile``, and a bar is ``significant`` when
    its persistence exceeds ``2 * radius`` (essential bars are).  Every output is a value of the
    input's f32 distances, copied, compared, subtracted or doubled exactly, so a call is
    bit-reproducible.  One ``ripser_batch`` call on the full clouds and one ``tda_resample`` call.
    Returns a :class:`ConfidenceBands`."""
    _check_common(maxdim, 2, False, None, "euclidean")
    alpha = float(alpha)
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"alpha must be in (0, 1), got {alpha}")
    if method == "bottleneck":
        raise NotImplementedError('method="bottleneck" is not implemented: it needs the persistence pipeline and the bottleneck '
                                  'entry in one process (DESIGN.md, known limits); method="hausdorff" bounds it')
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    dims = list(range(int(maxdim) + 1)) if dims is None else [int(d) for d in dims]
    if not dims or any(not 0 <= d <= maxdim for d in dims):
        raise ValueError(f"dims must be dimensions in 0 .. maxdim = {maxdim}, got {dims}")
    if idx is None:
        B = _check_count("B", B)
        m = None if m is None else _check_count("m", m)
    inp = _cloud.table_input(X, distance_matrix, device)
    L, N = inp.L, inp.N
    idx = resample_indices(N, B, m, replace, seed) if idx is None else _check_idx(idx, L, N)
    B = int(idx.shape[-2])

    results = ripser_batch(inp.keep, maxdim=maxdim, thresh=thresh, distance_matrix=inp.is_dist, device=inp.device)
    stat = np.empty((len(dims), L, B), dtype=np.float64)
    stat[:] = 2.0 * _hausdorff(inp, idx)[0]

    cb = ConfidenceBands()
    cb.results, cb.stat, cb.idx, cb.method = results, stat, idx, method
    cb.quantile = order_quantile(stat, alpha)
    cb.radius = cb.quantile.copy()
    cb.significant = []
    cb.n_significant = np.zeros((len(dims), L), dtype=np.int64)
    for l, r in enumerate(results):
        masks = []
        for k, d in enumerate(dims):
            dg = r.dgms[d]
            sig = ~np.isfinite(dg[:, 1]) | (dg[:, 1] - dg[:, 0] > 2.0 * cb.radius[k, l])
            masks.append(sig)
            cb.n_significant[k, l] = int(np.count_nonzero(sig))
        cb.significant.append(masks)
    return cb
