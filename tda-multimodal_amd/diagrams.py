"""Distances between persistence diagrams, and their vectorisations, on the GPU (include/tda_dgm.h).

The reference imports ``persim`` next to ``ripser`` and uses it for
``plot_diagrams`` only; comparing the diagrams of a sweep (layer against layer,
condition against condition) needs a distance.  ``sliced_wasserstein`` has
persim's signature and semantics [upstream ``persim.sliced_wasserstein(PD1,
PD2, M=50)``]; ``sliced_wasserstein_matrix`` is the sweep-level form: every
pair of a list of diagrams in one library call.

    SW(A, B) = (1/pi) * sum_i (pi/M) * sum_k |sort(V1_i)[k] - sort(V2_i)[k]|

over M directions of the half circle, V1_i / V2_i the projections of each
diagram's points joined with the other's diagonal projections (tda_dgm.h has
the full definition).  Everything is float64; points with a non-finite
coordinate (the essential classes) are dropped first.  Per pair the two
diagrams may hold 4096 finite points together, and 1 <= M <= 1024.

``bottleneck`` has persim's signature too [upstream ``persim.bottleneck(dgm1,
dgm2, matching=False)``] and ``bottleneck_matrix`` is its sweep-level form.  It
is the distance of the stability theorem,

    d_B(A, B) = min over partial matchings of the largest cost paid,

a matched pair paying max(|b_p - b_q|, |d_p - d_q|) and an unmatched point its
distance to the diagonal |d - b| / 2, so that d_B(A, empty) is half of A's
maximum persistence.  The value is exact (one of those costs, bit for bit) and
a diagram may hold 512 finite points.

``wasserstein`` is ``persim.wasserstein(dgm1, dgm2, matching=False)`` [upstream]
and ``wasserstein_matrix`` its sweep-level form: the optimal-transport distance
in which every bar counts,

    W(A, B) = min over partial matchings of the sum of the costs paid,

a matched pair paying its Euclidean distance and an unmatched point its L2
distance to the diagonal (d - b) / sqrt(2).  The solver is exact up to the
rounding of its float64 duals (tda_dgm.h states the bounds); the matching can
be returned, and a diagram may hold 512 finite points.

``heat`` is ``persim.heat(dgm1, dgm2, sigma=0.4)`` [upstream], the distance of the
persistence scale-space kernel (Reininghaus et al. 2015); ``heat_matrix`` is its
sweep-level form and ``heat_kernel_matrix`` the kernel's Gram matrix, which is
positive semi-definite: the one distance here that kernel PCA, an SVM or an MMD
test can use as it is.  A double sum of exponentials, summed in an order that the
two point counts alone decide; a diagram may hold 4096 finite points.

``fisher`` is the persistence Fisher distance (Le and Yamada 2018; gudhi's
``PersistenceFisherDistance`` [upstream]), ``fisher_matrix`` its sweep-level form and
``fisher_kernel_matrix`` the kernel ``exp(-fisher / bandwidth)``: both diagrams smoothed
into densities on a common support, and the geodesic distance between them on the sphere.
Bounded by pi / 2 and not dominated by a few long bars; 4 (n1 + n2)^2 exponentials per
pair, a diagram may hold 1024 finite points.

``persistence_curves`` sums one term per point on a grid of filtration values (Chung and
Lawson 2019): ``betti_curves``, ``lifespan_curves``, ``entropy_curves`` and
``persistence_silhouettes`` are its named forms, the functions of the radius a layer study
plots.  Every value equals a numpy loop over the points in row order, bit for bit.

``persistence_landscapes`` and ``persistence_images`` are the two standard
vectorisations [upstream ``persim.landscapes``, ``persim.PersistenceImager``]:
one fixed-length vector per diagram, linear in the number of diagrams, no
matching, up to 4096 finite points per diagram.  The landscape is exact on its
grid; the image carries a derived error bound (tda_dgm.h).
"""
from __future__ import annotations

import ctypes
import warnings

import numpy as np

from . import _lib
from .ripser import LayerResult


def _check_M(M) -> int:
    if isinstance(M, bool) or int(M) != M:
        raise ValueError("M must be an integer")
    if M < 1:
        raise ValueError("M must be >= 1")
    if M > _lib.TDA_SW_MAX_DIRECTIONS:
        raise NotImplementedError(f"M > {_lib.TDA_SW_MAX_DIRECTIONS} directions is not supported")
    return int(M)


def _flatten(dgms, dim: int):
    """(points (total, 2) float64, offsets (S + 1,) int64) of a list of diagrams."""
    dgms = list(dgms)
    S = len(dgms)
    if S and all(isinstance(r, LayerResult) for r in dgms):
        b = dgms[0]._b
        if not 0 <= dim < b.nd:
            raise ValueError(f"dim = {dim}: the results hold dimensions 0 .. {b.nd - 1}")
        if all(r._b is b for r in dgms):
            # one batch: gather from its shared arrays, no per-layer work (pipeline.pack_results)
            ls = np.fromiter((r._l for r in dgms), dtype=np.int64, count=S)
            cnt, off = b.cnt[ls, dim].astype(np.int64), b.off[ls, dim].astype(np.int64)
            offsets = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
            rows = np.repeat(off - offsets[:-1], cnt) + np.arange(int(offsets[-1]))
            return np.ascontiguousarray(b.pairs[rows], dtype=np.float64).reshape(-1, 2), offsets
        dgms = [r.dgms[dim] for r in dgms]
    arrs = []
    for d in dgms:
        if isinstance(d, LayerResult):
            raise ValueError("a list of diagrams holds either arrays or LayerResults, not both")
        d = np.asarray(d, dtype=np.float64)
        if d.size == 0:
            d = d.reshape(0, 2)
        if d.ndim != 2 or d.shape[1] != 2:
            raise ValueError(f"a diagram must be an (n, 2) array of (birth, death), got shape {d.shape}")
        arrs.append(d)
    offsets = np.concatenate([[0], np.cumsum([len(d) for d in arrs])]).astype(np.int64)
    points = np.concatenate(arrs) if arrs else np.zeros((0, 2))
    return np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2), offsets


def _finite_counts(points, offsets):
    fin = np.isfinite(points).all(axis=1)
    c = np.concatenate([[0], np.cumsum(fin)])
    return c[offsets[1:]] - c[offsets[:-1]], int(len(fin) - c[-1])


# What a call is measured by against its entry's limit, from the finite counts of its S (+ S2) diagrams.
def _top_diagram(cnt, S, S2, block):
    """The largest diagram of the call (the heat kernel, the vectorisations)."""
    return cnt.max() if len(cnt) else 0


def _top_paired_diagram(cnt, S, S2, block):
    """The largest diagram of a call that holds a pair (bottleneck, Wasserstein)."""
    return cnt.max() if (S and S2 if block else S >= 2) else 0


def _top_pair(cnt, S, S2, block):
    """The two largest diagrams together or, with ``other``, the largest of each side (sliced Wasserstein)."""
    if block:
        return (cnt[:S].max() + cnt[S:].max()) if S and S2 else 0
    return np.sort(cnt)[-2:].sum() if S >= 2 else 0


def _inputs(dgms, other, dim: int, limit: int, top=_top_diagram, holds="a diagram holds {} finite points"):
    """(points, offsets, pairs or None, S, S') of a call on ``dgms`` or, with ``other``, on both lists
    and the pairs of the (S, S') block; the entry's limit checked (``top``: what is measured against
    it, ``holds``: how the refusal names it) and the non-finite points reported, before any library call."""
    pts, off = _flatten(dgms, dim)
    S = S2 = len(off) - 1
    pairs = None
    if other is not None:
        pts2, off2 = _flatten(other, dim)
        S2 = len(off2) - 1
        pts, off = np.concatenate([pts, pts2]), np.concatenate([off, off[-1] + off2[1:]])
        pairs = np.stack(np.meshgrid(np.arange(S), S + np.arange(S2), indexing="ij"), -1).reshape(-1, 2).astype(np.int32)
    cnt, dropped = _finite_counts(pts, off)
    n = top(cnt, S, S2, other is not None)
    if n > limit:
        raise NotImplementedError(f"{holds.format(int(n))}: more than {limit} is not supported")
    if dropped:
        warnings.warn(f"the diagrams hold {dropped} points with a non-finite coordinate; ignoring those points")
    return pts, off, pairs, S, S2


def _matrix(values, S: int, S2: int, block: bool):
    """The (S, S') block of a call with ``other``, or the symmetric (S, S) matrix with a zero diagonal."""
    if block:
        return values.reshape(S, S2)
    D = np.zeros((S, S))
    D[np.triu_indices(S, 1)] = values  # row-major i < j: the order of the library's all-pairs result
    return D + D.T


def _library_call(entry: str, points, offsets, pairs, read, **fields):
    """One call of an entry of tda_dgm.h (_lib.DGM_ENTRIES): the common fields and ``fields`` set, the
    return code checked; returns ``read(result struct)`` (owned arrays: _owned) and frees the result."""
    a = _lib.DGM_ENTRIES[entry][2]()
    a.points = points.ctypes.data if len(points) else None
    a.offsets = offsets.ctypes.data
    a.S = len(offsets) - 1
    if pairs is not None:
        a.pairs, a.P = pairs.ctypes.data, len(pairs)
    for name, value in fields.items():
        setattr(a, name, value)
    with _lib.result(entry, a) as r:
        return read(r)


def _owned(p, n: int, dtype=np.float64):
    """n values at the result's pointer p, copied: they outlive the result."""
    return np.frombuffer(ctypes.string_at(p, n * np.dtype(dtype).itemsize), dtype=dtype).copy() if n else np.zeros(0, dtype)


def _no_pair(offsets, pairs) -> bool:
    return len(offsets) < 3 if pairs is None else not len(pairs)


def _call_dist(entry: str, points, offsets, pairs, **fields):
    """One tda_sliced_wasserstein or tda_bottleneck call: (dist (P,), device_ms)."""
    if _no_pair(offsets, pairs):  # nothing to launch
        return np.zeros(0), 0.0
    return _library_call(entry, points, offsets, pairs, lambda r: (_owned(r.dist, r.P), float(r.device_ms)), **fields)


def sliced_wasserstein_matrix(dgms, M: int = 50, other=None, device: int = 0, dim: int = 1, return_time: bool = False):
    """Sliced Wasserstein distances between every pair of diagrams, one library call.

    dgms: a list of (n, 2) arrays of (birth, death), or a list of
    :class:`LayerResult` (then diagram ``dim`` of each is taken; the results of
    one ``ripser_batch`` call are gathered from the batch's shared arrays).
    other: a second such list.  Returns the (S, S) float64 matrix of ``dgms``
    against itself -- symmetric, zero diagonal -- or the (S, S') matrix of
    ``dgms`` against ``other``; with ``return_time`` also the call's device
    time in ms.  A pair's value is the same bits in any call that holds it."""
    M = _check_M(M)
    pts, off, pairs, S, S2 = _inputs(dgms, other, dim, _lib.TDA_SW_MAX_POINTS, _top_pair, "a pair of diagrams holds {} finite points together")
    dist, ms = _call_dist("sw", pts, off, pairs, M=M, device=int(device))
    D = _matrix(dist, S, S2, other is not None)
    return (D, ms) if return_time else D


def sliced_wasserstein(PD1, PD2, M: int = 50, device: int = 0) -> float:
    """``persim.sliced_wasserstein(PD1, PD2, M=50)`` [upstream] on the GPU: the
    sliced Wasserstein distance of two (n, 2) diagrams over M directions.
    Points with a non-finite coordinate are ignored, with a warning."""
    for d in (PD1, PD2):
        if isinstance(d, LayerResult):
            raise ValueError("PD1 and PD2 are (n, 2) arrays (for LayerResults: sliced_wasserstein_matrix)")
    return float(sliced_wasserstein_matrix([PD1], M=M, other=[PD2], device=device)[0, 0])


def bottleneck_matrix(dgms, other=None, device: int = 0, dim: int = 1, return_time: bool = False):
    """Bottleneck distances between every pair of diagrams, one library call.

    The arguments and the result are those of :func:`sliced_wasserstein_matrix`
    (without M): ``dgms`` and ``other`` are lists of (n, 2) arrays or of
    :class:`LayerResult`; the (S, S) matrix is symmetric with a zero diagonal,
    the (S, S') matrix is ``dgms`` against ``other``.  Every value is exact, and
    the same bits in any call that holds the pair, in either orientation."""
    pts, off, pairs, S, S2 = _inputs(dgms, other, dim, _lib.TDA_BN_MAX_POINTS, _top_paired_diagram)
    dist, ms = _call_dist("bn", pts, off, pairs, device=int(device))
    D = _matrix(dist, S, S2, other is not None)
    return (D, ms) if return_time else D


def bottleneck(dgm1, dgm2, matching: bool = False, device: int = 0) -> float:
    """``persim.bottleneck(dgm1, dgm2, matching=False)`` [upstream] on the GPU:
    the bottleneck distance of two (n, 2) diagrams.  Points with a non-finite
    coordinate are ignored, with a warning.  The matching itself is not
    returned: ``matching=True`` raises NotImplementedError."""
    if matching:
        raise NotImplementedError("matching=True (returning the matching) is not supported")
    for d in (dgm1, dgm2):
        if isinstance(d, LayerResult):
            raise ValueError("dgm1 and dgm2 are (n, 2) arrays (for LayerResults: bottleneck_matrix)")
    return float(bottleneck_matrix([dgm1], other=[dgm2], device=device)[0, 0])


_SQRT1_2 = 0.70710678118654752440  # the factor of a point's L2 distance to the diagonal (tda_dgm.h)


def _call_ws(points, offsets, pairs, device: int, want_matching: bool = False):
    """One tda_wasserstein call: (dist (P,), device_ms, match_off (P + 1,) or None, match or None)."""
    if _no_pair(offsets, pairs):  # nothing to launch
        return np.zeros(0), 0.0, None, None
    flags = _lib.TDA_WS_WANT_MATCHING if want_matching else 0

    def read(r):
        moff = match = None
        if want_matching:
            moff = _owned(r.match_off, r.P + 1, np.int64)
            match = _owned(r.match, int(moff[-1]), np.int32)
        return _owned(r.dist, r.P), float(r.device_ms), moff, match

    return _library_call("ws", points, offsets, pairs, read, device=int(device), flags=flags)


def _ws_inputs(dgms, other, dim: int):
    """:func:`_inputs` of a Wasserstein call."""
    return _inputs(dgms, other, dim, _lib.TDA_WS_MAX_POINTS, _top_paired_diagram)


def wasserstein_matrix(dgms, other=None, device: int = 0, dim: int = 1, return_time: bool = False):
    """Wasserstein distances between every pair of diagrams, one library call.

    The arguments and the result are those of :func:`bottleneck_matrix`: ``dgms``
    and ``other`` are lists of (n, 2) arrays or of :class:`LayerResult`; the
    (S, S) matrix is symmetric with a zero diagonal, the (S, S') matrix is
    ``dgms`` against ``other``.  A value is the same bits in any call that holds
    the pair, in either orientation."""
    pts, off, pairs, S, S2 = _ws_inputs(dgms, other, dim)
    dist, ms, _, _ = _call_ws(pts, off, pairs, device)
    D = _matrix(dist, S, S2, other is not None)
    return (D, ms) if return_time else D


def wasserstein(dgm1, dgm2, matching: bool = False, device: int = 0):
    """``persim.wasserstein(dgm1, dgm2, matching=False)`` [upstream] on the GPU:
    the 1-Wasserstein distance (Euclidean ground metric) of two (n, 2) diagrams.
    Points with a non-finite coordinate are ignored, with a warning.  With
    ``matching`` the result is ``(distance, (K, 3) float64 array)`` of rows
    ``[i, j, cost]`` as persim returns them: the points of ``dgm1`` in their
    order, each with its partner in ``dgm2`` or -1 for the diagonal, then
    ``[-1, j, cost]`` for the points of ``dgm2`` left to the diagonal.  The
    indices count the rows with a finite (birth, death)."""
    for d in (dgm1, dgm2):
        if isinstance(d, LayerResult):
            raise ValueError("dgm1 and dgm2 are (n, 2) arrays (for LayerResults: wasserstein_matrix)")
    pts, off, pairs, _, _ = _ws_inputs([dgm1], [dgm2], 1)
    dist, _, _, match = _call_ws(pts, off, pairs, device, want_matching=bool(matching))
    if not matching:
        return float(dist[0])
    A, B = (d[np.isfinite(d).all(axis=1)] for d in (pts[:off[1]], pts[off[1]:]))
    i = np.arange(len(A))
    hit = match >= 0
    free = np.setdiff1d(np.arange(len(B)), match[hit])
    db, dd = A[hit, 0] - B[match[hit], 0], A[hit, 1] - B[match[hit], 1]
    cost = (A[:, 1] - A[:, 0]) * _SQRT1_2
    cost[hit] = np.sqrt(db * db + dd * dd)
    rows = np.concatenate([np.stack([i, match, cost], 1),
                           np.stack([np.full(len(free), -1.0), free, (B[free, 1] - B[free, 0]) * _SQRT1_2], 1)])
    return float(dist[0]), rows


def sliced_wasserstein_kernel(D, sigma: float):
    """The sliced Wasserstein kernel exp(-D / (2 sigma^2)) (Carriere, Cuturi, Oudot 2017) of distances D."""
    return np.exp(-np.asarray(D, dtype=np.float64) / (2.0 * float(sigma) ** 2))


# ---------------------------------------------------------------- the heat kernel (tda_heat_kernel)
_8PI = 25.132741228718345908  # the rounded constant of cn = 1 / (8 pi sigma) (tda_dgm.h)


def _check_sigma(sigma) -> float:
    sigma = float(sigma)
    if not (np.isfinite(sigma) and sigma > 0):
        raise ValueError(f"sigma must be finite and > 0, got {sigma}")
    with np.errstate(all="ignore"):
        c = np.array([1.0 / (np.float64(8.0) * sigma), 1.0 / (np.float64(_8PI) * sigma)])
    if not (np.isfinite(c).all() and (c >= np.finfo(np.float64).tiny).all()):
        raise ValueError(f"sigma = {sigma}: 1 / (8 sigma) and 1 / (8 pi sigma) must be finite normal numbers")
    return sigma


def _call_hk(points, offsets, pairs, sigma: float, device: int):
    """One tda_heat_kernel call: (kern (P,), self (S,), dist (P,), device_ms)."""
    S = len(offsets) - 1
    read = lambda r: (_owned(r.kern, r.P), _owned(r.self, S), _owned(r.dist, r.P), float(r.device_ms))  # noqa: E731
    return _library_call("hk", points, offsets, pairs, read, sigma=sigma, device=int(device))


def _hk_inputs(dgms, other, dim: int):
    """:func:`_inputs` of a heat kernel call."""
    return _inputs(dgms, other, dim, _lib.TDA_HK_MAX_POINTS)


def _hk_matrix(dgms, sigma, other, device: int, dim: int, want_kernel: bool):
    sigma = _check_sigma(sigma)
    pts, off, pairs, S, S2 = _hk_inputs(dgms, other, dim)
    # the distances of fewer than two diagrams and the Gram matrix of none: nothing to launch
    if S == 0 or S2 == 0 or (other is None and S == 1 and not want_kernel):
        return np.zeros((S, S2)), 0.0
    kern, self_, dist, ms = _call_hk(pts, off, pairs, sigma, device)
    D = _matrix(kern if want_kernel else dist, S, S2, other is not None)
    if want_kernel and other is None:
        D[np.diag_indices(S)] = self_
    return D, ms


def heat_matrix(dgms, sigma: float = 0.4, other=None, device: int = 0, dim: int = 1, return_time: bool = False):
    """Heat kernel distances between every pair of diagrams, one library call.

    The arguments and the result are those of :func:`bottleneck_matrix`, with the
    kernel's scale ``sigma``: the (S, S) matrix is symmetric with an exactly zero
    diagonal, the (S, S') matrix is ``dgms`` against ``other``.  A diagram may hold
    4096 finite points.  A value is the same bits in any call that holds the pair,
    in either orientation; tda_dgm.h derives its error bound."""
    D, ms = _hk_matrix(dgms, sigma, other, device, dim, False)
    return (D, ms) if return_time else D


def heat_kernel_matrix(dgms, sigma: float = 0.4, other=None, device: int = 0, dim: int = 1, return_time: bool = False):
    """The Gram matrix of the persistence scale-space kernel (Reininghaus et al. 2015),

        k(F, G) = 1 / (8 pi sigma) * sum_{p in F, q in G} exp(-|p - q|^2 / (8 sigma)) - exp(-|p - q'|^2 / (8 sigma)),

    q' the mirror image (d, b) of q: (S, S) and symmetric, with k(F, F) on its diagonal, or
    (S, S') with ``other``.  It is positive semi-definite up to the rounding bound of
    tda_dgm.h, so it can go into kernel PCA, an SVM or an MMD test as it is.  The arguments
    are those of :func:`heat_matrix`, whose values are sqrt(k(F, F) + k(G, G) - 2 k(F, G)).
    The library evaluates k(F, F) of every diagram of a call; with ``other`` this function does not
    return them, so a block of few large diagrams costs up to twice its own terms."""
    K, ms = _hk_matrix(dgms, sigma, other, device, dim, True)
    return (K, ms) if return_time else K


def heat(dgm1, dgm2, sigma: float = 0.4, device: int = 0) -> float:
    """``persim.heat(dgm1, dgm2, sigma=0.4)`` [upstream] on the GPU: the distance the
    persistence scale-space kernel induces between two (n, 2) diagrams.  Points with a
    non-finite coordinate are ignored, with a warning."""
    for d in (dgm1, dgm2):
        if isinstance(d, LayerResult):
            raise ValueError("dgm1 and dgm2 are (n, 2) arrays (for LayerResults: heat_matrix)")
    return float(heat_matrix([dgm1], sigma, other=[dgm2], device=device)[0, 0])


# ---------------------------------------------------------------- the persistence Fisher distance (tda_persistence_fisher)
def _check_sigma_pf(sigma) -> float:
    sigma = float(sigma)
    if not (np.isfinite(sigma) and sigma > 0):
        raise ValueError(f"sigma must be finite and > 0, got {sigma}")
    with np.errstate(all="ignore"):
        c2 = np.float64(1.0) / (np.float64(2.0) * (np.float64(sigma) * np.float64(sigma)))
    if not (np.isfinite(c2) and c2 >= np.finfo(np.float64).tiny):
        raise ValueError(f"sigma = {sigma}: 1 / (2 sigma^2) must be a finite normal number")
    return sigma


def _check_bandwidth(bandwidth) -> float:
    bandwidth = float(bandwidth)
    if not (np.isfinite(bandwidth) and bandwidth > 0):
        raise ValueError(f"bandwidth must be finite and > 0, got {bandwidth}")
    return bandwidth


def _call_pf(points, offsets, pairs, sigma: float, device: int):
    """One tda_persistence_fisher call: (a (P,), b (P,), h (P,), dist (P,), device_ms)."""
    if _no_pair(offsets, pairs):  # nothing to launch
        return np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0), 0.0
    read = lambda r: (_owned(r.a, r.P), _owned(r.b, r.P), _owned(r.h, r.P), _owned(r.dist, r.P), float(r.device_ms))  # noqa: E731
    return _library_call("pf", points, offsets, pairs, read, sigma=sigma, device=int(device))


def fisher_matrix(dgms, sigma: float = 1.0, other=None, device: int = 0, dim: int = 1, return_time: bool = False):
    """Persistence Fisher distances (Le and Yamada 2018; gudhi's ``PersistenceFisherDistance``
    [upstream]) between every pair of diagrams, one library call.

    Each pair is smoothed, with a Gaussian of standard deviation ``sigma``, into two densities
    on the points of both diagrams and of their projections on the diagonal; the value is the
    arccos of the two densities' Bhattacharyya affinity, between 0 and pi / 2.  The arguments
    and the result are those of :func:`heat_matrix`: the (S, S) matrix is symmetric with an
    exactly zero diagonal, the (S, S') matrix is ``dgms`` against ``other``.  A diagram may hold
    1024 finite points.  A value is the same bits in any call that holds the pair, in either
    orientation; tda_dgm.h derives its error bound."""
    sigma = _check_sigma_pf(sigma)
    pts, off, pairs, S, S2 = _inputs(dgms, other, dim, _lib.TDA_PF_MAX_POINTS, _top_paired_diagram)
    _, _, _, dist, ms = _call_pf(pts, off, pairs, sigma, device)
    D = _matrix(dist, S, S2, other is not None)
    return (D, ms) if return_time else D


def fisher_kernel_matrix(dgms, sigma: float = 1.0, bandwidth: float = 1.0, other=None, device: int = 0, dim: int = 1,
                         return_time: bool = False):
    """The persistence Fisher kernel ``exp(-fisher / bandwidth)`` (gudhi's
    ``PersistenceFisherKernel`` [upstream]) of :func:`fisher_matrix`: (S, S) and symmetric with a
    unit diagonal, or (S, S') with ``other``.  The exponential is numpy's, on the host.  The
    kernel is positive definite for the continuous construction; the discrete support here
    depends on the pair, so nothing is promised for the matrix's smallest eigenvalue."""
    bandwidth = _check_bandwidth(bandwidth)
    D, ms = fisher_matrix(dgms, sigma, other, device, dim, return_time=True)
    K = np.exp(-D / bandwidth)
    return (K, ms) if return_time else K


def fisher(dgm1, dgm2, sigma: float = 1.0, device: int = 0) -> float:
    """The persistence Fisher distance of two (n, 2) diagrams (:func:`fisher_matrix`).  Points
    with a non-finite coordinate are ignored, with a warning."""
    for d in (dgm1, dgm2):
        if isinstance(d, LayerResult):
            raise ValueError("dgm1 and dgm2 are (n, 2) arrays (for LayerResults: fisher_matrix)")
    return float(fisher_matrix([dgm1], sigma, other=[dgm2], device=device)[0, 0])


# ---------------------------------------------------------------- vectorisations (tda_landscape, tda_persistence_image)
def _vec_inputs(dgms, dim: int):
    """(points, offsets, S): :func:`_inputs` of a landscape or image call."""
    pts, off, _, S, _ = _inputs(dgms, None, dim, _lib.TDA_VEC_MAX_POINTS)
    return pts, off, S


def _check_int(name: str, v, hi: int) -> int:
    if isinstance(v, bool) or int(v) != v:
        raise ValueError(f"{name} must be an integer")
    if v < 1:
        raise ValueError(f"{name} must be >= 1")
    if v > hi:
        raise NotImplementedError(f"{name} > {hi} is not supported")
    return int(v)


def _check_out(S: int, F: int):
    if S * F > _lib.TDA_VEC_MAX_OUT:
        raise NotImplementedError(f"{S} diagrams of {F} values: more than 2^24 values in one call is not supported (split the diagrams)")


def _linspace_grid(start, stop, G: int, births, deaths):
    """``np.linspace(start, stop, G)``; an end left None is the smallest of ``births`` / the largest of ``deaths``."""
    if (start is None and not len(births)) or (stop is None and not len(deaths)):
        raise ValueError("no diagram holds a finite point: start and stop must be given")
    start = float(births.min()) if start is None else float(start)
    stop = float(deaths.max()) if stop is None else float(stop)
    if not (np.isfinite(start) and np.isfinite(stop)):
        raise ValueError("start and stop must be finite")
    with np.errstate(all="ignore"):
        grid = np.ascontiguousarray(np.linspace(start, stop, G), dtype=np.float64)
    if not np.isfinite(grid).all():
        raise ValueError("start and stop span more than float64 holds")
    return grid


def _call_pl(points, offsets, grid, K: int, device: int):
    """One tda_landscape call: (values (S, K, G), device_ms)."""
    read = lambda r: (_owned(r.values, r.S * r.F).reshape(r.S, K, len(grid)), float(r.device_ms))  # noqa: E731
    return _library_call("pl", points, offsets, None, read, grid=grid.ctypes.data, G=len(grid), K=K, device=int(device))


def persistence_landscapes(dgms, start=None, stop=None, num_steps: int = 500, depth: int = 10, dim: int = 1, device: int = 0,
                           return_grid: bool = False, return_time: bool = False):
    """Persistence landscapes (Bubenik 2015; ``persim.landscapes`` [upstream]) of a list of
    diagrams, one library call: the (S, depth, num_steps) float64 array of
    lambda_k(t) = the k-th largest of max(0, min(t - b, d - t)) over a diagram's points, k = 1 ..
    depth, at t in ``np.linspace(start, stop, num_steps)``.

    dgms: a list of (n, 2) arrays of (birth, death) or of :class:`LayerResult` (then diagram ``dim``
    of each).  ``start`` / ``stop`` default to the smallest birth / the largest death over all finite
    points of the call (a call without one needs both given).  This is the exact landscape sampled on
    the grid, every value one rounded subtraction or +0.0: persim's ``PersLandscapeApprox`` snaps the
    bars to the grid first and so differs between grid values of a bar's ends.  A diagram's rows are
    the same bits in any call that holds it.  Points with a non-finite coordinate are ignored, with a
    warning; a diagram may hold 4096 finite points, depth <= 64, num_steps <= 4096.  With
    ``return_grid`` also the grid, with ``return_time`` also the call's device time in ms."""
    K = _check_int("depth", depth, _lib.TDA_PL_MAX_DEPTH)
    G = _check_int("num_steps", num_steps, _lib.TDA_PL_MAX_STEPS)
    pts, off, S = _vec_inputs(dgms, dim)
    fin = pts[np.isfinite(pts).all(axis=1)]
    grid = _linspace_grid(start, stop, G, fin[:, 0], fin[:, 1])
    _check_out(S, K * G)
    out, ms = (np.zeros((0, K, G)), 0.0) if S == 0 else _call_pl(pts, off, grid, K, device)
    res = (out,) + ((grid,) if return_grid else ()) + ((ms,) if return_time else ())
    return res if len(res) > 1 else out


def persistence_landscape(dgm, start=None, stop=None, num_steps: int = 500, depth: int = 10, device: int = 0, return_grid: bool = False):
    """The (depth, num_steps) landscape of one (n, 2) diagram (:func:`persistence_landscapes`)."""
    if isinstance(dgm, LayerResult):
        raise ValueError("dgm is an (n, 2) array (for LayerResults: persistence_landscapes)")
    r = persistence_landscapes([dgm], start, stop, num_steps, depth, device=device, return_grid=return_grid)
    return (r[0][0], r[1]) if return_grid else r[0]


def _call_pi(points, offsets, xe, ye, sigma: float, power: float, device: int):
    """One tda_persistence_image call: (values (S, W, H), device_ms)."""
    W, H = len(xe) - 1, len(ye) - 1
    read = lambda r: (_owned(r.values, r.S * r.F).reshape(r.S, W, H), float(r.device_ms))  # noqa: E731
    return _library_call("pi", points, offsets, None, read, x_edges=xe.ctypes.data, y_edges=ye.ctypes.data, W=W, H=H, sigma=sigma,
                         weight_power=power, device=int(device))


def _edges(name: str, rng, n: int):
    try:
        lo, hi = (float(x) for x in rng)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a (low, high) pair") from None
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError(f"{name} must be finite with low < high, got ({lo}, {hi})")
    with np.errstate(all="ignore"):
        e = np.ascontiguousarray(np.linspace(lo, hi, n + 1), dtype=np.float64)
    if not (np.isfinite(e).all() and (np.diff(e) > 0).all()):
        raise ValueError(f"{name} = ({lo}, {hi}) does not split into {n} pixels of positive width")
    return e


def persistence_images(dgms, birth_range, pers_range, resolution, sigma: float, weight_power: float = 1.0, dim: int = 1,
                       device: int = 0, return_time: bool = False):
    """Persistence images (Adams et al. 2017; ``persim.PersistenceImager`` [upstream]) of a list of
    diagrams, one library call: the (S, nb, npers) float64 array, ``resolution = (nb, npers)`` (or
    one integer for both), pixel [i, j] covering births ``np.linspace(*birth_range, nb + 1)[i : i + 2]``
    and persistences ``np.linspace(*pers_range, npers + 1)[j : j + 2]``.

    Every finite point (b, d) becomes (b, d - b), weighted with (d - b) ** weight_power (0 for
    d <= b) and spread by a Gaussian of standard deviation ``sigma`` in both axes, integrated exactly
    over each pixel (a difference of two erf per axis).  persim's ``kernel_params["sigma"]`` is the
    covariance, here ``sigma ** 2`` times the identity, and its default ``skew=True`` (the
    birth-persistence coordinates) is what is implemented.  Each pixel lies within
    (2 * 16 + 9 + n) * 2^-53 * sum(weights) of the exact value (tda_dgm.h), and a diagram's image is
    the same bits in any call that holds it.  dgms, dim, the non-finite points and the 4096-point
    limit are those of :func:`persistence_landscapes`; at most 256 pixels per axis."""
    res = (resolution, resolution) if np.ndim(resolution) == 0 else tuple(resolution)
    if len(res) != 2:
        raise ValueError("resolution must be an integer or a pair (nb, npers)")
    W, H = (_check_int("resolution", r, _lib.TDA_PI_MAX_PIXELS) for r in res)
    sigma, power = float(sigma), float(weight_power)
    if not (np.isfinite(sigma) and sigma > 0):
        raise ValueError(f"sigma must be finite and > 0, got {sigma}")
    if not (np.isfinite(power) and power >= 0):
        raise ValueError(f"weight_power must be finite and >= 0, got {power}")
    xe, ye = _edges("birth_range", birth_range, W), _edges("pers_range", pers_range, H)
    pts, off, S = _vec_inputs(dgms, dim)
    _check_out(S, W * H)
    out, ms = (np.zeros((0, W, H)), 0.0) if S == 0 else _call_pi(pts, off, xe, ye, sigma, power, device)
    return (out, ms) if return_time else out


def persistence_image(dgm, birth_range, pers_range, resolution, sigma: float, weight_power: float = 1.0, device: int = 0):
    """The (nb, npers) image of one (n, 2) diagram (:func:`persistence_images`)."""
    if isinstance(dgm, LayerResult):
        raise ValueError("dgm is an (n, 2) array (for LayerResults: persistence_images)")
    return persistence_images([dgm], birth_range, pers_range, resolution, sigma, weight_power, device=device)[0]


# ---------------------------------------------------------------- persistence curves (tda_persistence_curve)
_PC_KERNELS = {"indicator": _lib.TDA_PC_INDICATOR, "tent": _lib.TDA_PC_TENT}


def _call_pc(points, offsets, coef, grid, kernel: int, flags: int, device: int):
    """One tda_persistence_curve call: (values (S, G), device_ms)."""
    read = lambda r: (_owned(r.values, r.S * r.F).reshape(r.S, len(grid)), float(r.device_ms))  # noqa: E731
    return _library_call("pc", points, offsets, None, read, coef=None if coef is None else coef.ctypes.data, grid=grid.ctypes.data,
                         G=len(grid), kernel=kernel, flags=flags, device=int(device))


def _pc_inputs(dgms, dim: int, essential: bool):
    """(points, offsets, kept) of a curve call: ``kept`` marks the rows the library keeps, those with a
    finite birth and a finite death or, with ``essential``, a death of +inf.  The point limit is checked
    and the dropped rows are reported, before any library call."""
    pts, off = _flatten(dgms, dim)
    b, d = pts[:, 0], pts[:, 1]
    kept = np.isfinite(b) & (np.isfinite(d) | (d == np.inf)) if essential else np.isfinite(pts).all(axis=1)
    c = np.concatenate([[0], np.cumsum(kept)])
    cnt = c[off[1:]] - c[off[:-1]]
    if len(cnt) and cnt.max() > _lib.TDA_VEC_MAX_POINTS:
        raise NotImplementedError(f"a diagram holds {int(cnt.max())} finite points: more than {_lib.TDA_VEC_MAX_POINTS} is not supported")
    dropped = int(len(kept) - c[-1])
    if dropped:
        warnings.warn(f"the diagrams hold {dropped} points with a non-finite coordinate; ignoring those points")
    return pts, off, kept


def _run_pc(pts, off, kept, coef, grid, kernel: str, normalize: bool, essential: bool, device: int):
    """The call of the entries below, after their checks: (values (S, G), device_ms)."""
    S, G = len(off) - 1, len(grid)
    if coef is not None and not np.isfinite(coef[kept]).all():
        raise ValueError("coef holds a non-finite value on a row with a finite (birth, death)")
    _check_out(S, G)
    flags = (_lib.TDA_PC_NORMALIZE if normalize else 0) | (_lib.TDA_PC_KEEP_ESSENTIAL if essential else 0)
    return (np.zeros((0, G)), 0.0) if S == 0 else _call_pc(pts, off, coef, grid, _PC_KERNELS[kernel], flags, device)


def persistence_curves(dgms, grid, coef=None, kernel: str = "indicator", normalize: bool = False, essential: bool = False, dim: int = 1,
                       device: int = 0, return_time: bool = False):
    """Persistence curves (Chung and Lawson 2019) of a list of diagrams on ``grid``, one library call:
    the (S, G) float64 array

        F_s(t) = sum over the points p of diagram s, in row order, of coef[s][p] * K(b_p, d_p, t),

    K the indicator of ``b <= t < d`` (``kernel="indicator"``) or the tent ``max(0, min(t - b, d - t))``
    (``kernel="tent"``).  ``coef`` is a list of S arrays, one coefficient per row of each diagram, or
    None for all ones; with ``normalize`` every curve is divided by the sum of its diagram's
    coefficients (a diagram whose sum is 0 gives zeros).  Rows with a non-finite coordinate are
    ignored, with a warning, and their coefficients with them; with ``essential`` (indicator only) the
    rows with a death of +inf are kept and count from their birth on.

    Every value is the sum ``acc = acc + coef * K`` over the points with K > 0, from +0.0 in row order,
    each product and each sum rounded once: a numpy loop gives the same bits, and a diagram's curve is
    the same bits in any call that holds it.  ``grid`` holds 1 .. 4096 finite values in any order; a
    diagram may hold 4096 kept rows.  dgms and dim are those of :func:`persistence_landscapes`; with
    ``return_time`` also the call's device time in ms."""
    if kernel not in _PC_KERNELS:
        raise ValueError(f"kernel must be 'indicator' or 'tent', got {kernel!r}")
    if essential and kernel == "tent":
        raise ValueError("essential=True needs kernel='indicator': a tent has no value on a bar without a death")
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    if grid.ndim != 1 or len(grid) < 1:
        raise ValueError("grid must be a one-dimensional array of at least one value")
    if len(grid) > _lib.TDA_PL_MAX_STEPS:
        raise NotImplementedError(f"a grid of more than {_lib.TDA_PL_MAX_STEPS} values is not supported")
    if not np.isfinite(grid).all():
        raise ValueError("grid holds a non-finite value")
    pts, off, kept = _pc_inputs(dgms, dim, bool(essential))
    if coef is not None:
        coef = [np.asarray(c, dtype=np.float64).reshape(-1) for c in coef]
        if [len(c) for c in coef] != np.diff(off).tolist():
            raise ValueError("coef must hold one array per diagram with one coefficient per row")
        coef = np.ascontiguousarray(np.concatenate(coef) if coef else np.zeros(0), dtype=np.float64)
    out, ms = _run_pc(pts, off, kept, coef, grid, kernel, bool(normalize), bool(essential), device)
    return (out, ms) if return_time else out


def _lifespan_coef(b, d):
    return d - b


def _entropy_coef(b, d):
    l = d - b  # noqa: E741
    p = l / l.sum()
    return -p * np.log(p)


def _named_curves(dgms, coef_of, kernel, normalize, essential, start, stop, num_steps, dim, device, return_grid, return_time,
                  per_diagram: bool = True):
    """The named curves: the grid of :func:`persistence_landscapes` over the kept rows, the coefficients
    ``coef_of(births, deaths)`` of every diagram's kept rows (of all kept rows at once where the
    formula is row by row), one :func:`persistence_curves` call."""
    G = _check_int("num_steps", num_steps, _lib.TDA_PL_MAX_STEPS)
    pts, off, kept = _pc_inputs(dgms, dim, essential)
    grid = _linspace_grid(start, stop, G, pts[kept, 0], pts[kept & np.isfinite(pts[:, 1]), 1])
    coef = None
    if coef_of is not None:
        coef = np.zeros(len(pts))
        with np.errstate(all="ignore"):
            if per_diagram:
                for s in range(len(off) - 1):
                    rows = off[s] + np.flatnonzero(kept[off[s]:off[s + 1]])
                    coef[rows] = coef_of(pts[rows, 0], pts[rows, 1])
            else:
                coef[kept] = coef_of(pts[kept, 0], pts[kept, 1])
    out, ms = _run_pc(pts, off, kept, coef, grid, kernel, normalize, essential, device)
    res = (out,) + ((grid,) if return_grid else ()) + ((ms,) if return_time else ())
    return res if len(res) > 1 else out


def _one_curve(many, dgm, return_grid: bool, **kw):
    if isinstance(dgm, LayerResult):
        raise ValueError(f"dgm is an (n, 2) array (for LayerResults: {many.__name__})")
    r = many([dgm], return_grid=return_grid, **kw)
    return (r[0][0], r[1]) if return_grid else r[0]


def betti_curves(dgms, start=None, stop=None, num_steps: int = 100, dim: int = 1, essential: bool = True, device: int = 0,
                 return_grid: bool = False, return_time: bool = False):
    """Betti curves of a list of diagrams, one library call: the (S, num_steps) float64 array of the
    number of points with ``b <= t < d`` at t in ``np.linspace(start, stop, num_steps)`` -- the classes
    of H_dim alive at radius t.  It is :func:`persistence_curves` with the indicator and no coefficients.
    With ``essential`` (the default) a point with a death of +inf counts from its birth on, and is not
    reported as non-finite.  ``start`` / ``stop`` default to the smallest birth / the largest finite
    death of the points that count (a call without one needs both given); dgms, dim and the limits are
    those of :func:`persistence_curves`.  With ``return_grid`` also the grid, with ``return_time`` also
    the call's device time in ms."""
    return _named_curves(dgms, None, "indicator", False, bool(essential), start, stop, num_steps, dim, device, return_grid, return_time)


def betti_curve(dgm, start=None, stop=None, num_steps: int = 100, essential: bool = True, device: int = 0, return_grid: bool = False):
    """The (num_steps,) Betti curve of one (n, 2) diagram (:func:`betti_curves`)."""
    return _one_curve(betti_curves, dgm, return_grid, start=start, stop=stop, num_steps=num_steps, essential=essential, device=device)


def lifespan_curves(dgms, start=None, stop=None, num_steps: int = 100, dim: int = 1, device: int = 0, return_grid: bool = False,
                    return_time: bool = False):
    """Lifespan curves of a list of diagrams: the (S, num_steps) float64 array of the total lifetime of
    the points alive at t, :func:`persistence_curves` with the indicator and the coefficients
    ``c = d - b``.  Points with a non-finite coordinate are ignored, with a warning; the grid and the
    other arguments are those of :func:`betti_curves`."""
    return _named_curves(dgms, _lifespan_coef, "indicator", False, False, start, stop, num_steps, dim, device, return_grid, return_time,
                         per_diagram=False)


def lifespan_curve(dgm, start=None, stop=None, num_steps: int = 100, device: int = 0, return_grid: bool = False):
    """The (num_steps,) lifespan curve of one (n, 2) diagram (:func:`lifespan_curves`)."""
    return _one_curve(lifespan_curves, dgm, return_grid, start=start, stop=stop, num_steps=num_steps, device=device)


def entropy_curves(dgms, start=None, stop=None, num_steps: int = 100, dim: int = 1, device: int = 0, return_grid: bool = False,
                   return_time: bool = False):
    """Entropy summary functions (Atienza, Gonzalez-Diaz, Soriano-Trigueros 2020) of a list of
    diagrams: the (S, num_steps) float64 array of :func:`persistence_curves` with the indicator and,
    per diagram, over its rows with a finite (birth, death),

        l = d - b,  p = l / l.sum(),  c = -p * np.log(p).

    A row with d <= b has no such coefficient (ValueError).  Points with a non-finite coordinate are
    ignored, with a warning; the grid and the other arguments are those of :func:`betti_curves`."""
    return _named_curves(dgms, _entropy_coef, "indicator", False, False, start, stop, num_steps, dim, device, return_grid, return_time)


def entropy_curve(dgm, start=None, stop=None, num_steps: int = 100, device: int = 0, return_grid: bool = False):
    """The (num_steps,) entropy summary function of one (n, 2) diagram (:func:`entropy_curves`)."""
    return _one_curve(entropy_curves, dgm, return_grid, start=start, stop=stop, num_steps=num_steps, device=device)


def persistence_silhouettes(dgms, start=None, stop=None, num_steps: int = 100, dim: int = 1, device: int = 0, return_grid: bool = False,
                            return_time: bool = False, power: float = 1.0):
    """Persistence silhouettes (Chazal et al. 2014) of a list of diagrams: the (S, num_steps) float64
    array of the weighted average of the tents ``max(0, min(t - b, d - t))``, :func:`persistence_curves`
    with the tent, normalised, and per diagram the coefficients

        c = np.power(d - b, power)

    over its rows with a finite (birth, death) (a row whose coefficient is not finite, d < b under a
    fractional power, is a ValueError).  Points with a non-finite coordinate are ignored, with a
    warning; the grid and the other arguments are those of :func:`betti_curves`."""
    power = float(power)
    if not np.isfinite(power):
        raise ValueError(f"power must be finite, got {power}")
    return _named_curves(dgms, lambda b, d: np.power(d - b, power), "tent", True, False, start, stop, num_steps, dim, device, return_grid,
                         return_time)


def persistence_silhouette(dgm, start=None, stop=None, num_steps: int = 100, device: int = 0, return_grid: bool = False, power: float = 1.0):
    """The (num_steps,) silhouette of one (n, 2) diagram (:func:`persistence_silhouettes`)."""
    return _one_curve(persistence_silhouettes, dgm, return_grid, start=start, stop=stop, num_steps=num_steps, device=device, power=power)
