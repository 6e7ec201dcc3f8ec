"""ripser-compatible Python entry points backed by the MI355X HIP library.

Drop-in for the reference's hot path ``result = ripser(cloud_low_dim,
maxdim=MAX_DIM); dgms = result['dgms']`` (debug_tda_pipeline.py:109-110,
analyze_tda_over_layers.py:76, analyze_adversarial_tda.py:100).  The signature
and the result dict mirror the third-party ``ripser.ripser`` (scikit-tda
ripser.py, unpinned at README.md:28) [upstream]:

    ripser(X, maxdim=1, thresh=np.inf, coeff=2, distance_matrix=False,
           do_cocycles=False, metric='euclidean', n_perm=None)
    -> {'dgms', 'cocycles', 'num_edges', 'dperm2all', 'idx_perm', 'r_cover'}

``ripser_batch`` is the layer-loop entry: (L, N, D) clouds (numpy, or a torch
tensor already resident on the GPU) -> one result per layer, one library call.
``ripser_batch(X, n_perm=k)`` is ripser.py's greedy subsampling: k furthest-point
landmarks per layer chosen on the GPU (``greedy_perm_batch``), persistence on
the landmarks only.
"""
from __future__ import annotations

import contextlib
import ctypes
import warnings
import weakref

import numpy as np

from . import _cloud, _lib
from ._cloud import is_torch as _is_torch


class _Batch:
    """Host copies of one batched call's outputs; LayerResults are views into it."""

    __slots__ = ("L", "nd", "N", "pairs", "cnt", "off", "bidx", "didx", "thr", "ne", "cs", "na", "nc", "nr", "nadd", "dist", "sil",
                 "tn", "dg", "dist64", "ip", "rc")


class LayerResult(tuple):
    """Persistence of one layer (all arrays on the host).

    ``dgms`` (list of (n_k, 2) float64 arrays, ripser's emission order) and
    the other fields are views into the batch's shared arrays, made on first
    access.  (A (batch, layer) tuple: one batched call makes L of them.)
    """

    __slots__ = ()

    @property
    def _b(self):
        return self[0]

    @property
    def _l(self):
        return self[1]

    def _seg(self, arr):
        b, l = self
        return [arr[o:o + c] for o, c in zip(b.off[l].tolist(), b.cnt[l].tolist())]

    @property
    def dgms(self) -> list:
        b, l = self
        if b.dg is None:  # first access: every layer's views in one C call (L x (maxdim+1) slices)
            b.dg = _lib.hostviews().segments(b.pairs, b.off.ravel(), b.cnt.ravel(), b.nd)
        return b.dg[l]

    @property
    def birth_idx(self):
        return self._seg(self[0].bidx)

    @property
    def death_idx(self):
        return self._seg(self[0].didx)

    @property
    def num_edges(self) -> int:
        return int(self[0].ne[self[1]])

    @property
    def thresh(self) -> float:
        return float(self[0].thr[self[1]])

    @property
    def checksum(self) -> list:
        return self[0].cs[self[1]].tolist()

    @property
    def n_all_pairs(self) -> list:
        return self[0].na[self[1]].tolist()

    @property
    def n_columns(self) -> list:
        return self[0].nc[self[1]].tolist()

    @property
    def n_residual(self) -> list:
        return self[0].nr[self[1]].tolist()

    @property
    def n_adds(self) -> list:
        return self[0].nadd[self[1]].tolist()

    @property
    def silhouette(self) -> list:
        """Silhouette score per label set passed to ``ripser_batch(labels=...)``
        (sklearn.metrics.silhouette_score semantics), or [] when none."""
        b = self[0]
        return [] if b.sil is None else b.sil[self[1]].tolist()

    @property
    def twonn(self) -> float:
        """TwoNN intrinsic dimension of the layer's cloud (``ripser_batch(twonn=True)``;
        metrics.py:113-208 semantics, NaN where the reference gives NaN), or None."""
        b = self[0]
        return None if b.tn is None else float(b.tn[self[1]])

    @property
    def dist(self):
        b = self[0]
        return None if b.dist is None else b.dist[self[1]]

    @property
    def dist64(self):
        """float64 distance matrix (float64 point clouds with want_dist64), else None."""
        b = self[0]
        return None if b.dist64 is None else b.dist64[self[1]]

    @property
    def idx_perm(self):
        """Indices of the points persistence ran on: the greedy landmarks of
        ``ripser_batch(n_perm=k)`` in selection order, else ``arange(N)``."""
        b = self[0]
        return np.arange(b.N) if b.ip is None else b.ip[self[1]]

    @property
    def r_cover(self) -> float:
        """Covering radius of the landmarks (every point is within it of one;
        the diagrams are within 2 * r_cover of the full cloud's in bottleneck
        distance); 0.0 without subsampling."""
        b = self[0]
        return 0.0 if b.rc is None else float(b.rc[self[1]])


def _arr(ptr, n, dtype):
    """Copy n elements of a library-owned C array (one memcpy, no per-element work)."""
    if n == 0:
        return np.zeros(0, dtype=dtype)
    return np.frombuffer(ctypes.string_at(ptr, n * np.dtype(dtype).itemsize), dtype=dtype)


def _unpack(res_p, want_dist: bool, n_sets: int = 0) -> tuple[list, dict]:
    r = res_p.contents
    L, md, N = r.L, r.maxdim, r.N
    nd = md + 1
    total = r.n_pairs
    b = _Batch()
    b.L, b.nd, b.N = L, nd, N
    # one copy of the result blob (tda_rips.h: meta | num_edges | idx | thresh | birth, death) and
    # its views, made in one C call; pairs (total, 2) float64: every diagram is a view into it
    (b.cnt, b.off, b.cs, b.na, b.nc, b.nr, b.nadd, b.ne, b.bidx, b.didx, b.thr,
     b.pairs) = _lib.hostviews().blob_arrays(r.blob or 0, r.blob_bytes, L, nd, total)
    b.dg = None
    b.ip = b.rc = None  # set by ripser_batch(n_perm=k)
    b.dist = _arr(r.dist, L * N * N, np.float32).reshape(L, N, N) if want_dist and bool(r.dist) else None
    b.dist64 = _arr(r.dist64, L * N * N, np.float64).reshape(L, N, N) if want_dist and bool(r.dist64) else None
    b.tn = _arr(r.twonn, L, np.float32) if bool(r.twonn) else None
    b.sil = _arr(r.silhouette, L * n_sets, np.float64).reshape(L, n_sets) if bool(r.silhouette) else None
    out = _lib.hostviews().layer_tuples(LayerResult, b, L)
    ns = r.n_stages
    stages = [(r.stage_name[i].decode(), float(r.stage_ms[i])) for i in range(ns)] if ns else []
    return out, {"device_ms": r.device_ms, "stages": stages, "cap_reruns": int(r.n_cap_reruns)}


def _call_batch(args: _lib.RipsArgs, want_dist: bool):
    L = _lib.lib()
    res = ctypes.POINTER(_lib.RipsResult)()
    _lib.check(L.tda_rips_batch(ctypes.byref(args), ctypes.byref(res)))
    try:
        return _unpack(res, want_dist, int(args.n_label_sets))
    finally:
        L.tda_rips_free(res)


def _check_common(maxdim, coeff, do_cocycles, n_perm, metric):
    if coeff != 2:
        raise NotImplementedError("only coeff=2 (Z/2) is implemented (the reference never overrides it)")
    if do_cocycles:
        raise NotImplementedError("do_cocycles=True is not implemented")
    if n_perm is not None:
        raise NotImplementedError("greedy subsampling (n_perm) is implemented by the batch entry: "
                                  "ripser_batch(X[None], n_perm=k)[0] (INTEGRATION.md)")
    if metric != "euclidean":
        raise NotImplementedError("only metric='euclidean' is implemented")
    if int(maxdim) != maxdim or maxdim < 0:
        raise ValueError("maxdim must be a non-negative integer")
    if maxdim > 2:
        raise NotImplementedError("maxdim > 2 is not implemented")


def encode_labels(label_sets, n: int) -> np.ndarray:
    """sklearn LabelEncoder codes (sorted unique classes -> 0..K-1) of each
    label set, as a contiguous (S, n) int32 array; checks sklearn's
    ``check_number_of_labels`` bound (2 <= K <= n - 1)."""
    rows = []
    for lab in label_sets:
        lab = np.asarray(lab)
        if lab.ndim != 1 or lab.shape[0] != n:
            raise ValueError(f"labels must have one entry per point ({n})")
        _, codes = np.unique(lab, return_inverse=True)
        k = int(codes.max()) + 1 if n else 0
        if not 2 <= k <= n - 1:
            raise ValueError(f"Number of labels is {k}. Valid values are 2 to n_samples - 1 (inclusive)")
        if k > 32:
            raise NotImplementedError("silhouette with more than 32 clusters is not implemented")
        rows.append(codes.astype(np.int32))
    return np.ascontiguousarray(np.stack(rows)) if rows else np.zeros((0, n), np.int32)


def _fill_call_args(a, N, maxdim, thresh, distance_matrix, want_dist, stage_times, stage_serial, one_stream, input_ready,
                    persistence, want_dist64, labels, twonn, discard_fraction, eps):
    """The arguments of a batch call that do not depend on its input array, into ``a``
    (ripser_batch's own, and the template of a native SweepPipeline call).  Returns
    (want_dist as the result must be unpacked, the label codes ``a.labels`` points into)."""
    a.is_dist = 1 if distance_matrix else 0
    a.maxdim = int(maxdim)
    a.thresh = float(thresh) if np.isfinite(thresh) else float("inf")
    a.modulus = 2
    a.want_dist = 1 if want_dist else 0
    a.flags = (_lib.TDA_FLAG_STAGE_TIMES | (_lib.TDA_FLAG_STAGE_SERIAL if stage_serial else 0)) if stage_times else 0
    if one_stream:
        a.flags |= _lib.TDA_FLAG_ONE_STREAM
    if input_ready:
        a.flags |= _lib.TDA_FLAG_INPUT_READY
    if not persistence:
        if maxdim != 0:
            raise ValueError("persistence=False needs maxdim=0")
        a.flags |= _lib.TDA_FLAG_NO_PERSISTENCE
    if want_dist64:  # f64 points: the f64 distance matrix too (ripser.py's dperm2all)
        a.flags |= _lib.TDA_FLAG_DIST64
        a.want_dist = 1
        want_dist = True
    lab = None
    if labels is not None:
        lab = encode_labels(labels, N)
        a.labels = lab.ctypes.data
        a.n_label_sets = lab.shape[0]
    if twonn:
        a.want_twonn = 1
        a.twonn_discard = float(discard_fraction)
        a.twonn_eps = float(eps)
    return want_dist, lab


def ripser_batch(X, maxdim: int = 1, thresh: float = np.inf, distance_matrix: bool = False, device: int = 0,
                 want_dist: bool = False, return_time: bool = False, stage_times: bool = False, labels=None,
                 stage_serial: bool = False, twonn: bool = False, discard_fraction: float = 0.1, eps: float = 1e-10,
                 want_dist64: bool = False, slot: int = 0, persistence: bool = True,
                 one_stream: bool = False, input_ready: bool = False, n_perm=None):
    """Persistence of L layers in one call.

    X: (L, N, D) point clouds or (L, N, N) distance matrices (distance_matrix=True);
       numpy array on the host, or a contiguous torch CUDA tensor (consumed in
       place, ordered on torch's current stream); or a list of up to
       TDA_MAX_PARTS such arrays of one shape (consecutive sweeps of a
       dynamically batched call): their layers are processed as one batch
       (the library gathers them on the device; ABI 6 ``x_parts``).
    Returns a list of ``LayerResult``; with return_time also a dict
    {"device_ms", "stages": [(name, ms), ...]} (stages filled when stage_times,
    timed with HIP events on the library's stream).
    labels: optional sequence of label sets (each N labels, shared by every
    layer); each layer's ``silhouette`` then holds sklearn's
    ``silhouette_score(cloud, labels)`` per set, computed on the GPU from the
    same distance matrix (debug_tda_pipeline.py:117-118).
    twonn: also estimate each layer's TwoNN intrinsic dimension on the same
    distance matrix (metrics.py:113-208, ``discard_fraction`` / ``eps`` as
    there); read it from ``LayerResult.twonn``.
    want_dist64: float64 point clouds also return the float64 distance matrix
    (``LayerResult.dist64``: sqrt in f64, what sklearn returns for f64 points).
    slot: the device workspace (0 .. 7) the call runs in; calls from different
    host threads on different slots run concurrently on the GPU (see
    :class:`SweepPipeline`).
    input_ready: a CUDA tensor X is already complete (the caller synchronised
    after producing it): the call skips its event on torch's current stream.
    one_stream: every kernel of the call on the slot's one stream
    (TDA_FLAG_ONE_STREAM): slower alone, but each slot then holds one hardware
    queue, so several slots in flight run side by side.
    persistence=False (maxdim 0 only): distances and the side metrics asked for
    (``twonn``, ``labels``) without any persistence; every diagram is empty.
    n_perm=k: ripser.py's greedy subsampling.  k furthest-point landmarks per
    layer are chosen on the GPU (:func:`greedy_perm_batch`) and persistence
    runs on them alone, their distance matrices never leaving the device; N may
    be up to 8192, the point-count limits then apply to k.  Each result's
    ``idx_perm`` / ``r_cover`` say which points and how well they cover;
    ``dist``, ``thresh`` and ``num_edges`` describe the landmark matrix.
    float32 points or distance matrices only (float64 points raise
    NotImplementedError); ``labels``, ``twonn`` and list-of-parts input raise
    ValueError with it.
    """
    _check_common(maxdim, 2, False, None, "euclidean")
    if n_perm is not None:
        return _ripser_batch_landmarks(X, n_perm, maxdim=maxdim, thresh=thresh, distance_matrix=distance_matrix, device=device,
                                       want_dist=want_dist, return_time=return_time, stage_times=stage_times, labels=labels,
                                       stage_serial=stage_serial, twonn=twonn, want_dist64=want_dist64, slot=slot,
                                       persistence=persistence, one_stream=one_stream, input_ready=input_ready)
    a = _lib.RipsArgs()
    if isinstance(X, (list, tuple)):  # ABI 6 x_parts: consecutive sweeps of one dynamically batched call
        if not 1 <= len(X) <= _lib.TDA_MAX_PARTS:
            raise ValueError(f"X as parts needs 1 .. {_lib.TDA_MAX_PARTS} arrays")
        parts = [_cloud.prepare(x, _cloud.RIPSER, device, input_ready) for x in X]
        inp = parts[0]
        for i in parts[1:]:
            if i.keep.shape != inp.keep.shape or (i.on_dev, i.device, i.dtype) != (inp.on_dev, inp.device, inp.dtype):
                raise ValueError("parts must share shape, dtype and device")
    else:
        parts, inp = None, _cloud.prepare(X, _cloud.RIPSER, device, input_ready)
    _cloud.fill_head(a, inp, parts=parts)  # with the finite check of host input: before the shape's
    _, N, D = inp.shape
    if distance_matrix and D != N:
        raise ValueError("Distance matrix is not square")
    a.slot = int(slot)
    want_dist, lab = _fill_call_args(a, N, maxdim, thresh, distance_matrix, want_dist, stage_times, stage_serial, one_stream,
                                     input_ready, persistence, want_dist64, labels, twonn, discard_fraction, eps)
    out, info = _call_batch(a, want_dist)
    return (out, info) if return_time else out


_RIPSER_BATCH = ripser_batch  # the library's own batch call: what SweepPipeline's native workers stand for


class GreedyPerm:
    """Greedy furthest-point landmarks of L layers (:func:`greedy_perm_batch`).

    ``idx_perm`` (L, k) int64: the landmarks in selection order (the first is
    point 0); ``lambdas`` (L, k) float64 holding f32 values: insertion radii;
    ``r_cover`` (L,) = ``lambdas[:, -1]``: the covering radius; ``dperm2all``
    (L, k, N) float32: the landmarks' distances to every point, or None.
    ``device_ms`` / ``select_ms``: device time of the call and, of it, of the
    selection kernel."""

    __slots__ = ("idx_perm", "lambdas", "r_cover", "dperm2all", "device_ms", "select_ms")


@contextlib.contextmanager
def _greedy_call(X, n_perm, distance_matrix, device, want_dperm2all, input_ready=False):
    """One tda_greedy_perm call: yields (the prepared input, k, the library-owned result); the
    result, and with it the landmark matrices on the device, lives until the block ends."""
    if isinstance(X, (list, tuple)):
        raise ValueError("n_perm needs one (L, N, D) array: input in parts is not supported with it")
    if n_perm is None or int(n_perm) != n_perm:
        raise ValueError("n_perm must be an integer")
    inp = _cloud.prepare(X, _cloud.RIPSER, device, input_ready)
    inp.is_dist = bool(distance_matrix)
    _, N, D = inp.shape
    if distance_matrix and D != N:
        raise ValueError("Distance matrix is not square")
    if not 1 <= n_perm <= N:
        raise ValueError(f"n_perm must be in [1, N = {N}]")
    if inp.dtype == _lib.TDA_F64 and not distance_matrix:
        raise NotImplementedError("n_perm with float64 point clouds is not implemented (sklearn's row-wise and full "
                                  "float64 distances disagree): pass float32 points or a distance matrix")
    a = _lib.GreedyArgs()
    _cloud.fill_head(a, inp)
    a.n_perm = int(n_perm)
    a.want_dperm2all = 1 if want_dperm2all else 0
    with _lib.result("greedy", a) as r:
        yield inp, int(n_perm), r


def _greedy_unpack(inp, k, r) -> GreedyPerm:
    L, N, _ = inp.shape
    g = GreedyPerm()
    g.idx_perm = _arr(r.idx_perm, L * k, np.int64).reshape(L, k)
    g.lambdas = _arr(r.lambdas, L * k, np.float32).reshape(L, k).astype(np.float64)
    g.r_cover = g.lambdas[:, -1].copy()
    g.dperm2all = _arr(r.dperm2all, L * k * N, np.float32).reshape(L, k, N) if bool(r.dperm2all) else None
    g.device_ms, g.select_ms = float(r.device_ms), float(r.select_ms)
    return g


def greedy_perm_batch(X, n_perm: int, distance_matrix: bool = False, device: int = 0, want_dperm2all: bool = True) -> GreedyPerm:
    """ripser.py's ``get_greedy_perm`` for L layers in one call on the GPU.

    X: (L, N, D) float32 point clouds or (L, N, N) distance matrices
    (distance_matrix=True; upper triangle used, diagonal taken as 0), numpy or
    a torch CUDA tensor; N <= 8192.  Per layer, on the library's own f32
    distance matrix: start at point 0, then n_perm - 1 times take the point
    furthest from the landmarks so far (the lowest index among equal maxima,
    as numpy's argmax).  Returns a :class:`GreedyPerm`; every value in it is
    copied from the distance matrix, so it equals the host loop exactly."""
    with _greedy_call(X, n_perm, distance_matrix, device, want_dperm2all) as (inp, k, r):
        return _greedy_unpack(inp, k, r)


def greedy_perm(X, n_perm: int, distance_matrix: bool = False):
    """Single-cloud form of :func:`greedy_perm_batch`, returning ``(idx_perm,
    lambdas, dperm2all)`` like ripser.py's ``get_greedy_perm``."""
    X = X if _is_torch(X) else np.asarray(X)
    if X.ndim != 2:
        raise ValueError("X must be a 2-D array")
    g = greedy_perm_batch(X[None], n_perm, distance_matrix=distance_matrix)
    return g.idx_perm[0], g.lambdas[0], g.dperm2all[0]


def _ripser_batch_landmarks(X, n_perm, maxdim, thresh, distance_matrix, device, want_dist, return_time, stage_times, labels,
                            stage_serial, twonn, want_dist64, slot, persistence, one_stream, input_ready):
    """ripser_batch(n_perm=k): landmarks (tda_greedy_perm), then persistence of
    their (L, k, k) matrices where they lie on the device (tda_rips_batch with
    is_dist, x_on_device and TDA_FLAG_INPUT_READY: the greedy call has
    synchronised), then the landmarks' release."""
    if labels is not None or twonn:
        raise ValueError("labels / twonn with n_perm are not supported: on the landmarks alone they are not the "
                         "reference's scores of the cloud")
    if want_dist64:
        raise NotImplementedError("want_dist64 needs float64 point clouds, which n_perm does not take")
    with _greedy_call(X, n_perm, distance_matrix, device, False, input_ready) as (inp, k, r):
        g = _greedy_unpack(inp, k, r)
        L = inp.shape[0]
        a = _lib.RipsArgs()
        _cloud.fill_head(a, _cloud.on_device(r.sub_dev, (L, k, k), inp.device))
        a.slot = int(slot)
        want_dist, _ = _fill_call_args(a, k, maxdim, thresh, True, want_dist, stage_times, stage_serial, one_stream, True,
                                       persistence, False, None, False, 0.0, 0.0)
        out, info = _call_batch(a, want_dist)
    b = out[0][0]
    b.ip, b.rc = g.idx_perm, g.r_cover
    info = dict(info, greedy_device_ms=g.device_ms, greedy_select_ms=g.select_ms)
    return (out, info) if return_time else out


def ripser(X, maxdim: int = 1, thresh: float = np.inf, coeff: int = 2, distance_matrix: bool = False,
           do_cocycles: bool = False, metric: str = "euclidean", n_perm=None):
    """Drop-in for ``ripser.ripser`` (Vietoris-Rips persistence over Z/2).

    Returns the same dict as ripser.py: ``dgms`` (list of (n_k, 2) float64
    arrays, f32 values widened, ``inf`` for essential classes), ``cocycles``
    (empty lists), ``num_edges``, ``dperm2all`` (the N x N distance matrix:
    float32 for float32 points, float64 for float64 points as sklearn's
    pairwise_distances returns it; the given matrix for distance_matrix=True),
    ``idx_perm`` (arange N) and ``r_cover`` (0.0).
    ``n_perm`` raises here: the one-cloud entry is ``ripser_batch(X[None], n_perm=k)[0]``.
    """
    _check_common(maxdim, coeff, do_cocycles, n_perm, metric)
    if hasattr(X, "tocoo"):
        raise NotImplementedError("sparse distance matrices are not implemented")
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError("X must be a 2-D array")
    if distance_matrix:
        if X.shape[0] != X.shape[1]:
            raise ValueError("Distance matrix is not square")
        if np.any(np.diagonal(X) != 0):
            raise NotImplementedError("non-zero diagonal (lower-star filtration) is not implemented")
    elif X.shape[1] > X.shape[0]:
        warnings.warn("The input point cloud has more columns than rows; did you mean to transpose?")
    f64 = X.dtype == np.float64 and not distance_matrix
    res = ripser_batch(X[None], maxdim=maxdim, thresh=thresh, distance_matrix=distance_matrix, want_dist=True,
                       want_dist64=f64)[0]
    N = X.shape[0]
    return {
        "dgms": res.dgms,
        "cocycles": [[] for _ in range(maxdim + 1)],
        "num_edges": res.num_edges,
        "dperm2all": X if distance_matrix else (res.dist64 if f64 else res.dist),
        "idx_perm": np.arange(N),
        "r_cover": 0.0,
    }


def persistence_pairs(X, maxdim: int = 1, thresh: float = np.inf, distance_matrix: bool = False) -> LayerResult:
    """Like ``ripser`` but returns the LayerResult with simplex pair indices."""
    X = np.asarray(X)
    return ripser_batch(X[None], maxdim=maxdim, thresh=thresh, distance_matrix=distance_matrix, want_dist=True)[0]


def rips_dm(D_condensed, maxdim: int = 1, thresh: float = np.inf) -> LayerResult:
    """Condensed f32 distance vector (i<j row-major) -> LayerResult via the
    C entry ``tda_rips_dm`` that replaces ripser.py's ``rips_dm``."""
    D = np.ascontiguousarray(D_condensed, dtype=np.float32)
    L = _lib.lib()
    res = ctypes.POINTER(_lib.RipsResult)()
    thr = float(thresh) if np.isfinite(thresh) else float("inf")
    _lib.check(L.tda_rips_dm(D.ctypes.data_as(_lib._f32p), D.shape[0], 2, int(maxdim), thr, 0, ctypes.byref(res)))
    try:
        return _unpack(res, False)[0][0]
    finally:
        L.tda_rips_free(res)


def silhouette_score(X, labels) -> float:
    """Drop-in for the reference's ``sklearn.metrics.silhouette_score(cloud,
    labels)`` (debug_tda_pipeline.py:117-118; metric='euclidean'), computed by
    k_silhouette on the GPU distance matrix (one call, H0 only)."""
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError("X must be a 2-D array")
    return ripser_batch(X[None], maxdim=0, labels=[labels])[0].silhouette[0]


class _SweepFuture:
    """One submitted sweep of a SweepPipeline: ``result()`` is its own
    ``ripser_batch`` result (its layers of the coalesced call)."""

    def __init__(self, pipe, lo, hi):
        self._pipe, self._lo, self._hi = pipe, lo, hi
        self._call = None  # concurrent future of the coalesced call, once dispatched

    def result(self, timeout=None):
        if self._call is None:
            self._pipe._dispatch_pending(self)
        out = self._call.result(timeout)
        if isinstance(out, tuple):  # return_time: (results, info)
            res, info = out
            call = self._call
            shared = getattr(call, "_sweep_info", None)
            if shared is None:  # once per call: its sweeps share the dict
                shared = call._sweep_info = dict(info, coalesced=self._n)
            return res[self._lo:self._hi], shared
        return out[self._lo:self._hi]

    def done(self):
        return self._call is not None and self._call.done()


class _CallTemplate:
    """The arguments one native pipeline call shares with every call of the same
    keyword arguments: the C template (``tda_pipe_submit``'s ``tmpl``), what
    ``_unpack`` needs to read its results, and the label codes it points into.
    ``given`` holds the caller's own argument objects: the template is found
    by their identity (``SweepPipeline._args_key``), so they must not be freed,
    and their ids reused, while it can still be found."""

    __slots__ = ("id", "args", "ref", "want_dist", "n_sets", "return_time", "is_dist", "lab", "given")

    def __init__(self, tid, given, N, device, maxdim=1, thresh=np.inf, distance_matrix=False, want_dist=False,
                 return_time=False, stage_times=False, labels=None, stage_serial=False, twonn=False, discard_fraction=0.1,
                 eps=1e-10, want_dist64=False, persistence=True, one_stream=False, input_ready=False, n_perm=None):
        _check_common(maxdim, 2, False, n_perm, "euclidean")
        self.given = given
        a = _lib.RipsArgs()
        a.device = int(device)
        self.want_dist, self.lab = _fill_call_args(a, N, maxdim, thresh, distance_matrix, want_dist, stage_times, stage_serial,
                                                   one_stream, input_ready, persistence, want_dist64, labels, twonn,
                                                   discard_fraction, eps)
        self.id, self.args, self.ref = tid, a, ctypes.byref(a)
        self.n_sets, self.return_time, self.is_dist = int(a.n_label_sets), bool(return_time), bool(distance_matrix)


class _NativeFuture:
    """One sweep submitted to the library's own pipeline (``tda_pipe_*``): it
    holds the sweep's ticket.  ``result()`` blocks in one C call (no interpreter
    lock held).  The sweep's input array is kept alive by the pipeline, not by
    the future (``SweepPipeline._keeps``): a worker reads it whether or not
    anybody still wants the result."""

    __slots__ = ("_pipe", "_ticket", "_tmpl", "_out", "_exc", "__weakref__")

    def __init__(self, pipe, ticket, tmpl, exc=None):
        self._pipe, self._ticket, self._tmpl, self._out, self._exc = pipe, ticket, tmpl, None, exc

    def result(self, timeout=None):
        if self._ticket is not None:
            self._pipe._resolve(self, timeout)
        if self._exc is not None:
            raise self._exc
        return self._out

    def done(self):
        return self._ticket is None or self._pipe._poll(self._ticket, _lib.TDA_PIPE_POLL)

    def __del__(self):
        if self._ticket is not None:  # dropped unread: the pipeline hands the ticket back once its call has run
            self._pipe._abandon(self._ticket)


class SweepPipeline:
    """Consecutive layer-loop batches in flight at once: ``depth`` host threads,
    each on its own device workspace slot (streams, buffers, graphs), so batch
    i + 1 runs on the GPU while batch i finishes -- the dense small-N path is a
    chain of latency-bound kernels that leaves most CUs idle, and independent
    sweeps fill them.  ``submit(X)`` returns a future whose ``result()`` is
    ``ripser_batch(X, **kw)``'s; results come back in submission order when
    waited on in order.

    Host numpy input, and CUDA tensors submitted with ``input_ready=True``, run
    on the library's own pipeline (``tda_pipe_*``, csrc/sweep_pipe.h): native
    worker threads coalesce, call and hand results over, ``submit`` is one
    short C call and ``result()`` one blocking one, and the interpreter lock is
    never taken by a worker.  ``run=`` stand-ins and CUDA tensors that must wait
    for their producer's stream keep the Python path: one host thread per slot
    whose ctypes call releases the GIL, so the threads overlap their GPU waits.
    WHICH PATH RUNS: the native workers call the library's ``tda_rips_batch``
    and nothing else, so the native path is taken only while this module's
    ``ripser_batch`` is the library's own (``_RIPSER_BATCH``).  Replacing the
    module attribute (``ripser.ripser_batch = stand_in``: tests/test_api.py
    does so to record calls, tools/host_timeline.py to time the Python path)
    is honoured like ``run=stand_in`` -- every call goes through the stand-in on
    the Python threads.  There is no other switch; ``type(future)`` tells the
    path (``_NativeFuture`` / ``_SweepFuture``).
    On the native path ``result()`` of one call's sweeps shares one ``info``
    dict, and ``result(timeout)`` raises ``TimeoutError`` like the Python path.

    coalesce=c (dynamic batching): up to c consecutive submissions of the same
    shape, dtype and arguments run as ONE call over their concatenated layers
    (passed as parts: the library gathers them into its own input buffer, so
    the slot's captured graph is reused whatever the inputs' addresses)
    (a layer's result does not depend on the batch it is in:
    tests/test_gpu_parity.py batch-invariance tests); each future still returns
    its own sweep's layers.  A batch is dispatched when it holds c sweeps, when
    a different submission arrives, when one of its futures is waited on, or
    at flush() / close().
    run: the batch call (default :func:`ripser_batch`).
    one_stream: run each call on its slot's one stream (TDA_FLAG_ONE_STREAM),
    so every slot keeps to one hardware queue; the default is one_stream when
    depth > 1.  The calls run on the top ``depth`` workspace slots (slot 0,
    where plain ripser_batch calls run, is left alone).
    input_ready=True (a ripser_batch argument, passed through ``**kw``) is
    worth giving when the inputs are complete before submission: each call
    then skips its event on the caller's stream, whose hardware queue a slot
    may share."""

    def __init__(self, depth: int = 2, device: int = 0, coalesce: int = 1, one_stream=None, run=None, **kw):
        import threading
        from concurrent.futures import ThreadPoolExecutor

        if not 1 <= depth <= _lib.TDA_MAX_SLOTS:
            raise ValueError(f"depth must be in [1, {_lib.TDA_MAX_SLOTS}]")
        if not 1 <= coalesce <= _lib.TDA_MAX_PARTS:
            raise ValueError(f"coalesce must be in [1, {_lib.TDA_MAX_PARTS}]")
        self._check_kw(kw)
        self.depth, self.device, self.coalesce = depth, device, int(coalesce)
        self.kw = dict(kw, one_stream=depth > 1 if one_stream is None else bool(one_stream))
        # the top `depth` workspace slots: slot 0 (every plain ripser_batch call) keeps its
        # streams to itself, and the slots' streams each get a hardware queue of their own
        self.slots = list(range(_lib.TDA_MAX_SLOTS - depth, _lib.TDA_MAX_SLOTS))
        self._ex = [ThreadPoolExecutor(max_workers=1) for _ in range(depth)]  # one thread per slot: calls on a slot stay ordered
        self._n = 0
        self._lock = threading.Lock()
        self._pending = []  # (X, args, future, producer event or None) not yet dispatched
        self._plen = 0  # layers in _pending
        self._pkey = None
        self._kw_key = self._args_key(self.kw)
        self._run = run  # the batch call (default ripser_batch; CPU tests pass a stand-in)
        # the native path (run is None): the library's pipe, made at the first sweep it takes
        self._np = None
        self._closed = False
        self._tmpl = {}  # (argument key, device, N when labels are given) -> _CallTemplate
        self._tmpl_n = 0  # templates made so far: their ids are never reused
        # ticket -> (input array, template) until the ticket's call has run: a worker reads the
        # array (and the template's label codes) whether or not the future is still alive
        self._keeps = {}
        self._orphans = []  # tickets of futures dropped unread whose calls had not run yet
        self._tickets = {}  # ticket -> weak reference to its unread future (close() reads them)
        self._calls = {}  # call id -> (results, info) of a call some of whose futures are unread
        self._ulock = threading.RLock()  # one unpack per call (re-entrant: a collected future's __del__ may run under it)

    @staticmethod
    def _check_kw(kw):
        for k in ("slot", "device"):
            if k in kw:
                raise TypeError(f"SweepPipeline picks the {k} itself; do not pass {k}=")
        if kw.get("n_perm") is not None:
            raise NotImplementedError("SweepPipeline does not take n_perm: the greedy stage runs outside the slots "
                                      "(call ripser_batch(X, n_perm=k))")

    @staticmethod
    def _in_key(X):
        """Sweeps coalesce only with the same FULL shape (the C ABI's parts are
        equal: L % n_parts == 0), dtype, device and arguments (_args_key)."""
        return type(X).__module__, (X.device.type, X.device.index) if _is_torch(X) else None, tuple(X.shape), X.dtype

    @staticmethod
    def _args_key(args):
        """Scalar arguments compare by value; anything else (label arrays,
        lists) by identity -- a repr() of a large numpy array is summarised and
        two different arrays could compare equal."""

        def val(v):
            return ("v", v) if v is None or isinstance(v, (bool, int, float, str)) else ("id", id(v))

        return tuple(sorted((k, val(v)) for k, v in args.items()))

    def submit(self, X, **kw):
        if kw:
            self._check_kw(kw)
            args = dict(self.kw, **kw)
        else:  # the pipeline's own arguments (never mutated: a dispatch copies them)
            args = self.kw
        if not (_is_torch(X) and X.is_cuda):
            X = np.asarray(X)
        if X.ndim != 3:
            raise ValueError("X must be (L, N, D)")
        # a replaced module-level ripser_batch is a stand-in like run= (class docstring, WHICH PATH RUNS)
        if self._run is None and ripser_batch is _RIPSER_BATCH and (type(X) is np.ndarray or bool(args.get("input_ready"))):
            return self._submit_native(X, args, kw)
        if self._np is not None:  # a sweep for the Python path closes the native path's batch
            _lib.lib().tda_pipe_flush(self._np)
        ev = None
        if _is_torch(X) and X.is_cuda and not args.get("input_ready"):
            # ordered after the SUBMITTING thread's current stream, as of now: the call may be
            # dispatched later, from another thread (a future's result()), or after the caller
            # left a `with torch.cuda.stream(...)` block
            import torch

            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(X.device))
        with self._lock:
            # without call arguments the argument half of the key is the pipeline's own, computed once
            key = (self._in_key(X), self._args_key(args) if kw else self._kw_key)
            if self._pending and (key != self._pkey or self.coalesce == 1):
                self._dispatch_locked()
            lo = self._plen
            self._plen += int(X.shape[0])
            f = _SweepFuture(self, lo, self._plen)
            self._pending.append((X, args, f, ev))
            self._pkey = key
            if len(self._pending) >= self.coalesce:
                self._dispatch_locked()
            return f

    def _template(self, args, kw, device, N):
        """The native call template of these arguments (made once per argument key).
        Non-scalar arguments are keyed by identity; the template holds them
        (``given``), so an id in a key cannot pass to another object.  Per-submit
        arguments make a template each: past _MAX_TEMPLATES the table starts
        again (templates of calls still to run are held by ``_keeps``)."""
        key = (self._args_key(args) if kw else self._kw_key, device, N if args.get("labels") is not None else None)
        t = self._tmpl.get(key)
        if t is None:
            with self._lock:
                t = self._tmpl.get(key)
                if t is None:
                    if len(self._tmpl) >= self._MAX_TEMPLATES:
                        self._tmpl.clear()
                    self._tmpl_n += 1
                    t = self._tmpl[key] = _CallTemplate(self._tmpl_n, args, N, device, **args)
        return t

    _MAX_TEMPLATES = 64

    def _submit_native(self, X, args, kw):
        """One sweep into the library's pipe.  A bad submission raises from its
        future's result(), like a failed call."""
        if self._closed:
            raise RuntimeError("cannot submit to a closed SweepPipeline")
        if self._pending:  # a sweep for the native path closes the Python path's batch
            self.flush()
        if self._orphans:
            self._reap()
        L = _lib.lib()
        try:
            inp = _cloud.prepare(X, _cloud.RIPSER, self.device, True)
            Ls, N, D = inp.shape
            t = self._template(args, kw, inp.device, N)
            if t.is_dist and D != N:
                raise ValueError("Distance matrix is not square")
            if self._np is None:
                with self._lock:
                    if self._np is None:
                        h = ctypes.c_void_p()
                        _lib.check(L.tda_pipe_create(self.depth, self.coalesce, ctypes.byref(h)))
                        self._np = h
            ticket = ctypes.c_uint64()
            _lib.check(L.tda_pipe_submit(self._np, t.ref, t.id, inp.ptr if inp.on_dev else inp.keep.ctypes.data, Ls, N, D,
                                         inp.dtype, 1 if inp.on_dev else 0, ctypes.byref(ticket)))
        except Exception as e:
            return _NativeFuture(self, None, None, e)
        # from here on a worker may read the array: the pipeline holds it until the call has run
        self._keeps[ticket.value] = (inp.keep, t)
        f = _NativeFuture(self, ticket.value, t)
        self._tickets[f._ticket] = weakref.ref(f)
        return f

    def _poll(self, ticket, mode) -> bool:
        """Has the ticket's call run?  (mode TDA_PIPE_DISPATCH sends its batch off first.)"""
        res, lo, hi = ctypes.POINTER(_lib.RipsResult)(), ctypes.c_int64(), ctypes.c_int64()
        n, call = ctypes.c_int32(), ctypes.c_uint64()
        return _lib.lib().tda_pipe_wait(self._np, ticket, ctypes.byref(res), ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(n),
                                        ctypes.byref(call), mode) != _lib.TDA_PIPE_BUSY

    def _resolve(self, f, timeout=None):
        """Wait for the future's call, read its result (the first waiter of a
        call unpacks it for all of them) and hand the ticket back."""
        import time

        L = _lib.lib()
        ticket = f._ticket
        if ticket is None:  # another thread read it meanwhile
            return
        if timeout is not None:  # the C wait has no deadline: dispatch, then poll
            end = time.monotonic() + timeout
            mode = _lib.TDA_PIPE_DISPATCH
            while not self._poll(ticket, mode):
                if time.monotonic() >= end:
                    raise TimeoutError()
                mode = _lib.TDA_PIPE_POLL
                time.sleep(1e-4)
        res, lo, hi = ctypes.POINTER(_lib.RipsResult)(), ctypes.c_int64(), ctypes.c_int64()
        n, call = ctypes.c_int32(), ctypes.c_uint64()
        rc = L.tda_pipe_wait(self._np, ticket, ctypes.byref(res), ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(n),
                             ctypes.byref(call), _lib.TDA_PIPE_BLOCK)
        msg = L.tda_last_error().decode(errors="replace") if rc != 0 else None  # this thread's, before any other call
        with self._ulock:
            if f._ticket is None:  # another thread read it meanwhile
                return
            t = f._tmpl
            try:
                if rc != 0:
                    f._exc = _lib.ERRORS.get(rc, RuntimeError)(msg)
                else:
                    ent = self._calls.get(call.value)
                    if ent is None:
                        out, info = _unpack(res, t.want_dist, t.n_sets)
                        info["coalesced"] = n.value
                        ent = self._calls[call.value] = (out, info)
                    sl = ent[0][lo.value:hi.value]
                    f._out = (sl, ent[1]) if t.return_time else sl
            except Exception as e:
                f._exc = e
            finally:
                f._ticket = None
                self._tickets.pop(ticket, None)
                self._keeps.pop(ticket, None)  # the blocking wait returned: the call has run
                if L.tda_pipe_release(self._np, ticket) <= 0:  # the call's last ticket
                    self._calls.pop(call.value, None)

    def _abandon(self, ticket):
        """A future was dropped unread.  Its call may be pending, queued or
        running, and reads the sweep's array until it is done: the ticket is
        parked, and handed back (with the array) once a poll says the call ran."""
        if self._np is None:
            return
        self._tickets.pop(ticket, None)
        self._orphans.append(ticket)
        self._reap()

    def _reap(self):
        """Hand back the parked tickets whose calls have run; the others stay."""
        L = _lib.lib()
        res, lo, hi = ctypes.POINTER(_lib.RipsResult)(), ctypes.c_int64(), ctypes.c_int64()
        n, call = ctypes.c_int32(), ctypes.c_uint64()
        with self._ulock:
            if self._np is None:
                return
            parked, self._orphans = self._orphans, []
            for ticket in parked:
                rc = L.tda_pipe_wait(self._np, ticket, ctypes.byref(res), ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(n),
                                     ctypes.byref(call), _lib.TDA_PIPE_POLL)
                if rc == _lib.TDA_PIPE_BUSY:
                    self._orphans.append(ticket)
                    continue
                self._keeps.pop(ticket, None)
                if L.tda_pipe_release(self._np, ticket) <= 0:
                    self._calls.pop(call.value, None)

    def flush(self):
        """Dispatch the sweeps still waiting for a full batch."""
        with self._lock:
            if self._pending:
                self._dispatch_locked()
        if self._np is not None:
            _lib.lib().tda_pipe_flush(self._np)

    def _dispatch_pending(self, fut):
        with self._lock:
            if fut._call is None:
                self._dispatch_locked()

    def _dispatch_locked(self):
        batch, self._pending, self._plen = self._pending, [], 0
        run = self._run or ripser_batch
        e = self._n % self.depth  # executor (host thread) of this call
        s = self.slots[e]
        self._n += 1
        args = dict(batch[0][1])
        Xs = [b[0] for b in batch]
        evs = [b[3] for b in batch if b[3] is not None]
        X = Xs[0] if len(Xs) == 1 else Xs  # parts: gathered on the device by the library (ABI 6)
        if evs:
            # every part's producer, as recorded at its submit(): the slot's worker thread waits
            # for those events on the host, then calls with the input marked complete -- no extra
            # HIP stream per slot, whose hardware queue could be shared with another slot's
            # library stream
            args["input_ready"] = True

            def call():
                for ev in evs:
                    ev.synchronize()
                return run(X, device=self.device, slot=s, **args)

            cf = self._ex[e].submit(call)
        else:
            cf = self._ex[e].submit(run, X, device=self.device, slot=s, **args)
        for b in batch:
            b[2]._call, b[2]._n = cf, len(batch)

    def close(self):
        self.flush()
        for e in self._ex:
            e.shutdown(wait=True)
        self._closed = True
        if self._np is not None:
            # futures not read yet keep their results: read them now, the pipe takes every ticket with it
            for ref in list(self._tickets.values()):
                f = ref()
                if f is not None and f._ticket is not None:
                    self._resolve(f)
            self._destroy()

    def _destroy(self):
        """Destroy the pipe: it runs what is still pending or queued and joins its
        workers, and only then do the arrays those calls read go."""
        with self._ulock:
            h, self._np = self._np, None
        if h is not None:
            _lib.lib().tda_pipe_destroy(h)
        self._orphans = []
        self._keeps.clear()
        self._calls.clear()

    def __del__(self):
        # never closed.  No future is alive (each holds the pipeline), but calls of futures dropped
        # unread may still be pending or running: _keeps holds their arrays until the workers are joined
        if getattr(self, "_np", None) is not None:
            self._destroy()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
