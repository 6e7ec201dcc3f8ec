"""Geodesic distances over the neighbourhood graph on the GPU (include/tda_rips.h tda_geodesic).

Activations lie on curved sets, where the ambient Rips complex shortcuts across folds.  The
deterministic remedy is the graph geodesic: take the k-nearest-neighbour (or radius) graph of a layer
and use shortest-path lengths in it as the metric.  This is Isomap's metric, and what Naitzat,
Zhitnikov and Lim 2020 ("Topology of deep neural networks") feed to persistent homology.

One ``tda_geodesic`` call serves every layer: the layers' distance matrices on the device (the
kernels of ``ripser_batch``), the graph and its min-plus closure in place on them.  The result is a
distance matrix for every entry that takes ``distance_matrix=True``.
"""
from __future__ import annotations

import math

import numpy as np

from . import _cloud, _lib
from ._cloud import check_count as _check_count
from .ripser import _arr


class GeodesicDistances:
    """The geodesic distances of L layers (:func:`geodesic_distances`).

    ``dist`` (L, N, N) float32: the shortest-path lengths (or the graph's weights with
    ``graph_only``), ``inf`` between points of different components; ``n_components`` (L,) int32
    (-1 with ``graph_only``); ``n_edges`` (L,) int64: the undirected edges of the graph;
    ``connected`` (L,) bool: one component (None with ``graph_only``); ``device_ms``: the device
    time of the library call."""

    __slots__ = ("dist", "n_components", "n_edges", "connected", "device_ms")

    def filled(self, value) -> np.ndarray:
        """A copy of ``dist`` with ``inf`` replaced by the finite ``value``."""
        value = float(value)
        if not math.isfinite(value):
            raise ValueError(f"value must be finite, got {value}")
        out = self.dist.copy()
        out[np.isinf(out)] = value
        return out


def _check_graph(n_neighbors, radius):
    """(k, radius) as the C entry takes them: (k >= 1, -1.0) or (0, radius >= 0)."""
    if (n_neighbors is None) == (radius is None):
        raise ValueError("give exactly one of n_neighbors and radius")
    if n_neighbors is not None:
        k = _check_count("n_neighbors", n_neighbors)
        return min(k, 2 ** 31 - 1), -1.0
    radius = float(radius)
    if math.isnan(radius) or radius < 0.0:
        raise ValueError(f"radius must be >= 0 (inf allowed), got {radius}")
    return 0, radius


def geodesic_distances(X, n_neighbors=None, radius=None, distance_matrix: bool = False, graph_only: bool = False,
                       device: int = 0) -> GeodesicDistances:
    """Shortest-path distances in the neighbourhood graph of every layer, one library call.

    X: (L, N, D) float32 point clouds or (L, N, N) distance matrices (distance_matrix=True; upper
    triangle used, diagonal taken as 0; host matrices must be finite and >= 0), numpy or a torch
    CUDA tensor; N <= 8192 and L * N * N <= 2^28.  Exactly one of ``n_neighbors`` (k >= 1: every
    point is joined to its min(k, N - 1) nearest others, the lowest index winning ties, and an edge
    stands if either end chose it) and ``radius`` (>= 0, ``inf`` allowed: the pairs at distance
    <= radius) defines the graph on the library's own f32 distances.  ``dist[l]`` is the min-plus
    closure of the edge weights in f32: symmetric bit for bit, zero on the diagonal, within
    ``((1 + 2^-24)^c - 1)`` relative of the exact shortest length (c = N - 1 for N <= 128,
    66 * ceil(N / 64) above), exact for weights whose path sums are exact in f32, and ``inf``
    exactly between different components.  ``graph_only=True`` returns the graph's weights
    (``inf`` off the edges) and skips the closure.

    A disconnected layer (``connected[l]`` False: k or radius too small) holds ``inf``, which
    ``ripser_batch`` refuses in host matrices.  Raise ``n_neighbors`` or ``radius`` until the
    layer is connected, or pass ``filled(value)`` with a finite value above every finite distance:
    the components then merge at ``value`` in H0 and nothing else is added below it.

    Returns a :class:`GeodesicDistances`."""
    k, radius = _check_graph(n_neighbors, radius)
    inp = _cloud.table_input(X, distance_matrix, device)
    a = _lib.GeodesicArgs()
    _cloud.fill_head(a, inp)
    a.n_neighbors = k
    a.radius = radius
    a.graph_only = 1 if graph_only else 0
    g = GeodesicDistances()
    with _lib.result("geo", a) as r:
        L, N = inp.L, inp.N
        g.dist = _arr(r.dist, L * N * N, np.float32).reshape(L, N, N).copy()
        g.n_components = _arr(r.n_components, L, np.int32).copy()
        g.n_edges = _arr(r.n_edges, L, np.int64).copy()
        g.device_ms = float(r.device_ms)
    g.connected = None if graph_only else g.n_components == 1
    return g
