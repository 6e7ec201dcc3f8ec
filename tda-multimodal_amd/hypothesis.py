"""Do two (or more) sets of persistence diagrams differ?  The permutation test of Robinson and
Turner (2017, "Hypothesis testing for topological data analysis") on the GPU
(include/tda_rips.h tda_permutation_test).

From the pairwise distances D between all diagrams and their group labels, the statistic is the
weighted within-group sum ``sigma^2 = sum_g 1 / (2 n_g (n_g - 1)) sum_{i, j in g} D[i, j]^q``; the
null distribution is the same statistic under B random relabellings, and the p-value is
``(1 + #{b : T_b <= T_obs}) / (B + 1)`` (Phipson and Smyth 2010: never 0).

The library defines the statistic as a function of the partition alone, every addition in a pinned
order (tda_rips.h), so two relabellings that describe the same split of the diagrams give the same
bits and ``T_b <= T_obs`` is never decided by rounding: with small groups, where relabellings
often reproduce the observed split, numpy's gathers or one-hot products do not give that.

Every input already comes from this package: the ``*_matrix`` entries of :mod:`diagrams` give
bitwise-symmetric float64 distance matrices, and ``resample_indices`` with ``ripser_batch`` many
diagrams per condition.
"""
from __future__ import annotations

import numpy as np

from . import _lib, diagrams
from ._cloud import check_count as _check_count

METRICS = ("sliced_wasserstein", "bottleneck", "wasserstein", "heat", "fisher")


def _codes(labels):
    """(groups, uint8 codes) of any hashable labels, coded by np.unique."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or labels.size == 0:
        raise ValueError(f"labels must be a non-empty 1-d sequence, got shape {labels.shape}")
    groups, codes = np.unique(labels, return_inverse=True)
    if len(groups) > _lib.TDA_PERM_MAX_GROUPS:
        raise NotImplementedError(f"{len(groups)} groups: at most {_lib.TDA_PERM_MAX_GROUPS} are supported")
    return groups, np.ascontiguousarray(codes.reshape(-1), dtype=np.uint8)


def label_permutations(labels, B: int, seed: int = 0) -> np.ndarray:
    """B random relabellings: a (B, S) uint8 table whose rows are permutations of the codes of
    ``labels`` (``np.unique`` order), drawn with ``numpy.random.default_rng(seed).permuted`` (the
    same seed gives the same table).  The counterpart of ``resample_indices``."""
    B = _check_count("B", B)
    _, codes = _codes(labels)
    return np.ascontiguousarray(np.random.default_rng(seed).permuted(np.tile(codes, (B, 1)), axis=1))


def pvalue_from_null(null, t_obs: float):
    """(count, pvalue) of a null distribution: ``count = #{b : null[b] <= t_obs}`` and
    ``pvalue = (1 + count) / (B + 1)``, what the library returns."""
    null = np.asarray(null, dtype=np.float64).reshape(-1)
    count = int(np.count_nonzero(null <= np.float64(t_obs)))
    return count, float(np.float64(1 + count) / np.float64(null.size + 1))


class PermutationTest:
    """Result of :func:`permutation_test`.  ``statistic``: T of the observed labels; ``pvalue``
    = (1 + ``count``) / (``B`` + 1) with ``count`` the relabellings whose statistic is <= the
    observed one; ``groups``: the distinct labels in code order; ``null``: the (B,) float64
    statistics of the relabellings (``return_null=True``) or None; ``device_ms``: the call's
    device time."""

    __slots__ = ("statistic", "pvalue", "count", "B", "groups", "null", "device_ms")

    def __repr__(self):
        return f"PermutationTest(statistic={self.statistic!r}, pvalue={self.pvalue!r}, count={self.count}, B={self.B})"


def permutation_test(D, labels, B: int = 9999, q: float = 1.0, seed: int = 0, permutations=None, device: int = 0,
                     return_null: bool = False) -> PermutationTest:
    """The permutation test of Robinson and Turner on an (S, S) distance matrix.

    D: symmetric (bit for bit), zero diagonal, finite and >= 0, as the ``*_matrix`` entries return
    it; S <= 2048.  labels: S hashable values, coded by ``np.unique``; at most 64 groups, each of
    at least 2 members.  The statistic is taken on ``W = D`` for q == 1, else ``np.power(D, q)``.
    The B relabellings are ``label_permutations(labels, B, seed)`` or the given ``permutations``,
    a (B, S) table of codes whose rows are permutations of the observed codes (B is then its);
    B * S <= 2^27.  One library call.  Returns a :class:`PermutationTest`; every value is
    bit-reproducible and depends on the partitions only (module docstring)."""
    q = float(q)
    if not (np.isfinite(q) and q > 0):
        raise ValueError(f"q must be finite and > 0, got {q}")
    D = np.asarray(D, dtype=np.float64)
    if D.ndim != 2 or D.shape[0] != D.shape[1]:
        raise ValueError(f"D must be a square matrix, got shape {D.shape}")
    S = int(D.shape[0])
    groups, obs = _codes(labels)
    if obs.size != S:
        raise ValueError(f"labels must hold one label per row of D: {obs.size} labels for S = {S}")
    with np.errstate(all="ignore"):
        W = np.ascontiguousarray(D if q == 1.0 else np.power(D, q))
    if not np.isfinite(W).all():
        raise ValueError("D ** q holds a non-finite value")
    if permutations is None:
        lab = label_permutations(labels, B, seed)
    else:
        lab = np.asarray(permutations)
        if lab.dtype.kind not in "iu" or lab.ndim != 2 or lab.shape[0] < 1 or lab.shape[1] != S:
            raise ValueError(f"permutations must be a non-empty (B, S = {S}) integer table, got dtype {lab.dtype}, shape {lab.shape}")
        if lab.min() < 0 or lab.max() >= len(groups):
            raise ValueError(f"permutations must hold codes in 0 .. {len(groups) - 1}, got {int(lab.min())} .. {int(lab.max())}")
        lab = np.ascontiguousarray(lab, dtype=np.uint8)
    a = _lib.PermArgs()
    a.w, a.obs, a.lab = W.ctypes.data, obs.ctypes.data, lab.ctypes.data
    a.S, a.B, a.G = S, int(lab.shape[0]), len(groups)
    a.device, a.reserved = int(device), 0
    with _lib.result("perm", a) as r:
        out = PermutationTest()
        out.statistic, out.pvalue, out.count, out.B = float(r.t_obs), float(r.pvalue), int(r.count), int(r.B)
        out.groups, out.device_ms = groups, float(r.device_ms)
        out.null = np.ctypeslib.as_array(r.null, shape=(out.B,)).copy() if return_null else None
        return out


def diagram_permutation_test(dgms, labels, metric: str = "wasserstein", dim: int = 1, M: int = 50, sigma: float = 0.4, device: int = 0,
                             **kw) -> PermutationTest:
    """The permutation test between groups of diagrams: one call to the ``metric``'s matrix entry
    (``wasserstein_matrix``, ``bottleneck_matrix``, ``sliced_wasserstein_matrix`` over ``M``
    directions, ``heat_matrix`` or ``fisher_matrix`` at scale ``sigma``), then :func:`permutation_test` on it with
    the remaining arguments (B, q, seed, permutations, return_null).  ``dgms`` is whatever those
    entries accept: a list of (n, 2) arrays, or of ``LayerResult`` (then diagram ``dim`` of each)."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    if metric == "sliced_wasserstein":
        D = diagrams.sliced_wasserstein_matrix(dgms, M=M, device=device, dim=dim)
    elif metric == "heat":
        D = diagrams.heat_matrix(dgms, sigma=sigma, device=device, dim=dim)
    elif metric == "fisher":
        D = diagrams.fisher_matrix(dgms, sigma=sigma, device=device, dim=dim)
    elif metric == "bottleneck":
        D = diagrams.bottleneck_matrix(dgms, device=device, dim=dim)
    else:
        D = diagrams.wasserstein_matrix(dgms, device=device, dim=dim)
    return permutation_test(D, labels, device=device, **kw)
