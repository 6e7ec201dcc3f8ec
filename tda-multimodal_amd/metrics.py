"""Layer metrics of the reference's metrics.py on the GPU.

``compute_effective_dimensionality`` mirrors metrics.py:5-44 (normalised
participation ratio of the singular values) through the C entry
``tda_effective_dim``: f64 Gram matrix on the FP64 matrix cores, Jacobi
eigenvalues on the GPU (csrc/ed_kernels.h).

``compute_intrinsic_dimensionality`` mirrors the reference's TorchScript
function of the same name (metrics.py:113-208: TwoNN with regression and
outlier discarding) -- same arguments, same (batch,) float32 result, NaN in the
same cases -- but runs as one library call: the distance kernel (FP64 MFMA Gram
tiles for D >= 32) and k_twonn (two nearest neighbours, sort, regression) for
all batch items at once.

``matrix_entropy`` / ``matrix_entropy_profile`` (metrics.py:344-399) take the
spectrum the effective dimensionality is computed from and apply the Renyi
epilogue of k_ed_jacobi to it (``tda_matrix_entropy``), several orders per
call.  ``compute_fixed_window_ed`` (metrics.py:47-109) and
``compute_fixed_window_id`` (metrics.py:211-265) are the two entries above
over non-overlapping token windows, one library call each.

There is no CPU fallback.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _cloud, _lib
from .ripser import ripser_batch


def compute_effective_dimensionality(activations_batch):
    """Normalised effective dimensionality (sum S)^2 / sum S^2 / min(n, d) of
    every (n_samples, embed_dim) item of ``activations_batch`` (batch, n, d),
    S = its singular values (metrics.py:5-44; the input is taken as float32,
    metrics.py:25).  Returns (batch,) float32: a torch tensor on the input's
    device for torch input, else a numpy array.

    Limit: min(n, d) <= 1024 (the f64 Gram matrix of the smaller side is
    eigen-solved in one workgroup); a full-sequence call with more than 1024
    tokens at D = 4096 (metrics.py:86) raises NotImplementedError."""
    inp = _cloud.prepare(activations_batch, _cloud.METRICS, ndim=None)
    x = inp.keep
    if x.ndim == 3:  # the order of these checks is the one callers have met since the entry exists
        inp.require_finite()
    if x.ndim == 3 and min(int(x.shape[1]), int(x.shape[2])) > 1024:
        raise NotImplementedError("compute_effective_dimensionality: min(n_samples, embed_dim) <= 1024 is supported")
    if x.ndim != 3:
        raise ValueError("activations_batch must be (batch_size, n_samples, embed_dim)")
    inp.shape = tuple(int(v) for v in x.shape)
    out = np.zeros(inp.L, np.float32)
    if inp.L:
        a = _lib.EdArgs()
        _cloud.fill_head(a, inp, names=("B", "N"))
        _lib.check(_lib.lib().tda_effective_dim(ctypes.byref(a), out.ctypes.data_as(_lib._f32p)))
    return _like_input(out, inp.like)


def _check_spectral_shape(what, n, d):
    """The Gram and Jacobi kernels' limits (include/tda_rips.h), before the library loads."""
    if n < 1 or d < 1:
        raise ValueError(f"{what}: every matrix needs at least one row and one column")
    if min(n, d) > 1024:
        raise NotImplementedError(f"{what}: min(n_samples, embed_dim) <= 1024 is supported")
    if n > 8192 and n <= d:
        raise NotImplementedError(f"{what}: n_samples <= 8192 is supported")


def _spectral_call(entry, inp, B, S, D, n_windows, out, alphas=None, eps=0.0):
    a = _lib.SpectralArgs()
    inp.shape = (B, S, D)
    _cloud.fill_head(a, inp, names=("B", "S"))
    a.n_windows = n_windows
    if alphas is not None:
        a.n_alpha, a.alphas, a.eps = len(alphas), alphas.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), eps
    _lib.check(getattr(_lib.lib(), entry)(ctypes.byref(a), out.ctypes.data_as(_lib._f32p)))


def matrix_entropy_profile(matrix, alphas, eps: float = 1e-10):
    """Matrix-based Renyi entropy (the reference's matrix_entropy,
    metrics.py:344-399) of every (N, D) matrix of ``matrix`` (..., N, D) at
    each order of ``alphas``, from one library call: the spectrum is computed
    once per matrix (f64 Gram matrix, Jacobi eigenvalues) and every order is
    evaluated on it.  Returns (..., len(alphas)) float32: a torch tensor on the
    input's device for torch input, else a numpy array.

    The spectrum is that of the smaller Gram matrix (min(N, D) eigenvalues):
    for N > D the reference's further N - D eigenvalues are zeros in exact
    arithmetic and add nothing for alpha > 0.  Orders alpha <= 0, where the
    reference's answer is decided by float32 noise in those zeros, raise
    ValueError; so do more than 16 orders in one call.  Limit:
    min(N, D) <= 1024 (NotImplementedError above)."""
    al = np.ascontiguousarray(np.asarray(alphas, dtype=np.float64).ravel())
    if not 1 <= al.size <= _lib.TDA_MAX_ALPHAS:
        raise ValueError(f"matrix entropy: 1 .. {_lib.TDA_MAX_ALPHAS} orders per call, got {al.size}")
    if not np.all(np.isfinite(al) & (al > 0.0)):
        raise ValueError("matrix entropy: every order alpha must be finite and > 0")
    if not eps >= 0.0:
        raise ValueError("matrix entropy: eps must be >= 0")
    inp = _cloud.prepare(matrix, _cloud.METRICS, ndim=None)
    x = inp.keep
    if x.ndim < 2:
        raise ValueError("matrix must be (..., N, D)")
    lead = tuple(int(v) for v in x.shape[:-2])
    n, d = int(x.shape[-2]), int(x.shape[-1])
    _check_spectral_shape("matrix_entropy", n, d)
    inp.require_finite()
    B = int(np.prod(lead, dtype=np.int64))
    out = np.zeros((B, al.size), np.float32)
    if B:
        _spectral_call("tda_matrix_entropy", inp, B, n, d, 0, out, al, float(eps))
    return _like_input(out.reshape(lead + (al.size,)), inp.like)


def matrix_entropy(matrix, alpha: float = 1.0, eps: float = 1e-10):
    """The reference's matrix_entropy (metrics.py:344-399) on the GPU: the
    Renyi entropy of order ``alpha`` (Shannon's for |alpha - 1| < eps) of the
    normalised Gram spectrum of every (N, D) matrix of ``matrix`` (..., N, D).
    Returns float32 of the leading shape; see matrix_entropy_profile."""
    return matrix_entropy_profile(matrix, [alpha], eps)[..., 0]


def compute_fixed_window_ed(activations_batch, n_windows: int):
    """compute_effective_dimensionality over ``n_windows`` non-overlapping
    windows of seq_len // n_windows tokens of ``activations_batch`` (batch,
    seq_len, embed_dim); the last seq_len % n_windows tokens are dropped
    (metrics.py:47-109).  Returns (batch, n_windows) float32.  ``n_windows <=
    0`` raises ValueError; ``n_windows > seq_len`` is taken as seq_len (every
    token its own window), as in the reference."""
    n_windows = int(n_windows)
    if n_windows <= 0:
        raise ValueError("n_windows must be positive")
    inp = _cloud.prepare(activations_batch, _cloud.METRICS, ndim=None)
    x = inp.keep
    if x.ndim != 3:
        raise ValueError("activations_batch must be (batch_size, seq_len, embed_dim)")
    B, S, D = (int(v) for v in x.shape)
    if S < 1:
        raise ValueError("compute_fixed_window_ed: seq_len >= 1 is needed")
    W = min(n_windows, S)  # metrics.py:63-73
    _check_spectral_shape("compute_fixed_window_ed", S // W, D)
    inp.require_finite()
    out = np.zeros((B, W), np.float32)
    if B:
        _spectral_call("tda_effective_dim_windows", inp, B, S, D, W, out)
    return _like_input(out, inp.like)


_TWONN_EPS = 1e-10  # compute_intrinsic_dimensionality's default, and what its windowed form passes


def compute_fixed_window_id(activations_batch, n_windows: int, discard_fraction: float = 0.1):
    """compute_intrinsic_dimensionality (TwoNN) over ``n_windows``
    non-overlapping windows of seq_len // n_windows tokens (metrics.py:211-265):
    one ripser_batch call over all batch * n_windows windows.  Returns (batch,
    n_windows) float32, all NaN in the reference's cases: n_windows <= 0,
    seq_len < n_windows, seq_len < 6 or a window of fewer than 6 tokens."""
    n_windows = int(n_windows)
    inp = _cloud.prepare(activations_batch, _cloud.METRICS, ndim=None)
    x = inp.keep
    if x.ndim != 3:
        raise ValueError("activations_batch must be (batch_size, seq_len, embed_dim)")
    B, S, D = (int(v) for v in x.shape)
    ws = S // n_windows if n_windows > 0 else 0
    if n_windows <= 0 or S < n_windows or S < 6 or ws < 6:  # metrics.py:228-245
        return _like_input(np.full((B, max(n_windows, 0)), np.nan, dtype=np.float32), inp.like)
    # no remainder: a view of the input; else the kept tokens, copied contiguous
    windows = x[:, : n_windows * ws, :].reshape(B * n_windows, ws, D)
    return _like_input(_twonn(windows, discard_fraction, _TWONN_EPS).reshape(B, n_windows), inp.like)


def _like_input(out, dev):
    """A torch tensor on ``dev`` for torch input (dev is not None), else the numpy array."""
    if dev is None:
        return out
    import torch

    return torch.from_numpy(np.ascontiguousarray(out)).to(dev)


def compute_intrinsic_dimensionality(data, discard_fraction: float = 0.1, eps: float = _TWONN_EPS):
    """TwoNN intrinsic dimension of each (n_samples, embed_dim) item of
    ``data`` (batch, n_samples, embed_dim).  Returns a torch float32 tensor on
    the input's device for torch input, else a numpy float32 array.

    The distances are the hot path's (sklearn's f64-accumulated Euclidean form
    rounded to f32) where the reference uses torch.cdist in f32; estimates
    agree within the tolerance stated in tests/test_gpu_parity.py.  No
    persistence is computed (TDA_FLAG_NO_PERSISTENCE).  n_samples <= 8192 (the
    per-item ratio sort runs in LDS); the reference has no such limit."""
    inp = _cloud.prepare(data, _cloud.METRICS, ndim=None)  # float32: metrics.py:140
    if inp.keep.ndim != 3:
        raise ValueError("data must be (batch_size, n_samples, embed_dim)")
    return _like_input(_twonn(inp.keep, discard_fraction, eps), inp.like)


def _twonn(x, discard_fraction, eps) -> np.ndarray:
    """(batch,) float32 TwoNN estimates of prepared (batch, n, d) float32 input."""
    B, n = int(x.shape[0]), int(x.shape[1])
    if n <= 5 or B == 0:  # metrics.py:136-137
        return np.full(B, np.nan, dtype=np.float32)
    # distances + k_twonn only (TDA_FLAG_NO_PERSISTENCE): the reference computes no persistence here
    res = ripser_batch(x, maxdim=0, twonn=True, discard_fraction=discard_fraction, eps=eps, persistence=False)
    return np.array([r.twonn for r in res], dtype=np.float32)
