"""The one way a point cloud or a distance matrix gets from the caller into an args struct.

Every entry that takes (L, N, D) clouds or (L, N, N) matrices -- ripser_batch and what is built on
it, greedy_perm_batch, hausdorff_resamples, h0_subsamples, the spectral metrics, TwoNN, umap_batch
-- prepares its input with :func:`prepare` and writes the shared head of its args struct with
:func:`fill_head`.  Where the entries differ on purpose, a Policy says so: RIPSER, METRICS, UMAP.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import _lib


class Policy(NamedTuple):
    host_kept: tuple  # the numpy dtypes a host array keeps
    host_else: np.dtype  # what any other host dtype is converted to
    dev_kept: tuple  # the torch dtypes (by name) a CUDA tensor keeps
    dev_else: str | None  # what any other is converted to on the device; None: ValueError, no conversion
    finite_in_c: bool  # host input is checked for NaN / infinity by fill_head (hostviews().finite_ptrs, every part of
    #                    a call at once); else by the caller, where CloudInput.require_finite() stands in its order of checks
    device_from_argument: bool  # a CUDA tensor without a device index: the ``device`` argument; else torch's current device
    cpu_tensor: str | None  # a torch CPU tensor: "numpy": .detach().cpu().numpy(); a torch dtype name: converted to it in torch
    #                         first (what numpy has no dtype for, bfloat16, gets through); None: np.asarray, which refuses requires_grad


_F32, _F64 = np.dtype(np.float32), np.dtype(np.float64)  # dtype objects: comparing a dtype with a scalar type converts it first
RIPSER = Policy((_F32, _F64), _F64, ("float32", "float64"), "float64", True, False, "numpy")
METRICS = Policy((_F32,), _F32, ("float32",), "float32", False, False, "float32")
UMAP = Policy((_F64,), _F32, ("float32", "float64"), None, False, True, None)


def is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def raw_stream(device: int) -> int:
    """torch's current stream on that device, as a raw handle (no Stream object per call); 0: the null stream."""
    import torch

    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    return raw(device) if raw else torch.cuda.current_stream(device).cuda_stream


class CloudInput:
    """One prepared input.  ``keep``: the contiguous array the library reads (a numpy array, or a
    CUDA tensor when ``on_dev``), referenced from here until the call has returned; ``device``: the
    ordinal the call runs on; ``dtype``: TDA_F32 / TDA_F64; ``shape``: the (L, N, D) written into
    the struct (None until the caller sets it, for input not checked to be 3-d); ``is_dist``: set
    by the caller; ``finite_in_c``: its Policy's.  ``stream``, ``like`` and ``ptr`` are None for
    numpy input; torch input is a TorchInput."""

    __slots__ = ("keep", "on_dev", "device", "dtype", "shape", "finite_in_c", "is_dist")
    stream = like = ptr = None

    def __init__(self, keep, on_dev, device, dtype, shape, finite_in_c):
        self.keep = keep
        self.on_dev = on_dev
        self.device = device
        self.dtype = dtype
        self.shape = shape
        self.finite_in_c = finite_in_c
        self.is_dist = False

    L = property(lambda self: self.shape[0])  # for the callers' checks; fill_head reads ``shape``
    N = property(lambda self: self.shape[1])
    D = property(lambda self: self.shape[2])

    @property
    def is64(self) -> bool:
        return self.dtype == _lib.TDA_F64

    def require_finite(self):
        """The finite check of the families whose callers place it (Policy.finite_in_c False); device input is never checked."""
        if not self.on_dev and not np.all(np.isfinite(self.keep)):
            raise ValueError("Input contains NaN or infinity")


class TorchInput(CloudInput):
    """A prepared torch tensor.  ``stream``: the caller's stream a call on a CUDA tensor is ordered
    after, or None (a CPU tensor, ``input_ready``, the null stream); ``like``: the tensor's torch
    device, for ``metrics._like_input``; ``ptr``: the data pointer of device input."""

    __slots__ = ("stream", "like", "ptr")

    def __init__(self, keep, on_dev, device, dtype, shape, finite_in_c, stream, like, ptr):
        self.keep = keep
        self.on_dev = on_dev
        self.device = device
        self.dtype = dtype
        self.shape = shape
        self.finite_in_c = finite_in_c
        self.is_dist = False
        self.stream = stream
        self.like = like
        self.ptr = ptr


_KEPT = {}  # Policy.dev_kept -> those torch dtypes (torch is imported by the first call that sees a tensor)


def prepare(X, policy: Policy, device: int = 0, input_ready: bool = False, ndim: int | None = 3) -> CloudInput:
    """Torch or numpy, device or host: ``X`` as the contiguous array the library reads.

    ``device``: where a call on host input runs (for device input the tensor's own device wins).
    ``input_ready``: the caller has synchronised after producing a CUDA tensor, so no stream to
    order the call after.  ``ndim``: 3 raises "X must be (L, N, D)" for anything else, before any
    conversion; None leaves the shape to the caller."""
    like = None
    if type(X) is not np.ndarray:
        if is_torch(X):
            import torch

            if X.is_cuda:
                if ndim is not None and X.dim() != ndim:
                    raise ValueError("X must be (L, N, D)")
                kept = _KEPT.get(policy.dev_kept)
                if kept is None:
                    kept = _KEPT[policy.dev_kept] = tuple(getattr(torch, n) for n in policy.dev_kept)
                if X.dtype not in kept:
                    if policy.dev_else is None:
                        raise ValueError("X must be float32 or float64")
                    X = X.to(getattr(torch, policy.dev_else))
                keep = X.contiguous()  # no detach: the library reads the data pointer, which a tensor that requires grad has too
                like = keep.device
                if like.index is not None:
                    device = like.index
                else:
                    device = int(device) if policy.device_from_argument else torch.cuda.current_device()
                # input_ready: no device-side ordering on the caller's stream (whose queue a pipeline slot may share)
                stream = None if input_ready else (raw_stream(device) or None)
                return TorchInput(keep, True, device, _lib.TDA_F64 if keep.dtype == torch.float64 else _lib.TDA_F32,
                                  keep.shape if ndim == 3 else None, policy.finite_in_c, stream, like, keep.data_ptr())
            like = X.device
            if policy.cpu_tensor == "numpy":
                X = X.detach().cpu().numpy()
            elif policy.cpu_tensor is not None:
                X = X.detach().to(getattr(torch, policy.cpu_tensor)).numpy()
        X = np.asarray(X)
    if ndim is not None and X.ndim != ndim:
        raise ValueError("X must be (L, N, D)")
    if X.dtype not in policy.host_kept:
        X = X.astype(policy.host_else)
    keep = np.ascontiguousarray(X)
    dtype = _lib.TDA_F64 if keep.dtype == _F64 else _lib.TDA_F32
    shape = keep.shape if ndim == 3 else None
    if like is None:
        return CloudInput(keep, False, int(device), dtype, shape, policy.finite_in_c)
    return TorchInput(keep, False, int(device), dtype, shape, policy.finite_in_c, None, like, None)


def on_device(ptr: int, shape: tuple, device: int) -> TorchInput:
    """float32 distance matrices the library itself left on the device, complete (no stream to wait for)."""
    inp = TorchInput(None, True, int(device), _lib.TDA_F32, shape, False, None, None, ptr)
    inp.is_dist = True
    return inp


def table_input(X, distance_matrix: bool, device: int) -> CloudInput:
    """One prepared (L, N, D) input of the index-table entries (tda_resample, tda_subsample_h0),
    checked before any library call."""
    if isinstance(X, (list, tuple)):
        raise ValueError("resampling needs one (L, N, D) array: input in parts is not supported")
    inp = prepare(X, RIPSER, device)
    inp.is_dist = bool(distance_matrix)
    if inp.is_dist and inp.D != inp.N:
        raise ValueError("Distance matrix is not square")
    if inp.is64 and not inp.is_dist:
        raise NotImplementedError("resampling of float64 point clouds is not implemented (sklearn's row-wise and full "
                                  "float64 distances disagree): pass float32 points or a distance matrix")
    return inp


def fill_table_head(a, inp: CloudInput, idx: np.ndarray):
    """The shared head and the index table of a tda_resample or tda_subsample_h0 call."""
    fill_head(a, inp)
    a.B, a.m = int(idx.shape[-2]), int(idx.shape[-1])
    a.idx_per_layer = 1 if idx.ndim == 3 else 0
    a.idx = idx.ctypes.data


def fill_head(a, inp, names=None, parts=None):
    """The shared head of a fresh args struct: ``x``, ``dtype``, ``x_on_device``, the shape (as
    ``L``, ``N``, ``D``; ``names`` gives the first two where the struct calls them ``B`` or ``S``),
    ``is_dist``, ``device``, ``stream``.  ``parts``: a list of equal inputs, ``inp`` the first, for
    ``x_parts`` / ``n_parts`` (ABI 6: their layers one batch) in place of ``x``.  The data pointers
    are taken here, and with them the ripser family's finite check of host input.  The caller holds
    its inputs until the call has returned; the struct holds the parts' pointer array."""
    L, N, a.D = inp.shape
    if parts:
        L *= len(parts)
        ptrs = [i.ptr for i in parts] if inp.on_dev else _lib.hostviews().finite_ptrs([i.keep for i in parts])
        a._parts = (ctypes.c_void_p * len(parts))(*ptrs)
        a.x_parts = ctypes.cast(a._parts, ctypes.c_void_p)
        a.n_parts = len(parts)
    elif inp.on_dev:
        a.x = inp.ptr
    elif inp.finite_in_c:
        a.x = _lib.hostviews().finite_ptrs((inp.keep,))[0]
    else:
        a.x = inp.keep.ctypes.data
    if names is None:
        a.L = L
        a.N = N
    else:
        setattr(a, names[0], L)
        setattr(a, names[1], N)
    a.dtype = inp.dtype
    a.device = inp.device
    if inp.on_dev:
        a.x_on_device = 1
        a.stream = inp.stream
    if inp.is_dist:
        a.is_dist = 1


def check_count(name: str, v) -> int:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        if not (isinstance(v, (float, np.floating)) and float(v).is_integer()):
            raise ValueError(f"{name} must be a positive integer, got {v!r}")
    if v < 1:
        raise ValueError(f"{name} must be a positive integer, got {v!r}")
    return int(v)


def check_table(idx, sizes, L: int, N: int):
    """idx as a contiguous int32 (B, m) or (L, B, m) table and sizes as int32 (B,), None meaning every
    row whole: 1 <= sizes[b] <= m and the first sizes[b] entries of every row are indices into
    0 .. N-1 (the rest is never read)."""
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
