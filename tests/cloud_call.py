"""What reaches the library from the entries that take point clouds or distance matrices: a
recording stand-in for ``_lib.lib()`` and the grid of calls tests/test_cloud_call_cpu.py pins
against tests/golden/cloud_call_args.json (written by tests/golden/make_golden_cloud_call.py).

The stand-in records every entry's symbol and a snapshot of its args struct, then refuses (-1,
``tda_last_error`` = REFUSAL).  Scalar fields are recorded by value (floats as ``float.hex``), a
pointer field as NULL or the SHA-256 of the bytes it points to, their length taken from the other
fields; a device pointer (``x_on_device``) is recorded as the number it is.  ``tda_greedy_perm``
alone succeeds, with a fabricated result whose ``sub_dev`` is SUB_DEV, so that the persistence call
of ``ripser_batch(n_perm=k)`` is recorded too.  No device is needed: _hostviews.so is (the finite
check of the ripser family runs in it).
"""
from __future__ import annotations

import ctypes
import hashlib
import importlib

import numpy as np

REFUSAL = "stand-in: recorded and refused"
SUB_DEV = 0x5EED0000
PIPE = 0x7070
L, N, D = 2, 5, 3


def _sha(ptr, nbytes: int) -> str:
    return hashlib.sha256(ctypes.string_at(ptr, nbytes) if nbytes else b"").hexdigest()


def _addr(v):
    if v is None or isinstance(v, int):
        return v or None
    return ctypes.cast(v, ctypes.c_void_p).value


def snapshot(a, **known) -> dict:
    """One args struct as JSON: see the module docstring.  ``known``: fields to take lengths from
    where the struct leaves them 0 (a pipeline template's N comes with the submit)."""
    f = {name: getattr(a, name) for name, _ in a._fields_}
    sized = dict(f, **known)
    item = 8 if f.get("dtype") == 1 else 4
    lead = f["L"] if "L" in f else f.get("B", 0)
    cloud = lead * f.get("N", f.get("S", 0)) * f.get("D", 0) * item
    n_parts = f.get("n_parts", 0)
    length = {
        "x": cloud,
        "idx": (f.get("L", 1) if f.get("idx_per_layer") else 1) * f.get("B", 0) * f.get("m", 0) * 4,
        "sizes": f.get("B", 0) * 4,
        "labels": f.get("n_label_sets", 0) * sized.get("N", 0) * 4,
        "alphas": f.get("n_alpha", 0) * 8,
    }
    out = {}
    for name, ctype in a._fields_:
        v = f[name]
        if name in ("out", "graph_out"):  # where the library writes: only whether it is given
            out[name] = "NULL" if not _addr(v) else "given"
        elif name == "x" and f.get("x_on_device") and _addr(v):
            out[name] = {"device_pointer": _addr(v)}
        elif name == "x_parts":
            p = _addr(v)
            if not p:
                out[name] = "NULL"
            else:
                ptrs = (ctypes.c_void_p * n_parts).from_address(p)
                out[name] = ["NULL" if not q else _sha(q, cloud // n_parts) for q in ptrs]
        elif name in length:
            p = _addr(v)
            out[name] = "NULL" if not p else _sha(p, length[name])
        elif ctype in (ctypes.c_float, ctypes.c_double):
            out[name] = float(v).hex()
        elif ctype is ctypes.c_void_p:
            out[name] = "NULL" if not v else int(v)
        else:
            out[name] = int(v)
    return out


class StandIn:
    """The recording library.  ``calls``: [symbol, args snapshot or None] in call order."""

    def __init__(self, lb):
        self.lb = lb
        self.calls = []
        self._held = []
        self._tickets = 0

    def tda_last_error(self):
        return REFUSAL.encode()

    def tda_greedy_perm(self, a, res):
        a = a._obj
        self.calls.append(["tda_greedy_perm", snapshot(a)])
        k = int(a.n_perm)
        r = self.lb.GreedyResult()
        idx = (ctypes.c_int64 * (a.L * k))(*([0] * (a.L * k)))
        lam = (ctypes.c_float * (a.L * k))(*([0.5] * (a.L * k)))
        r.L, r.N, r.n_perm, r.device, r.sub_dev = a.L, a.N, k, a.device, SUB_DEV
        r.idx_perm = ctypes.cast(idx, ctypes.POINTER(ctypes.c_int64))
        r.lambdas = ctypes.cast(lam, ctypes.POINTER(ctypes.c_float))
        r.device_ms, r.select_ms = 0.25, 0.125
        self._held.append((r, idx, lam))
        res._obj.contents = r
        return 0

    def tda_pipe_create(self, depth, coalesce, h):
        self.calls.append(["tda_pipe_create", {"depth": int(depth), "coalesce": int(coalesce)}])
        h._obj.value = PIPE
        return 0

    def tda_pipe_submit(self, pipe, tmpl, tid, ptr, Ls, n, d, dtype, on_dev, ticket):
        nbytes = int(Ls) * int(n) * int(d) * (8 if dtype == 1 else 4)
        self.calls.append(["tda_pipe_submit", {"template": snapshot(tmpl._obj, N=int(n)), "template_id": int(tid), "L": int(Ls), "N": int(n),
                                               "D": int(d), "dtype": int(dtype), "x_on_device": int(on_dev),
                                               "x": {"device_pointer": int(ptr)} if on_dev else _sha(ptr, nbytes)}])
        self._tickets += 1
        ticket._obj.value = self._tickets
        return 0

    def tda_pipe_wait(self, *a):
        return -1

    def tda_pipe_flush(self, *a):
        return 0

    def tda_pipe_release(self, *a):
        return 0

    def tda_pipe_destroy(self, *a):
        return None

    def __getattr__(self, name):
        if not name.startswith("tda_"):
            raise AttributeError(name)

        def entry(*args):
            first = getattr(args[0], "_obj", None) if args else None
            if isinstance(first, ctypes.Structure) and type(first).__name__.endswith("Args"):
                self.calls.append([name, snapshot(first)])
                return -1
            self.calls.append([name, None])  # a free
            return None

        return entry


# ---------------------------------------------------------------- the inputs
def _points(l=L, n=N, d=D) -> np.ndarray:
    """Multiples of 1/8 in [-2, 2): exact in every float format used here."""
    return np.random.default_rng(11).integers(-16, 16, size=(l, n, d)).astype(np.float64) / 8.0


def _matrices(l=L, n=N) -> np.ndarray:
    p = np.random.default_rng(12).integers(1, 16, size=(l, n, n)).astype(np.float64) / 8.0
    m = np.triu(p, 1)
    return m + m.transpose(0, 2, 1)


FORMS = ("np_f32", "np_f64", "np_f16", "np_i64", "np_f32_strided", "np_f32_fortran", "list", "torch_f32", "torch_f64", "torch_f16",
         "torch_bf16", "torch_grad")


def form(base: np.ndarray, name: str):
    """``base`` (float64, exact in f16) in one of FORMS."""
    import torch

    if name == "np_f32":
        return np.ascontiguousarray(base, dtype=np.float32)
    if name == "np_f64":
        return base.copy()
    if name == "np_f16":
        return base.astype(np.float16)
    if name == "np_i64":
        return np.round(base * 8.0).astype(np.int64)
    if name == "np_f32_strided":
        wide = np.full(base.shape[:-1] + (2 * base.shape[-1],), 99.0, np.float32)
        wide[..., ::2] = base
        v = wide[..., ::2]
        assert not v.flags.c_contiguous
        return v
    if name == "np_f32_fortran":
        v = np.asfortranarray(base.astype(np.float32))
        assert not v.flags.c_contiguous
        return v
    if name == "list":
        return base.tolist()
    if name == "torch_f32":
        return torch.from_numpy(base.astype(np.float32))
    if name == "torch_f64":
        return torch.from_numpy(base.copy())
    if name == "torch_f16":
        return torch.from_numpy(base.astype(np.float16))
    if name == "torch_bf16":
        return torch.from_numpy(base.astype(np.float32)).to(torch.bfloat16)
    if name == "torch_grad":
        return torch.from_numpy(base.astype(np.float32)).requires_grad_(True)
    raise KeyError(name)


def _with(base: np.ndarray, value: float) -> np.ndarray:
    x = base.astype(np.float32)
    x.reshape(-1)[-2] = value
    return x


# ---------------------------------------------------------------- the grid
def cases(pkg) -> dict:
    """name -> a callable of no arguments that makes the call (inputs built inside it)."""
    rp = importlib.import_module(pkg.__name__ + ".ripser")
    mt = importlib.import_module(pkg.__name__ + ".metrics")
    bs = importlib.import_module(pkg.__name__ + ".bootstrap")
    ph = importlib.import_module(pkg.__name__ + ".phdim")
    um = importlib.import_module(pkg.__name__ + ".umap")

    P, M = _points(), _matrices()
    f32 = lambda b=P: form(b, "np_f32")  # noqa: E731
    labels = [np.arange(N) % 2, ["a", "b", "b", "c", "a"]]
    shared = np.array([[0, 2, 4], [1, 1, 3]], dtype=np.int64)  # (B = 2, m = 3)
    per_layer = np.stack([shared, shared[::-1]]).astype(np.int16)  # (L, B, m)
    sizes = np.array([3, 2])
    umap_kw = dict(n_neighbors=3, n_components=2, n_epochs=7, random_state=7, a=1.5, b=0.875)

    def pipeline(X, **kw):
        def run():
            with rp.SweepPipeline(depth=2, coalesce=2, device=kw.pop("device", 0), maxdim=kw.pop("maxdim", 1), **kw) as pipe:
                f = pipe.submit(X)
                f.result()

        return run

    entries = {  # entry name -> (call on points, call on matrices or None)
        "ripser_batch": (lambda X: rp.ripser_batch(X, maxdim=1), lambda X: rp.ripser_batch(X, maxdim=2, distance_matrix=True)),
        "ripser_batch_n_perm": (lambda X: rp.ripser_batch(X, n_perm=3), lambda X: rp.ripser_batch(X, n_perm=3, distance_matrix=True)),
        "greedy_perm_batch": (lambda X: rp.greedy_perm_batch(X, 3), lambda X: rp.greedy_perm_batch(X, 2, distance_matrix=True, device=1,
                                                                                                  want_dperm2all=False)),
        "hausdorff_resamples": (lambda X: bs.hausdorff_resamples(X, shared), lambda X: bs.hausdorff_resamples(X, per_layer, distance_matrix=True,
                                                                                                            device=1)),
        "h0_subsamples": (lambda X: ph.h0_subsamples(X, shared), lambda X: ph.h0_subsamples(X, per_layer, sizes, alpha=2.0, deaths=True,
                                                                                         distance_matrix=True, device=1)),
        "effective_dim": (mt.compute_effective_dimensionality, None),
        "fixed_window_ed": (lambda X: mt.compute_fixed_window_ed(X, 2), None),
        "entropy_profile": (lambda X: mt.matrix_entropy_profile(X, [1.0, 2.0, 0.5], eps=1e-8), None),
        "umap_batch": (lambda X: um.umap_batch(X, **umap_kw), None),
        "sweep_pipeline": (lambda X: pipeline(X)(), lambda X: pipeline(X, distance_matrix=True)()),
    }
    P6, P12 = _points(L, 6, D), _points(L, 12, D)
    c = {}
    for fm in FORMS:
        for name, (on_points, on_matrices) in entries.items():
            c[f"{name}/points/{fm}"] = lambda fm=fm, call=on_points: call(form(P, fm))
            if on_matrices is not None:
                c[f"{name}/matrices/{fm}"] = lambda fm=fm, call=on_matrices: call(form(M, fm))
        c[f"intrinsic_dim/points/{fm}"] = lambda fm=fm: mt.compute_intrinsic_dimensionality(form(P6, fm), 0.2, eps=1e-9)
        c[f"fixed_window_id/points/{fm}"] = lambda fm=fm: mt.compute_fixed_window_id(form(P12, fm), 2, 0.2)
    c["intrinsic_dim/no_call_below_6"] = lambda: mt.compute_intrinsic_dimensionality(f32())

    # ripser_batch and ripser_batch(n_perm=3): each option
    options = {
        "want_dist": dict(want_dist=True), "persistence_off": dict(maxdim=0, persistence=False),
        "persistence_off_maxdim1": dict(maxdim=1, persistence=False), "stage_times": dict(stage_times=True, return_time=True),
        "stage_serial": dict(stage_times=True, stage_serial=True), "stage_serial_alone": dict(stage_serial=True),
        "one_stream": dict(one_stream=True), "input_ready": dict(input_ready=True), "slot": dict(slot=5), "device": dict(device=3),
        "thresh": dict(thresh=1.25), "thresh_inf": dict(thresh=float("inf")), "maxdim2": dict(maxdim=2),
        "all": dict(maxdim=0, thresh=0.75, want_dist=True, stage_times=True, stage_serial=True, persistence=False, one_stream=True,
                    input_ready=True, slot=7, device=2),
    }
    for name, kw in options.items():
        c[f"ripser_batch/option/{name}"] = lambda kw=kw: rp.ripser_batch(f32(), **kw)
        c[f"ripser_batch_n_perm/option/{name}"] = lambda kw=kw: rp.ripser_batch(f32(), n_perm=3, **kw)
        c[f"ripser_batch_n_perm/matrices/option/{name}"] = lambda kw=kw: rp.ripser_batch(f32(M), n_perm=2, distance_matrix=True, **kw)
        c[f"sweep_pipeline/option/{name}"] = pipeline(f32(), **{k: v for k, v in kw.items() if k not in ("slot",)})
    for name, kw in {"labels": dict(labels=labels), "twonn": dict(twonn=True, discard_fraction=0.25, eps=1e-6),
                     "labels_twonn_maxdim0": dict(maxdim=0, labels=labels[:1], twonn=True)}.items():
        c[f"ripser_batch/option/{name}"] = lambda kw=kw: rp.ripser_batch(f32(), **kw)
        c[f"ripser_batch_n_perm/option/{name}"] = lambda kw=kw: rp.ripser_batch(f32(), n_perm=3, **kw)
        c[f"sweep_pipeline/option/{name}"] = pipeline(f32(), **kw)
    c["ripser_batch/option/want_dist64"] = lambda: rp.ripser_batch(form(P, "np_f64"), want_dist64=True)
    c["ripser_batch/option/want_dist64_f32"] = lambda: rp.ripser_batch(f32(), want_dist64=True)
    c["ripser_batch_n_perm/option/want_dist64"] = lambda: rp.ripser_batch(f32(), n_perm=3, want_dist64=True)
    c["sweep_pipeline/option/want_dist64"] = pipeline(form(P, "np_f64"), want_dist64=True)
    c["ripser/points_f32"] = lambda: rp.ripser(f32()[0])
    c["ripser/points_f64"] = lambda: rp.ripser(P[0])

    # input in parts
    c["ripser_batch/parts/two_f32"] = lambda: rp.ripser_batch([f32(), f32(P[::-1])], maxdim=1, slot=2)
    c["ripser_batch/parts/two_f64_tuple"] = lambda: rp.ripser_batch((P.copy(), P[::-1]), want_dist64=True)
    c["ripser_batch/parts/two_matrices_mixed_forms"] = lambda: rp.ripser_batch([form(M, "np_f32_fortran"), form(M, "torch_f32")],
                                                                             distance_matrix=True, device=1)
    c["ripser_batch/parts/one"] = lambda: rp.ripser_batch([f32()])
    c["ripser_batch/parts/none"] = lambda: rp.ripser_batch([])
    c["ripser_batch/parts/seventeen"] = lambda: rp.ripser_batch([f32()] * 17)
    c["ripser_batch/parts/unequal_shape"] = lambda: rp.ripser_batch([f32(), f32(P6)])
    c["ripser_batch/parts/unequal_dtype"] = lambda: rp.ripser_batch([f32(), P.copy()])
    c["ripser_batch/parts/second_holds_nan"] = lambda: rp.ripser_batch([f32(), _with(P, np.nan)])
    c["ripser_batch/parts/unequal_shape_and_nan"] = lambda: rp.ripser_batch([_with(P, np.nan), f32(P6)])
    c["ripser_batch/parts/one_is_2d"] = lambda: rp.ripser_batch([f32(), f32()[0]])

    # the index-table entries: tables and orders
    for a in (1.0, 2.0, 1.5):
        c[f"h0_subsamples/alpha_{a}"] = lambda a=a: ph.h0_subsamples(f32(), shared, alpha=a)
        c[f"h0_subsamples/alpha_{a}_sizes_deaths"] = lambda a=a: ph.h0_subsamples(f32(), shared, sizes, alpha=a, deaths=True)
    c["h0_subsamples/per_layer_sizes"] = lambda: ph.h0_subsamples(f32(), per_layer, sizes)
    c["h0_subsamples/deaths_no_sizes"] = lambda: ph.h0_subsamples(f32(), shared, deaths=True)
    c["h0_subsamples/unused_entries_out_of_range"] = lambda: ph.h0_subsamples(f32(), np.array([[0, 1, 2**40], [1, 2, -7]]), [2, 2])
    c["ph_dimension/default"] = lambda: ph.ph_dimension(f32(_points(L, 12, D)), n_trials=2, seed=3)
    c["ph_dimension/given_table"] = lambda: ph.ph_dimension(f32(), idx=shared, sizes=sizes, alpha=2.0, device=1)
    c["hausdorff_resamples/shared"] = lambda: bs.hausdorff_resamples(f32(), shared, device=2)
    c["hausdorff_resamples/per_layer"] = lambda: bs.hausdorff_resamples(f32(), per_layer)
    c["confidence_bands/default_table"] = lambda: bs.confidence_bands(f32(), B=4, seed=5, device=1)

    # refusals, and which comes first
    flat = f32()[0]
    cloud_entries = {k: v[0] for k, v in entries.items()}
    cloud_entries["intrinsic_dim"] = mt.compute_intrinsic_dimensionality
    cloud_entries["fixed_window_id"] = lambda X: mt.compute_fixed_window_id(X, 2)
    for name, call in cloud_entries.items():
        c[f"refuse/ndim2/{name}"] = lambda call=call: call(flat)
        c[f"refuse/ndim4/{name}"] = lambda call=call: call(f32()[None])
        big = P12 if name == "fixed_window_id" else P6 if name == "intrinsic_dim" else P
        c[f"refuse/nan/{name}"] = lambda call=call, big=big: call(_with(big, np.nan))
        c[f"refuse/inf/{name}"] = lambda call=call, big=big: call(_with(big, -np.inf))
        c[f"refuse/nan_f64/{name}"] = lambda call=call, big=big: call(_with(big, np.nan).astype(np.float64))
        c[f"refuse/nan_torch/{name}"] = lambda call=call, big=big: call(__import__("torch").from_numpy(_with(big, np.nan)))
    c["refuse/ndim1/entropy_profile"] = lambda: mt.matrix_entropy_profile(flat[0], [1.0])
    c["entropy_profile/ndim2"] = lambda: mt.matrix_entropy_profile(flat, [1.0])
    c["entropy_profile/ndim4"] = lambda: mt.matrix_entropy_profile(f32()[None], [2.0])
    for name, (_, call) in entries.items():
        if call is not None:
            c[f"refuse/not_square/{name}"] = lambda call=call: call(f32())
            c[f"refuse/not_square_and_nan/{name}"] = lambda call=call: call(_with(P, np.nan))
            c[f"refuse/square_nan/{name}"] = lambda call=call: call(_with(M, np.nan))
            c[f"refuse/square_inf_f64/{name}"] = lambda call=call: call(_with(M, np.inf).astype(np.float64))
    for name in ("ripser_batch_n_perm", "greedy_perm_batch", "hausdorff_resamples", "h0_subsamples"):
        call = entries[name][0]
        c[f"refuse/list_of_arrays/{name}"] = lambda call=call: call([f32(), f32()])
        c[f"refuse/tuple_of_arrays/{name}"] = lambda call=call: call((f32(),))
        c[f"refuse/f64_and_nan/{name}"] = lambda call=call: call(_with(P, np.nan).astype(np.float64))
    c["refuse/order/ndim2_and_bad_n_perm"] = lambda: rp.ripser_batch(flat, n_perm=2.5)
    c["refuse/order/ndim2_and_n_perm_none"] = lambda: rp.greedy_perm_batch(flat, None)
    c["refuse/order/ndim2_and_n_perm_too_large"] = lambda: rp.ripser_batch(flat, n_perm=9)
    c["refuse/order/nan_and_n_perm_too_large"] = lambda: rp.ripser_batch(_with(P, np.nan), n_perm=9)
    c["refuse/order/f64_and_n_perm_zero"] = lambda: rp.greedy_perm_batch(P.copy(), 0)
    c["refuse/order/n_perm_with_labels"] = lambda: rp.ripser_batch(flat, n_perm=2, labels=labels)
    c["refuse/order/n_perm_persistence_off_maxdim1_nan"] = lambda: rp.ripser_batch(_with(P, np.nan), n_perm=2, persistence=False)
    c["refuse/order/bad_maxdim_and_ndim2"] = lambda: rp.ripser_batch(flat, maxdim=3)
    c["refuse/order/nan_and_persistence_off_maxdim1"] = lambda: rp.ripser_batch(_with(P, np.nan), persistence=False)
    c["refuse/order/nan_and_bad_labels"] = lambda: rp.ripser_batch(_with(P, np.nan), labels=[np.zeros(N)])
    c["refuse/order/ed_nan_and_too_large"] = lambda: mt.compute_effective_dimensionality(_with(np.zeros((1, 1025, 1025)), np.nan))
    c["refuse/order/ed_too_large"] = lambda: mt.compute_effective_dimensionality(np.zeros((1, 1025, 1025), np.float32))
    c["refuse/order/ed_ndim2_and_nan"] = lambda: mt.compute_effective_dimensionality(_with(P, np.nan)[0])
    c["refuse/order/entropy_nan_and_too_large"] = lambda: mt.matrix_entropy_profile(_with(np.zeros((1, 1025, 1025)), np.nan), [1.0])
    c["refuse/order/entropy_bad_alpha_and_ndim1"] = lambda: mt.matrix_entropy_profile(flat[0], [0.0])
    c["refuse/order/window_ed_nan_and_too_large"] = lambda: mt.compute_fixed_window_ed(_with(np.zeros((1, 1025, 1025)), np.nan), 1)
    c["refuse/order/window_ed_bad_windows_and_ndim2"] = lambda: mt.compute_fixed_window_ed(flat, 0)
    c["refuse/order/window_id_ndim2_and_bad_windows"] = lambda: mt.compute_fixed_window_id(flat, 0)
    c["refuse/order/umap_bad_metric_and_ndim2"] = lambda: um.umap_batch(flat, metric="manhattan")
    c["refuse/order/umap_nan_f64"] = lambda: um.umap_batch(_with(P, np.nan).astype(np.float64), **umap_kw)
    c["refuse/order/hausdorff_bad_idx_and_nan"] = lambda: bs.hausdorff_resamples(_with(P, np.nan), [[0, 9]])
    c["refuse/order/hausdorff_f64_and_bad_idx"] = lambda: bs.hausdorff_resamples(P.copy(), [[0, 9]])
    c["refuse/order/hausdorff_idx_floats"] = lambda: bs.hausdorff_resamples(f32(), [[0.0, 1.0]])
    c["refuse/order/hausdorff_idx_layers"] = lambda: bs.hausdorff_resamples(f32(), np.zeros((3, 2, 2), int))
    c["refuse/order/hausdorff_idx_empty"] = lambda: bs.hausdorff_resamples(f32(), np.zeros((0, 2), int))
    c["refuse/order/h0_bad_alpha_and_ndim2"] = lambda: ph.h0_subsamples(flat, shared, alpha=0.0)
    c["refuse/order/h0_bad_sizes_and_nan"] = lambda: ph.h0_subsamples(_with(P, np.nan), shared, [4, 1])
    c["refuse/order/h0_bad_idx"] = lambda: ph.h0_subsamples(f32(), [[0, 5]])
    c["refuse/order/bands_bad_B_and_ndim2"] = lambda: bs.confidence_bands(flat, B=0)
    c["refuse/order/phdim_bad_trials_and_ndim2"] = lambda: ph.ph_dimension(flat, n_trials=0)
    return c


def _outcome(call):
    try:
        out = call()
    except Exception as e:  # the type and the whole message are part of the pin
        return [type(e).__name__, str(e)]
    if type(out).__module__.startswith("torch"):
        return ["returned", f"torch {str(out.dtype)} {tuple(out.shape)} {out.device} {np.asarray(out).tolist()!r}"]
    if isinstance(out, np.ndarray):
        return ["returned", f"numpy {out.dtype} {out.shape} {out.tolist()!r}"]
    return ["returned", type(out).__name__]


def record(pkg, monkeypatch_setattr) -> dict:
    """Run the whole grid against the stand-in: name -> {"calls": [...], "outcome": [type, text]}."""
    out = {}
    for name, call in cases(pkg).items():
        stand_in = StandIn(pkg._lib)
        monkeypatch_setattr(pkg._lib, "lib", lambda s=stand_in: s)
        out[name] = {"calls": stand_in.calls, "outcome": _outcome(call)}
    return out
