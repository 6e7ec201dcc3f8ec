"""GPU tests of the spectral metrics beside tda_effective_dim: matrix_entropy /
matrix_entropy_profile (the Renyi epilogue of k_ed_jacobi, tda_matrix_entropy),
compute_fixed_window_ed (tda_effective_dim_windows) and compute_fixed_window_id
(TwoNN over windows), against the reference's own outputs
(tests/golden/entropy.json) and the float64 restatement (tests/spectral_ref.py).

Tolerances (relative, spectral_ref.rel_gap): ED_TOL = 1e-5 against the
restatement in every case and against the reference goldens in every strict
case; for N > D at alpha = 0.5, where the reference's float32 noise eigenvalues
go under a square root and move its own answer about 1.7e-3 off float64, twice
the gap recorded in entropy.json.  TWONN_TOL = 1e-4 for the window ID.
"""
import json
import os

import numpy as np
import pytest

import spectral_ref
from conftest import GOLDEN
from golden.make_golden_entropy import ALPHAS, dec, entropy_inputs, sha, window_inputs

pytestmark = pytest.mark.gpu

ED_TOL = 1e-5
TWONN_TOL = 1e-4


@pytest.fixture(scope="module")
def gpu(pkg, built_lib):
    import torch  # a process that hands torch CUDA tensors to the library initialises torch's device first

    torch.cuda.init()
    assert pkg.lib().tda_device_ok(0) == 1, "no gfx950 device visible"
    return pkg


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "entropy.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def profiles(gpu):
    """name -> matrix_entropy_profile(X, ALPHAS) of every entropy case, computed once."""
    return {name: gpu.matrix_entropy_profile(X, ALPHAS) for name, X in entropy_inputs().items()}


def test_entropy_vs_f64_restatement(profiles):
    for name, X in entropy_inputs().items():
        got = profiles[name]
        assert got.dtype == np.float32 and got.shape == X.shape[:-2] + (len(ALPHAS),), name
        for k, al in enumerate(ALPHAS):
            want = spectral_ref.matrix_entropy(X, al)
            for g, w in zip(got[..., k].ravel(), np.ravel(want)):
                gap = spectral_ref.rel_gap(g, w, spectral_ref.F32_ULP)  # the result is stored as float32
                print(name, al, float(g), float(w), gap)
                assert gap <= ED_TOL, (name, al, float(g), float(w))


def test_entropy_vs_reference_goldens(profiles, golden):
    for name, X in entropy_inputs().items():
        rec = golden["entropy"][name]
        assert rec["sha"] == sha(X), name
        for k, al in enumerate(ALPHAS):
            r = rec["alphas"][repr(al)]
            for i, g in enumerate(profiles[name][..., k].ravel()):
                want = dec(r["ref"][i])
                bound = ED_TOL if r["strict"] else 2.0 * dec(r["gap"][i])
                gap = spectral_ref.rel_gap(g, want, spectral_ref.F32_ULP)
                print(name, al, float(g), want, gap, bound)
                assert gap <= bound, (name, al, i, float(g), want)


def test_profile_equals_single_orders_and_device_input(gpu, profiles):
    import torch

    for name, X in entropy_inputs().items():
        prof = profiles[name]
        for k, al in enumerate(ALPHAS):
            one = gpu.matrix_entropy(X, al)
            assert one.dtype == np.float32 and one.shape == X.shape[:-2], (name, al)
            assert np.array_equal(one, prof[..., k], equal_nan=True), (name, al)
        gt = gpu.matrix_entropy_profile(torch.from_numpy(X).to("cuda:0"), ALPHAS)
        assert gt.device.type == "cuda" and gt.dtype == torch.float32
        assert np.array_equal(gt.cpu().numpy(), prof, equal_nan=True), name
    # the default order is Shannon's
    X = entropy_inputs()["gauss_n20_d24"]
    assert np.array_equal(gpu.matrix_entropy(X), profiles["gauss_n20_d24"][..., 1])


def test_window_ed(gpu, golden):
    import torch

    for name, (X, W) in window_inputs().items():
        rec = golden["windows"][name]
        assert rec["sha"] == sha(X) and rec["n_windows"] == W, name
        got = gpu.compute_fixed_window_ed(X, W)
        assert got.dtype == np.float32 and list(got.shape) == rec["ed_shape"], name
        w = spectral_ref.windows(X, W)
        sliced = np.stack([gpu.compute_effective_dimensionality(np.ascontiguousarray(w[:, k])) for k in range(w.shape[1])], 1)
        assert np.array_equal(got, sliced), name
        for g, ref in zip(got.ravel(), rec["ed"]):
            gap = spectral_ref.rel_gap(g, dec(ref), 0.0)
            print(name, float(g), ref, gap)
            assert gap <= ED_TOL, (name, float(g), ref)
        gt = gpu.compute_fixed_window_ed(torch.from_numpy(X).to("cuda:0"), W)
        assert gt.device.type == "cuda" and np.array_equal(gt.cpu().numpy(), got), name


def test_window_id(gpu, golden):
    for name, (X, W) in window_inputs().items():
        rec = golden["windows"][name]
        got = gpu.compute_fixed_window_id(X, W)
        assert got.dtype == np.float32 and list(got.shape) == rec["id_shape"], name
        want = np.array([dec(v) for v in rec["id"]]).reshape(got.shape)
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        if np.all(np.isnan(want)):
            continue
        for g, ref in zip(got.ravel(), want.ravel()):
            print(name, float(g), ref)
            assert abs(g - ref) <= TWONN_TOL * abs(ref), (name, float(g), ref)
        w = spectral_ref.windows(X, W)
        sliced = np.stack([gpu.compute_intrinsic_dimensionality(np.ascontiguousarray(w[:, k])) for k in range(W)], 1)
        assert np.array_equal(got, sliced), name


def test_error_cases(gpu):
    X = np.ones((1, 4, 6), np.float32)
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError):
            gpu.matrix_entropy(X, bad)
    with pytest.raises(ValueError):
        gpu.matrix_entropy_profile(X, np.linspace(0.5, 4.0, 17))
    with pytest.raises(NotImplementedError):
        gpu.matrix_entropy(np.zeros((1, 1025, 1025), np.float32))
    # the same refusals from the C entry itself
    _lib = gpu._lib
    import ctypes

    out = np.zeros(17, np.float32)
    al = np.array([1.0, 0.0] + [1.0] * 15)
    a = _lib.SpectralArgs()
    a.x, a.dtype, a.B, a.S, a.D = X.ctypes.data, _lib.TDA_F32, 1, 4, 6
    a.n_alpha, a.alphas, a.eps = 2, al.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1e-10
    L = gpu.lib()
    assert L.tda_matrix_entropy(ctypes.byref(a), out.ctypes.data_as(_lib._f32p)) == -1  # alpha = 0
    a.alphas = al[2:].ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    a.n_alpha = 17
    assert L.tda_matrix_entropy(ctypes.byref(a), out.ctypes.data_as(_lib._f32p)) == -1  # 17 orders
    a.n_alpha = 1
    assert L.tda_effective_dim_windows(ctypes.byref(a), out.ctypes.data_as(_lib._f32p)) == -1  # n_windows = 0
    assert L.tda_matrix_entropy(ctypes.byref(a), out.ctypes.data_as(_lib._f32p)) == 0
