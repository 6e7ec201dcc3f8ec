"""CPU tests of the spectral metrics (no GPU): the float64 restatement
(tests/spectral_ref.py) reproduces the reference's outputs in
tests/golden/entropy.json within the gaps recorded there, the seeded inputs are
the pinned ones, the ctypes mirror of tda_spectral_args has the C header's
layout, and bad arguments are refused before the library is needed."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import spectral_ref
from conftest import GOLDEN
from golden.make_golden_entropy import ALPHAS, STRICT_GAP, dec, entropy_inputs, is_strict, sha, window_inputs


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "entropy.json")) as f:
        return json.load(f)


def _within(got, refs, gaps, floor):
    """got reproduces the reference's values within the recorded gaps (and the last bits of the LAPACK in use)."""
    for g, r, gap in zip(np.ravel(got), refs, gaps):
        assert spectral_ref.rel_gap(dec(r), g, floor) <= dec(gap) * (1.0 + 1e-3) + 1e-9, (float(g), r, gap)


def test_restatement_reproduces_entropy_goldens(golden):
    assert set(golden["entropy"]) == set(entropy_inputs())
    for name, X in entropy_inputs().items():
        rec = golden["entropy"][name]
        assert rec["sha"] == sha(X) and rec["shape"] == list(X.shape), name
        for al in ALPHAS:
            r = rec["alphas"][repr(al)]
            assert r["strict"] == is_strict(X, al)
            if r["strict"]:
                assert max(dec(g) for g in r["gap"]) <= STRICT_GAP, (name, al)
            _within(spectral_ref.matrix_entropy(X, al), r["ref"], r["gap"], spectral_ref.F32_ULP)


def test_restatement_reproduces_window_goldens(golden):
    assert set(golden["windows"]) == set(window_inputs())
    for name, (X, W) in window_inputs().items():
        rec = golden["windows"][name]
        assert rec["sha"] == sha(X) and rec["shape"] == list(X.shape) and rec["n_windows"] == W, name
        ed, idv = spectral_ref.fixed_window_ed(X, W), spectral_ref.fixed_window_id(X, W)
        assert list(ed.shape) == rec["ed_shape"] and list(idv.shape) == rec["id_shape"], name
        _within(ed, rec["ed"], rec["ed_gap"], spectral_ref.F32_ULP)
        _within(idv, rec["id"], rec["id_gap"], spectral_ref.F32_ULP)


def test_entropy_restatement_closed_forms():
    """k orthonormal rows: p is uniform over k, every order gives log k; one row gives 0."""
    q = np.linalg.qr(np.random.default_rng(0).standard_normal((12, 5)))[0].T  # (5, 12), orthonormal rows
    for al in ALPHAS:
        assert abs(spectral_ref.matrix_entropy(3.0 * q, al) - np.log(5.0)) < 1e-9
        assert abs(spectral_ref.matrix_entropy(q[:1], al)) < 1e-9


def test_spectral_args_match_header_layout(pkg, tmp_path):
    lb = pkg._lib
    fields = [n for n, _ in lb.SpectralArgs._fields_]
    src = tmp_path / "slayout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tda_rips.h"\nint main(void){printf("%zu", sizeof(tda_spectral_args));\n'
                   + "".join(f'printf(" %zu", offsetof(tda_spectral_args, {f}));\n' for f in fields) + "return 0;}\n")
    exe = tmp_path / "slayout"
    subprocess.run(["gcc", "-I", lb.INCLUDE, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(lb.SpectralArgs)] + [getattr(lb.SpectralArgs, f).offset for f in fields]


def test_new_symbols_exported(pkg, built_lib):
    assert {"tda_matrix_entropy", "tda_effective_dim_windows"} <= set(pkg.EXPORTS)
    lib = ctypes.CDLL(built_lib)
    assert hasattr(lib, "tda_matrix_entropy") and hasattr(lib, "tda_effective_dim_windows")
    for name in ("matrix_entropy", "matrix_entropy_profile", "compute_fixed_window_ed", "compute_fixed_window_id"):
        assert callable(getattr(pkg, name)) and name in pkg.__all__


def test_python_validation_before_the_library(pkg, monkeypatch):
    def no_lib():
        raise AssertionError("the library must not be needed to refuse these")

    monkeypatch.setattr(pkg._lib, "lib", no_lib)
    X = np.ones((2, 4, 6), np.float32)
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            pkg.matrix_entropy(X, bad)
    with pytest.raises(ValueError):
        pkg.matrix_entropy_profile(X, [])
    with pytest.raises(ValueError):
        pkg.matrix_entropy_profile(X, [1.0] * 17)
    with pytest.raises(ValueError):
        pkg.matrix_entropy(np.ones(5, np.float32))
    with pytest.raises(ValueError):
        pkg.matrix_entropy(np.full((1, 2, 2), np.nan, np.float32))
    with pytest.raises(NotImplementedError):
        pkg.matrix_entropy(np.zeros((1, 1025, 1025), np.float32))
    for bad in (0, -3):
        with pytest.raises(ValueError):
            pkg.compute_fixed_window_ed(X, bad)
    with pytest.raises(ValueError):
        pkg.compute_fixed_window_ed(X[0], 2)
    with pytest.raises(NotImplementedError):
        pkg.compute_fixed_window_ed(np.zeros((1, 1025, 1025), np.float32), 1)
    # empty batches need no device either
    assert pkg.matrix_entropy_profile(np.zeros((0, 4, 6), np.float32), [0.5, 2.0]).shape == (0, 2)
    assert pkg.compute_fixed_window_ed(np.zeros((0, 4, 6), np.float32), 9).shape == (0, 4)
    # window ID: all NaN in the reference's cases (metrics.py:228-245), of the reference's shape
    for S, W in ((50, 10), (3, 5), (5, 1), (64, 11)):
        got = pkg.compute_fixed_window_id(np.ones((2, S, 3), np.float32), W)
        assert got.shape == (2, W) and got.dtype == np.float32 and np.all(np.isnan(got)), (S, W)
    assert pkg.compute_fixed_window_id(X, 0).shape == (2, 0)


def test_c_entries_refuse_before_device(pkg, built_lib):
    """No GPU here: valid arguments end in TDA_E_NODEVICE (-5), bad ones in their own code first."""
    L, lb = pkg.lib(), pkg._lib
    X = np.ones((2, 7, 6), np.float32)
    out = np.zeros(64, np.float32)
    po = out.ctypes.data_as(lb._f32p)
    al = np.array([0.5, 1.0, 2.0])
    a = lb.SpectralArgs()
    a.x, a.dtype, a.B, a.S, a.D, a.device = X.ctypes.data, lb.TDA_F32, 2, 7, 6, 12345
    a.n_alpha, a.alphas, a.eps = 3, al.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1e-10
    assert L.tda_matrix_entropy(ctypes.byref(a), po) == -5
    assert L.tda_effective_dim_windows(ctypes.byref(a), po) == -1  # n_windows = 0
    a.n_windows = -1
    assert L.tda_matrix_entropy(ctypes.byref(a), po) == -1
    a.n_windows = 3
    assert L.tda_effective_dim_windows(ctypes.byref(a), po) == -5
    a.n_windows = 100  # > S: clamped
    assert L.tda_effective_dim_windows(ctypes.byref(a), po) == -5
    a.n_windows = 0
    for n_alpha in (0, 17):
        a.n_alpha = n_alpha
        assert L.tda_matrix_entropy(ctypes.byref(a), po) == -1
    a.n_alpha, al[1] = 3, -1.0
    assert L.tda_matrix_entropy(ctypes.byref(a), po) == -1
    assert b"alpha" in L.tda_last_error()
    al[1], a.alphas = 1.0, None
    assert L.tda_matrix_entropy(ctypes.byref(a), po) == -1
    a.alphas, a.S, a.D = al.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1025, 1025
    assert L.tda_matrix_entropy(ctypes.byref(a), po) == -2  # min(N, D) > 1024 (x is not read)
    a.n_windows = 2  # windows of 512 rows
    assert L.tda_effective_dim_windows(ctypes.byref(a), po) == -5
    assert L.tda_matrix_entropy(ctypes.byref(a), None) == -1
