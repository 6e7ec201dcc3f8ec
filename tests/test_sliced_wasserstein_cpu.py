"""CPU tests of the sliced Wasserstein boundary (no device): the float64
restatement against a closed form, the new symbols and the ctypes mirrors of
include/tda_dgm.h, and the argument errors raised before any device work."""
import ctypes
import importlib
import math
import subprocess

import numpy as np
import pytest

import sw_ref


def test_restatement_converges_to_closed_form():
    """A = {(0, 1)}, B = {}: V1 = {sin t}, V2 = {(cos t + sin t) / 2}, so the
    summand is f(t) = |sin t - cos t| / 2, of period pi, and SW_M is its left
    Riemann sum over one period divided by pi.  The integral of |sin t - cos t|
    over a period is 2 sqrt 2, so SW_M -> sqrt(2) / pi.

    For M a multiple of 4 the kink of f (t = pi / 4) is a grid point, f is
    smooth on every cell, and the left Riemann sum of a periodic function over a
    period is its trapezoid sum: each of the M cells is off by at most
    h^3 max|f''| / 12 with h = pi / M and |f''| <= sqrt(2) / 2, together
    pi h^2 sqrt(2) / 24, and after the division by pi
        |SW_M - sqrt(2) / pi| <= sqrt(2) h^2 / 24.
    The error is of second order in h, so doubling M divides it by 4.

    Observed: error 3.7025e-05 at M = 100, 9.2560e-06 at M = 200 (ratio 4.00005),
    3.7024e-07 at M = 1000 against the bound 5.8157e-07."""
    exact = math.sqrt(2) / math.pi
    err = {M: abs(sw_ref.sliced_wasserstein([[0.0, 1.0]], np.zeros((0, 2)), M) - exact) for M in (100, 200, 1000)}
    print("closed form errors:", err, "ratio", err[100] / err[200], "bound", math.sqrt(2) * (math.pi / 1000) ** 2 / 24)
    assert 3.9 < err[100] / err[200] < 4.1
    assert err[1000] <= math.sqrt(2) * (math.pi / 1000) ** 2 / 24


def test_restatement_basic_properties():
    rng = np.random.default_rng(5)
    b = rng.uniform(0, 5, 12)
    A = np.stack([b, b + rng.uniform(0.1, 5, 12)], 1)
    B = A[:7] + 0.25
    assert sw_ref.sliced_wasserstein(A, A, 9) == 0.0
    assert sw_ref.sliced_wasserstein(A, B, 9) == sw_ref.sliced_wasserstein(B, A, 9) > 0
    assert sw_ref.sliced_wasserstein(np.zeros((0, 2)), np.zeros((0, 2)), 9) == 0.0
    withinf = np.concatenate([A, [[0.0, np.inf], [1.0, np.inf]]])
    assert sw_ref.sliced_wasserstein(withinf, B, 9) == sw_ref.sliced_wasserstein(A, B, 9)


def test_sw_structs_match_header_layout(pkg, tmp_path):
    lb = pkg._lib
    src = tmp_path / "swlayout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "tda_dgm.h"\n'
        'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %lld\\n", sizeof(tda_sw_args),'
        ' offsetof(tda_sw_args, offsets), offsetof(tda_sw_args, S), offsetof(tda_sw_args, pairs), offsetof(tda_sw_args, P),'
        ' offsetof(tda_sw_args, M), offsetof(tda_sw_args, device), sizeof(tda_sw_result), offsetof(tda_sw_result, dist),'
        ' offsetof(tda_sw_result, device_ms), TDA_SW_MAX_POINTS, TDA_SW_MAX_DIRECTIONS, (long long)TDA_SW_MAX_WORK); return 0;}\n')
    exe = tmp_path / "swlayout"
    subprocess.run(["gcc", "-I", lb.INCLUDE, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    A, R = lb.SwArgs, lb.SwResult
    assert got == [ctypes.sizeof(A), A.offsets.offset, A.S.offset, A.pairs.offset, A.P.offset, A.M.offset, A.device.offset,
                   ctypes.sizeof(R), R.dist.offset, R.device_ms.offset, lb.TDA_SW_MAX_POINTS, lb.TDA_SW_MAX_DIRECTIONS,
                   lb.TDA_SW_MAX_WORK]


def test_sw_symbols_exported_and_abi_version_unchanged(pkg, built_lib):
    lib = ctypes.CDLL(built_lib)
    assert hasattr(lib, "tda_sliced_wasserstein") and hasattr(lib, "tda_sw_free")
    assert set(pkg.DGM_EXPORTS) == {"tda_sliced_wasserstein", "tda_sw_free"}
    assert not set(pkg.DGM_EXPORTS) & set(pkg.EXPORTS)
    assert pkg.lib().tda_version() == 8  # symbols added only: no existing struct changed


def test_sw_invalid_arguments_rejected_before_device(pkg, built_lib):
    L = pkg.lib()
    lb = pkg._lib
    res = ctypes.POINTER(lb.SwResult)()
    pts = np.tile(np.array([[0.0, 1.0]]), (4097, 1))
    off = np.array([0, 2048, 4096, 4097], np.int64)  # diagrams of 2048, 2048 and 1 points
    pr = np.array([[0, 2]], np.int32)

    def call(**kw):
        a = lb.SwArgs()
        a.points, a.offsets, a.S, a.pairs, a.P, a.M = pts.ctypes.data, off.ctypes.data, 3, pr.ctypes.data, 1, 50
        a.device = 12345  # never a device: a valid call ends at the device check
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.tda_sliced_wasserstein(ctypes.byref(a), ctypes.byref(res))
        assert not res  # no result on failure
        return rc

    assert call(M=0) == -1 and b"M" in L.tda_last_error()
    assert call(M=1025) == -2 and b"1024" in L.tda_last_error()
    assert call(offsets=None) == -1 and call(points=None) == -1 and call(S=-1) == -1 and call(P=-1) == -1
    bad = np.array([0, 5, 3, 4097], np.int64)
    assert call(offsets=bad.ctypes.data) == -1 and b"non-decreasing" in L.tda_last_error()
    bad = np.array([1, 5, 6, 7], np.int64)
    assert call(offsets=bad.ctypes.data) == -1
    for q in ([[0, 3]], [[-1, 0]]):
        q = np.array(q, np.int32)
        assert call(pairs=q.ctypes.data) == -1 and b"outside" in L.tda_last_error()
    # 2048 + 2048 + 1 finite points in one pair, explicitly and among all pairs (pairs == NULL)
    q = np.array([[0, 1]], np.int32)
    assert call(pairs=q.ctypes.data) == -5  # 4096 together: valid, ends at the device check
    big = np.array([0, 2049, 4097], np.int64)
    assert call(offsets=big.ctypes.data, S=2, pairs=q.ctypes.data) == -2 and b"4096" in L.tda_last_error()
    assert call(offsets=big.ctypes.data, S=2, pairs=None) == -2
    # non-finite rows do not count towards the limit
    pinf = pts.copy()
    pinf[0, 1] = np.inf
    assert call(points=pinf.ctypes.data, offsets=big.ctypes.data, S=2, pairs=None) == -5
    assert call(pairs=None, M=1024) == -5  # (0, 1), (0, 2), (1, 2): all within the limit
    # pairs x directions per call
    many = np.zeros(((1 << 27) // 1024 + 1, 2), np.int32)
    assert call(pairs=many.ctypes.data, P=len(many), M=1024) == -2 and b"split" in L.tda_last_error()
    assert L.tda_sliced_wasserstein(None, ctypes.byref(res)) == -1
    assert L.tda_sliced_wasserstein(ctypes.byref(lb.SwArgs()), None) == -1
    L.tda_sw_free(None)  # a no-op


def test_python_entries_refuse_bad_arguments_before_the_library(pkg):
    A = np.array([[0.0, 1.0], [0.5, 2.0]])
    for M in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            pkg.sliced_wasserstein(A, A, M=M)
        with pytest.raises(ValueError):
            pkg.sliced_wasserstein_matrix([A, A], M=M)
    with pytest.raises(NotImplementedError):
        pkg.sliced_wasserstein(A, A, M=1025)
    for bad in (np.zeros((3, 3)), np.zeros(3), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            pkg.sliced_wasserstein(A, bad)
        with pytest.raises(ValueError):
            pkg.sliced_wasserstein_matrix([A, bad])
        with pytest.raises(ValueError):
            pkg.sliced_wasserstein_matrix([A], other=[bad])
    big = np.tile(A, (1024, 1))  # 2048 points
    with pytest.raises(NotImplementedError):
        pkg.sliced_wasserstein(big, np.concatenate([big, A[:1]]))  # 4097 together
    with pytest.raises(NotImplementedError):
        pkg.sliced_wasserstein_matrix([A, big, np.concatenate([big, A[:1]])])
    with pytest.raises(NotImplementedError):
        pkg.sliced_wasserstein_matrix([A, big], other=[A, np.concatenate([big, A[:1]])])
    # nothing to compute: no library call, no device needed
    assert pkg.sliced_wasserstein_matrix([]).shape == (0, 0)
    assert pkg.sliced_wasserstein_matrix([A]).tolist() == [[0.0]]
    assert pkg.sliced_wasserstein_matrix([A], other=[]).shape == (1, 0)
    with pytest.raises(ValueError):
        pkg.layer_distance_matrix([A, A], M=0)


def test_kernel_of_distances(pkg):
    D = np.array([[0.0, 2.0], [2.0, 0.0]])
    K = pkg.sliced_wasserstein_kernel(D, sigma=0.5)
    assert K.tolist() == np.exp(-D / 0.5).tolist() and K[0, 0] == 1.0


def test_flatten_gathers_one_batch_without_per_layer_work(pkg):
    """LayerResults of one batch: points and offsets come from the batch's
    shared arrays in the order of the list, equal to the per-layer slices."""
    rp = importlib.import_module(pkg.__name__ + ".ripser")  # pkg.ripser is the function
    rng = np.random.default_rng(2)
    b = rp._Batch()
    b.L, b.nd = 4, 2
    b.cnt = np.array([[3, 2], [3, 0], [3, 4], [3, 1]], np.int64)
    b.off = (np.cumsum(b.cnt.ravel()) - b.cnt.ravel()).reshape(4, 2)
    b.pairs = rng.uniform(0, 1, (int(b.cnt.sum()), 2))
    res = [rp.LayerResult((b, l)) for l in (2, 0, 3, 1)]
    for dim in (0, 1):
        pts, off = pkg.diagrams._flatten(res, dim)
        want = [b.pairs[b.off[l, dim]:b.off[l, dim] + b.cnt[l, dim]] for l in (2, 0, 3, 1)]
        assert off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
        assert pts.tolist() == np.concatenate(want).tolist() and pts.dtype == np.float64 and off.dtype == np.int64
    with pytest.raises(ValueError):
        pkg.diagrams._flatten(res, 2)
    with pytest.raises(ValueError):
        pkg.diagrams._flatten([res[0], np.zeros((1, 2))], 1)
