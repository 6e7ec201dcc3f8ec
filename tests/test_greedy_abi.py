"""CPU tests of the greedy-subsampling boundary (no device): the ctypes mirrors
of tda_greedy_args / tda_greedy_result have the header's layout, bad arguments
come back with the documented codes before any device work, and the Python
entries refuse what they do not support."""
import ctypes
import subprocess

import numpy as np
import pytest


def test_greedy_structs_match_header_layout(pkg, tmp_path):
    lb = pkg._lib
    src = tmp_path / "glayout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "tda_rips.h"\n'
        'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(tda_greedy_args),'
        ' offsetof(tda_greedy_args, L), offsetof(tda_greedy_args, is_dist), offsetof(tda_greedy_args, n_perm),'
        ' offsetof(tda_greedy_args, stream), offsetof(tda_greedy_args, want_dperm2all), sizeof(tda_greedy_result),'
        ' offsetof(tda_greedy_result, idx_perm), offsetof(tda_greedy_result, dperm2all), offsetof(tda_greedy_result, sub_dev),'
        ' offsetof(tda_greedy_result, device), offsetof(tda_greedy_result, select_ms)); return 0;}\n')
    exe = tmp_path / "glayout"
    subprocess.run(["gcc", "-I", lb.INCLUDE, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    A, R = lb.GreedyArgs, lb.GreedyResult
    assert got == [ctypes.sizeof(A), A.L.offset, A.is_dist.offset, A.n_perm.offset, A.stream.offset, A.want_dperm2all.offset,
                   ctypes.sizeof(R), R.idx_perm.offset, R.dperm2all.offset, R.sub_dev.offset, R.device.offset, R.select_ms.offset]


def test_greedy_symbols_exported_and_abi_version_unchanged(pkg, built_lib):
    lib = ctypes.CDLL(built_lib)
    assert hasattr(lib, "tda_greedy_perm") and hasattr(lib, "tda_greedy_free")
    assert {"tda_greedy_perm", "tda_greedy_free"} <= set(pkg.EXPORTS)
    assert pkg.lib().tda_version() == 8  # symbols added only: no existing struct changed


def test_greedy_invalid_arguments_rejected_before_device(pkg, built_lib):
    L = pkg.lib()
    lb = pkg._lib
    res = ctypes.POINTER(lb.GreedyResult)()
    X = np.zeros((1, 6, 3), np.float32)

    def call(**kw):
        a = lb.GreedyArgs()
        a.x, a.dtype, a.L, a.N, a.D, a.n_perm = X.ctypes.data, lb.TDA_F32, 1, 6, 3, 4
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.tda_greedy_perm(ctypes.byref(a), ctypes.byref(res))
        assert not res  # no result on failure
        return rc

    assert call(n_perm=0) == -1 and b"n_perm" in L.tda_last_error()
    assert call(n_perm=7) == -1  # N + 1
    assert call(N=9000, n_perm=16) == -2 and b"8192" in L.tda_last_error()
    assert call(dtype=lb.TDA_F64) == -2 and b"float64" in L.tda_last_error()  # f64 points
    assert call(x=None) == -1
    assert call(L=0) == -1 and call(D=0) == -1 and call(dtype=5) == -1
    assert L.tda_greedy_perm(None, ctypes.byref(res)) == -1
    # valid arguments get as far as the device check: f32 points, and f64 distance matrices
    assert call() == -5
    M = np.zeros((1, 6, 6), np.float64)
    assert call(x=M.ctypes.data, dtype=lb.TDA_F64, is_dist=1, D=6) == -5
    L.tda_greedy_free(None)  # a no-op


def test_python_entries_refuse_unsupported_combinations(pkg, built_lib):
    X = np.random.default_rng(0).standard_normal((2, 10, 3)).astype(np.float32)
    with pytest.raises(ValueError):
        pkg.ripser_batch(X, n_perm=5, labels=[np.arange(10) % 2])
    with pytest.raises(ValueError):
        pkg.ripser_batch(X, n_perm=5, twonn=True)
    with pytest.raises(ValueError):
        pkg.ripser_batch([X, X], n_perm=5)  # input in parts
    with pytest.raises(ValueError):
        pkg.greedy_perm_batch([X, X], 5)
    for k in (0, 11, 2.5):
        with pytest.raises(ValueError):
            pkg.greedy_perm_batch(X, k)
        with pytest.raises(ValueError):
            pkg.ripser_batch(X, n_perm=k)
    with pytest.raises(ValueError):
        pkg.greedy_perm_batch(np.zeros((1, 4, 5), np.float32), 2, distance_matrix=True)  # not square
    with pytest.raises(ValueError):
        pkg.greedy_perm(X, 5)  # the single-cloud form takes a 2-D array
    Xn = X.copy()
    Xn[1, 2, 0] = np.nan
    with pytest.raises(ValueError):
        pkg.greedy_perm_batch(Xn, 5)
    # float64 point clouds: no exact contract with sklearn, refused; float64 distance matrices are not
    with pytest.raises(NotImplementedError):
        pkg.greedy_perm_batch(X.astype(np.float64), 5)
    with pytest.raises(NotImplementedError):
        pkg.ripser_batch(X.astype(np.float64), n_perm=5)
    with pytest.raises(NotImplementedError):
        pkg.greedy_perm_batch(np.zeros((1, 9000, 2), np.float32), 16)  # N > 8192
    with pytest.raises(RuntimeError):  # valid: fails only at the device check (no gfx950 here)
        pkg.greedy_perm_batch(np.zeros((1, 6, 6), np.float64), 3, distance_matrix=True)
    with pytest.raises(RuntimeError):
        pkg.ripser_batch(X, maxdim=1, n_perm=5)
    # the pipeline's slots do not run the greedy stage
    with pytest.raises(NotImplementedError):
        pkg.SweepPipeline(depth=2, maxdim=1, n_perm=5)
    with pkg.SweepPipeline(depth=1, maxdim=1) as pipe:
        with pytest.raises(NotImplementedError):
            pipe.submit(X, n_perm=5)


def test_ripser_single_cloud_n_perm_still_raises(pkg):
    X = np.random.default_rng(0).standard_normal((10, 3)).astype(np.float32)
    with pytest.raises(NotImplementedError):
        pkg.ripser(X, n_perm=5)
