"""CPU tests of the resampling boundary (no device): the ctypes mirrors of tda_resample_args /
tda_resample_result have the header's layout, bad arguments come back with the documented codes
before any device work, the index tables and the quantile rule are what bootstrap.py documents, and
the Python entries refuse what they do not support before any library call."""
import ctypes
import subprocess

import numpy as np
import pytest

import resample_ref as rr


def test_resample_structs_match_header_layout(pkg, tmp_path):
    lb = pkg._lib
    a_fields = ["L", "N", "D", "is_dist", "device", "stream", "B", "m", "idx_per_layer", "idx"]
    r_fields = ["L", "N", "B", "m", "hausdorff", "device", "device_ms"]
    fmt = " ".join(["%zu"] * (2 + len(a_fields) + len(r_fields)))
    args = ", ".join(["sizeof(tda_resample_args)"] + [f"offsetof(tda_resample_args, {f})" for f in a_fields]
                     + ["sizeof(tda_resample_result)"] + [f"offsetof(tda_resample_result, {f})" for f in r_fields])
    src = tmp_path / "rlayout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tda_rips.h"\n'
                   f'int main(void){{printf("{fmt}\\n", {args}); return 0;}}\n')
    exe = tmp_path / "rlayout"
    subprocess.run(["gcc", "-I", lb.INCLUDE, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    A, R = lb.ResampleArgs, lb.ResampleResult
    assert got == ([ctypes.sizeof(A)] + [getattr(A, f).offset for f in a_fields]
                   + [ctypes.sizeof(R)] + [getattr(R, f).offset for f in r_fields])


def test_resample_constants_match_sources(pkg):
    import os
    import re

    lb = pkg._lib
    hdr = open(os.path.join(lb.INCLUDE, "tda_rips.h")).read()
    shift = re.search(r"#define TDA_RESAMPLE_MAX_OUT \((\d+)ll << (\d+)\)", hdr)
    assert shift and int(shift.group(1)) << int(shift.group(2)) == lb.TDA_RESAMPLE_MAX_OUT
    ker = open(os.path.join(lb.CSRC, "resample_kernels.h")).read()
    assert int(re.search(r"constexpr int kRsLdsN = (\d+);", ker).group(1)) == lb.TDA_RS_LDS_N
    assert lb.TDA_RS_LDS_N ** 2 * 4 <= 64 * 1024 < (lb.TDA_RS_LDS_N + 1) ** 2 * 4  # the largest tile in 64 KiB of static LDS


def test_resample_symbols_exported_and_abi_version_unchanged(pkg, built_lib):
    lib = ctypes.CDLL(built_lib)
    assert hasattr(lib, "tda_resample") and hasattr(lib, "tda_resample_free")
    assert {"tda_resample", "tda_resample_free"} <= set(pkg.EXPORTS)
    assert pkg.lib().tda_version() == 8  # symbols added only: no existing struct changed


def test_resample_invalid_arguments_rejected_before_device(pkg, built_lib):
    L = pkg.lib()
    lb = pkg._lib
    res = ctypes.POINTER(lb.ResampleResult)()
    X = np.zeros((2, 6, 3), np.float32)
    idx = np.array([[0, 1, 5], [2, 2, 3]], np.int32)  # (B = 2, m = 3)
    big = np.zeros(17 * 8193, np.int32)

    def call(**kw):
        a = lb.ResampleArgs()
        a.x, a.dtype, a.L, a.N, a.D, a.B, a.m, a.idx = X.ctypes.data, lb.TDA_F32, 2, 6, 3, 2, 3, idx.ctypes.data
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.tda_resample(ctypes.byref(a), ctypes.byref(res))
        assert not res  # no result on failure
        return rc

    # NULL pointers
    assert L.tda_resample(None, ctypes.byref(res)) == -1
    assert call(x=None) == -1 and b"x is NULL" in L.tda_last_error()
    assert call(idx=None) == -1 and b"idx is NULL" in L.tda_last_error()
    a = lb.ResampleArgs()
    assert L.tda_resample(ctypes.byref(a), None) == -1 and b"out is NULL" in L.tda_last_error()
    # counts
    assert call(B=0) == -1 and b"B must be" in L.tda_last_error()
    assert call(B=-3) == -1
    assert call(m=0) == -1 and b"m must be" in L.tda_last_error()
    assert call(L=0) == -1 and call(N=0) == -1 and call(D=0) == -1 and call(dtype=5) == -1
    # an index outside [0, N): below, above, and in the last layer's table only
    for bad in (-1, 6):
        t = idx.copy()
        t[1, 2] = bad
        assert call(idx=t.ctypes.data) == -1 and b"outside [0, N = 6)" in L.tda_last_error()
    per = np.stack([idx, idx])
    assert call(idx=per.ctypes.data, idx_per_layer=1) == -5
    per[1, 1, 0] = 6
    assert call(idx=per.ctypes.data, idx_per_layer=1) == -1 and b"idx[9] = 6" in L.tda_last_error()
    assert call(idx=per.ctypes.data, idx_per_layer=0) == -5  # the shared table ends before it
    # unsupported sizes and dtypes
    assert call(N=8193) == -2 and b"N > 8192" in L.tda_last_error()
    assert call(N=8192) == -5
    assert call(idx=big.ctypes.data, B=1, m=8193) == -2 and b"m > 8192" in L.tda_last_error()
    assert call(dtype=lb.TDA_F64) == -2 and b"float64" in L.tda_last_error()  # f64 points
    # more than 2^27 resamples in one call (refused before the table is read)
    assert call(B=2 ** 26 + 1) == -2 and b"2^27" in L.tda_last_error() and b"split B" in L.tda_last_error()
    # valid arguments get as far as the device check: f32 points and f64 distance matrices
    assert call() == -5 and b"gfx950" in L.tda_last_error()
    M = np.zeros((2, 6, 6), np.float64)
    assert call(x=M.ctypes.data, dtype=lb.TDA_F64, is_dist=1, D=6) == -5
    L.tda_resample_free(None)  # a no-op


def test_resample_indices(pkg):
    a, b = pkg.resample_indices(36, 50, seed=3), pkg.resample_indices(36, 50, seed=3)
    assert a.dtype == np.int32 and a.shape == (50, 36) and a.flags.c_contiguous
    assert a.tobytes() == b.tobytes()  # the same seed: the same bits
    assert a.tobytes() != pkg.resample_indices(36, 50, seed=4).tobytes()
    assert a.min() >= 0 and a.max() <= 35 and len(np.unique(a)) == 36
    assert any(len(set(r.tolist())) < 36 for r in a)  # with replacement: rows repeat points
    c = pkg.resample_indices(36, 50, m=7, seed=3)
    assert c.shape == (50, 7) and c.min() >= 0 and c.max() <= 35
    assert pkg.resample_indices(5, 4, m=9).shape == (4, 9)  # with replacement m may exceed N
    w = pkg.resample_indices(36, 50, m=20, replace=False, seed=3)
    assert w.dtype == np.int32 and w.shape == (50, 20) and w.min() >= 0 and w.max() <= 35
    assert all(len(set(r.tolist())) == 20 for r in w)  # rows unique
    assert w.tobytes() == pkg.resample_indices(36, 50, m=20, replace=False, seed=3).tobytes()
    full = pkg.resample_indices(9, 6, replace=False)
    assert all(sorted(r.tolist()) == list(range(9)) for r in full)  # m = N: permutations
    assert len({tuple(r.tolist()) for r in full}) > 1
    with pytest.raises(ValueError):
        pkg.resample_indices(36, 50, m=37, replace=False)
    for bad in (dict(N=0, B=1), dict(N=4, B=0), dict(N=4, B=2, m=0), dict(N=4, B=2.5), dict(N=4, B=2, m=1.5)):
        with pytest.raises(ValueError):
            pkg.resample_indices(**bad)


def test_quantile_is_an_order_statistic(pkg):
    bs = pkg.bootstrap
    # the rank ceil((1 - alpha) * B), within 1 .. B
    assert [bs.quantile_rank(1000, 0.05), bs.quantile_rank(16, 0.05), bs.quantile_rank(20, 0.05), bs.quantile_rank(20, 0.5)] == [950, 16, 19, 10]
    assert bs.quantile_rank(1, 0.5) == 1 and bs.quantile_rank(1, 0.999) == 1  # B = 1: the one statistic
    assert bs.quantile_rank(10, 0.01) == 10 and bs.quantile_rank(7, 1e-9) == 7  # ceil((1 - alpha) B) = B: the maximum
    assert bs.quantile_rank(10, 0.95) == 1
    for B, al in ((1000, 0.05), (16, 0.05), (7, 0.3), (1, 0.5), (10, 0.01)):
        assert bs.quantile_rank(B, al) == rr.rank(B, al)
    s = np.array([5.0, 1.0, 4.0, 2.0, 3.0])
    assert bs.order_quantile(s, 0.2) == 4.0 and bs.order_quantile(s, 0.21) == 4.0 and bs.order_quantile(s, 0.4) == 3.0  # never interpolated
    assert bs.order_quantile(s, 0.01) == 5.0 and bs.order_quantile(s, 0.99) == 1.0
    assert bs.order_quantile(np.array([7.5]), 0.05) == 7.5
    ties = np.array([2.0, 1.0, 2.0, 2.0, 0.5, 2.0, 3.0, 0.5])  # sorted: .5 .5 1 2 2 2 2 3
    assert [float(bs.order_quantile(ties, al)) for al in (0.8, 0.7, 0.5, 0.2, 0.1)] == [0.5, 1.0, 2.0, 2.0, 3.0]
    assert bs.order_quantile(np.full(9, 0.25), 0.05) == 0.25
    # along the last axis of a (K, L, B) block, against the counting restatement
    rng = np.random.default_rng(0)
    st = rng.integers(0, 6, size=(2, 3, 16)).astype(np.float64) / 4  # many ties
    for al in (0.05, 0.25, 0.5, 0.9):
        q = bs.order_quantile(st, al)
        assert q.shape == (2, 3) and np.array_equal(q, rr.quantile(st, al))
        assert all(q[p] in st[p] for p in np.ndindex(2, 3))


def test_python_entries_refuse_before_any_library_call(pkg, monkeypatch):
    # any library call would raise this: the refusals below come first
    def no_lib():
        raise AssertionError("the library was called")

    monkeypatch.setattr(pkg._lib, "lib", no_lib)
    X = np.random.default_rng(0).standard_normal((2, 10, 3)).astype(np.float32)
    idx = pkg.resample_indices(10, 4)
    cb = pkg.confidence_bands
    for al in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            cb(X, B=4, alpha=al)
    for B in (0, -2, 2.5, "3", None, True):
        with pytest.raises(ValueError, match="B must"):
            cb(X, B=B)
    for m in (0, -1, 1.5):
        with pytest.raises(ValueError, match="m must"):
            cb(X, B=4, m=m)
    with pytest.raises(ValueError):
        cb(X, B=4, m=11, replace=False)
    with pytest.raises(ValueError, match="method"):
        cb(X, B=4, method="wasserstein")
    with pytest.raises(NotImplementedError, match="bottleneck"):
        cb(X, B=4, method="bottleneck")  # needs the pipeline and the bottleneck entry in one process (known limits)
    with pytest.raises(ValueError, match="dims"):
        cb(X, B=4, maxdim=1, dims=[2])
    with pytest.raises(NotImplementedError):
        cb(X, B=4, maxdim=3)
    bad_idx = (idx[0], idx[None, None], np.zeros((0, 3), np.int32), np.stack([idx] * 3), idx.astype(np.float32), idx + 7, idx - 1,
               np.full((2, 2), 2 ** 40, np.int64))
    entries = (lambda Y, t, **kw: cb(Y, idx=t, **kw), pkg.hausdorff_resamples)
    for fn in entries:
        for t in bad_idx:  # the shape, the dtype, the range
            with pytest.raises(ValueError, match="idx"):
                fn(X, t)
        with pytest.raises(ValueError, match="parts"):
            fn([X, X], idx)  # a list of parts
        with pytest.raises(NotImplementedError, match="float64"):
            fn(X.astype(np.float64), idx)  # float64 points
        with pytest.raises(ValueError, match="square"):
            fn(np.zeros((1, 4, 5), np.float32), np.zeros((2, 3), np.int32), distance_matrix=True)
        with pytest.raises(ValueError):
            fn(X[0], idx)  # not (L, N, D)


def test_valid_python_calls_reach_the_device_check(pkg, built_lib):
    X = np.random.default_rng(0).standard_normal((2, 10, 3)).astype(np.float32)
    idx = pkg.resample_indices(10, 4)
    with pytest.raises(RuntimeError, match="gfx950"):
        pkg.hausdorff_resamples(X, idx)
    with pytest.raises(RuntimeError, match="gfx950"):
        pkg.hausdorff_resamples(np.zeros((2, 10, 10), np.float64), np.stack([idx, idx]).astype(np.int64), distance_matrix=True)
    with pytest.raises(RuntimeError, match="gfx950"):
        pkg.confidence_bands(X, B=4)
    with pytest.raises(RuntimeError, match="gfx950"):
        pkg.confidence_bands(X, B=4, method="hausdorff")


def test_twice_hausdorff_bounds_the_bottleneck_distance(oracle):
    """What the Hausdorff band rests on, d_B(dgm(X), dgm(X*)) <= 2 d_GH <= 2 H(X, X*) for the
    diameter-parameterised Rips filtration (Chazal, de Silva, Oudot 2014), on centred
    standard-normal clouds with the oracle and bn_ref.  The margin 2^-20 max(dm) covers the
    f32-rounded distances failing the triangle inequality by a few ulps: four roundings of at most
    2^-24 max(dm) each, about 2^-22 max(dm), times four."""
    import bn_ref

    L, N, B = 3, 36, 16
    X = np.random.default_rng(2014).standard_normal((L, N, 3)).astype(np.float32)
    X -= X.mean(axis=1, keepdims=True)
    idx = np.random.default_rng(2014).integers(0, N, size=(B, N), dtype=np.int32)
    for l in range(L):
        dm = oracle.distances(X[l])
        full = oracle.rips(X[l], maxdim=1)["dgms"]
        H = rr.hausdorff(dm[None], idx)[0]
        margin = 2.0 ** -20 * float(dm.max())
        for b in range(B):
            dg = oracle.rips(rr.sub(dm, idx[b]), maxdim=1, distance_matrix=True)["dgms"]
            for d in range(2):
                assert bn_ref.bottleneck(full[d], dg[d]) <= 2.0 * H[b] + margin, (l, b, d)
