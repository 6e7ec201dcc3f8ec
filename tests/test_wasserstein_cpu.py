"""CPU tests of the Wasserstein boundary (no device): the reference
tests/ws_ref.py against brute force and closed forms, the pair orientation of
csrc/dgm_plan.h (a sanitized host program of its own), the new symbols and the
ctypes mirrors of include/tda_dgm.h, the argument errors raised before any
device work, and the Python entries' argument handling."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ws_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tda-multimodal_amd", "csrc")
E = np.zeros((0, 2))


def brute_force(A, B) -> np.longdouble:
    """min over ALL partial matchings of the sum of the costs paid (longdouble), by recursion over the
    points of A: unmatched, or matched to a point of B not yet used."""
    C, cA, cB = (x.astype(np.longdouble) for x in ws_ref.costs(A, B))
    n1, n2 = len(A), len(B)

    def rec(i, used):
        if i == n1:
            return sum([cB[j] for j in range(n2) if not used >> j & 1], np.longdouble(0))
        best = cA[i] + rec(i + 1, used)
        for j in range(n2):
            if not used >> j & 1:
                best = min(best, C[i, j] + rec(i + 1, used | 1 << j))
        return best

    return rec(0, 0)


def small(n, rng):
    """n points on a coarse grid (many equal costs) with a few long bars."""
    b = rng.integers(0, 6, n).astype(np.float64) / 2
    return np.stack([b, b + rng.integers(1, 9, n) / 4 * rng.choice([1.0, 1.0, 3.0], n)], 1)


@pytest.mark.parametrize("n1", range(5))
@pytest.mark.parametrize("n2", range(5))
def test_reference_equals_brute_force(n1, n2):
    """The reference is a float64 solver itself, so it is held to the bound it holds the library to;
    on this grid two matchings either tie or differ by far more."""
    for seed in range(8):
        rng = np.random.default_rng(1000 * n1 + 100 * n2 + seed)
        A, B = small(n1, rng), small(n2, rng)
        if seed % 2 and n1 and n2:
            B[0] = A[0] + [0.25, -0.125]  # a close pair: matching it beats two diagonal costs
        ref, bf = ws_ref.value(A, B), brute_force(A, B)
        assert abs(ref - bf) <= ws_ref.bound(A, B), (A, B, ref, bf)
        assert abs(ws_ref.value_reduced(A, B) - bf) <= ws_ref.bound(A, B)


def chain(k, seed=0):
    """A_i = (2i, 2i + 100), B_i = (2i + 1, 2i + 101), each shuffled: A_i is at sqrt(2) from B_i and
    B_(i-1), at 3 sqrt(2) or more from the rest, and every point at 100 / sqrt(2) from the diagonal."""
    rng = np.random.default_rng(seed)
    i = np.arange(k, dtype=np.float64)
    A, B = np.stack([2 * i, 2 * i + 100], 1), np.stack([2 * i + 1, 2 * i + 101], 1)
    return A[rng.permutation(k)], B[rng.permutation(k)]


def test_reference_closed_forms():
    rng = np.random.default_rng(3)
    b = rng.uniform(0, 5, 40)
    A = np.stack([b, b + rng.uniform(0.1, 5, 40)], 1)
    cA = ((A[:, 1] - A[:, 0]) * ws_ref.SQRT1_2).astype(np.longdouble).sum()
    assert ws_ref.value(A, E) == ws_ref.value(E, A) == cA
    assert ws_ref.value(E, E) == 0.0
    assert ws_ref.value(A, A) == 0.0 and ws_ref.value(A, A[::-1]) == 0.0
    withinf = np.concatenate([A, [[0.0, np.inf], [1.0, np.inf]]])
    assert ws_ref.value(withinf, A[:7]) == ws_ref.value(A, A[:7])
    assert ws_ref.check_matching(A[:3], A[:2], np.array([1, -1, 0])) > 0
    for bad in ([0, 0, -1], [0, 2, -1], [0, -2, 1], [0, 1]):
        with pytest.raises(AssertionError):
            ws_ref.check_matching(A[:3], A[:2], np.array(bad))
    for k in (2, 65, 200):
        A, B = chain(k, k)
        W = k * np.sqrt(np.longdouble(2))
        assert abs(ws_ref.value(A, B) - W) <= 2 * k * ws_ref.U * W
        assert (ws_ref.solve(A, B) >= 0).all()
        W1 = (k - 1) * np.sqrt(np.longdouble(2)) + 100 * np.longdouble(ws_ref.SQRT1_2)
        assert abs(ws_ref.value(A[1:], B) - W1) <= 2 * k * ws_ref.U * W1
        m = ws_ref.solve(B, A[1:])
        assert (m < 0).sum() == 1


@pytest.fixture(scope="module")
def orient_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ws_plan") / "ws_plan")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "ws_plan_main.cpp")], check=True)
    return exe


def orient(exe, dgms, pairs):
    off = np.concatenate([[0], np.cumsum([len(d) for d in dgms])])
    pts = np.concatenate([np.asarray(d, np.float64).reshape(-1, 2) for d in dgms])
    text = " ".join(map(str, [len(dgms), *off, len(pts), *(repr(float(x)) for x in pts.ravel()), len(pairs), *np.asarray(pairs).ravel()]))
    r = subprocess.run([exe], input=text + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]  # a sanitizer report ends the program with a non-zero status
    return [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]


def test_orientation_is_canonical(orient_exe):
    rng = np.random.default_rng(5)

    def dg(n):
        b = rng.uniform(0, 5, n)
        return np.stack([b, b + rng.uniform(0.1, 5, n)], 1)

    a5, b5, c70, e0 = dg(5), dg(5), dg(70), E
    lo = a5.copy()
    lo[3, 1] = np.nextafter(lo[3, 1], -np.inf)  # differs from a5 in its 8th number alone, and is smaller there
    neg = np.array([[-0.0, 1.0]])
    pos = np.array([[0.0, 1.0]])
    junk = np.concatenate([[[np.nan, 1.0]], a5[:2], [[0.0, np.inf]], a5[2:]])  # a5's finite rows among others
    dgms = [a5, b5, c70, e0, a5.copy(), lo, neg, pos, junk]
    pairs = [(i, j) for i in range(len(dgms)) for j in range(len(dgms))]
    got = orient(orient_exe, dgms, pairs)
    by = {p: g for p, g in zip(pairs, got)}
    for (i, j), (f, s, sw) in by.items():
        assert (f, s) == ((j, i) if sw else (i, j))
        f2, s2, sw2 = by[j, i]
        same_input = all(ws_ref.finite_points(dgms[x]).tobytes() == ws_ref.finite_points(dgms[y]).tobytes()
                         for x, y in ((f, f2), (s, s2)))
        assert same_input, (i, j)  # both orientations upload the same two point arrays in the same order
        assert len(ws_ref.finite_points(dgms[f])) >= len(ws_ref.finite_points(dgms[s]))
    assert by[0, 2] == (2, 0, 1) and by[2, 0] == (2, 0, 0)  # more points first
    assert by[3, 0] == (0, 3, 1)
    first = 0 if tuple(a5.ravel()) < tuple(b5.ravel()) else 1
    assert by[0, 1][0] == by[1, 0][0] == first  # equal counts: the lexicographically smaller array first
    assert by[0, 5] == (5, 0, 1) and by[5, 0] == (5, 0, 0)
    assert by[6, 7] == (6, 7, 0) and by[7, 6] == (6, 7, 1)  # -0 below +0: equal means the same bits
    assert by[0, 4] == (0, 4, 0) and by[4, 0] == (4, 0, 0) and by[0, 0] == (0, 0, 0)  # equal arrays: as given
    assert by[0, 8] == (0, 8, 0) and by[8, 0] == (8, 0, 0)  # the non-finite rows do not count


def test_ws_structs_match_header_layout(pkg, tmp_path):
    lb = pkg._lib
    src = tmp_path / "wslayout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "tda_dgm.h"\n'
        'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(tda_ws_args),'
        ' offsetof(tda_ws_args, offsets), offsetof(tda_ws_args, S), offsetof(tda_ws_args, pairs), offsetof(tda_ws_args, P),'
        ' offsetof(tda_ws_args, device), offsetof(tda_ws_args, flags), sizeof(tda_ws_result), offsetof(tda_ws_result, dist),'
        ' offsetof(tda_ws_result, device_ms), offsetof(tda_ws_result, match_off), offsetof(tda_ws_result, match),'
        ' TDA_WS_MAX_POINTS, TDA_WS_WANT_MATCHING); return 0;}\n')
    exe = tmp_path / "wslayout"
    subprocess.run(["gcc", "-I", lb.INCLUDE, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    A, R = lb.WsArgs, lb.WsResult
    assert got == [ctypes.sizeof(A), A.offsets.offset, A.S.offset, A.pairs.offset, A.P.offset, A.device.offset, A.flags.offset,
                   ctypes.sizeof(R), R.dist.offset, R.device_ms.offset, R.match_off.offset, R.match.offset,
                   lb.TDA_WS_MAX_POINTS, lb.TDA_WS_WANT_MATCHING]
    assert lb.TDA_WS_MAX_POINTS == 512 and lb.TDA_WS_WANT_MATCHING == 1
    assert [f[0] for f in A._fields_[:6]] == [f[0] for f in lb.BnArgs._fields_[:6]]  # tda_bn_args' fields, then flags


def test_ws_symbols_exported_and_abi_version_unchanged(pkg, built_lib):
    lib = ctypes.CDLL(built_lib)
    assert hasattr(lib, "tda_wasserstein") and hasattr(lib, "tda_ws_free")
    assert pkg.WASSERSTEIN_EXPORTS == ("tda_wasserstein", "tda_ws_free")
    assert not set(pkg.WASSERSTEIN_EXPORTS) & (set(pkg.EXPORTS) | set(pkg.DGM_EXPORTS) | set(pkg.BOTTLENECK_EXPORTS))
    assert pkg.lib().tda_version() == 8  # symbols added only: no existing struct changed


def test_ws_invalid_arguments_rejected_before_device(pkg, built_lib):
    L = pkg.lib()
    lb = pkg._lib
    res = ctypes.POINTER(lb.WsResult)()
    pts = np.tile(np.array([[0.0, 1.0]]), (1030, 1))
    off = np.array([0, 512, 1024, 1025], np.int64)  # diagrams of 512, 512 and 1 points
    pr = np.array([[0, 2]], np.int32)

    def call(**kw):
        a = lb.WsArgs()
        a.points, a.offsets, a.S, a.pairs, a.P = pts.ctypes.data, off.ctypes.data, 3, pr.ctypes.data, 1
        a.device = 12345  # never a device: a valid call ends at the device check
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.tda_wasserstein(ctypes.byref(a), ctypes.byref(res))
        assert not res  # no result on failure
        return rc

    assert call() == -5 and call(pairs=None) == -5 and call(flags=1) == -5
    for f in (2, 3, 4, -1, 1 << 30):
        assert call(flags=f) == -1 and b"flags" in L.tda_last_error()
    assert call(offsets=None) == -1 and call(points=None) == -1 and call(S=-1) == -1 and call(P=-1) == -1
    bad = np.array([0, 5, 3, 1025], np.int64)
    assert call(offsets=bad.ctypes.data) == -1 and b"non-decreasing" in L.tda_last_error()
    bad = np.array([1, 5, 6, 7], np.int64)
    assert call(offsets=bad.ctypes.data) == -1
    for q in ([[0, 3]], [[-1, 0]]):
        q = np.array(q, np.int32)
        assert call(pairs=q.ctypes.data) == -1 and b"outside" in L.tda_last_error()
    # 513 finite points in one diagram, explicitly and among all pairs (pairs == NULL), with and without the matching
    big = np.array([0, 513, 1025], np.int64)
    q = np.array([[0, 1]], np.int32)
    assert call(offsets=big.ctypes.data, S=2, pairs=q.ctypes.data) == -2 and b"512" in L.tda_last_error()
    assert call(offsets=big.ctypes.data, S=2, pairs=q[:, ::-1].copy().ctypes.data, flags=1) == -2
    assert call(offsets=big.ctypes.data, S=2, pairs=None) == -2
    # a diagram above the limit that no requested pair holds is no error
    three = np.array([0, 513, 1025, 1030], np.int64)
    q = np.array([[1, 2]], np.int32)
    assert call(offsets=three.ctypes.data, pairs=q.ctypes.data) == -5
    # 512 finite points and 4 non-finite rows in one diagram: those do not count towards the limit
    pinf = pts.copy()
    pinf[[0, 100, 515], 1] = np.inf
    pinf[7, 0] = np.nan
    wide = np.array([0, 516, 1028], np.int64)  # 516 - 4 = 512 finite, and 512
    assert call(points=pinf.ctypes.data, offsets=wide.ctypes.data, S=2, pairs=None) == -5
    assert call(points=pts.ctypes.data, offsets=wide.ctypes.data, S=2, pairs=None) == -2
    # argument errors come before the device check even with the right device ordinal
    assert call(flags=2, device=0) == -1
    assert L.tda_wasserstein(None, ctypes.byref(res)) == -1
    assert L.tda_wasserstein(ctypes.byref(lb.WsArgs()), None) == -1
    L.tda_ws_free(None)  # a no-op


def test_python_entries_refuse_bad_arguments_before_the_library(pkg, monkeypatch):
    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(pkg._lib, "lib", no_library)
    A = np.array([[0.0, 1.0], [0.5, 2.0]])
    for bad in (np.zeros((3, 3)), np.zeros(3), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            pkg.wasserstein(A, bad)
        with pytest.raises(ValueError):
            pkg.wasserstein_matrix([A, bad])
        with pytest.raises(ValueError):
            pkg.wasserstein_matrix([A], other=[bad])
    big = np.tile(A, (257, 1))[:513]
    with pytest.raises(NotImplementedError, match="512"):
        pkg.wasserstein(A, big)
    with pytest.raises(NotImplementedError, match="512"):
        pkg.wasserstein(big, A, matching=True)
    with pytest.raises(NotImplementedError):
        pkg.wasserstein_matrix([A, A, big])
    with pytest.raises(NotImplementedError):
        pkg.wasserstein_matrix([A], other=[A, big])
    # nothing to compute: no library call, no device needed
    assert pkg.wasserstein_matrix([]).shape == (0, 0)
    assert pkg.wasserstein_matrix([A]).tolist() == [[0.0]]
    assert pkg.wasserstein_matrix([big]).tolist() == [[0.0]]  # no pair holds it
    assert pkg.wasserstein_matrix([A], other=[]).shape == (1, 0)
    assert pkg.wasserstein_matrix([], other=[A]).shape == (0, 1)
    D, ms = pkg.wasserstein_matrix([A], return_time=True)
    assert D.shape == (1, 1) and ms == 0.0
    assert {"wasserstein", "wasserstein_matrix", "layer_distance_matrix"} <= set(pkg.__all__)


def test_matching_format(pkg, monkeypatch):
    """matching=True: persim's (K, 3) rows [i, j, cost], -1 for the diagonal side, the indices into the
    diagrams without their non-finite rows; the library call replaced by a given map."""
    dg = importlib_module(pkg, "diagrams")
    A = np.array([[0.0, 1.0], [0.0, np.inf], [0.5, 2.0], [3.0, 3.5]])  # 3 finite rows
    B = np.array([[np.nan, 1.0], [0.25, 1.0], [4.0, 9.0], [0.5, 2.25]])  # 3 finite rows
    seen = {}

    def fake(points, offsets, pairs, device, want_matching=False):
        seen.update(points=points.copy(), offsets=offsets.copy(), pairs=pairs.copy(), device=device, want=want_matching)
        return np.array([1.25]), 0.5, (np.array([0, 3]) if want_matching else None), (np.array([0, 2, -1], np.int32) if want_matching else None)

    monkeypatch.setattr(dg, "_call_ws", fake)
    with pytest.warns(UserWarning, match="non-finite"):
        got = pkg.wasserstein(A, B, device=3)
    assert got == 1.25 and isinstance(got, float) and not seen["want"] and seen["device"] == 3
    assert seen["pairs"].tolist() == [[0, 1]] and seen["offsets"].tolist() == [0, 4, 8]
    with pytest.warns(UserWarning, match="non-finite"):
        d, M = pkg.wasserstein(A, B, matching=True)
    assert d == 1.25 and seen["want"] and M.shape == (4, 3) and M.dtype == np.float64
    Af, Bf = ws_ref.finite_points(A), ws_ref.finite_points(B)
    C, cA, cB = ws_ref.costs(Af, Bf)
    assert M.tolist() == [[0, 0, C[0, 0]], [1, 2, C[1, 2]], [2, -1, cA[2]], [-1, 1, cB[1]]]
    assert float(ws_ref.check_matching(A, B, M[M[:, 0] >= 0, 1].astype(np.int64))) == pytest.approx(M[:, 2].sum(), rel=1e-15)


def importlib_module(pkg, name):
    return __import__("importlib").import_module(pkg.__name__ + "." + name)


def test_layer_results_are_refused_by_the_pair_entry(pkg):
    rp = importlib_module(pkg, "ripser")  # pkg.ripser is the function
    b = rp._Batch()
    b.L, b.nd = 1, 2
    b.cnt = np.array([[1, 1]], np.int64)
    b.off = np.array([[0, 1]], np.int64)
    b.pairs = np.array([[0.0, 1.0], [0.5, 0.75]])
    r = rp.LayerResult((b, 0))
    with pytest.raises(ValueError, match="wasserstein_matrix"):
        pkg.wasserstein(r, E)
    with pytest.raises(ValueError, match="wasserstein_matrix"):
        pkg.wasserstein(E, r, matching=True)
    with pytest.raises(ValueError):
        pkg.wasserstein_matrix([r, np.zeros((1, 2))])


def test_layer_distance_matrix_routes_by_metric(pkg, monkeypatch):
    """metric="wasserstein" goes to wasserstein_matrix with dim and device and without M; the default
    and "bottleneck" go where they went, and an unknown name is still a ValueError naming `metric`."""
    pl = importlib_module(pkg, "pipeline")
    calls = []
    monkeypatch.setattr(pl, "wasserstein_matrix", lambda results, **kw: calls.append(("ws", results, kw)) or "WS")
    monkeypatch.setattr(pl, "bottleneck_matrix", lambda results, **kw: calls.append(("bn", results, kw)) or "BN")
    monkeypatch.setattr(pl, "sliced_wasserstein_matrix", lambda results, **kw: calls.append(("sw", results, kw)) or "SW")
    r = [E] * 2
    assert pkg.layer_distance_matrix(r, dim=0, M=0, device=3, metric="wasserstein") == "WS"  # M is not even checked
    assert pkg.layer_distance_matrix(r, metric="bottleneck") == "BN"
    assert pkg.layer_distance_matrix(r) == "SW" and pkg.layer_distance_matrix(r, 0, 7, 2) == "SW"
    assert calls == [("ws", r, {"device": 3, "dim": 0}), ("bn", r, {"device": 0, "dim": 1}),
                     ("sw", r, {"M": 50, "device": 0, "dim": 1}), ("sw", r, {"M": 7, "device": 2, "dim": 0})]
    for bad in ("Wasserstein", "w1", ""):
        with pytest.raises(ValueError, match="metric"):
            pkg.layer_distance_matrix(r, metric=bad)
    assert len(calls) == 4
