"""CPU tests of the heat kernel boundary (no device): the references of tests/hk_ref.py
against each other and closed forms, the host plan of csrc/dgm_plan.h (hk_plan, a sanitized
host program of its own), the new symbols and the ctypes mirrors of include/tda_dgm.h, the
argument errors raised before any device work, the Python entries' argument handling and
the routing of layer_distance_matrix(metric="heat")."""
import ctypes
import os
import subprocess

import mpmath
import numpy as np
import pytest

import hk_ref
from test_wasserstein import diagram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tda-multimodal_amd", "csrc")
E = np.zeros((0, 2))
SIGMAS = (0.01, 0.4, 5.0)


# ---------------------------------------------------------------- the references
def test_constants_and_bound_functions():
    c8, cn = hk_ref.constants(0.4)
    assert c8 == 1.0 / 3.2 and cn == 1.0 / (25.132741228718345908 * 0.4)
    assert hk_ref.depth(1, 1) == 1 + 12 + 1 and hk_ref.depth(4096, 4096) == 256 + 12 + 16 and hk_ref.depth(65, 3) == 3 + 12 + 1
    assert hk_ref.C(1, 1) == 2 * 3 + 8 + 14 and hk_ref.C(3, 65) == hk_ref.C(65, 3) == 195 * (14 + 16)
    assert hk_ref.C(0, 7) == 0 and hk_ref.bound_k(4096, 4096, 0.4) == 4096 * 4096 * (14 + 284) * 2.0 ** -53 * cn
    assert hk_ref.EXP_ULP == 3 and (hk_ref.ROWS, hk_ref.CHUNK) == (64, 256)


def test_exact_reference_closed_forms():
    with mpmath.workdps(40):
        P = np.array([[1.0, 3.0]])
        c8, cn = (mpmath.mpf(c) for c in hk_ref.constants(0.4))
        assert abs(hk_ref.exact_k(P, P, 0.4) - cn * (1 - mpmath.exp(-c8 * 8))) < mpmath.mpf(10) ** -38  # r2 = 0, m2 = 2 * 2^2
        assert hk_ref.exact_k(P, E, 0.4) == 0 and hk_ref.exact_k(E, E, 0.4) == 0
        A, B = diagram(7, 1), diagram(5, 2)
        assert abs(hk_ref.exact_k(A, B, 5.0) - hk_ref.exact_k(B, A, 5.0)) < mpmath.mpf(10) ** -36
        withinf = np.concatenate([A[:3], [[0.0, np.inf], [np.nan, 1.0]], A[3:]])
        assert hk_ref.exact_k(withinf, B, 0.4) == hk_ref.exact_k(A, B, 0.4)
        diag = np.array([[2.0, 2.0]])  # a point on the diagonal is its own mirror image: it adds nothing
        assert hk_ref.exact_k(diag, A, 0.4) == 0
        # a kernel: the squared distance of two different diagrams is positive
        assert hk_ref.d2(hk_ref.exact_k(A, A, 0.4), hk_ref.exact_k(B, B, 0.4), hk_ref.exact_k(A, B, 0.4)) > 0


@pytest.mark.parametrize("sigma", SIGMAS)
def test_longdouble_reference_is_good_enough_to_judge(sigma):
    """The condition (not a measurement) under which ld_k may stand in for the exact value at the
    large sizes: on 1 to 65 points it stays below 1 / 16 of the bound."""
    assert np.finfo(hk_ref.LD).nmant >= 63
    worst = 0.0
    for n1, n2 in ((1, 1), (2, 1), (7, 5), (33, 64), (65, 65), (65, 1)):
        F, G = diagram(n1, 100 + n1), diagram(n2, 200 + n2)
        for X, Y in ((F, G), (F, F)):
            with mpmath.workdps(40):
                err = float(abs(hk_ref.to_mpf(hk_ref.ld_k(X, Y, sigma)) - hk_ref.exact_k(X, Y, sigma)))
            tol = hk_ref.bound_k(len(X), len(Y), sigma) / 16
            worst = max(worst, err / tol)
            assert err <= tol, (n1, n2, sigma, err, tol)
            rest = abs(hk_ref.restatement_k(X, Y, sigma) - float(hk_ref.ld_k(X, Y, sigma)))
            assert rest <= hk_ref.bound_k(len(X), len(Y), sigma)  # the numpy restatement is inside the bound too
    print(f"sigma={sigma}: longdouble against mpmath, largest error over bound / 16: {worst:.3e}")


# ---------------------------------------------------------------- the sanitized plan program
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hk_plan") / "hk_plan")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "hk_plan_main.cpp")], check=True)
    return exe


def run_plan(exe, words):
    r = subprocess.run([exe], input=" ".join(map(str, words)) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]  # a sanitizer report ends the program with a non-zero status
    if r.stdout.startswith("err"):
        _, code, msg = r.stdout.strip().split(" ", 2)
        return int(code), msg
    out = {}
    for line in r.stdout.splitlines():
        k, *v = line.split()
        out[k] = [float.fromhex(x) for x in v] if k in ("pts", "c") else [int(x) for x in v]
    return 0, out


def hk_case(exe, dgms, pairs=None, P=None, sigma=0.4, reserved=0, offsets=None, points=True, S=None):
    off = np.concatenate([[0], np.cumsum([len(d) for d in dgms])]).astype(int) if offsets is None else offsets
    pts = np.concatenate([np.asarray(d, np.float64).reshape(-1, 2) for d in dgms]) if dgms else E
    head = [len(off) - 1 if not isinstance(off, str) else len(dgms), *(["null"] if isinstance(off, str) else off)]
    head = head if S is None else [S]  # S < 0: the program reads no offsets
    head += [len(pts), *[repr(float(x)) for x in pts.ravel()]] if points else [-1]
    pr = [-1] if pairs is None else [len(pairs), *np.asarray(pairs, int).reshape(-1)]
    return run_plan(exe, ["hk", *head, *pr, (0 if pairs is None else len(pairs)) if P is None else P, repr(float(sigma)), reserved])


def test_plan_work_list_orientation_and_parts(plan_exe):
    sizes = [65, 0, 64, 300, 513, 4096, 1]
    dgms = [diagram(n, n) for n in sizes]
    pairs = [(0, 2), (2, 0), (1, 3), (3, 4), (4, 3), (5, 6), (6, 5), (5, 5), (1, 1), (2, 2)]
    rc, p = hk_case(plan_exe, dgms, pairs)
    assert rc == 0 and p["P"] == [10] and p["S"] == [7]
    assert p["c"] == list(hk_ref.constants(0.4))
    assert np.array(p["pts"]).tobytes() == np.concatenate(dgms).ravel().tobytes()
    got = np.array(p["pairs"]).reshape(-1, 2)
    assert len(got) == 17
    # the longer diagram first: (i, j) and (j, i) are the same evaluation
    assert got[:10].tolist() == [[0, 2], [0, 2], [3, 1], [4, 3], [4, 3], [5, 6], [5, 6], [5, 5], [1, 1], [2, 2]]
    assert got[10:].tolist() == [[s, s] for s in range(7)]  # the self pairs, after the caller's
    n = np.array(sizes)
    parts = [int(-(-n[i] // 64) * -(-n[j] // 256)) for i, j in got]
    assert p["part_off"] == np.concatenate([[0], np.cumsum(parts)]).tolist()
    assert parts[0] == 2 and parts[2] == 0 and parts[3] == 9 * 2 and parts[5] == 64 and parts[7] == 1024 and parts[8] == 0
    big = np.array([max(n[i], n[j]) for i, j in got])
    cls = np.where(big <= 64, 0, np.where(big <= 512, 1, 2))
    assert p["order"] == [int(w) for c in range(3) for w in np.flatnonzero(cls == c)]
    assert p["cnt"] == [int((cls == c).sum()) for c in range(3)]
    assert p["cls_parts"] == [max(np.array(parts)[cls == c]) for c in range(3)] == [1, 10, 1024]
    # equal counts: the lexicographically smaller point array first, whichever way the pair is named
    A, B = diagram(9, 1), diagram(9, 2)
    first = 0 if A.ravel().tolist() < B.ravel().tolist() else 1
    rc, p = hk_case(plan_exe, [A, B], [(0, 1), (1, 0)])
    assert np.array(p["pairs"]).reshape(-1, 2)[:2].tolist() == [[first, 1 - first]] * 2
    rc, p = hk_case(plan_exe, [A, A.copy()], [(0, 1), (1, 0)])  # equal arrays: as named, and it does not matter
    assert rc == 0 and np.array(p["pairs"]).reshape(-1, 2)[:2].tolist() == [[0, 1], [1, 0]]
    # pairs == NULL: every i < j, row-major, then the selfs
    rc, p = hk_case(plan_exe, [diagram(3, 1), diagram(4, 2), diagram(5, 3)])
    assert rc == 0 and p["P"] == [3]
    assert np.array(p["pairs"]).reshape(-1, 2).tolist() == [[1, 0], [2, 0], [2, 1], [0, 0], [1, 1], [2, 2]]
    rc, p = hk_case(plan_exe, [])
    assert rc == 0 and p["P"] == [0] and p["pairs"] == [] and p["part_off"] == [0] and p["off"] == [0]
    rc, p = hk_case(plan_exe, [E])  # one empty diagram: a self without parts
    assert rc == 0 and p["pairs"] == [0, 0] and p["part_off"] == [0, 0] and p["cls_parts"] == [0, 0, 0]
    # non-finite rows are dropped before anything is counted
    junk = np.array([[np.nan, 1.0], [0.5, 1.5], [0.0, np.inf], [-0.0, 2.0]])
    rc, p = hk_case(plan_exe, [junk])
    assert rc == 0 and p["off"] == [0, 2] and np.array(p["pts"]).tobytes() == junk[[1, 3]].ravel().tobytes()


def test_plan_errors_in_the_header_order(plan_exe):
    D = [diagram(5, 1), diagram(70, 2)]
    assert hk_case(plan_exe, D, [(0, 1)])[0] == 0
    assert run_plan(plan_exe, ["null"]) == (-1, "args is NULL")
    # each case carries the faults of all later checks too: the earlier check answers
    late = dict(offsets=[0, 50, 5], pairs=[(0, 9)])
    assert hk_case(plan_exe, D, S=-1, reserved=1, sigma=0.0, **late) == (-1, "S must be >= 0")
    assert hk_case(plan_exe, D, offsets="null", reserved=1, sigma=0.0, pairs=[(0, 9)]) == (-1, "offsets is NULL")
    assert hk_case(plan_exe, D, reserved=1, sigma=0.0, **late) == (-1, "reserved must be 0")
    for s in (0.0, -1.0, -0.0, np.nan, np.inf, -np.inf):
        assert hk_case(plan_exe, D, sigma=s, **late) == (-1, "sigma must be finite and > 0"), s
    for s in (5e-310, 5e-324, 1e307, 1e308, 1.7e308):  # c8 or cn overflows, or is subnormal
        rc, msg = hk_case(plan_exe, D, sigma=s, **late)
        assert rc == -1 and "normal" in msg, s
    for s in (1e-300, 1e300, 1e-6):
        assert hk_case(plan_exe, D, [(0, 1)], sigma=s)[0] == 0
    assert hk_case(plan_exe, D, offsets=[1, 5, 75], pairs=[(0, 9)])[0] == -1
    rc, msg = hk_case(plan_exe, D, **late)
    assert rc == -1 and "non-decreasing" in msg
    assert hk_case(plan_exe, D, points=False, pairs=[(0, 9)]) == (-1, "points is NULL")
    assert hk_case(plan_exe, D, pairs=[(0, 9)], P=-1) == (-1, "P must be >= 0")
    rc, msg = hk_case(plan_exe, D, pairs=[(0, 1)], P=(1 << 27) + 1)  # refused before the pairs are read
    assert rc == -2 and "2^27" in msg
    big = [diagram(5, 1), diagram(4097, 3)]
    for bad in ([(0, 2)], [(-1, 0)], [(0, 1), (2, 2)]):
        rc, msg = hk_case(plan_exe, big, bad)
        assert rc == -1 and "outside" in msg  # before the size limit
    # the 4096 / 4097 limit, on finite rows, whether a pair names the diagram or not
    rc, msg = hk_case(plan_exe, big, [(0, 0)])
    assert rc == -2 and "4096" in msg
    rc, msg = hk_case(plan_exe, big)
    assert rc == -2 and "4096" in msg
    wide = np.concatenate([diagram(4096, 4), [[0.0, np.inf]] * 3])
    rc, p = hk_case(plan_exe, [wide, diagram(1, 5)])
    assert rc == 0 and p["part_off"] == [0, 64, 64 + 1024, 64 + 1024 + 1]
    # the scratch limit, the header's last case: 2^27 parts of the call's P + S evaluations pass, more do not.
    # Two diagrams of 4096 points: 1024 parts per evaluation, the two selfs included
    two = [diagram(4096, 6), diagram(4096, 7)]
    rc, p = hk_case(plan_exe, two, np.tile([[0, 1]], (131070, 1)))
    assert rc == 0 and p["P"] == [131070] and p["part_off"][-1] == 1 << 27 and p["cnt"] == [0, 0, 131072]
    for npairs in (131071, 131072):
        rc, msg = hk_case(plan_exe, two, np.tile([[0, 1]], (npairs, 1)))
        assert rc == -2 and "2^27 parts" in msg, npairs
    rc, msg = hk_case(plan_exe, two + [diagram(4097, 8)], np.tile([[0, 1]], (131072, 1)))  # the point limit answers first
    assert rc == -2 and "4096 finite points" in msg
    rc, msg = hk_case(plan_exe, two, np.concatenate([np.tile([[0, 1]], (131072, 1)), [[0, 2]]]))  # and so does a bad index
    assert rc == -1 and "outside" in msg


# ---------------------------------------------------------------- the ABI
def test_hk_structs_match_header_layout(pkg, tmp_path):
    lb = pkg._lib
    src = tmp_path / "hklayout.c"
    names = {"tda_hk_args": ["offsets", "S", "pairs", "P", "sigma", "device", "reserved"],
             "tda_hk_result": ["kern", "self", "dist", "device_ms"]}
    body = "".join(f'printf("%zu ", sizeof({t}));' + "".join(f'printf("%zu ", offsetof({t}, {f}));' for f in fs) for t, fs in names.items())
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tda_dgm.h"\nint main(void){' + body +
                   'printf("%d %d\\n", TDA_HK_MAX_POINTS, TDA_HK_EXP_ULP); return 0;}\n')
    exe = tmp_path / "hklayout"
    subprocess.run(["gcc", "-I", lb.INCLUDE, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for t, fs in zip((lb.HkArgs, lb.HkResult), names.values()):
        want += [ctypes.sizeof(t)] + [getattr(t, f).offset for f in fs]
        assert [f[0] for f in t._fields_[1:]] == fs  # every field after the first is compared
    want += [lb.TDA_HK_MAX_POINTS, lb.TDA_HK_EXP_ULP]
    assert got == want and want[-2:] == [4096, 3] and hk_ref.EXP_ULP == lb.TDA_HK_EXP_ULP
    assert [f[0] for f in lb.HkArgs._fields_[:5]] == [f[0] for f in lb.BnArgs._fields_[:5]]  # as in tda_bn_args


def test_hk_symbols_exported_and_abi_version_unchanged(pkg, built_lib):
    """The library cross-compiles for gfx950 through the project's build() (built_lib) and exports the
    new symbols beside the old ones."""
    lib = ctypes.CDLL(built_lib)
    assert pkg.HEAT_EXPORTS == ("tda_heat_kernel", "tda_hk_free")
    assert all(hasattr(lib, s) for s in pkg.HEAT_EXPORTS)
    others = set(pkg.EXPORTS) | set(pkg.DGM_EXPORTS) | set(pkg.BOTTLENECK_EXPORTS) | set(pkg.WASSERSTEIN_EXPORTS) | set(pkg.VECTOR_EXPORTS)
    assert not set(pkg.HEAT_EXPORTS) & others and all(hasattr(lib, s) for s in others)
    assert pkg.lib().tda_version() == 8  # symbols added only: no existing struct changed


def test_hk_invalid_arguments_rejected_before_device(pkg, built_lib):
    L, lb = pkg.lib(), pkg._lib
    pts = np.tile(np.array([[0.0, 1.0]]), (4200, 1))
    off = np.array([0, 5, 4101], np.int64)  # 5 and 4096 points
    pairs = np.array([[0, 1], [1, 0], [1, 1]], np.int32)
    res = ctypes.POINTER(lb.HkResult)()

    def hk(**kw):
        a = lb.HkArgs()
        a.points, a.offsets, a.S, a.pairs, a.P, a.sigma = pts.ctypes.data, off.ctypes.data, 2, pairs.ctypes.data, 3, 0.4
        a.device = 12345  # never a device: a valid call ends at the device check
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.tda_heat_kernel(ctypes.byref(a), ctypes.byref(res))
        assert not res  # no result on failure
        return rc

    def invalid(**kw):
        rc = hk(**kw)
        assert rc in (-1, -2) and L.tda_last_error(), kw
        return rc

    assert hk() == -5 and hk(pairs=None) == -5 and hk(S=0, P=0) == -5 and hk(sigma=1e-6) == -5
    assert invalid(reserved=1) == -1 and b"reserved" in L.tda_last_error()
    assert invalid(reserved=2, device=0) == -1  # before the device check even with the right ordinal
    for s in (0.0, -0.4, float("nan"), float("inf"), 5e-310, 1e307, 1.7e308):
        assert invalid(sigma=s) == -1 and b"sigma" in L.tda_last_error(), s
    assert invalid(offsets=None) == -1 and invalid(points=None) == -1 and invalid(S=-1) == -1 and invalid(P=-1) == -1
    bad = np.array([0, 50, 5], np.int64)
    assert invalid(offsets=bad.ctypes.data) == -1 and b"non-decreasing" in L.tda_last_error()
    bad = np.array([1, 5, 6], np.int64)
    assert invalid(offsets=bad.ctypes.data) == -1
    for p in ([[0, 2]], [[-1, 0]]):
        p = np.array(p, np.int32)
        assert invalid(pairs=p.ctypes.data, P=1) == -1 and b"outside" in L.tda_last_error()
    big = np.array([0, 4097, 4200], np.int64)
    assert invalid(offsets=big.ctypes.data) == -2 and b"4096" in L.tda_last_error()  # 4097 finite points
    assert invalid(offsets=big.ctypes.data, pairs=None) == -2
    p = np.array([[1, 1]], np.int32)
    assert invalid(offsets=big.ctypes.data, pairs=p.ctypes.data, P=1) == -2  # no pair names it: its self does
    pinf = pts.copy()  # 4096 finite points and non-finite rows in one diagram: those do not count
    pinf[[0, 100, 4000], 1] = np.inf
    pinf[7, 0] = np.nan
    wide = np.array([0, 4100, 4200], np.int64)
    assert hk(points=pinf.ctypes.data, offsets=wide.ctypes.data) == -5 and invalid(offsets=wide.ctypes.data) == -2
    assert invalid(P=(1 << 27) + 1) == -2 and b"2^27" in L.tda_last_error()
    assert L.tda_heat_kernel(None, ctypes.byref(res)) == -1 and L.tda_heat_kernel(ctypes.byref(lb.HkArgs()), None) == -1
    L.tda_hk_free(None)  # a no-op


# ---------------------------------------------------------------- the Python entries
def importlib_module(pkg, name):
    return __import__("importlib").import_module(pkg.__name__ + "." + name)


def test_python_entries_refuse_bad_arguments_before_the_library(pkg, monkeypatch):
    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(pkg._lib, "lib", no_library)
    A = np.array([[0.0, 1.0], [0.5, 2.0]])
    for s in (0, 0.0, -0.4, np.nan, np.inf, -np.inf, 5e-310, 1e307, 1.7e308):
        for call in (lambda: pkg.heat(A, A, s), lambda: pkg.heat(A, A, sigma=s), lambda: pkg.heat_matrix([A, A], s),
                     lambda: pkg.heat_kernel_matrix([A], sigma=s), lambda: pkg.heat_matrix([], s), lambda: pkg.heat_matrix([A], s, other=[])):
            with pytest.raises(ValueError, match="sigma"):
                call()
    for bad in (np.zeros((3, 3)), np.zeros(3), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            pkg.heat(A, bad)
        with pytest.raises(ValueError):
            pkg.heat_matrix([A, bad])
        with pytest.raises(ValueError):
            pkg.heat_kernel_matrix([A], other=[bad])
    big = np.tile(A, (2049, 1))[:4097]
    for call in (lambda: pkg.heat(A, big), lambda: pkg.heat_matrix([A, big]), lambda: pkg.heat_matrix([big]),
                 lambda: pkg.heat_kernel_matrix([A], other=[A, big])):
        with pytest.raises(NotImplementedError, match="4096"):
            call()
    # nothing to compute: no library call, no device needed
    assert pkg.heat_matrix([]).shape == (0, 0) and pkg.heat_kernel_matrix([]).shape == (0, 0)
    assert pkg.heat_matrix([A]).tolist() == [[0.0]]
    assert pkg.heat_matrix([A], other=[]).shape == (1, 0) and pkg.heat_matrix([], other=[A]).shape == (0, 1)
    assert pkg.heat_kernel_matrix([A], other=[]).shape == (1, 0) and pkg.heat_kernel_matrix([], other=[A, A]).shape == (0, 2)
    for out in (pkg.heat_matrix([A], return_time=True), pkg.heat_matrix([], 0.4, [A], return_time=True),
                pkg.heat_kernel_matrix([], return_time=True)):
        assert isinstance(out, tuple) and out[0].dtype == np.float64 and out[1] == 0.0
    assert {"heat", "heat_matrix", "heat_kernel_matrix", "layer_distance_matrix"} <= set(pkg.__all__)


def test_what_reaches_the_library_and_how_the_matrices_are_filled(pkg, monkeypatch):
    dg = importlib_module(pkg, "diagrams")
    seen = {}

    def fake(points, offsets, pairs, sigma, device):
        seen.update(points=points.copy(), offsets=offsets.copy(), pairs=None if pairs is None else pairs.copy(), sigma=sigma, device=device)
        S = len(offsets) - 1
        P = S * (S - 1) // 2 if pairs is None else len(pairs)
        return 100.0 + np.arange(P), 10.0 + np.arange(S), 1.0 + np.arange(P), 0.75

    monkeypatch.setattr(dg, "_call_hk", fake)
    A, B, C = np.array([[0.5, 1.0], [0.25, np.inf]]), np.array([[0.375, 0.5]]), E
    with pytest.warns(UserWarning, match="non-finite"):
        D, ms = pkg.heat_matrix([A, B, C], 0.25, device=2, return_time=True)
    assert ms == 0.75 and seen["pairs"] is None and (seen["sigma"], seen["device"]) == (0.25, 2) and seen["offsets"].tolist() == [0, 2, 3, 3]
    assert D.tolist() == [[0.0, 1.0, 2.0], [1.0, 0.0, 3.0], [2.0, 3.0, 0.0]]
    K = pkg.heat_kernel_matrix([B, B, C])
    assert K.tolist() == [[10.0, 100.0, 101.0], [100.0, 11.0, 102.0], [101.0, 102.0, 12.0]] and seen["sigma"] == 0.4
    assert pkg.heat_kernel_matrix([B]).tolist() == [[10.0]]  # one diagram still has a self
    D = pkg.heat_matrix([B, C], other=[B, B, C])
    assert D.tolist() == [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]] and seen["pairs"].tolist() == [[0, 2], [0, 3], [0, 4], [1, 2], [1, 3], [1, 4]]
    assert seen["pairs"].dtype == np.int32 and seen["offsets"].tolist() == [0, 1, 1, 2, 3, 3]
    assert pkg.heat_kernel_matrix([B, C], other=[B])[1, 0] == 101.0
    assert pkg.heat(B, C, 2, device=1) == 1.0 and (seen["sigma"], seen["device"]) == (2.0, 1)


def test_layer_results_are_refused_by_the_pair_entry(pkg):
    rp = importlib_module(pkg, "ripser")  # pkg.ripser is the function
    b = rp._Batch()
    b.L, b.nd = 1, 2
    b.cnt = np.array([[1, 1]], np.int64)
    b.off = np.array([[0, 1]], np.int64)
    b.pairs = np.array([[0.0, 1.0], [0.5, 0.75]])
    r = rp.LayerResult((b, 0))
    with pytest.raises(ValueError, match="heat_matrix"):
        pkg.heat(r, E)
    with pytest.raises(ValueError, match="heat_matrix"):
        pkg.heat(E, r)
    with pytest.raises(ValueError):
        pkg.heat_matrix([r, np.zeros((1, 2))])
    with pytest.raises(ValueError, match="dim"):
        pkg.heat_kernel_matrix([r], dim=2)


def test_layer_distance_matrix_routes_heat(pkg, monkeypatch):
    """metric="heat" goes to heat_matrix with sigma, dim and device and without M; the other three get
    exactly the keywords they got, and an unknown name is still a ValueError naming `metric`."""
    pl = importlib_module(pkg, "pipeline")
    calls = []
    monkeypatch.setattr(pl, "heat_matrix", lambda results, **kw: calls.append(("hk", results, kw)) or "HK")
    monkeypatch.setattr(pl, "wasserstein_matrix", lambda results, **kw: calls.append(("ws", results, kw)) or "WS")
    monkeypatch.setattr(pl, "bottleneck_matrix", lambda results, **kw: calls.append(("bn", results, kw)) or "BN")
    monkeypatch.setattr(pl, "sliced_wasserstein_matrix", lambda results, **kw: calls.append(("sw", results, kw)) or "SW")
    r = [E] * 2
    assert pkg.layer_distance_matrix(r, dim=0, M=0, device=3, metric="heat", sigma=2.5) == "HK"  # M is not even checked
    assert pkg.layer_distance_matrix(r, metric="heat") == "HK"
    assert pkg.layer_distance_matrix(r, metric="wasserstein", sigma=-1.0) == "WS"  # only "heat" reads sigma
    assert pkg.layer_distance_matrix(r, metric="bottleneck", sigma=9.0) == "BN"
    assert pkg.layer_distance_matrix(r, sigma=9.0) == "SW" and pkg.layer_distance_matrix(r, 0, 7, 2) == "SW"
    assert calls == [("hk", r, {"sigma": 2.5, "device": 3, "dim": 0}), ("hk", r, {"sigma": 0.4, "device": 0, "dim": 1}),
                     ("ws", r, {"device": 0, "dim": 1}), ("bn", r, {"device": 0, "dim": 1}),
                     ("sw", r, {"M": 50, "device": 0, "dim": 1}), ("sw", r, {"M": 7, "device": 2, "dim": 0})]
    for bad in ("Heat", "heat_kernel", ""):
        with pytest.raises(ValueError, match="metric.*'sliced_wasserstein', 'bottleneck', 'wasserstein' or 'heat'"):
            pkg.layer_distance_matrix(r, metric=bad)
    assert len(calls) == 6
