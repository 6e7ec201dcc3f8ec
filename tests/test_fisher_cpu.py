"""CPU tests of the persistence Fisher boundary (no device): the references of tests/pf_ref.py
against closed forms and each other within the header's bound, the host plan of csrc/dgm_plan.h
(pf_plan, a sanitized host program of its own), the new symbols and the ctypes mirrors of
include/tda_dgm.h, the argument errors raised before any device work, the Python entries'
argument handling and the routing of layer_distance_matrix / diagram_permutation_test with
metric="fisher"."""
import ctypes
import os
import subprocess

import mpmath
import numpy as np
import pytest

import pf_ref
from test_wasserstein import diagram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tda-multimodal_amd", "csrc")
E = np.zeros((0, 2))
SIGMAS = (0.05, 1.0, 5.0)


# ---------------------------------------------------------------- the references
def test_constants_and_bound_functions():
    assert pf_ref.c2_of(0.5) == 2.0 and pf_ref.c2_of(1.0) == 0.5 and pf_ref.c2_of(0.05) == 1.0 / (2.0 * (0.05 * 0.05))
    assert pf_ref.T == 6 * 708 + 2 * 3 + 2 == 4256 and pf_ref.R(3, 5) == 4264
    assert pf_ref.bound(3, 5) == (2 * 4264 + 30) * 2.0 ** -53 + 24 * 2.0 ** -510
    assert pf_ref.bound(1024, 1024) == (2 * (4256 + 2048) + 30) * 2.0 ** -53 + 3 * 2048 * 2.0 ** -510
    assert pf_ref.bound(1024, 1024) < 1.5e-12  # what the derivation gives at the limit
    assert (pf_ref.LANES, pf_ref.CHUNK, pf_ref.CUT, pf_ref.MAX_POINTS) == (64, 128, 708, 1024)
    # two row orders: 2 (2 M + 30) u stays below B for every M the entry accepts (promise 4)
    assert 2 * (2 * 2048 + 30) <= 2 * pf_ref.R(1024, 1024) + 30
    B = pf_ref.bound(8, 8)
    assert pf_ref.bound_dist(0.5, B) < 4 * B + 4 * pf_ref.U_ and 0.9 * np.sqrt(2 * B) < pf_ref.bound_dist(1.0, B) < 1.1 * np.sqrt(2 * B)


def test_closed_forms_against_exact():
    with mpmath.workdps(50):
        eps = mpmath.mpf(10) ** -45
        # F = {p}, G empty: affinity 2 sqrt(g) / (1 + g), g = exp(-c2 pers^2 / 2)
        p = np.array([[1.0, 3.0]])
        for sigma in SIGMAS:
            g = mpmath.exp(-mpmath.mpf(pf_ref.c2_of(sigma)) * 2)
            want = 2 * mpmath.sqrt(g) / (1 + g)
            for X, Y in ((p, E), (E, p)):
                aff, dist = pf_ref.exact(X, Y, sigma)
                assert abs(aff - want) < eps and abs(dist - mpmath.acos(want)) < eps
            a, b, h = pf_ref.sums(p, E, sigma)
            assert a == b and abs(mpmath.mpf(a) - (1 + g)) < 4 * pf_ref.U_ and abs(pf_ref.affinity_of(a, b, h) - want) <= pf_ref.bound(1, 0)
        # two single points with every cross argument below -708: h == 0.0, the distance arccos(0)
        p, q = np.array([[0.0, 10.0]]), np.array([[100.0, 130.0]])
        aff, dist = pf_ref.exact(p, q, 0.05)
        assert aff == 0 and abs(dist - mpmath.pi / 2) < eps
        a, b, h = pf_ref.sums(p, q, 0.05)
        assert (a, b, h) == (2.0, 2.0, 0.0) and pf_ref.restatement(p, q, 0.05) == np.arccos(0.0)
        # F == G
        A = diagram(7, 1)
        aff, dist = pf_ref.exact(A, A.copy(), 1.0)
        assert abs(aff - 1) < eps and dist < mpmath.mpf(10) ** -20  # arccos is steep at 1
        assert pf_ref.exact(E, E, 1.0) == (1, 0) and pf_ref.restatement(E, E, 1.0) == 0.0 and pf_ref.sums(E, E, 1.0) == (0.0, 0.0, 0.0)
        # non-finite rows do not count
        withinf = np.concatenate([A[:3], [[0.0, np.inf], [np.nan, 1.0]], A[3:]])
        B_ = diagram(5, 2)
        assert pf_ref.exact(withinf, B_, 1.0) == pf_ref.exact(A, B_, 1.0) and pf_ref.sums(withinf, B_, 1.0) == pf_ref.sums(A, B_, 1.0)


@pytest.mark.parametrize("sigma", SIGMAS)
def test_restatement_within_the_bound_exactly_symmetric_and_zero_on_equal(sigma):
    worst = 0.0
    cases = [(1, 0), (1, 1), (2, 1), (3, 3), (5, 8), (8, 8), (8, 0), (7, 4)]
    for n1, n2 in cases:
        F, G = diagram(n1, 100 + n1), diagram(n2, 200 + n2)
        a, b, h = pf_ref.sums(F, G, sigma)
        a2, b2, h2 = pf_ref.sums(G, F, sigma)
        assert (a, b, h) == (b2, a2, h2)  # bit for bit
        got, d = pf_ref.affinity_of(a, b, h), pf_ref.restatement(F, G, sigma)
        assert d == pf_ref.restatement(G, F, sigma) and 0.0 <= d <= np.arccos(0.0)
        B = pf_ref.bound(n1, n2)
        with mpmath.workdps(50):
            aff, dist = pf_ref.exact(F, G, sigma)
            err, derr = float(abs(mpmath.mpf(got) - aff)), float(abs(mpmath.mpf(d) - dist))
        worst = max(worst, err / B)
        assert err <= B, (n1, n2, sigma, err, B)
        assert derr <= pf_ref.bound_dist(got, B), (n1, n2, sigma, derr)
        for X in (F, G):
            a, b, h = pf_ref.sums(X, X.copy(), sigma)
            assert a == b == h and pf_ref.restatement(X, X.copy(), sigma) == 0.0 and not np.signbit(pf_ref.restatement(X, X, sigma))
        # another row order: within the bound (promise 4)
        perm = np.random.default_rng(n1 + n2).permutation(n1)
        assert abs(pf_ref.affinity_of(*pf_ref.sums(F[perm], G, sigma)) - got) <= B
    print(f"sigma={sigma}: restatement against mpmath, largest share of the bound: {worst:.3e}")


def test_orientation_of_the_restatement_is_the_plans():
    A, B = diagram(9, 1), diagram(9, 2)
    first = A if A.ravel().tolist() < B.ravel().tolist() else B
    assert pf_ref.orient(A, B)[0] is not None and np.array_equal(pf_ref.orient(A, B)[0], first) and np.array_equal(pf_ref.orient(B, A)[0], first)
    assert pf_ref.orient(diagram(3, 1), diagram(4, 2))[2] and not pf_ref.orient(diagram(4, 2), diagram(3, 1))[2]
    neg, pos = np.array([[-0.0, 1.0]]), np.array([[0.0, 1.0]])
    assert pf_ref.orient(pos, neg)[2] and not pf_ref.orient(neg, pos)[2]  # -0 below +0


# ---------------------------------------------------------------- the sanitized plan program
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pf_plan") / "pf_plan")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "pf_plan_main.cpp")], check=True)
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


def pf_case(exe, dgms, pairs=None, P=None, sigma=1.0, reserved=0, offsets=None, points=True, S=None):
    off = np.concatenate([[0], np.cumsum([len(d) for d in dgms])]).astype(int) if offsets is None else offsets
    pts = np.concatenate([np.asarray(d, np.float64).reshape(-1, 2) for d in dgms]) if dgms else E
    head = [len(off) - 1 if not isinstance(off, str) else len(dgms), *(["null"] if isinstance(off, str) else off)]
    head = head if S is None else [S]  # S < 0: the program reads no offsets
    head += [len(pts), *[repr(float(x)) for x in pts.ravel()]] if points else [-1]
    if isinstance(pairs, int):  # that many times the pair (0, 1), as one string: the lists of millions of pairs
        npairs, pr = pairs, [pairs, "0 1 " * pairs]
    else:
        npairs = 0 if pairs is None else len(pairs)
        pr = [-1] if pairs is None else [npairs, *np.asarray(pairs, int).reshape(-1).tolist()]
    return run_plan(exe, ["pf", *head, *pr, npairs if P is None else P, repr(float(sigma)), reserved])


def test_plan_work_list_orientation_and_parts(plan_exe):
    sizes = [65, 0, 64, 300, 513, 1024, 1]
    dgms = [diagram(n, n) for n in sizes]
    pairs = [(0, 2), (2, 0), (1, 3), (3, 4), (4, 3), (5, 6), (6, 5), (5, 5), (1, 1), (2, 2), (1, 6)]
    rc, p = pf_case(plan_exe, dgms, pairs, sigma=0.05)
    assert rc == 0 and p["P"] == [11] and p["c"] == [pf_ref.c2_of(0.05)]
    assert np.array(p["pts"]).tobytes() == np.concatenate(dgms).ravel().tobytes()
    got = np.array(p["pairs"]).reshape(-1, 2)
    # the longer diagram first: (i, j) and (j, i) are the same evaluation; no selfs are added
    assert got.tolist() == [[0, 2], [0, 2], [3, 1], [4, 3], [4, 3], [5, 6], [5, 6], [5, 5], [1, 1], [2, 2], [6, 1]]
    assert p["swapped"] == [0, 1, 1, 1, 0, 0, 1, 0, 0, 0, 1]
    n = np.array(sizes)
    M = np.array([n[i] + n[j] for i, j in got])
    parts = [int(-(-2 * m // 64)) for m in M]
    assert p["part_off"] == np.concatenate([[0], np.cumsum(parts)]).tolist()
    assert parts[0] == 5 and parts[2] == 10 and parts[7] == 64 and parts[8] == 0 and parts[9] == 4 and parts[10] == 1
    cls = np.where(M <= 64, 0, np.where(M <= 512, 1, 2))
    assert p["order"] == [int(w) for c in range(3) for w in np.flatnonzero(cls == c)]
    assert p["cnt"] == [int((cls == c).sum()) for c in range(3)]
    assert p["cls_parts"] == [max(np.array(parts)[cls == c]) for c in range(3)] == [1, 10, 64]
    # equal counts: the lexicographically smaller point array first, whichever way the pair is named
    A, B = diagram(9, 1), diagram(9, 2)
    first = 0 if A.ravel().tolist() < B.ravel().tolist() else 1
    rc, p = pf_case(plan_exe, [A, B], [(0, 1), (1, 0)])
    assert np.array(p["pairs"]).reshape(-1, 2).tolist() == [[first, 1 - first]] * 2 and sorted(p["swapped"]) == [0, 1]
    rc, p = pf_case(plan_exe, [A, A.copy()], [(0, 1), (1, 0)])  # equal arrays: as named, and it does not matter
    assert rc == 0 and np.array(p["pairs"]).reshape(-1, 2).tolist() == [[0, 1], [1, 0]] and p["swapped"] == [0, 0]
    # pairs == NULL: every i < j, row-major
    rc, p = pf_case(plan_exe, [diagram(3, 1), diagram(4, 2), diagram(5, 3)])
    assert rc == 0 and p["P"] == [3] and np.array(p["pairs"]).reshape(-1, 2).tolist() == [[1, 0], [2, 0], [2, 1]]
    rc, p = pf_case(plan_exe, [])
    assert rc == 0 and p["P"] == [0] and p["pairs"] == [] and p["part_off"] == [0] and p["off"] == [0]
    rc, p = pf_case(plan_exe, [E, E])  # two empty diagrams: a pair without parts
    assert rc == 0 and p["pairs"] == [0, 1] and p["part_off"] == [0, 0] and p["cls_parts"] == [0, 0, 0]
    # non-finite rows are dropped before anything is counted
    junk = np.array([[np.nan, 1.0], [0.5, 1.5], [0.0, np.inf], [-0.0, 2.0]])
    rc, p = pf_case(plan_exe, [junk, E])
    assert rc == 0 and p["off"] == [0, 2, 2] and np.array(p["pts"]).tobytes() == junk[[1, 3]].ravel().tobytes() and p["part_off"] == [0, 1]


def test_plan_errors_in_the_header_order(plan_exe):
    D = [diagram(5, 1), diagram(70, 2)]
    assert pf_case(plan_exe, D, [(0, 1)])[0] == 0
    assert run_plan(plan_exe, ["null"]) == (-1, "args is NULL")
    # each case carries the faults of all later checks too: the earlier check answers
    late = dict(offsets=[0, 50, 5], pairs=[(0, 9)])
    assert pf_case(plan_exe, D, S=-1, reserved=1, sigma=0.0, **late) == (-1, "S must be >= 0")
    assert pf_case(plan_exe, D, offsets="null", reserved=1, sigma=0.0, pairs=[(0, 9)]) == (-1, "offsets is NULL")
    assert pf_case(plan_exe, D, reserved=1, sigma=0.0, **late) == (-1, "reserved must be 0")
    for s in (0.0, -1.0, -0.0, np.nan, np.inf, -np.inf):
        assert pf_case(plan_exe, D, sigma=s, **late) == (-1, "sigma must be finite and > 0"), s
    for s in (1e-200, 5e-324, 1e154, 1e160, 1.7e308):  # sigma^2 under- or overflows, or c2 is subnormal
        rc, msg = pf_case(plan_exe, D, sigma=s, **late)
        assert rc == -1 and "normal" in msg, s
    for s in (1e-150, 1e150, 1e-6):
        assert pf_case(plan_exe, D, [(0, 1)], sigma=s)[0] == 0
    assert pf_case(plan_exe, D, offsets=[1, 5, 75], pairs=[(0, 9)])[0] == -1
    rc, msg = pf_case(plan_exe, D, **late)
    assert rc == -1 and "non-decreasing" in msg
    assert pf_case(plan_exe, D, points=False, pairs=[(0, 9)]) == (-1, "points is NULL")
    assert pf_case(plan_exe, D, pairs=[(0, 9)], P=-1) == (-1, "P must be >= 0")
    rc, msg = pf_case(plan_exe, D, pairs=[(0, 1)], P=(1 << 27) + 1)  # refused before the pairs are read
    assert rc == -2 and "2^27" in msg
    big = [diagram(5, 1), diagram(1025, 3), diagram(6, 4)]
    for bad in ([(0, 3)], [(-1, 0)], [(0, 1), (3, 3)]):
        rc, msg = pf_case(plan_exe, big, bad)
        assert rc == -1 and "outside" in msg  # before the size limit
    # the 1024 / 1025 limit, on finite rows, and only where a pair names the diagram
    for named in ([(0, 1)], [(1, 0)], [(1, 1)], [(0, 2), (2, 1)]):
        rc, msg = pf_case(plan_exe, big, named)
        assert rc == -2 and "1024" in msg, named
    rc, msg = pf_case(plan_exe, big)  # every i < j names it
    assert rc == -2 and "1024" in msg
    rc, p = pf_case(plan_exe, big, [(0, 2), (2, 0), (0, 0)])
    assert rc == 0 and p["P"] == [3] and p["off"] == [0, 5, 1030, 1036]
    wide = np.concatenate([diagram(1024, 4), [[0.0, np.inf]] * 3])
    rc, p = pf_case(plan_exe, [wide, diagram(1, 5), diagram(1024, 6)])
    assert rc == 0 and p["part_off"] == [0, 33, 33 + 64, 33 + 64 + 33] and p["cnt"] == [0, 0, 3]
    # the scratch limit, the header's last case: 2^27 parts pass, more do not.  Two diagrams of 1024 points: 64 parts a pair
    two = [diagram(1024, 6), diagram(1024, 7)]
    rc, p = pf_case(plan_exe, two, 1 << 21)
    assert rc == 0 and p["P"] == [1 << 21] and p["part_off"][-1] == 1 << 27 and p["cnt"] == [0, 0, 1 << 21]
    rc, msg = pf_case(plan_exe, two, (1 << 21) + 1)
    assert rc == -2 and "2^27 parts" in msg


# ---------------------------------------------------------------- the ABI
def test_pf_structs_match_header_layout(pkg, tmp_path):
    lb = pkg._lib
    src = tmp_path / "pflayout.c"
    names = {"tda_pf_args": ["offsets", "S", "pairs", "P", "sigma", "device", "reserved"],
             "tda_pf_result": ["a", "b", "h", "dist", "device_ms"]}
    body = "".join(f'printf("%zu ", sizeof({t}));' + "".join(f'printf("%zu ", offsetof({t}, {f}));' for f in fs) for t, fs in names.items())
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tda_dgm.h"\nint main(void){' + body +
                   'printf("%d %d %d %d %d\\n", TDA_PF_MAX_POINTS, TDA_PF_EXP_ULP, TDA_PF_CUT, TDA_PF_LANES, TDA_PF_CHUNK); return 0;}\n')
    exe = tmp_path / "pflayout"
    subprocess.run(["gcc", "-I", lb.INCLUDE, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for t, fs in zip((lb.PfArgs, lb.PfResult), names.values()):
        want += [ctypes.sizeof(t)] + [getattr(t, f).offset for f in fs]
        assert [f[0] for f in t._fields_[1:]] == fs  # every field after the first is compared
    want += [lb.TDA_PF_MAX_POINTS, lb.TDA_PF_EXP_ULP, lb.TDA_PF_CUT, lb.TDA_PF_LANES, lb.TDA_PF_CHUNK]
    assert got == want and want[-5:] == [pf_ref.MAX_POINTS, pf_ref.EXP_ULP, pf_ref.CUT, pf_ref.LANES, pf_ref.CHUNK]
    assert [f[0] for f in lb.PfArgs._fields_] == [f[0] for f in lb.HkArgs._fields_]  # as tda_hk_args


def test_pf_symbols_exported_and_abi_version_unchanged(pkg, built_lib):
    lib = ctypes.CDLL(built_lib)
    assert pkg.FISHER_EXPORTS == ("tda_persistence_fisher", "tda_persistence_fisher_free")
    assert all(hasattr(lib, s) for s in pkg.FISHER_EXPORTS)
    others = (set(pkg.EXPORTS) | set(pkg.DGM_EXPORTS) | set(pkg.BOTTLENECK_EXPORTS) | set(pkg.WASSERSTEIN_EXPORTS) | set(pkg.VECTOR_EXPORTS)
              | set(pkg.HEAT_EXPORTS) | set(pkg.CURVE_EXPORTS))
    assert not set(pkg.FISHER_EXPORTS) & others and all(hasattr(lib, s) for s in others)
    assert pkg.lib().tda_version() == 8  # symbols added only: no existing struct changed


def test_pf_invalid_arguments_rejected_before_device(pkg, built_lib):
    L, lb = pkg.lib(), pkg._lib
    pts = np.tile(np.array([[0.0, 1.0]]), (1100, 1))
    off = np.array([0, 5, 1029], np.int64)  # 5 and 1024 points
    pairs = np.array([[0, 1], [1, 0], [1, 1]], np.int32)
    res = ctypes.POINTER(lb.PfResult)()

    def pf(**kw):
        a = lb.PfArgs()
        a.points, a.offsets, a.S, a.pairs, a.P, a.sigma = pts.ctypes.data, off.ctypes.data, 2, pairs.ctypes.data, 3, 1.0
        a.device = 12345  # never a device: a valid call ends at the device check
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.tda_persistence_fisher(ctypes.byref(a), ctypes.byref(res))
        assert not res  # no result on failure
        return rc

    def invalid(**kw):
        rc = pf(**kw)
        assert rc in (-1, -2) and L.tda_last_error(), kw
        return rc

    assert pf() == -5 and pf(pairs=None) == -5 and pf(S=0, P=0) == -5 and pf(sigma=1e-6) == -5
    assert invalid(reserved=1) == -1 and b"reserved" in L.tda_last_error()
    assert invalid(reserved=2, device=0) == -1  # before the device check even with the right ordinal
    for s in (0.0, -0.4, float("nan"), float("inf"), 1e-200, 1e160, 1.7e308):
        assert invalid(sigma=s) == -1 and b"sigma" in L.tda_last_error(), s
    assert invalid(offsets=None) == -1 and invalid(points=None) == -1 and invalid(S=-1) == -1 and invalid(P=-1) == -1
    bad = np.array([0, 50, 5], np.int64)
    assert invalid(offsets=bad.ctypes.data) == -1 and b"non-decreasing" in L.tda_last_error()
    bad = np.array([1, 5, 6], np.int64)
    assert invalid(offsets=bad.ctypes.data) == -1
    for p in ([[0, 2]], [[-1, 0]]):
        p = np.array(p, np.int32)
        assert invalid(pairs=p.ctypes.data, P=1) == -1 and b"outside" in L.tda_last_error()
    big = np.array([0, 1025, 1100], np.int64)
    assert invalid(offsets=big.ctypes.data) == -2 and b"1024" in L.tda_last_error()  # 1025 finite points, named
    assert invalid(offsets=big.ctypes.data, pairs=None) == -2
    p = np.array([[1, 1]], np.int32)
    assert pf(offsets=big.ctypes.data, pairs=p.ctypes.data, P=1) == -5  # no pair names it: accepted
    pinf = pts.copy()  # 1024 finite points and non-finite rows in one diagram: those do not count
    pinf[[0, 100, 1000], 1] = np.inf
    pinf[7, 0] = np.nan
    wide = np.array([0, 1028, 1100], np.int64)
    assert pf(points=pinf.ctypes.data, offsets=wide.ctypes.data) == -5 and invalid(offsets=wide.ctypes.data) == -2
    assert invalid(P=(1 << 27) + 1) == -2 and b"2^27" in L.tda_last_error()
    assert L.tda_persistence_fisher(None, ctypes.byref(res)) == -1 and L.tda_persistence_fisher(ctypes.byref(lb.PfArgs()), None) == -1
    L.tda_persistence_fisher_free(None)  # a no-op


# ---------------------------------------------------------------- the Python entries
def importlib_module(pkg, name):
    return __import__("importlib").import_module(pkg.__name__ + "." + name)


def test_python_entries_refuse_bad_arguments_before_the_library(pkg, monkeypatch):
    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(pkg._lib, "lib", no_library)
    A = np.array([[0.0, 1.0], [0.5, 2.0]])
    for s in (0, 0.0, -0.4, np.nan, np.inf, -np.inf, 1e-200, 1e160, 1.7e308):
        for call in (lambda: pkg.fisher(A, A, s), lambda: pkg.fisher(A, A, sigma=s), lambda: pkg.fisher_matrix([A, A], s),
                     lambda: pkg.fisher_kernel_matrix([A], sigma=s), lambda: pkg.fisher_matrix([], s), lambda: pkg.fisher_matrix([A], s, other=[])):
            with pytest.raises(ValueError, match="sigma"):
                call()
    for bw in (0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="bandwidth"):
            pkg.fisher_kernel_matrix([A, A], bandwidth=bw)
    for bad in (np.zeros((3, 3)), np.zeros(3), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            pkg.fisher(A, bad)
        with pytest.raises(ValueError):
            pkg.fisher_matrix([A, bad])
        with pytest.raises(ValueError):
            pkg.fisher_kernel_matrix([A], other=[bad])
    big = np.tile(A, (513, 1))[:1025]
    for call in (lambda: pkg.fisher(A, big), lambda: pkg.fisher_matrix([A, big]), lambda: pkg.fisher_kernel_matrix([A], other=[A, big])):
        with pytest.raises(NotImplementedError, match="1024"):
            call()
    # nothing to compute: no library call, no device needed -- and a large diagram that no pair names is accepted
    assert pkg.fisher_matrix([]).shape == (0, 0) and pkg.fisher_kernel_matrix([]).shape == (0, 0)
    assert pkg.fisher_matrix([A]).tolist() == [[0.0]] and pkg.fisher_matrix([big]).tolist() == [[0.0]]
    assert pkg.fisher_kernel_matrix([A]).tolist() == [[1.0]]
    assert pkg.fisher_matrix([A], other=[]).shape == (1, 0) and pkg.fisher_matrix([], other=[A]).shape == (0, 1)
    assert pkg.fisher_kernel_matrix([A], other=[]).shape == (1, 0) and pkg.fisher_kernel_matrix([], other=[A, A]).shape == (0, 2)
    for out in (pkg.fisher_matrix([A], return_time=True), pkg.fisher_matrix([], 0.4, [A], return_time=True),
                pkg.fisher_kernel_matrix([], return_time=True)):
        assert isinstance(out, tuple) and out[0].dtype == np.float64 and out[1] == 0.0
    assert {"fisher", "fisher_matrix", "fisher_kernel_matrix", "layer_distance_matrix"} <= set(pkg.__all__)


def test_what_reaches_the_library_and_how_the_matrices_are_filled(pkg, monkeypatch):
    dg = importlib_module(pkg, "diagrams")
    seen = {}

    def fake(points, offsets, pairs, sigma, device):
        seen.update(points=points.copy(), offsets=offsets.copy(), pairs=None if pairs is None else pairs.copy(), sigma=sigma, device=device)
        S = len(offsets) - 1
        P = S * (S - 1) // 2 if pairs is None else len(pairs)
        return 300.0 + np.arange(P), 200.0 + np.arange(P), 100.0 + np.arange(P), 0.25 * (1.0 + np.arange(P)), 0.75

    monkeypatch.setattr(dg, "_call_pf", fake)
    A, B, C = np.array([[0.5, 1.0], [0.25, np.inf]]), np.array([[0.375, 0.5]]), E
    with pytest.warns(UserWarning, match="non-finite"):
        D, ms = pkg.fisher_matrix([A, B, C], 0.25, device=2, return_time=True)
    assert ms == 0.75 and seen["pairs"] is None and (seen["sigma"], seen["device"]) == (0.25, 2) and seen["offsets"].tolist() == [0, 2, 3, 3]
    assert D.tolist() == [[0.0, 0.25, 0.5], [0.25, 0.0, 0.75], [0.5, 0.75, 0.0]]
    K = pkg.fisher_kernel_matrix([B, B, C], bandwidth=0.5)
    assert seen["sigma"] == 1.0 and np.array_equal(K, np.exp(-np.array([[0.0, 0.25, 0.5], [0.25, 0.0, 0.75], [0.5, 0.75, 0.0]]) / 0.5))
    assert np.array_equal(np.diag(K), np.ones(3))
    D = pkg.fisher_matrix([B, C], other=[B, B, C])
    assert D.tolist() == [[0.25, 0.5, 0.75], [1.0, 1.25, 1.5]] and seen["pairs"].tolist() == [[0, 2], [0, 3], [0, 4], [1, 2], [1, 3], [1, 4]]
    assert seen["pairs"].dtype == np.int32 and seen["offsets"].tolist() == [0, 1, 1, 2, 3, 3]
    K, ms = pkg.fisher_kernel_matrix([B, C], 2.0, 4.0, other=[B], return_time=True)
    assert ms == 0.75 and seen["sigma"] == 2.0 and K.tolist() == np.exp(-np.array([[0.25], [0.5]]) / 4.0).tolist()
    assert pkg.fisher(B, C, 2, device=1) == 0.25 and (seen["sigma"], seen["device"]) == (2.0, 1)


def _layer_results(pkg):
    rp = importlib_module(pkg, "ripser")  # pkg.ripser is the function
    b = rp._Batch()
    b.L, b.nd = 2, 2
    b.cnt = np.array([[1, 1], [0, 2]], np.int64)
    b.off = np.array([[0, 1], [2, 2]], np.int64)
    b.pairs = np.array([[0.0, 1.0], [0.5, 0.75], [0.25, 0.5], [1.0, 3.0]])
    return [rp.LayerResult((b, 0)), rp.LayerResult((b, 1))]


def test_layer_results_go_through_the_matrix_entries_only(pkg, monkeypatch):
    dg = importlib_module(pkg, "diagrams")
    seen = {}

    def fake(points, offsets, pairs, sigma, device):
        seen.update(points=points.copy(), offsets=offsets.copy())
        return np.zeros(1), np.zeros(1), np.zeros(1), np.full(1, 0.5), 0.0

    monkeypatch.setattr(dg, "_call_pf", fake)
    rs = _layer_results(pkg)
    assert pkg.fisher_matrix(rs).tolist() == [[0.0, 0.5], [0.5, 0.0]]  # dim = 1
    assert seen["offsets"].tolist() == [0, 1, 3] and seen["points"].tolist() == [[0.5, 0.75], [0.25, 0.5], [1.0, 3.0]]
    pkg.fisher_kernel_matrix(rs, dim=0)
    assert seen["offsets"].tolist() == [0, 1, 1] and seen["points"].tolist() == [[0.0, 1.0]]
    with pytest.raises(ValueError, match="fisher_matrix"):
        pkg.fisher(rs[0], E)
    with pytest.raises(ValueError, match="fisher_matrix"):
        pkg.fisher(E, rs[0])
    with pytest.raises(ValueError):
        pkg.fisher_matrix([rs[0], np.zeros((1, 2))])
    with pytest.raises(ValueError, match="dim"):
        pkg.fisher_kernel_matrix(rs, dim=2)


def test_layer_distance_matrix_and_permutation_test_route_fisher(pkg, monkeypatch):
    """metric="fisher" goes to fisher_matrix with sigma, dim and device and without M, in both; the
    other metrics get exactly the keywords they got, and an unknown name is still a ValueError that
    begins as before and names the new metric too."""
    pl, hy = importlib_module(pkg, "pipeline"), pkg.hypothesis
    calls = []
    monkeypatch.setattr(pl, "fisher_matrix", lambda results, **kw: calls.append(("pf", results, kw)) or "PF")
    monkeypatch.setattr(pl, "heat_matrix", lambda results, **kw: calls.append(("hk", results, kw)) or "HK")
    monkeypatch.setattr(pl, "sliced_wasserstein_matrix", lambda results, **kw: calls.append(("sw", results, kw)) or "SW")
    r = [E] * 2
    assert pkg.layer_distance_matrix(r, dim=0, M=0, device=3, metric="fisher", sigma=2.5) == "PF"  # M is not even checked
    assert pkg.layer_distance_matrix(r, metric="fisher") == "PF"
    assert pkg.layer_distance_matrix(r, metric="heat", sigma=2.5) == "HK" and pkg.layer_distance_matrix(r, sigma=9.0) == "SW"
    assert calls == [("pf", r, {"sigma": 2.5, "device": 3, "dim": 0}), ("pf", r, {"sigma": 0.4, "device": 0, "dim": 1}),
                     ("hk", r, {"sigma": 2.5, "device": 0, "dim": 1}), ("sw", r, {"M": 50, "device": 0, "dim": 1})]
    for bad in ("Fisher", "persistence_fisher", ""):
        with pytest.raises(ValueError, match="metric must be 'sliced_wasserstein', 'bottleneck', 'wasserstein' or 'heat'.*'fisher'"):
            pkg.layer_distance_matrix(r, metric=bad)
    assert len(calls) == 4
    # the permutation test
    assert hy.METRICS[-1] == "fisher" and hy.METRICS[:4] == ("sliced_wasserstein", "bottleneck", "wasserstein", "heat")
    D = np.zeros((6, 6))
    got, seen = [], []
    monkeypatch.setattr(hy.diagrams, "fisher_matrix", lambda dgms, **kw: got.append((dgms, kw)) or D)
    monkeypatch.setattr(hy, "permutation_test", lambda D_, labels, **kw: seen.append((D_, labels, kw)) or "result")
    dgs, labels = [object()] * 6, list("aaabbb")
    assert hy.diagram_permutation_test(dgs, labels, metric="fisher", sigma=0.7, dim=0, device=2, B=99) == "result"
    assert got == [(dgs, dict(sigma=0.7, device=2, dim=0))] and seen[0][0] is D and seen[0][1] is labels and seen[0][2] == dict(device=2, B=99)
    with pytest.raises(ValueError, match="fisher"):
        hy.diagram_permutation_test(dgs, labels, metric="Fisher")
    assert len(got) == 1 and len(seen) == 1
