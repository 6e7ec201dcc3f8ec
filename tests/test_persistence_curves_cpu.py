"""CPU tests of the persistence curves' boundary (no device): the reference tests/pc_ref.py
against independent definitions, the plan of csrc/dgm_plan.h (pc_plan, a sanitized host program
of its own), the new symbols and the ctypes mirror of include/tda_dgm.h, the argument errors
raised before any device work, and the Python entries' argument handling."""
import ctypes
import os
import subprocess
import warnings

import numpy as np
import pytest

import pc_ref
import pl_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tda-multimodal_amd", "csrc")
E = np.zeros((0, 2))
INDICATOR, TENT, NORMALIZE, ESSENTIAL = 0, 1, 1, 2


def bars(n, seed=0):
    rng = np.random.default_rng(seed)
    b = rng.uniform(0.0, 5.0, n)
    return np.stack([b, b + rng.uniform(1e-3, 5.0, n)], 1)


# ---------------------------------------------------------------- the reference
def test_betti_curve_is_a_difference_of_two_counts():
    D = bars(200, 3)
    D[::7] = D[1::7][:len(D[::7])]  # repeated bars
    grid = np.concatenate([np.linspace(-1.0, 11.0, 57), D[:20, 0], D[:20, 1], [-0.0]])
    want = np.searchsorted(np.sort(D[:, 0]), grid, "right") - np.searchsorted(np.sort(D[:, 1]), grid, "right")
    got = pc_ref.curve(D, grid)
    assert np.array_equal(got, want) and got.dtype == np.float64 and not np.signbit(got).any()
    assert got[57:77].min() >= 1  # closed at the birth
    one = pc_ref.curve(np.array([[1.0, 2.0]]), np.array([1.0, 1.5, 2.0]))
    assert one.tolist() == [1.0, 1.0, 0.0]  # and open at the death


def test_one_point_silhouette_is_the_landscape():
    grid = np.linspace(-1.0, 6.0, 71)
    for D in (np.array([[0.5, 4.25]]), np.array([[1.0, 1.0 + 2.0 ** -20]])):
        lam = pl_ref.landscape(D, grid, 1)[0]
        assert np.array_equal(pc_ref.curve(D, grid, kernel="tent"), lam)
        assert np.array_equal(pc_ref.silhouette(D, grid, 0.0), lam)  # the weight 1 divides out
    D = np.array([[0.0, 4.0], [1.0, 3.0]])  # weights 4 and 2: (4 f1 + 2 f2) / 6
    s = pc_ref.silhouette(D, np.array([2.0, 0.5, 5.0]))
    assert s.tolist() == [(4.0 * 2.0 + 2.0 * 1.0) / 6.0, (4.0 * 0.5) / 6.0, 0.0]


def test_lifespan_of_equal_lifetimes_is_lifetime_times_betti():
    b = np.random.default_rng(5).uniform(0.0, 4.0, 40)
    D = np.stack([b, b + 0.75], 1)
    D = D[D[:, 1] - D[:, 0] == 0.75]  # the bars whose float64 lifetime is 0.75 exactly
    assert len(D) > 10
    grid = np.linspace(-0.5, 5.5, 61)
    assert np.array_equal(pc_ref.lifespan(D, grid), 0.75 * pc_ref.betti(D, grid))


def test_essential_bars_count_only_when_asked_and_other_rows_never():
    D = np.array([[0.5, np.inf], [1.0, 2.0], [np.nan, 3.0], [-np.inf, 1.5], [0.25, -np.inf], [0.0, np.inf], [np.inf, np.inf]])
    grid = np.array([-1.0, 0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 1e300])
    assert pc_ref.curve(D, grid, essential=True).tolist() == [0.0, 1.0, 1.0, 2.0, 3.0, 3.0, 2.0, 2.0]
    assert pc_ref.curve(D, grid).tolist() == [0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0]
    c = np.arange(1.0, 8.0)  # a dropped row drops its coefficient: only 1, 2 and 6 are read
    assert pc_ref.curve(D, grid, c, essential=True).tolist() == [0.0, 6.0, 6.0, 7.0, 9.0, 9.0, 7.0, 7.0]
    assert pc_ref.curve(D, grid, c, essential=True, normalize=True).tolist() == (np.array([0.0, 6.0, 6.0, 7.0, 9.0, 9.0, 7.0, 7.0]) / 9.0).tolist()
    c[2] = np.nan  # on a dropped row: not read
    assert pc_ref.curve(D, grid, c).tolist() == [0.0, 0.0, 0.0, 0.0, 2.0, 2.0, 0.0, 0.0]


def test_reference_zeros_are_positive_and_the_sum_runs_in_row_order():
    grid = np.array([-0.0, 0.5, 1.0])
    D = np.array([[0.0, 1.0], [0.0, 1.0]])
    for kw in (dict(coef=[1.0, -1.0]), dict(coef=[-1.0, -1.0], normalize=True), dict(coef=[1.0, -1.0], normalize=True),
               dict(coef=[-0.0, -0.0]), dict(coef=[-1e-300, 1e-300], kernel="tent"), dict(coef=[-3.0, 1.0], normalize=True, kernel="tent")):
        v = pc_ref.curve(D, grid, **kw)
        assert not np.signbit(v).any(), kw
    assert not pc_ref.curve(E, grid, normalize=True).any() and not pc_ref.curve(E, grid, [], kernel="tent").any()
    # 2^53 + 1 + 1 - 2^53: the order is visible
    big = 2.0 ** 53
    D = np.tile([[0.0, 1.0]], (4, 1))
    assert pc_ref.curve(D, [0.5], [big, 1.0, 1.0, -big])[0] == 0.0 and pc_ref.curve(D, [0.5], [1.0, 1.0, big, -big])[0] == 2.0
    assert pc_ref.curves([], grid).shape == (0, 3) and pc_ref.curves([D, E], grid).shape == (2, 3)
    ent = pc_ref.entropy_coef(np.array([[0.0, 1.0], [0.0, 1.0], [0.0, np.inf], [0.0, 2.0]]))
    assert np.array_equal(ent, -np.array([0.25, 0.25, 0.5]) * np.log(np.array([0.25, 0.25, 0.5])))
    assert np.array_equal(pc_ref.silhouette_coef(np.array([[1.0, 3.0], [0.0, 0.5]]), 2.0), [4.0, 0.25])


# ---------------------------------------------------------------- the sanitized plan program
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pc_plan") / "pc_plan")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "pc_plan_main.cpp")], check=True)
    return exe


def fmt(xs):
    return [repr(float(x)) for x in xs]


def arr(xs):
    return ["-1"] if xs is None else [str(len(xs)), *fmt(xs)]


def run_plan(exe, words):
    r = subprocess.run([exe], input=" ".join(map(str, words)) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]  # a sanitizer report ends the program with a non-zero status
    if r.stdout.startswith("err"):
        _, code, msg = r.stdout.strip().split(" ", 2)
        return int(code), msg
    out = {}
    for line in r.stdout.splitlines():
        k, *v = line.split()
        out[k] = [float.fromhex(x) for x in v] if k in ("pts", "wgt", "W") else [int(x) for x in v]
    return 0, out


def pc_case(exe, dgms, grid=(0.0, 1.0), G=None, kernel=INDICATOR, flags=0, reserved=0, coef=None, offsets=None, points=True):
    off = np.concatenate([[0], np.cumsum([len(d) for d in dgms])]).astype(int) if offsets is None else offsets
    pts = np.concatenate([np.asarray(d, np.float64).reshape(-1, 2) for d in dgms]) if dgms else E
    head = [len(off) - 1 if not isinstance(off, str) else len(dgms), *(["null"] if isinstance(off, str) else off)]
    head += [len(pts), *fmt(pts.ravel())] if points else [-1]
    G = (len(grid) if grid is not None else 2) if G is None else G
    return run_plan(exe, ["pc", *head, G, kernel, flags, reserved, *arr(grid), *arr(coef)])


JUNK = np.array([[np.nan, 1.0], [0.5, 1.5], [0.0, np.inf], [-0.0, 2.0], [-np.inf, 0.0], [3.0, 1.0], [1.0, -np.inf], [np.inf, np.inf]])


def test_plan_keeps_rows_coefficients_and_divisors(plan_exe):
    sizes = [65, 0, 64, 256, 257, 1024, 1025, 4096, 1, 63]
    dgms = [bars(n, n) for n in sizes] + [JUNK]
    total = sum(sizes) + len(JUNK)
    coef = np.random.default_rng(2).uniform(-1.0, 2.0, total)
    for flags in (0, NORMALIZE, ESSENTIAL, ESSENTIAL | NORMALIZE):
        ess = bool(flags & ESSENTIAL)
        keep = [pc_ref.kept_rows(d, ess) for d in dgms]
        kept = [d[k] for d, k in zip(dgms, keep)]
        assert len(kept[-1]) == (4 if ess else 3)
        for c in (None, coef):
            rc, p = pc_case(plan_exe, dgms, flags=flags, coef=c)
            assert rc == 0
            assert p["off"] == np.concatenate([[0], np.cumsum([len(f) for f in kept])]).tolist()
            assert np.array(p["pts"]).tobytes() == np.concatenate(kept).ravel().tobytes()  # rows in order, bit for bit (-0 and +inf kept)
            # class 0: n <= 64 (the packed launch), 1: <= 256, 2: <= 1024, 3: <= 4096 (the chunked launch); ascending ids
            assert p["order"] == [1, 2, 8, 9, 10, 0, 3, 4, 5, 6, 7]
            assert p["cnt"] == [5, 2, 2, 2] and p["cls_n"] == [64, 256, 1024, 4096]
            if c is None:
                assert p["wgt"] == [] and p["W"] == [float(len(f)) for f in kept]
            else:
                cs = np.split(c, np.cumsum([len(d) for d in dgms])[:-1])
                ck = [x[k] for x, k in zip(cs, keep)]
                assert np.array(p["wgt"]).tobytes() == np.concatenate(ck).tobytes()  # a coefficient follows its row
                want = []
                for x in ck:
                    w = np.float64(0.0)
                    for v in x:
                        w = w + v  # row order
                    want.append(float(w))
                assert np.array(p["W"]).tobytes() == np.array(want).tobytes()
    rc, p = pc_case(plan_exe, [E, JUNK[[0, 4, 6, 7]], bars(3)], coef=np.ones(7), flags=ESSENTIAL)  # empty, all rows dropped
    assert rc == 0 and p["off"] == [0, 0, 0, 3] and p["cnt"] == [3, 0, 0, 0] and p["cls_n"] == [3, 0, 0, 0] and p["W"] == [0.0, 0.0, 3.0]
    assert not np.signbit(p["W"]).any()
    rc, p = pc_case(plan_exe, [])
    assert rc == 0 and p["off"] == [0] and p["order"] == [] and p["pts"] == [] and p["W"] == []
    rc, p = pc_case(plan_exe, [bars(2)], coef=[1.5, -1.5], flags=NORMALIZE)
    assert rc == 0 and p["W"] == [0.0]
    # 4096 kept rows among dropped ones pass, 4097 do not; an essential row counts only when it is kept
    wide = np.concatenate([bars(4096, 1), [[0.0, np.inf]] * 3])
    assert pc_case(plan_exe, [wide])[0] == 0 and pc_case(plan_exe, [wide], kernel=TENT)[0] == 0
    rc, msg = pc_case(plan_exe, [E, wide], flags=ESSENTIAL)
    assert rc == -2 and "4096" in msg
    rc, msg = pc_case(plan_exe, [E, bars(4097, 2)], kernel=TENT)
    assert rc == -2 and "4096" in msg


def test_plan_argument_errors_in_the_headers_order(plan_exe):
    D = [bars(5), bars(70, 1)]
    ok = np.ones(75)
    assert pc_case(plan_exe, D)[0] == 0 and pc_case(plan_exe, D, kernel=TENT, flags=NORMALIZE, coef=ok)[0] == 0
    assert run_plan(plan_exe, ["null", 0]) == (-1, "args is NULL")
    assert pc_case(plan_exe, D, reserved=1, kernel=7) == (-1, "reserved must be 0")
    for k in (-1, 2, 7):
        rc, msg = pc_case(plan_exe, D, kernel=k, flags=4)
        assert rc == -1 and "kernel" in msg
    for f in (4, 8, -1 & ~3, 1 << 30):
        rc, msg = pc_case(plan_exe, D, flags=f, kernel=TENT)
        assert rc == -1 and "unknown bit" in msg
    for f in (ESSENTIAL, ESSENTIAL | NORMALIZE):
        rc, msg = pc_case(plan_exe, D, flags=f, kernel=TENT, G=0)
        assert rc == -1 and "TDA_PC_KEEP_ESSENTIAL" in msg
    assert pc_case(plan_exe, D, G=0, grid=None) == (-1, "G must be >= 1") and pc_case(plan_exe, D, G=-3)[0] == -1
    assert pc_case(plan_exe, D, grid=None, G=5000) == (-1, "grid is NULL")
    rc, msg = pc_case(plan_exe, D, grid=np.full(4097, np.nan))
    assert rc == -2 and "4096" in msg
    assert pc_case(plan_exe, D, grid=np.zeros(4096))[0] == 0
    for bad in (np.nan, np.inf, -np.inf):
        rc, msg = pc_case(plan_exe, D, grid=[0.0, bad, 1.0], offsets="null")
        assert rc == -1 and "grid" in msg and "non-finite" in msg
    assert pc_case(plan_exe, D, grid=[3.0, -1.0, 3.0, 0.0])[0] == 0  # any order, repeats
    assert pc_case(plan_exe, D, offsets="null") == (-1, "offsets is NULL")
    assert pc_case(plan_exe, D, points=False) == (-1, "points is NULL")
    assert pc_case(plan_exe, D, offsets=[1, 5, 75])[0] == -1
    rc, msg = pc_case(plan_exe, D, offsets=[0, 50, 5])
    assert rc == -1 and "non-decreasing" in msg
    assert run_plan(plan_exe, ["pc", -1, 0, 1, 0, 0, 0, 1, "0.0", -1]) == (-1, "S must be >= 0")
    # a non-finite coefficient: refused on a kept row only, and before the size limits
    for bad in (np.nan, np.inf, -np.inf):
        c = ok.copy()
        c[9] = bad
        rc, msg = pc_case(plan_exe, D, coef=c)
        assert rc == -1 and "coef" in msg
    J = [JUNK, bars(4097)]
    c = np.ones(len(JUNK) + 4097)
    c[[0, 2, 4, 6, 7]] = np.nan  # the rows the plain call drops
    rc, msg = pc_case(plan_exe, J, coef=c)
    assert rc == -2 and "4096" in msg
    rc, msg = pc_case(plan_exe, J, coef=c, flags=ESSENTIAL)  # row 2 is kept now
    assert rc == -1 and "coef" in msg
    many = [E] * 4097  # S * G: 4096 * 4096 = 2^24 passes, one diagram more does not
    assert pc_case(plan_exe, many[:4096], grid=np.zeros(4096))[0] == 0
    rc, msg = pc_case(plan_exe, many, grid=np.zeros(4096))
    assert rc == -2 and "2^24" in msg


# ---------------------------------------------------------------- the ABI
def test_pc_structs_match_header_layout(pkg, tmp_path):
    lb = pkg._lib
    src = tmp_path / "pclayout.c"
    names = {"tda_pc_args": ["offsets", "S", "coef", "grid", "G", "kernel", "flags", "device", "reserved"],
             "tda_pc_result": ["F", "values", "device_ms"]}
    body = "".join(f'printf("%zu ", sizeof({t}));' + "".join(f'printf("%zu ", offsetof({t}, {f}));' for f in fs) for t, fs in names.items())
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tda_dgm.h"\nint main(void){' + body +
                   'printf("%d %d %d %d\\n", TDA_PC_INDICATOR, TDA_PC_TENT, TDA_PC_NORMALIZE, TDA_PC_KEEP_ESSENTIAL); return 0;}\n')
    exe = tmp_path / "pclayout"
    subprocess.run(["gcc", "-I", lb.INCLUDE, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for t, fs in zip((lb.PcArgs, lb.PcResult), names.values()):
        want += [ctypes.sizeof(t)] + [getattr(t, f).offset for f in fs]
        assert [f[0] for f in t._fields_[1:]] == fs  # every field after the first is compared
    want += [lb.TDA_PC_INDICATOR, lb.TDA_PC_TENT, lb.TDA_PC_NORMALIZE, lb.TDA_PC_KEEP_ESSENTIAL]
    assert got == want and want[-4:] == [0, 1, 1, 2]
    assert [f[0] for f in lb.PcArgs._fields_[:3]] == [f[0] for f in lb.PlArgs._fields_[:3]]  # points, offsets, S as in tda_pl_args
    assert [(f[0], f[1]) for f in lb.PcResult._fields_] == [(f[0], f[1]) for f in lb.PlResult._fields_]  # the layout of tda_pl_result


def test_pc_symbols_exported_and_abi_version_unchanged(pkg, built_lib):
    lib = ctypes.CDLL(built_lib)
    assert pkg.CURVE_EXPORTS == ("tda_persistence_curve", "tda_pc_free")
    assert all(hasattr(lib, s) for s in pkg.CURVE_EXPORTS)
    others = set(pkg.EXPORTS) | set(pkg.DGM_EXPORTS) | set(pkg.BOTTLENECK_EXPORTS) | set(pkg.WASSERSTEIN_EXPORTS) | set(pkg.VECTOR_EXPORTS) | set(pkg.HEAT_EXPORTS)
    assert not set(pkg.CURVE_EXPORTS) & others
    assert pkg.lib().tda_version() == 8  # symbols added only: no existing struct changed


def test_pc_invalid_arguments_rejected_before_device(pkg, built_lib):
    L, lb = pkg.lib(), pkg._lib
    pts = np.tile(np.array([[0.0, 1.0]]), (4200, 1))
    off = np.array([0, 5, 4101], np.int64)  # 5 and 4096 points
    grid = np.linspace(0.0, 1.0, 7)
    coef = np.ones(4200)
    res = ctypes.POINTER(lb.PcResult)()

    def pc(**kw):
        a = lb.PcArgs()
        a.points, a.offsets, a.S, a.grid, a.G = pts.ctypes.data, off.ctypes.data, 2, grid.ctypes.data, 7
        a.device = 12345  # never a device: a valid call ends at the device check
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.tda_persistence_curve(ctypes.byref(a), ctypes.byref(res))
        assert not res  # no result on failure
        return rc

    def invalid(**kw):
        rc = pc(**kw)
        assert rc in (-1, -2) and L.tda_last_error(), kw
        return rc

    for kw in ({}, dict(S=0), dict(kernel=lb.TDA_PC_TENT), dict(flags=lb.TDA_PC_NORMALIZE), dict(flags=lb.TDA_PC_NORMALIZE | lb.TDA_PC_KEEP_ESSENTIAL),
               dict(coef=coef.ctypes.data), dict(coef=coef.ctypes.data, kernel=lb.TDA_PC_TENT, flags=lb.TDA_PC_NORMALIZE)):
        assert pc(**kw) == -5, kw
    assert invalid(reserved=1) == -1 and b"reserved" in L.tda_last_error()
    assert invalid(reserved=2, device=0) == -1  # before the device check even with the right ordinal
    assert invalid(kernel=2) == -1 and invalid(kernel=-1) == -1 and b"kernel" in L.tda_last_error()
    assert invalid(flags=4) == -1 and invalid(flags=-1) == -1 and b"unknown bit" in L.tda_last_error()
    assert invalid(kernel=lb.TDA_PC_TENT, flags=lb.TDA_PC_KEEP_ESSENTIAL) == -1 and b"TDA_PC_KEEP_ESSENTIAL" in L.tda_last_error()
    assert invalid(G=0) == -1 and invalid(G=-1) == -1 and invalid(G=4097) == -2 and invalid(grid=None) == -1
    for v in (np.nan, np.inf, -np.inf):
        g = grid.copy()
        g[3] = v
        assert invalid(grid=g.ctypes.data) == -1 and b"non-finite" in L.tda_last_error()
    g = grid[::-1].copy()
    assert pc(grid=g.ctypes.data) == -5  # any order
    assert invalid(offsets=None) == -1 and invalid(points=None) == -1 and invalid(S=-1) == -1
    bad = np.array([0, 50, 5], np.int64)
    assert invalid(offsets=bad.ctypes.data) == -1 and b"non-decreasing" in L.tda_last_error()
    bad = np.array([1, 5, 6], np.int64)
    assert invalid(offsets=bad.ctypes.data) == -1
    big = np.array([0, 4097, 4200], np.int64)
    assert invalid(offsets=big.ctypes.data) == -2 and b"4096" in L.tda_last_error()  # 4097 kept rows
    # 4096 finite rows and essential ones in one diagram: those count only with TDA_PC_KEEP_ESSENTIAL
    pinf = pts.copy()
    pinf[[0, 100, 4000], 1] = np.inf
    pinf[7, 0] = np.nan
    wide = np.array([0, 4100, 4200], np.int64)
    assert pc(points=pinf.ctypes.data, offsets=wide.ctypes.data) == -5
    assert invalid(points=pinf.ctypes.data, offsets=wide.ctypes.data, flags=lb.TDA_PC_KEEP_ESSENTIAL) == -2
    assert invalid(offsets=wide.ctypes.data) == -2
    # a non-finite coefficient counts on a kept row only
    c = coef.copy()
    c[7] = np.nan
    assert invalid(coef=c.ctypes.data) == -1 and b"coef" in L.tda_last_error()
    assert pc(coef=c.ctypes.data, points=pinf.ctypes.data) == -5  # row 7 is dropped there
    c[7], c[100] = 1.0, np.inf
    assert pc(coef=c.ctypes.data, points=pinf.ctypes.data) == -5
    assert invalid(coef=c.ctypes.data, points=pinf.ctypes.data, flags=lb.TDA_PC_KEEP_ESSENTIAL) == -1
    many = np.zeros(4098, np.int64)
    g = np.zeros(4096)
    assert pc(offsets=many.ctypes.data, S=4096, grid=g.ctypes.data, G=4096) == -5
    assert invalid(offsets=many.ctypes.data, S=4097, grid=g.ctypes.data, G=4096) == -2 and b"2^24" in L.tda_last_error()
    assert L.tda_persistence_curve(None, ctypes.byref(res)) == -1
    assert L.tda_persistence_curve(ctypes.byref(lb.PcArgs()), None) == -1
    L.tda_pc_free(None)  # a no-op


# ---------------------------------------------------------------- the Python entries
def importlib_module(pkg, name):
    return __import__("importlib").import_module(pkg.__name__ + "." + name)


NAMED = ("betti_curves", "lifespan_curves", "entropy_curves", "persistence_silhouettes")
SINGLE = ("betti_curve", "lifespan_curve", "entropy_curve", "persistence_silhouette")


def test_python_entries_refuse_bad_arguments_before_the_library(pkg, monkeypatch):
    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(pkg._lib, "lib", no_library)
    A = np.array([[0.0, 1.0], [0.5, 2.0]])
    g = np.linspace(0.0, 2.0, 5)
    for bad in (np.zeros((3, 3)), np.zeros(3), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            pkg.persistence_curves([A, bad], g)
        for name in NAMED:
            with pytest.raises(ValueError):
                getattr(pkg, name)([A, bad])
        for name in SINGLE:
            with pytest.raises(ValueError):
                getattr(pkg, name)(bad)
    big = np.tile(A, (2049, 1))[:4097]
    with pytest.raises(NotImplementedError, match="4096"):
        pkg.persistence_curves([A, big], g)
    with pytest.raises(NotImplementedError, match="4096"):
        pkg.betti_curve(big)
    for kw in (dict(kernel="Tent"), dict(kernel=1), dict(kernel="tent", essential=True), dict(grid=[]), dict(grid=np.zeros((2, 2))), dict(grid=[0.0, np.nan]),
               dict(grid=[np.inf]), dict(coef=[[1.0, 2.0]]), dict(coef=[[1.0], [1.0, 2.0]]), dict(coef=[[1.0, np.nan], [1.0, 2.0]]),
               dict(coef=[[1.0, 1.0], [np.inf, 2.0]])):
        with pytest.raises(ValueError):
            pkg.persistence_curves([A, A], **{"grid": g, **kw})
    with pytest.raises(NotImplementedError):
        pkg.persistence_curves([A], np.zeros(4097))
    with pytest.raises(NotImplementedError, match="2\\^24"):
        pkg.persistence_curves([A] * 4097, np.zeros(4096))
    for name in NAMED:
        fn = getattr(pkg, name)
        for kw in (dict(num_steps=0), dict(num_steps=2.5), dict(num_steps=True), dict(start=np.nan), dict(stop=np.inf),
                   dict(start=-1e308, stop=1e308, num_steps=3)):
            with pytest.raises(ValueError):
                fn([A], **kw)
        with pytest.raises(NotImplementedError):
            fn([A], num_steps=4097)
        with pytest.raises(NotImplementedError, match="2\\^24"):
            fn([A] * 4097, num_steps=4096)
        # nothing to compute: no library call, no device needed
        out, grid, ms = fn([], start=0.0, stop=1.0, num_steps=7, return_grid=True, return_time=True)
        assert out.shape == (0, 7) and out.dtype == np.float64 and np.array_equal(grid, np.linspace(0.0, 1.0, 7)) and ms == 0.0
        # an all-empty call has no default grid
        for dg in ([], [E], [E, np.array([[np.nan, 1.0]])]):
            with pytest.raises(ValueError, match="start and stop"), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                fn(dg, start=0.0)
    with pytest.raises(ValueError, match="power"):
        pkg.persistence_silhouettes([A], power=np.nan)
    flat = np.array([[0.0, 1.0], [1.0, 1.0]])
    with pytest.raises(ValueError, match="non-finite"):  # p = 0: -p log p is not a number
        pkg.entropy_curves([A, flat])
    with pytest.raises(ValueError, match="non-finite"):  # (-1) ** 0.5
        pkg.persistence_silhouettes([np.array([[0.0, 1.0], [2.0, 1.0]])], power=0.5)
    assert pkg.persistence_curves([], g).shape == (0, 5)
    out, ms = pkg.persistence_curves([], g, return_time=True)
    assert out.shape == (0, 5) and ms == 0.0
    assert {"persistence_curves", *NAMED, *SINGLE, "layer_features"} <= set(pkg.__all__)
    mm = __import__("importlib").import_module("tda_multimodal_amd")
    assert all(getattr(mm, n) is getattr(pkg, n) for n in ("betti_curves", "persistence_silhouettes", "lifespan_curves", "entropy_curves", "persistence_curves"))


@pytest.fixture
def seen(pkg, monkeypatch):
    """What reaches the library call, with zeros for a result."""
    dg = importlib_module(pkg, "diagrams")
    seen = {}

    def fake_pc(points, offsets, coef, grid, kernel, flags, device):
        seen.update(points=points.copy(), offsets=offsets.copy(), coef=None if coef is None else coef.copy(), grid=grid.copy(), kernel=kernel,
                    flags=flags, device=device, calls=seen.get("calls", 0) + 1)
        return np.arange(float((len(offsets) - 1) * len(grid))).reshape(len(offsets) - 1, len(grid)), 0.25

    monkeypatch.setattr(dg, "_call_pc", fake_pc)
    return seen


A3 = np.array([[0.5, 1.0], [0.25, np.inf], [0.75, 3.0]])
B1 = np.array([[0.375, 0.5]])


def test_routing_coefficients_and_flags(pkg, seen):
    lb = pkg._lib
    g = np.array([2.0, -1.0, 0.5])
    with pytest.warns(UserWarning, match="non-finite"):
        out, ms = pkg.persistence_curves([A3, E, B1], g, device=2, return_time=True)
    assert out.shape == (3, 3) and ms == 0.25 and (seen["kernel"], seen["flags"], seen["device"], seen["coef"]) == (lb.TDA_PC_INDICATOR, 0, 2, None)
    assert np.array_equal(seen["grid"], g) and seen["grid"].dtype == np.float64 and seen["offsets"].tolist() == [0, 3, 3, 4]
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the essential row is kept: nothing to report
        pkg.persistence_curves([A3, B1], g, coef=[[1, 2, 3], [4]], essential=True, normalize=True)
    assert (seen["kernel"], seen["flags"]) == (lb.TDA_PC_INDICATOR, lb.TDA_PC_NORMALIZE | lb.TDA_PC_KEEP_ESSENTIAL)
    assert seen["coef"].tolist() == [1.0, 2.0, 3.0, 4.0] and seen["coef"].dtype == np.float64 and seen["coef"].flags.c_contiguous
    with pytest.warns(UserWarning, match="non-finite"):
        pkg.persistence_curves([A3], g, coef=[[1.0, np.nan, 3.0]], kernel="tent", normalize=True)  # the dropped row's coefficient is not read
    assert (seen["kernel"], seen["flags"]) == (lb.TDA_PC_TENT, lb.TDA_PC_NORMALIZE)
    with pytest.raises(ValueError, match="coef"):
        pkg.persistence_curves([A3], g, coef=[[1.0, np.nan, 3.0]], essential=True)
    # the named entries
    calls = seen["calls"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = pkg.betti_curves([A3, B1], num_steps=9)
    assert out.shape == (2, 9) and (seen["kernel"], seen["flags"], seen["coef"]) == (lb.TDA_PC_INDICATOR, lb.TDA_PC_KEEP_ESSENTIAL, None)
    assert np.array_equal(seen["grid"], np.linspace(0.25, 3.0, 9))  # the essential row's birth counts, its death does not
    with pytest.warns(UserWarning, match="non-finite"):
        pkg.betti_curves([A3, B1], essential=False)
    assert seen["flags"] == 0 and np.array_equal(seen["grid"], np.linspace(0.375, 3.0, 100))
    with pytest.warns(UserWarning, match="1 points with a non-finite"):
        pkg.betti_curves([A3, np.array([[np.nan, 1.0]])])  # essential=True still reports what it drops
    with pytest.warns(UserWarning, match="non-finite"):
        pkg.lifespan_curves([A3, B1], device=3)
    assert (seen["kernel"], seen["flags"], seen["device"]) == (lb.TDA_PC_INDICATOR, 0, 3)
    assert seen["coef"][[0, 2, 3]].tolist() == [0.5, 2.25, 0.125] and np.isfinite(seen["coef"]).all()
    with pytest.warns(UserWarning, match="non-finite"):
        pkg.entropy_curves([A3, B1])
    assert (seen["kernel"], seen["flags"]) == (lb.TDA_PC_INDICATOR, 0)
    assert np.array_equal(seen["coef"][[0, 2]], pc_ref.entropy_coef(A3)) and np.array_equal(seen["coef"][3:], pc_ref.entropy_coef(B1))
    assert seen["coef"][3] == 0.0  # one bar: p = 1
    with pytest.warns(UserWarning, match="non-finite"):
        pkg.persistence_silhouettes([A3, B1], power=2)
    assert (seen["kernel"], seen["flags"]) == (lb.TDA_PC_TENT, lb.TDA_PC_NORMALIZE)
    assert np.array_equal(seen["coef"][[0, 2]], pc_ref.silhouette_coef(A3, 2.0)) and seen["coef"][3] == 0.125 ** 2
    pkg.persistence_silhouettes([B1])
    assert seen["coef"].tolist() == [0.125]
    assert seen["calls"] == calls + 7


def test_default_grid_single_forms_and_returns(pkg, seen):
    for many, one in zip(NAMED, SINGLE):
        fn, fn1 = getattr(pkg, many), getattr(pkg, one)
        out, grid, ms = fn([B1, E, B1], num_steps=9, return_grid=True, return_time=True)
        assert out.shape == (3, 9) and ms == 0.25 and np.array_equal(grid, np.linspace(0.375, 0.5, 9)) and np.array_equal(seen["grid"], grid)
        assert fn([B1]).shape == (1, 100)
        fn([B1], start=-1.0)
        assert np.array_equal(seen["grid"], np.linspace(-1.0, 0.5, 100))
        fn([B1], stop=7)
        assert np.array_equal(seen["grid"], np.linspace(0.375, 7.0, 100))
        out, ms = fn([B1, B1], return_time=True)
        assert out.shape == (2, 100) and ms == 0.25
        v, g = fn1(B1, 0.0, 1.0, 5, return_grid=True)
        assert v.shape == (5,) and np.array_equal(g, np.linspace(0.0, 1.0, 5)) and np.array_equal(v, np.arange(5.0))
        assert fn1(B1, num_steps=5).shape == (5,) and seen["offsets"].tolist() == [0, 1]
    pkg.persistence_silhouette(np.array([[0.0, 4.0]]), power=0.5)
    assert seen["coef"].tolist() == [2.0]
    with pytest.warns(UserWarning, match="non-finite"):
        pkg.betti_curve(A3, essential=False, start=0.0, stop=1.0)
    assert seen["flags"] == 0
    with pytest.raises(ValueError, match="start and stop"):
        pkg.betti_curve(np.array([[0.5, np.inf]]), start=0.0)  # a birth, but no finite death


def layer_results(pkg):
    rp = importlib_module(pkg, "ripser")  # pkg.ripser is the function
    b = rp._Batch()
    b.L, b.nd = 2, 2
    b.cnt = np.array([[1, 2], [2, 1]], np.int64)
    b.off = np.array([[0, 1], [3, 5]], np.int64)
    b.pairs = np.array([[0.0, np.inf], [0.5, 0.75], [0.25, 1.0], [0.0, 0.5], [0.0, np.inf], [0.125, 0.375]])
    return [rp.LayerResult((b, 0)), rp.LayerResult((b, 1))]


def test_layer_results_go_through_flatten(pkg, seen):
    res = layer_results(pkg)
    out = pkg.betti_curves(res, num_steps=4)
    assert out.shape == (2, 4) and seen["offsets"].tolist() == [0, 2, 3]
    assert seen["points"].tolist() == [[0.5, 0.75], [0.25, 1.0], [0.125, 0.375]]
    pkg.betti_curves(res, dim=0, num_steps=4)
    assert seen["offsets"].tolist() == [0, 1, 3] and seen["points"].tolist() == [[0.0, np.inf], [0.0, 0.5], [0.0, np.inf]]
    assert np.array_equal(seen["grid"], np.linspace(0.0, 0.5, 4))
    pkg.persistence_curves(res, [0.5], coef=[[1.0, 2.0], [3.0]], kernel="tent")
    assert seen["coef"].tolist() == [1.0, 2.0, 3.0]
    pkg.lifespan_curves(res)
    assert seen["coef"].tolist() == [0.25, 0.75, 0.25]
    for one in SINGLE:
        with pytest.raises(ValueError, match=NAMED[SINGLE.index(one)]):
            getattr(pkg, one)(res[0])
    with pytest.raises(ValueError):
        pkg.betti_curves([res[0], np.zeros((1, 2))])
    with pytest.raises(ValueError, match="dim"):
        pkg.entropy_curves(res, dim=2)


def test_layer_features_routes_the_four_kinds(pkg, seen, monkeypatch):
    lb = pkg._lib
    res = layer_results(pkg)
    want = {"betti": (lb.TDA_PC_INDICATOR, lb.TDA_PC_KEEP_ESSENTIAL), "silhouette": (lb.TDA_PC_TENT, lb.TDA_PC_NORMALIZE),
            "lifespan": (lb.TDA_PC_INDICATOR, 0), "entropy": (lb.TDA_PC_INDICATOR, 0)}
    for kind, (kernel, flags) in want.items():
        F = pkg.layer_features(res, kind)
        assert F.shape == (2, 100) and np.array_equal(F, np.arange(200.0).reshape(2, 100)) and (seen["kernel"], seen["flags"]) == (kernel, flags)
        F = pkg.layer_features([B1, E, B1], kind=kind, num_steps=7, start=0.0, stop=1.0, device=3)
        assert F.shape == (3, 7) and seen["device"] == 3 and np.array_equal(seen["grid"], np.linspace(0.0, 1.0, 7))
        with pytest.raises(ValueError, match="return_grid"):
            pkg.layer_features(res, kind, return_grid=True)
    assert (seen["coef"] is None) is False
    pkg.layer_features(res, "betti", dim=0)
    assert seen["offsets"].tolist() == [0, 1, 3] and seen["coef"] is None
    pkg.layer_features(res, "silhouette", power=2.0)
    assert seen["coef"].tolist() == [0.25 ** 2, 0.75 ** 2, 0.25 ** 2]
    calls = seen["calls"]
    for bad in ("Betti", "curves", "", "silhouettes"):
        with pytest.raises(ValueError, match="kind") as e:
            pkg.layer_features(res, kind=bad)
        assert all(k in str(e.value) for k in ("landscape", "image", "betti", "silhouette", "lifespan", "entropy"))
    assert seen["calls"] == calls
