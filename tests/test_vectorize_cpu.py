"""CPU tests of the landscape / image boundary (no device): the references
tests/pl_ref.py and tests/pi_ref.py against closed forms, the per-diagram plan of
csrc/dgm_plan.h (a sanitized host program of its own), the new symbols and the
ctypes mirrors of include/tda_dgm.h, the argument errors raised before any
device work, and the Python entries' argument handling."""
import ctypes
import os
import subprocess

import mpmath
import numpy as np
import pytest

import pi_ref
import pl_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tda-multimodal_amd", "csrc")
E = np.zeros((0, 2))


# ---------------------------------------------------------------- the references
def test_pl_ref_closed_forms():
    grid = np.array([-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 4.5])
    one = np.array([[0.0, 4.0]])
    tent = np.array([0.0, 0.0, 0.5, 1.0, 1.5, 2.0, 1.0, 0.0, 0.0])  # t at b, at d and at the midpoint 2
    L = pl_ref.landscape(one, grid, 3)
    assert np.array_equal(L[0], tent) and not L[1:].any() and not np.signbit(L).any()  # K > n: zero rows
    two = np.array([[1.0, 3.0], [0.0, 4.0]])  # nested: lambda_2 is the inner tent
    L = pl_ref.landscape(two, grid, 2)
    assert np.array_equal(L[0], tent)
    assert np.array_equal(L[1], [0.0, 0.0, 0.0, 0.0, 0.5, 1.0, 0.0, 0.0, 0.0])
    m = 5
    L = pl_ref.landscape(np.tile(one, (m, 1)), grid, m + 2)  # a bar m times: lambda_1 .. lambda_m equal
    assert all(np.array_equal(L[k], tent) for k in range(m)) and not L[m:].any()
    assert not pl_ref.landscape(np.array([[2.0, 2.0], [3.0, 1.0]]), grid, 2).any()  # d <= b: zeros
    assert not pl_ref.landscape(E, grid, 2).any()
    withinf = np.array([[0.0, np.inf], [0.0, 4.0], [np.nan, 1.0]])
    assert np.array_equal(pl_ref.landscape(withinf, grid, 3), pl_ref.landscape(one, grid, 3))
    z = pl_ref.landscape(np.array([[0.0, 1.0]]), np.array([-0.0]), 1)  # (-0) - (+0) is -0: still +0.0
    assert z[0, 0] == 0.0 and not np.signbit(z).any()
    assert pl_ref.landscapes([one, two], grid, 2).shape == (2, 2, len(grid)) and pl_ref.landscapes([], grid, 2).shape == (0, 2, len(grid))


def test_pi_ref_total_mass_separability_and_empty_bars():
    rng = np.random.default_rng(1)
    b = rng.uniform(0.0, 3.0, 12)
    D = np.stack([b, b + rng.uniform(0.1, 2.0, 12)], 1)
    sigma = 0.05
    xe, ye = np.linspace(-2.5, 5.5, 6), np.linspace(-2.5, 5.0, 5)  # >= 40 sigma beyond every point
    for power in (0.0, 1.0, 2.0):
        img = pi_ref.image(D, xe, ye, sigma, power)
        with mpmath.workdps(40):
            total, sw = mpmath.fsum(img.ravel().tolist()), mpmath.fsum(pi_ref.weights(D, power))
            assert float(abs(total - sw)) <= pi_ref.bound(D, weight_power=power)
        assert pi_ref.bound(D, weight_power=power) == pytest.approx((2 * 16 + 9 + 12) * 2.0 ** -53 * float(sw), rel=1e-12)
    # one point: the image is the outer product of its marginals
    P = np.array([[1.0, 2.5]])
    xe, ye = np.linspace(0.0, 2.0, 5), np.linspace(0.5, 2.5, 4)
    img = pi_ref.image(P, xe, ye, 0.4)
    with mpmath.workdps(40):
        rows = [mpmath.fsum(r) for r in img.tolist()]
        cols = [mpmath.fsum(img[:, j].tolist()) for j in range(img.shape[1])]
        tot = mpmath.fsum(rows)
        for i in range(img.shape[0]):
            for j in range(img.shape[1]):
                assert abs(img[i, j] * tot - rows[i] * cols[j]) < mpmath.mpf(10) ** -38
    assert float(tot) < 1.5 and float(img[1, 2]) > 0
    # d <= b adds nothing, nor do non-finite rows
    more = np.concatenate([D, [[1.0, 1.0], [2.0, 0.5], [0.0, np.inf]]])
    a, c = pi_ref.image(D, xe, ye, 0.4), pi_ref.image(more, xe, ye, 0.4)
    assert all(x == y for x, y in zip(a.ravel(), c.ravel()))
    assert all(v == 0 for v in pi_ref.image(E, xe, ye, 0.4).ravel())
    # the plain float64 restatement stays far inside the bound
    err = pi_ref.errors(pi_ref.restatement(D, xe, ye, 0.4), a)
    assert err.max() <= pi_ref.bound(D)


# ---------------------------------------------------------------- the sanitized plan program
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vec_plan") / "vec_plan")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "vec_plan_main.cpp")], check=True)
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
        out[k] = [float.fromhex(x) for x in v] if k in ("pts", "wgt") else [int(x) for x in v]
    return 0, out


def layout(dgms, offsets=None, points=True):
    off = np.concatenate([[0], np.cumsum([len(d) for d in dgms])]).astype(int) if offsets is None else offsets
    pts = np.concatenate([np.asarray(d, np.float64).reshape(-1, 2) for d in dgms]) if dgms else E
    head = [len(off) - 1 if not isinstance(off, str) else len(dgms), *(["null"] if isinstance(off, str) else off)]
    return head + ([len(pts), *fmt(pts.ravel())] if points else [-1])


def pl_case(exe, dgms, grid=(0.0, 1.0), K=3, G=None, reserved=0, **kw):
    G = (len(grid) if grid is not None else 2) if G is None else G
    return run_plan(exe, ["pl", *layout(dgms, **kw), G, K, reserved, *arr(grid)])


def pi_case(exe, dgms, xe=(0.0, 1.0, 2.0), ye=(0.0, 1.0), W=None, H=None, reserved=0, sigma=0.5, power=1.0, **kw):
    W = (len(xe) - 1 if xe is not None else 2) if W is None else W
    H = (len(ye) - 1 if ye is not None else 1) if H is None else H
    return run_plan(exe, ["pi", *layout(dgms, **kw), W, H, reserved, repr(float(sigma)), repr(float(power)), *arr(xe), *arr(ye)])


def bars(n, seed=0):
    rng = np.random.default_rng(seed)
    b = rng.uniform(0.0, 5.0, n)
    return np.stack([b, b + rng.uniform(1e-3, 5.0, n)], 1)


def test_plan_gathers_finite_rows_and_sorts_into_classes(plan_exe):
    junk = np.array([[np.nan, 1.0], [0.5, 1.5], [0.0, np.inf], [-0.0, 2.0], [-np.inf, 0.0], [3.0, 1.0]])
    sizes = [65, 0, 64, 256, 257, 1024, 1025, 4096, 1, 63]
    dgms = [bars(n, n) for n in sizes] + [junk]
    rc, p = pl_case(plan_exe, dgms)
    assert rc == 0
    fin = [pl_ref.finite_points(d) for d in dgms]
    assert p["off"] == np.concatenate([[0], np.cumsum([len(f) for f in fin])]).tolist()
    assert np.array(p["pts"]).tobytes() == np.concatenate(fin).ravel().tobytes()  # the rows, in order, bit for bit (-0 kept)
    # class 0: n <= 64, 1: <= 256, 2: <= 1024, 3: <= 4096; ascending ids within a class
    assert p["order"] == [1, 2, 8, 9, 10, 0, 3, 4, 5, 6, 7]
    assert p["cnt"] == [5, 2, 2, 2] and p["cls_n"] == [64, 256, 1024, 4096] and p["wgt"] == []
    rc, p = pl_case(plan_exe, [E, bars(3)])
    assert rc == 0 and p["cnt"] == [2, 0, 0, 0] and p["cls_n"] == [3, 0, 0, 0]
    rc, p = pl_case(plan_exe, [])
    assert rc == 0 and p["off"] == [0] and p["order"] == [] and p["pts"] == []
    # 4096 finite rows among non-finite ones pass, 4097 do not
    wide = np.concatenate([bars(4096, 1), [[0.0, np.inf]] * 3])
    assert pl_case(plan_exe, [wide])[0] == 0 and pi_case(plan_exe, [wide])[0] == 0
    for case in (pl_case, pi_case):
        rc, msg = case(plan_exe, [E, bars(4097, 2)])
        assert rc == -2 and "4096" in msg


def test_plan_image_weights(plan_exe):
    D = np.array([[0.5, 2.0], [1.0, 1.0], [2.0, 1.5], [0.1, 0.4], [0.0, np.inf], [1.0, 1.0 + 2.0 ** -30]])
    fin = pl_ref.finite_points(D)
    pers = fin[:, 1] - fin[:, 0]
    for power, want in ((0.0, np.where(pers > 0, 1.0, 0.0)), (1.0, np.where(pers > 0, pers, 0.0)),
                        (2.0, np.where(pers > 0, np.power(np.abs(pers), 2.0), 0.0))):
        rc, p = pi_case(plan_exe, [D, E], power=power)
        assert rc == 0 and p["off"] == [0, 5, 5]
        got = np.array(p["pts"]).reshape(-1, 2)
        assert np.array_equal(got[:, 0], fin[:, 0]) and np.array_equal(got[:, 1], pers)  # (b, pi)
        if power == 2.0:  # pow: within one ulp of the exact square
            assert np.all(np.abs(np.array(p["wgt"]) - want) <= np.spacing(want))
        else:
            assert np.array(p["wgt"]).tobytes() == want.tobytes()
        assert not np.signbit(p["wgt"]).any()


def test_plan_argument_errors_and_their_codes(plan_exe):
    D = [bars(5), bars(70, 1)]
    assert pl_case(plan_exe, D)[0] == 0 and pi_case(plan_exe, D)[0] == 0
    assert run_plan(plan_exe, ["null", 0])[0] == -1 and run_plan(plan_exe, ["null", 1])[0] == -1
    for case in (pl_case, pi_case):
        assert case(plan_exe, D, reserved=1) == (-1, "reserved must be 0")
        assert case(plan_exe, D, offsets="null") == (-1, "offsets is NULL")
        assert case(plan_exe, D, points=False) == (-1, "points is NULL")
        assert case(plan_exe, D, offsets=[1, 5, 75])[0] == -1
        rc, msg = case(plan_exe, D, offsets=[0, 50, 5])
        assert rc == -1 and "non-decreasing" in msg
        tail = [1, 1, 0, 1, "0.0"] if case is pl_case else [1, 1, 0, "0.5", "1.0", 2, "0.0", "1.0", 2, "0.0", "1.0"]
        assert run_plan(plan_exe, [case.__name__[:2], -1, 0, *tail]) == (-1, "S must be >= 0")
    # landscape
    for K, G, code in ((0, 2, -1), (-3, 2, -1), (65, 2, -2), (64, 2, 0), (3, 0, -1), (3, 4097, -2)):
        assert pl_case(plan_exe, D, K=K, G=G)[0] == code, (K, G)
    assert pl_case(plan_exe, D, grid=np.zeros(4096), K=1)[0] == 0
    assert pl_case(plan_exe, D, grid=None) == (-1, "grid is NULL")
    for bad in (np.nan, np.inf, -np.inf):
        rc, msg = pl_case(plan_exe, D, grid=[0.0, bad, 1.0])
        assert rc == -1 and "non-finite" in msg
    assert pl_case(plan_exe, D, grid=[3.0, -1.0, 3.0, 0.0])[0] == 0  # any order, repeats
    many = [E] * 65  # S * K * G: 64 * 64 * 4096 = 2^24 passes, one diagram more does not
    assert pl_case(plan_exe, many[:64], grid=np.zeros(4096), K=64)[0] == 0
    rc, msg = pl_case(plan_exe, many, grid=np.zeros(4096), K=64)
    assert rc == -2 and "2^24" in msg
    # image
    for kw in (dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=np.nan), dict(sigma=np.inf), dict(power=-0.5), dict(power=np.nan),
               dict(power=np.inf), dict(W=0), dict(H=0), dict(H=-1), dict(xe=None), dict(ye=None), dict(xe=[0.0, np.nan, 2.0]),
               dict(ye=[0.0, np.inf]), dict(xe=[0.0, 0.0, 1.0]), dict(xe=[0.0, 2.0, 1.0]), dict(ye=[1.0, 0.0])):
        rc, msg = pi_case(plan_exe, D, **kw)
        assert rc == -1 and msg, kw
    assert pi_case(plan_exe, D, xe=np.arange(257.0), ye=np.arange(257.0))[0] == 0
    rc, msg = pi_case(plan_exe, D, xe=np.arange(258.0))
    assert rc == -2 and "256" in msg
    assert pi_case(plan_exe, [E] * 256, xe=np.arange(257.0), ye=np.arange(257.0))[0] == 0  # 2^24 values
    rc, msg = pi_case(plan_exe, [E] * 257, xe=np.arange(257.0), ye=np.arange(257.0))
    assert rc == -2 and "2^24" in msg
    assert pi_case(plan_exe, D, power=0.0)[0] == 0 and pi_case(plan_exe, D, power=3.5)[0] == 0


# ---------------------------------------------------------------- the ABI
def test_vec_structs_match_header_layout(pkg, tmp_path):
    lb = pkg._lib
    src = tmp_path / "veclayout.c"
    names = {"tda_pl_args": ["offsets", "S", "grid", "G", "K", "device", "reserved"], "tda_pl_result": ["F", "values", "device_ms"],
             "tda_pi_args": ["offsets", "S", "x_edges", "y_edges", "W", "H", "sigma", "weight_power", "device", "reserved"],
             "tda_pi_result": ["F", "values", "device_ms"]}
    body = "".join(f'printf("%zu ", sizeof({t}));' + "".join(f'printf("%zu ", offsetof({t}, {f}));' for f in fs) for t, fs in names.items())
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tda_dgm.h"\nint main(void){' + body +
                   'printf("%d %lld %d %d %d %d\\n", TDA_VEC_MAX_POINTS, (long long)TDA_VEC_MAX_OUT, TDA_PL_MAX_DEPTH, TDA_PL_MAX_STEPS,'
                   ' TDA_PI_MAX_PIXELS, TDA_PI_ERF_ULP); return 0;}\n')
    exe = tmp_path / "veclayout"
    subprocess.run(["gcc", "-I", lb.INCLUDE, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for t, fs in zip((lb.PlArgs, lb.PlResult, lb.PiArgs, lb.PiResult), names.values()):
        want += [ctypes.sizeof(t)] + [getattr(t, f).offset for f in fs]
        assert [f[0] for f in t._fields_[1:]] == fs  # every field after the first is compared
    want += [lb.TDA_VEC_MAX_POINTS, lb.TDA_VEC_MAX_OUT, lb.TDA_PL_MAX_DEPTH, lb.TDA_PL_MAX_STEPS, lb.TDA_PI_MAX_PIXELS, lb.TDA_PI_ERF_ULP]
    assert got == want
    assert want[-6:] == [4096, 1 << 24, 64, 4096, 256, 16] and pi_ref.ERF_ULP == lb.TDA_PI_ERF_ULP
    assert [f[0] for f in lb.PlArgs._fields_[:3]] == [f[0] for f in lb.BnArgs._fields_[:3]]  # points, offsets, S as in tda_bn_args


def test_vec_symbols_exported_and_abi_version_unchanged(pkg, built_lib):
    lib = ctypes.CDLL(built_lib)
    assert pkg.VECTOR_EXPORTS == ("tda_landscape", "tda_pl_free", "tda_persistence_image", "tda_pi_free")
    assert all(hasattr(lib, s) for s in pkg.VECTOR_EXPORTS)
    others = set(pkg.EXPORTS) | set(pkg.DGM_EXPORTS) | set(pkg.BOTTLENECK_EXPORTS) | set(pkg.WASSERSTEIN_EXPORTS)
    assert not set(pkg.VECTOR_EXPORTS) & others
    assert pkg.lib().tda_version() == 8  # symbols added only: no existing struct changed


def test_vec_invalid_arguments_rejected_before_device(pkg, built_lib):
    L, lb = pkg.lib(), pkg._lib
    pts = np.tile(np.array([[0.0, 1.0]]), (4200, 1))
    off = np.array([0, 5, 4101], np.int64)  # 5 and 4096 points
    grid = np.linspace(0.0, 1.0, 7)
    xe, ye = np.linspace(0.0, 1.0, 5), np.linspace(0.0, 1.0, 4)
    plres, pires = ctypes.POINTER(lb.PlResult)(), ctypes.POINTER(lb.PiResult)()

    def pl(**kw):
        a = lb.PlArgs()
        a.points, a.offsets, a.S, a.grid, a.G, a.K = pts.ctypes.data, off.ctypes.data, 2, grid.ctypes.data, 7, 3
        a.device = 12345  # never a device: a valid call ends at the device check
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.tda_landscape(ctypes.byref(a), ctypes.byref(plres))
        assert not plres  # no result on failure
        return rc

    def pi(**kw):
        a = lb.PiArgs()
        a.points, a.offsets, a.S = pts.ctypes.data, off.ctypes.data, 2
        a.x_edges, a.y_edges, a.W, a.H, a.sigma, a.weight_power = xe.ctypes.data, ye.ctypes.data, 4, 3, 0.5, 1.0
        a.device = 12345
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.tda_persistence_image(ctypes.byref(a), ctypes.byref(pires))
        assert not pires
        return rc

    def invalid(call, **kw):
        rc = call(**kw)
        assert rc in (-1, -2) and L.tda_last_error(), kw
        return rc

    assert pl() == -5 and pi() == -5 and pl(S=0) == -5 and pi(weight_power=0.0) == -5
    big = np.array([0, 4097, 4200], np.int64)
    for call in (pl, pi):
        assert invalid(call, reserved=1) == -1 and b"reserved" in L.tda_last_error()
        assert invalid(call, offsets=None) == -1 and invalid(call, points=None) == -1 and invalid(call, S=-1) == -1
        bad = np.array([0, 50, 5], np.int64)
        assert invalid(call, offsets=bad.ctypes.data) == -1 and b"non-decreasing" in L.tda_last_error()
        bad = np.array([1, 5, 6], np.int64)
        assert invalid(call, offsets=bad.ctypes.data) == -1
        assert invalid(call, offsets=big.ctypes.data) == -2 and b"4096" in L.tda_last_error()  # 4097 finite points
        # 4096 finite points and non-finite rows in one diagram: those do not count towards the limit
        pinf = pts.copy()
        pinf[[0, 100, 4000], 1] = np.inf
        pinf[7, 0] = np.nan
        wide = np.array([0, 4100, 4200], np.int64)
        assert call(points=pinf.ctypes.data, offsets=wide.ctypes.data) == -5
        assert invalid(call, offsets=wide.ctypes.data) == -2
        assert invalid(call, reserved=2, device=0) == -1  # before the device check even with the right ordinal
    assert invalid(pl, K=0) == -1 and invalid(pl, K=65) == -2 and invalid(pl, G=0) == -1 and invalid(pl, G=4097) == -2
    assert invalid(pl, grid=None) == -1
    for v in (np.nan, np.inf):
        g = grid.copy()
        g[3] = v
        assert invalid(pl, grid=g.ctypes.data) == -1 and b"non-finite" in L.tda_last_error()
    g = grid[::-1].copy()
    assert pl(grid=g.ctypes.data) == -5  # any order
    many = np.zeros(66, np.int64)
    g = np.zeros(4096)
    assert pl(offsets=many.ctypes.data, S=64, grid=g.ctypes.data, G=4096, K=64) == -5
    assert invalid(pl, offsets=many.ctypes.data, S=65, grid=g.ctypes.data, G=4096, K=64) == -2 and b"2^24" in L.tda_last_error()
    for kw in (dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(weight_power=-1.0),
               dict(weight_power=float("nan")), dict(W=0), dict(H=0), dict(x_edges=None), dict(y_edges=None)):
        assert invalid(pi, **kw) == -1, kw
    for e in ([0.0, 0.5, 0.5, 0.75, 1.0], [0.0, 0.5, 0.25, 0.75, 1.0], [0.0, np.nan, 0.5, 0.75, 1.0], [0.0, 0.25, 0.5, 0.75, np.inf]):
        e = np.array(e)
        assert invalid(pi, x_edges=e.ctypes.data) == -1
        assert invalid(pi, y_edges=e.ctypes.data, H=4) == -1
    e = np.arange(258.0)
    assert pi(x_edges=e.ctypes.data, W=256, y_edges=e.ctypes.data, H=256) == -5
    assert invalid(pi, x_edges=e.ctypes.data, W=257) == -2 and invalid(pi, y_edges=e.ctypes.data, H=257) == -2
    many = np.zeros(258, np.int64)
    assert pi(offsets=many.ctypes.data, S=256, x_edges=e.ctypes.data, W=256, y_edges=e.ctypes.data, H=256) == -5
    assert invalid(pi, offsets=many.ctypes.data, S=257, x_edges=e.ctypes.data, W=256, y_edges=e.ctypes.data, H=256) == -2
    assert L.tda_landscape(None, ctypes.byref(plres)) == -1 and L.tda_persistence_image(None, ctypes.byref(pires)) == -1
    assert L.tda_landscape(ctypes.byref(lb.PlArgs()), None) == -1 and L.tda_persistence_image(ctypes.byref(lb.PiArgs()), None) == -1
    L.tda_pl_free(None)  # no-ops
    L.tda_pi_free(None)


# ---------------------------------------------------------------- the Python entries
def importlib_module(pkg, name):
    return __import__("importlib").import_module(pkg.__name__ + "." + name)


IMG = dict(birth_range=(0.0, 2.0), pers_range=(0.0, 3.0), resolution=(4, 3), sigma=0.5)


def test_python_entries_refuse_bad_arguments_before_the_library(pkg, monkeypatch):
    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(pkg._lib, "lib", no_library)
    A = np.array([[0.0, 1.0], [0.5, 2.0]])
    for bad in (np.zeros((3, 3)), np.zeros(3), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            pkg.persistence_landscapes([A, bad])
        with pytest.raises(ValueError):
            pkg.persistence_landscape(bad)
        with pytest.raises(ValueError):
            pkg.persistence_images([A, bad], **IMG)
        with pytest.raises(ValueError):
            pkg.persistence_image(bad, **IMG)
    big = np.tile(A, (2049, 1))[:4097]
    with pytest.raises(NotImplementedError, match="4096"):
        pkg.persistence_landscapes([A, big])
    with pytest.raises(NotImplementedError, match="4096"):
        pkg.persistence_image(big, **IMG)
    for kw in (dict(depth=0), dict(depth=2.5), dict(num_steps=0), dict(num_steps=True), dict(start=np.nan), dict(stop=np.inf),
               dict(start=-1e308, stop=1e308, num_steps=3)):
        with pytest.raises(ValueError):
            pkg.persistence_landscapes([A], **kw)
    for kw in (dict(depth=65), dict(num_steps=4097)):
        with pytest.raises(NotImplementedError):
            pkg.persistence_landscapes([A], **kw)
    with pytest.raises(NotImplementedError, match="2\\^24"):
        pkg.persistence_landscapes([A] * 65, num_steps=4096, depth=64)
    for kw in (dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=np.nan), dict(weight_power=-1.0), dict(weight_power=np.inf),
               dict(birth_range=(1.0, 1.0)), dict(birth_range=(2.0, 1.0)), dict(pers_range=(0.0, np.inf)), dict(pers_range=3.0),
               dict(birth_range=(0.0, 1.0, 2.0)), dict(resolution=0), dict(resolution=(4, 0)), dict(resolution=(4, 3, 2)),
               dict(resolution=2.5), dict(birth_range=(1.0, 1.0 + 2.0 ** -50), resolution=16)):
        with pytest.raises(ValueError):
            pkg.persistence_images([A], **{**IMG, **kw})
    with pytest.raises(NotImplementedError):
        pkg.persistence_images([A], **{**IMG, "resolution": 257})
    with pytest.raises(NotImplementedError, match="2\\^24"):
        pkg.persistence_images([A] * 257, **{**IMG, "resolution": 256})
    # nothing to compute: no library call, no device needed
    out = pkg.persistence_landscapes([], start=0.0, stop=1.0, num_steps=7, depth=2)
    assert out.shape == (0, 2, 7) and out.dtype == np.float64
    out, grid, ms = pkg.persistence_landscapes([], start=0.0, stop=1.0, num_steps=7, depth=2, return_grid=True, return_time=True)
    assert out.shape == (0, 2, 7) and np.array_equal(grid, np.linspace(0.0, 1.0, 7)) and ms == 0.0
    assert pkg.persistence_images([], **IMG).shape == (0, 4, 3)
    out, ms = pkg.persistence_images([], return_time=True, **{**IMG, "resolution": 5})
    assert out.shape == (0, 5, 5) and ms == 0.0
    # an all-empty call has no default grid
    for dg in ([], [E], [E, np.array([[0.0, np.inf]])]):
        with pytest.raises(ValueError, match="start and stop"), __import__("warnings").catch_warnings():
            __import__("warnings").simplefilter("ignore")
            pkg.persistence_landscapes(dg, start=0.0)
    assert {"persistence_landscape", "persistence_landscapes", "persistence_image", "persistence_images", "layer_features"} <= set(pkg.__all__)


def test_default_grid_and_what_reaches_the_library(pkg, monkeypatch):
    dg = importlib_module(pkg, "diagrams")
    seen = {}

    def fake_pl(points, offsets, grid, K, device):
        seen.update(points=points.copy(), offsets=offsets.copy(), grid=grid.copy(), K=K, device=device)
        return np.zeros((len(offsets) - 1, K, len(grid))), 0.25

    def fake_pi(points, offsets, xe, ye, sigma, power, device):
        seen.update(points=points.copy(), offsets=offsets.copy(), xe=xe.copy(), ye=ye.copy(), sigma=sigma, power=power, device=device)
        return np.zeros((len(offsets) - 1, len(xe) - 1, len(ye) - 1)), 0.5

    monkeypatch.setattr(dg, "_call_pl", fake_pl)
    monkeypatch.setattr(dg, "_call_pi", fake_pi)
    A = np.array([[0.5, 1.0], [0.25, np.inf], [0.75, 3.0]])  # the non-finite row does not set the range
    B = np.array([[0.375, 0.5]])
    with pytest.warns(UserWarning, match="non-finite"):
        out, grid, ms = pkg.persistence_landscapes([A, E, B], num_steps=9, depth=4, device=2, return_grid=True, return_time=True)
    assert out.shape == (3, 4, 9) and ms == 0.25 and seen["K"] == 4 and seen["device"] == 2
    assert np.array_equal(grid, np.linspace(0.375, 3.0, 9)) and np.array_equal(seen["grid"], grid)
    assert seen["offsets"].tolist() == [0, 3, 3, 4] and seen["grid"].dtype == np.float64 and seen["grid"].flags.c_contiguous
    out = pkg.persistence_landscapes([B], start=-1.0)
    assert out.shape == (1, 10, 500) and np.array_equal(seen["grid"], np.linspace(-1.0, 0.5, 500))
    pkg.persistence_landscapes([B], stop=7)
    assert np.array_equal(seen["grid"], np.linspace(0.375, 7.0, 500))
    one, g = pkg.persistence_landscape(B, 0.0, 1.0, 5, 2, return_grid=True)
    assert one.shape == (2, 5) and np.array_equal(g, np.linspace(0.0, 1.0, 5))
    assert pkg.persistence_landscape(B, num_steps=5, depth=2).shape == (2, 5)
    out, ms = pkg.persistence_images([B, E], (0.0, 2.0), (0.0, 3.0), (4, 3), 0.5, weight_power=2, device=1, return_time=True)
    assert out.shape == (2, 4, 3) and ms == 0.5 and (seen["sigma"], seen["power"], seen["device"]) == (0.5, 2.0, 1)
    assert np.array_equal(seen["xe"], np.linspace(0.0, 2.0, 5)) and np.array_equal(seen["ye"], np.linspace(0.0, 3.0, 4))
    assert pkg.persistence_images([B], (0.0, 2.0), (0.0, 3.0), 6, 0.5).shape == (1, 6, 6)
    assert pkg.persistence_image(B, **IMG).shape == (4, 3)


def test_layer_results_are_refused_by_the_single_forms(pkg):
    rp = importlib_module(pkg, "ripser")  # pkg.ripser is the function
    b = rp._Batch()
    b.L, b.nd = 1, 2
    b.cnt = np.array([[1, 1]], np.int64)
    b.off = np.array([[0, 1]], np.int64)
    b.pairs = np.array([[0.0, 1.0], [0.5, 0.75]])
    r = rp.LayerResult((b, 0))
    with pytest.raises(ValueError, match="persistence_landscapes"):
        pkg.persistence_landscape(r)
    with pytest.raises(ValueError, match="persistence_images"):
        pkg.persistence_image(r, **IMG)
    with pytest.raises(ValueError):
        pkg.persistence_landscapes([r, np.zeros((1, 2))])
    with pytest.raises(ValueError, match="dim"):
        pkg.persistence_images([r], dim=2, **IMG)


def test_layer_features_routes_by_kind(pkg, monkeypatch):
    pl = importlib_module(pkg, "pipeline")
    calls = []
    monkeypatch.setattr(pl, "persistence_landscapes", lambda results, **kw: calls.append(("pl", results, kw)) or np.arange(12.0).reshape(2, 2, 3))
    monkeypatch.setattr(pl, "persistence_images", lambda results, **kw: calls.append(("pi", results, kw)) or np.arange(24.0).reshape(2, 4, 3))
    r = [E] * 2
    F = pkg.layer_features(r)
    assert F.shape == (2, 6) and np.array_equal(F, np.arange(12.0).reshape(2, 6))
    F = pkg.layer_features(r, "image", dim=0, device=3, **IMG)
    assert F.shape == (2, 12) and np.array_equal(F[1], np.arange(12.0, 24.0))
    pkg.layer_features(r, kind="landscape", depth=2, num_steps=3, start=0.0, stop=1.0)
    assert calls == [("pl", r, {"dim": 1, "device": 0}), ("pi", r, {"dim": 0, "device": 3, **IMG}),
                     ("pl", r, {"dim": 1, "device": 0, "depth": 2, "num_steps": 3, "start": 0.0, "stop": 1.0})]
    for bad in ("Landscape", "images", ""):
        with pytest.raises(ValueError, match="kind"):
            pkg.layer_features(r, kind=bad)
    assert len(calls) == 3
