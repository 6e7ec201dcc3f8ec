"""CPU tests of the geodesic-distance entry (no device): the host plan (csrc/geo_plan.h) against a
Python restatement (geo_ref.plan) and every refusal with its code, its message and its place in the
order of checks; the same refusals through tda_geodesic itself, before the device check; the numpy
restatement (geo_ref.py) against brute force over all simple paths and on graphs with known answers;
the tie rule; and the Python entry's own checks.

tests/geo_plan_main.cpp includes only geo_plan.h; it is compiled with g++ under the address and
undefined-behaviour sanitizers and run as a program of its own, one case per line."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import geo_ref
import side_plan_ref as spr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tda-multimodal_amd", "csrc")
INVALID, UNSUPPORTED, NODEVICE = -1, -2, -5
F32, F64 = spr.F32, spr.F64
GIB4 = 4 << 30
INF = float("inf")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("geo_plan") / "geo_plan")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "geo_plan_main.cpp")], check=True)
    return exe


def run(exe, lines, lds_n=None):
    """-> per line ("err", code, message) or ("ok", {field: value})"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("TDA_")}
    if lds_n is not None:
        env.update(TDA_TEST_OVERRIDES="1", TDA_GEO_LDS_N=str(lds_n))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]  # a sanitizer report ends the program with a non-zero status
    out = []
    for line in r.stdout.splitlines():
        head = line.split(" ", 2)
        if head[0] == "err":
            out.append(("err", int(head[1]), head[2]))
        else:
            assert head[0] == "ok"
            out.append(("ok", {k: int(v) for k, v in (t.split("=") for t in line.split()[1:])}))
    assert len(out) == len(lines)
    return out


def line_of(c):
    xs = (c["args"], c["cap"], c["x"], c["dtype"], c["dev"], c["L"], c["N"], c["D"], c["is_dist"], c["k"], c["graph_only"], c["radius"], c["bad"])
    return " ".join(str(x) for x in xs)


BASE = dict(args=1, cap=GIB4, x=1, dtype=F32, dev=0, L=3, N=65, D=3, is_dist=0, k=6, graph_only=0, radius=-1.0, bad="-")
TOO_MANY = "geodesic distances: more than 2^28 values (L * N * N) in one call is not supported: split L over several calls"
F64_POINTS = "geodesic distances of float64 point clouds is not supported (pass float32 points or a distance matrix)"


# ---------------------------------------------------------------- 1. the plan against the restatement
GRID_N = (1, 2, 63, 64, 65, 127, 128, 129, 8192, 8193)


def test_plan_grid(plan_exe):
    """Every N around a tile, around the resident limit and around the size limit, L on both sides of
    L * N * N = 2^28, both graphs, under the default cap, a cap of one layer and of two; then the
    other input forms and the test-only resident limit."""
    cases = []
    for N, L, k in itertools.product(GRID_N, (1, 3, 4, 5), (0, 1, 6, 10000)):
        Ls = (L,) if N != 64 else (L, (1 << 16) + L - 4)  # N = 64: 2^16 layers are 2^28 values
        for LL in Ls:
            kw = dict(L=LL, N=N, D=3, dtype=F32, is_dist=False, host_in=True, n_neighbors=k)
            first = geo_ref.plan(**kw)
            caps = (GIB4,) if first[0] == "err" else (GIB4, first[1]["per_layer"], 2 * first[1]["per_layer"], 1)
            cases += [(kw, cap, None) for cap in caps]
    for N, (D, dtype, is_dist, host_in) in itertools.product((36, 128, 129), ((64, F32, 0, 1), (3, F32, 0, 0), (3, F32, 1, 1), (3, F64, 1, 1), (3, F64, 1, 0))):
        cases.append((dict(L=3, N=N, D=D, dtype=dtype, is_dist=bool(is_dist), host_in=bool(host_in), n_neighbors=6, graph_only=1), GIB4, None))
    for N, lds_n in itertools.product((1, 2, 64, 65, 129), (1, 64, 100000, 0)):
        cases.append((dict(L=2, N=N, D=3, dtype=F32, is_dist=False, host_in=True, n_neighbors=3), GIB4, lds_n))
    seen, paths = set(), set()
    for lds_n in sorted({c[2] for c in cases}, key=str):
        group = [c for c in cases if c[2] == lds_n]
        lines = [line_of(dict(BASE, cap=cap, dtype=kw["dtype"], dev=1 - kw["host_in"], L=kw["L"], N=kw["N"], D=kw["D"], is_dist=int(kw["is_dist"]),
                              k=kw["n_neighbors"], radius=-1.0 if kw["n_neighbors"] else 0.5, graph_only=kw.get("graph_only", 0))) for kw, cap, _ in group]
        for (kw, cap, _), got in zip(group, run(plan_exe, lines, lds_n)):
            want = geo_ref.plan(cap=cap, lds_n=lds_n, **kw)
            assert got == want, (kw, cap, lds_n)
            if got[0] == "err":
                continue
            p, L, N = got[1], kw["L"], kw["N"]
            Lc = p["Lc"]
            assert 1 <= Lc <= min(L, 65535) and (Lc == L or Lc == 65535 or (Lc + 1) * p["per_layer"] > cap) and (Lc == 1 or Lc * p["per_layer"] <= cap)
            assert p["resident"] == int(N <= p["lds_n"]) and p["lds_n"] <= 128
            assert p["resident"] or (p["tiles"] == -(-N // 64) and p["padded"] == 64 * p["tiles"] >= N > p["padded"] - 64)
            assert max(p["lds_select"], p["lds_resident"], p["lds_diag"], p["lds_product"]) <= 64 * 1024
            assert p["k"] == (min(kw["n_neighbors"], N - 1) if kw["n_neighbors"] else 0)
            arrays = [("o_ne", L * 8), ("o_nc", L * 4), ("o_thr", Lc * N * 8 if p["knn"] else 0), ("o_x", Lc * p["x_layer"] if kw["host_in"] else 0),
                      ("o_dm", Lc * N * N * 4), ("o_rm", Lc * N * 4)]
            end = 0
            for name, nbytes in arrays:
                assert p[name] % 256 == 0 and p[name] >= end, name  # aligned, increasing, not overlapping
                end = p[name] + nbytes
            assert p["total"] % 256 == 0 and p["total"] >= end
            seen.add(min(Lc, 2) if Lc < L else "all")
            paths.add((p["resident"], p["tiles"] if lds_n == 1 else min(p["tiles"], 4)))
    assert seen == {1, 2, "all"}
    assert {(1, 0), (0, 1), (0, 2), (0, 3), (0, 4)} <= paths  # resident; one, two and three tiles under the lowered limit


# ---------------------------------------------------------------- 2. the refusals, in the order of the checks
def test_refusals(plan_exe):
    """Case i has wrong what refusal i names and everything the later ones name: it must come back with
    refusal i, so no later check runs before an earlier one.  Then each alone."""
    refusals = [
        (dict(args=0), INVALID, "args is NULL"), (dict(x=0), INVALID, "x is NULL"), (dict(L=0), INVALID, "L must be >= 1"),
        (dict(N=0), INVALID, "N must be >= 1"), (dict(D=0), INVALID, "D must be >= 1"), (dict(dtype=-1), INVALID, "dtype must be TDA_F32 or TDA_F64"),
        (dict(k=-1), INVALID, "n_neighbors must be >= 1 (0: not given)"), (dict(radius="nan"), INVALID, "radius is NaN"),
        (dict(k=6, radius=0.5), INVALID, "give n_neighbors or radius, not both"),
        (dict(k=0, radius=-1.0), INVALID, "give n_neighbors >= 1 or radius >= 0"),
        (dict(N=8193), UNSUPPORTED, "geodesic distances: N > 8192 is not supported"),
        (dict(L=5, N=8192), UNSUPPORTED, TOO_MANY),
        (dict(dtype=F64), UNSUPPORTED, F64_POINTS)]
    lines = []
    for i in range(len(refusals)):
        c = dict(BASE)
        for wrong, _, _ in reversed(refusals[i:]):
            c.update(wrong)
        lines.append(line_of(c))
    lines += [line_of(dict(BASE, **wrong)) for wrong, _, _ in refusals]
    got = run(plan_exe, lines + [line_of(BASE)])
    assert got[-1][0] == "ok", got[-1]
    want = [("err", code, msg) for _, code, msg in refusals]
    assert got[:len(refusals)] == want
    assert got[len(refusals):-1] == want


def test_refusal_edges(plan_exe):
    M = dict(is_dist=1, L=2, N=5, D=5)
    cases = [
        (dict(k=0, radius=0.0), "ok"), (dict(k=0, radius="inf"), "ok"), (dict(k=0, radius="-inf"), ("err", INVALID, "give n_neighbors >= 1 or radius >= 0")),
        (dict(k=0, radius=-0.0), "ok"), (dict(k=1), "ok"), (dict(k=2 ** 31 - 1), "ok"), (dict(N=1), "ok"),
        # the limits themselves
        (dict(L=4, N=8192), "ok"), (dict(L=1 << 16, N=64), "ok"), (dict(L=(1 << 16) + 1, N=64), ("err", UNSUPPORTED, TOO_MANY)),
        # a host matrix is read last: after the sizes and the dtype
        (dict(M), "ok"), (dict(M, dtype=F64), "ok"), (dict(M, bad="7:-1"), ("err", INVALID, "x[0][1][2] = -1.000000 is not finite and >= 0")),
        (dict(M, bad="49:inf"), ("err", INVALID, "x[1][4][4] = inf is not finite and >= 0")),
        (dict(M, dtype=F64, bad="25:nan"), ("err", INVALID, "x[1][0][0] = nan is not finite and >= 0")),
        (dict(M, bad="7:-0.0"), "ok"), (dict(M, bad="7:-1", dev=1), "ok"),  # a device matrix is not read
        (dict(M, bad="7:-1", k=-1), ("err", INVALID, "n_neighbors must be >= 1 (0: not given)")),
        (dict(M, bad="7:-1", N=8193), ("err", UNSUPPORTED, "geodesic distances: N > 8192 is not supported")),
        (dict(dtype=F64, is_dist=1, D=0), "ok"),
    ]
    got = run(plan_exe, [line_of(dict(BASE, **wrong)) for wrong, _ in cases])
    for (wrong, want), g in zip(cases, got):
        assert (g[0] if want == "ok" else g) == want, (wrong, g)


# ---------------------------------------------------------------- 3. the boundary of the library
A_FIELDS = ["x", "dtype", "x_on_device", "L", "N", "D", "is_dist", "device", "stream", "n_neighbors", "graph_only", "radius"]
R_FIELDS = ["L", "N", "dist", "n_components", "n_edges", "device", "device_ms"]


def test_structs_match_header_layout(pkg, tmp_path):
    lb = pkg._lib
    fmt = " ".join(["%zu"] * (2 + len(A_FIELDS) + len(R_FIELDS)))
    args = ", ".join(["sizeof(tda_geodesic_args)"] + [f"offsetof(tda_geodesic_args, {f})" for f in A_FIELDS]
                     + ["sizeof(tda_geodesic_result)"] + [f"offsetof(tda_geodesic_result, {f})" for f in R_FIELDS])
    src = tmp_path / "geolayout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tda_rips.h"\n'
                   f'int main(void){{printf("{fmt}\\n", {args}); return 0;}}\n')
    exe = tmp_path / "geolayout"
    subprocess.run(["gcc", "-I", lb.INCLUDE, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    A, R = lb.GeodesicArgs, lb.GeodesicResult
    assert got == ([ctypes.sizeof(A)] + [getattr(A, f).offset for f in A_FIELDS] + [ctypes.sizeof(R)] + [getattr(R, f).offset for f in R_FIELDS])


def test_constants_match_sources(pkg):
    import re

    lb = pkg._lib
    hdr = open(os.path.join(lb.INCLUDE, "tda_rips.h")).read()
    shift = re.search(r"#define TDA_GEO_MAX_OUT \((\d+)ll << (\d+)\)", hdr)
    assert shift and int(shift.group(1)) << int(shift.group(2)) == lb.TDA_GEO_MAX_OUT == geo_ref.MAX_OUT
    ker = open(os.path.join(lb.CSRC, "geo_kernels.h")).read()
    plan = open(os.path.join(lb.CSRC, "geo_plan.h")).read()
    for kname, pname, value in (("kGeoLdsN", "kSideGeoLdsN", lb.TDA_GEO_LDS_N), ("kGeoTile", "kSideGeoTile", lb.TDA_GEO_TILE), ("kGeoT", "kSideGeoT", 256)):
        assert int(re.search(rf"constexpr int {kname} = (\d+);", ker).group(1)) == value
        assert int(re.search(rf"constexpr int {pname} = (\d+);", plan).group(1)) == value
    assert (lb.TDA_GEO_LDS_N, lb.TDA_GEO_TILE, lb.TDA_GEO_MAX_N) == (geo_ref.LDS_N, geo_ref.TILE, geo_ref.MAX_N)
    assert int(re.search(r"constexpr int kGeoMaxN = (\d+);", ker).group(1)) == lb.TDA_GEO_MAX_N


def test_symbols_exported_and_abi_version_unchanged(pkg, built_lib):
    lib = ctypes.CDLL(built_lib)
    names = ("tda_geodesic", "tda_geodesic_free")
    assert set(names) <= set(pkg.EXPORTS) and pkg._lib.SIDE_ENTRIES["geo"][:2] == names
    assert all(hasattr(lib, s) for s in names)
    hdr = open(os.path.join(pkg._lib.INCLUDE, "tda_rips.h")).read()
    assert all(f" {s}(" in hdr for s in names)
    assert pkg.lib().tda_version() == 8  # symbols added only: no existing struct changed
    assert {"geodesic_distances", "GeodesicDistances"} <= set(pkg.__all__)


def test_library_refuses_before_the_device_check(pkg, built_lib):
    """Every refusal of the plan through tda_geodesic itself: they come before need_device, so they come
    back here, where there is no device; a valid call gets as far as TDA_E_NODEVICE."""
    L = pkg.lib()
    lb = pkg._lib
    res = ctypes.POINTER(lb.GeodesicResult)()
    X = np.zeros((2, 6, 3), np.float32)
    M = np.ones((2, 6, 6), np.float64)
    Mbad = M.copy()
    Mbad[1, 2, 3] = -2.0
    Minf = M.astype(np.float32)
    Minf[0, 0, 5] = np.inf

    def call(**kw):
        a = lb.GeodesicArgs()
        a.x, a.dtype, a.L, a.N, a.D, a.n_neighbors, a.radius = X.ctypes.data, lb.TDA_F32, 2, 6, 3, 3, -1.0
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.tda_geodesic(ctypes.byref(a), ctypes.byref(res))
        assert not res  # no result on failure
        return rc, L.tda_last_error()

    assert L.tda_geodesic(None, ctypes.byref(res)) == INVALID and b"args is NULL" in L.tda_last_error()
    assert L.tda_geodesic(ctypes.byref(lb.GeodesicArgs()), None) == INVALID and b"out is NULL" in L.tda_last_error()
    mat = dict(x=M.ctypes.data, dtype=lb.TDA_F64, is_dist=1, D=6)
    for kw, code, msg in [
            (dict(x=None), INVALID, b"x is NULL"), (dict(L=0), INVALID, b"L must be"), (dict(N=0), INVALID, b"N must be"), (dict(D=0), INVALID, b"D must be"),
            (dict(dtype=5), INVALID, b"dtype"), (dict(n_neighbors=-2), INVALID, b"n_neighbors must be"),
            (dict(n_neighbors=0, radius=float("nan")), INVALID, b"radius is NaN"), (dict(radius=1.0), INVALID, b"not both"),
            (dict(n_neighbors=0), INVALID, b"give n_neighbors >= 1 or radius >= 0"),
            (dict(N=8193), UNSUPPORTED, b"N > 8192"), (dict(L=5, N=8192), UNSUPPORTED, b"2^28 values"),
            (dict(dtype=lb.TDA_F64), UNSUPPORTED, b"float64"),
            (dict(mat, x=Mbad.ctypes.data), INVALID, b"x[1][2][3] = -2.000000 is not finite and >= 0"),
            (dict(x=Minf.ctypes.data, is_dist=1, D=6), INVALID, b"x[0][0][5] = inf is not finite and >= 0")]:
        rc, err = call(**kw)
        assert rc == code and msg in err, (kw, rc, err)
    # the order: INVALID before UNSUPPORTED, the graph before the sizes, the matrix last
    assert b"n_neighbors" in call(n_neighbors=-1, N=8193, dtype=lb.TDA_F64)[1] and b"N > 8192" in call(N=8193, dtype=lb.TDA_F64)[1]
    assert b"not both" in call(**dict(mat, x=Mbad.ctypes.data, radius=2.0))[1]
    # valid arguments get as far as the device check: f32 points, f64 matrices, both graphs, graph_only, the limits
    for kw in (dict(), mat, dict(n_neighbors=0, radius=0.0), dict(n_neighbors=0, radius=float("inf"), graph_only=1), dict(n_neighbors=2 ** 31 - 1),
               dict(L=4, N=8192), dict(N=1)):
        rc, err = call(**kw)
        assert rc == NODEVICE and b"gfx950" in err, kw
    L.tda_geodesic_free(None)  # a no-op


# ---------------------------------------------------------------- 4. geo_ref against brute force and known answers
def brute_force(W):
    """Shortest lengths over all simple paths, float64 sums along each path, and the components."""
    n = W.shape[0]
    G = np.full((n, n), np.inf)
    for i in range(n):
        G[i, i] = 0.0
        for j in range(n):
            if i == j:
                continue
            mid = [v for v in range(n) if v not in (i, j)]
            for r in range(len(mid) + 1):
                for path in itertools.permutations(mid, r):
                    seq = (i, *path, j)
                    G[i, j] = min(G[i, j], sum(float(W[a, b]) for a, b in zip(seq, seq[1:])))
    return G


def cloud(n, d=3, seed=0):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def distances(X):
    X = np.asarray(X, dtype=np.float64)
    d = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)).astype(np.float32)
    return np.maximum(d, d.T)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7])
def test_ref_equals_brute_force(n):
    for seed, (k, radius) in itertools.product(range(2), ((1, None), (2, None), (n + 5, None), (None, 0.0), (None, 1.5), (None, INF))):
        dm = distances(cloud(n, 3, seed + 10 * n))
        if n >= 3:
            dm[0, 1] = dm[1, 0] = 0.0  # a duplicated point: an edge of weight 0 is an edge
        W, G, nc, ne = geo_ref.geodesic(dm, k, radius)
        B = brute_force(W)
        assert np.array_equal(np.isinf(G), np.isinf(B)) and np.allclose(G[np.isfinite(G)], B[np.isfinite(B)], rtol=1e-14, atol=0), (n, seed, k, radius)
        assert nc == sum(1 for i in range(n) if not np.isfinite(B[i, :i]).any())  # the header's count of components
        assert ne == np.count_nonzero(np.isfinite(W[np.triu_indices(n, 1)]))
        assert np.array_equal(W, W.T) and not W.diagonal().any()


def test_ref_on_a_path_and_a_ring():
    n = 9
    x = np.arange(n, dtype=np.float32)
    dm = np.abs(x[:, None] - x[None, :])
    W, G, nc, ne = geo_ref.geodesic(dm, n_neighbors=1)  # every point chooses a unit neighbour: with the union, the chain
    assert nc == 1 and ne == n - 1 and np.array_equal(G, dm.astype(np.float64))
    ang = 2 * np.pi * np.arange(12) / 12
    ring = distances(np.stack([np.cos(ang), np.sin(ang)], 1))
    W, G, nc, ne = geo_ref.geodesic(ring, radius=float(ring[0, 1]) * 1.001)
    assert nc == 1 and ne == 12
    hops = np.minimum(np.abs(np.arange(12)[:, None] - np.arange(12)[None, :]), 12 - np.abs(np.arange(12)[:, None] - np.arange(12)[None, :]))
    assert np.allclose(G, hops * float(ring[0, 1]), rtol=1e-6)  # the polygon's perimeter, not the chord


def two_clusters(m=6, gap=100.0, seed=3):
    a = cloud(m, 3, seed)
    b = cloud(m, 3, seed + 1) + np.float32(gap)
    return np.concatenate([a, b])


def test_ref_on_two_far_clusters():
    X = two_clusters()
    dm = distances(X)
    W, G, nc, ne = geo_ref.geodesic(dm, n_neighbors=3)
    assert nc == 2
    assert np.isinf(G[:6, 6:]).all() and np.isinf(G[6:, :6]).all() and np.isfinite(G[:6, :6]).all() and np.isfinite(G[6:, 6:]).all()
    assert geo_ref.geodesic(dm, radius=float(dm.max()))[2] == 1


def lattice4():
    i, j = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")
    return np.stack([i.ravel(), j.ravel()], 1).astype(np.float32)


def test_tie_rule_on_a_lattice():
    """On the 4 x 4 lattice every distance ties.  With k = 2 a corner takes both of its unit neighbours
    and an inner point the two LOWEST of its four (the one above, the one to the left).  With k = 1 every
    point takes the one above (the top row: the one to the left; point 0: point 1), so the union is a
    comb: every vertical edge and the top row."""
    dm = distances(lattice4())
    nb = geo_ref.neighbours(dm, 2)
    assert np.flatnonzero(nb[0]).tolist() == [1, 4] and np.flatnonzero(nb[5]).tolist() == [1, 4] and np.flatnonzero(nb[15]).tolist() == [11, 14]
    assert np.flatnonzero(nb[10]).tolist() == [6, 9] and not nb[10, 14] and nb[14, 10]
    assert geo_ref.graph(dm, 2)[1] == 24  # one end chose it: with the union, the whole lattice
    W, ne = geo_ref.graph(dm, 1)
    comb = np.zeros((16, 16), dtype=bool)
    for p in range(16):
        comb[p, p - 4 if p >= 4 else (p - 1 if p else 1)] = True
    assert ne == 15 and np.array_equal(np.isfinite(W) & ~np.eye(16, dtype=bool), comb | comb.T)
    assert geo_ref.closure(W)[0][12, 15] == 9.0 and geo_ref.closure(W)[1] == 1  # up a tooth, along the top, down another
    # the wrong definitions differ here, so the GPU test's lattice case tells them apart
    assert not np.array_equal(W, geo_ref.graph(dm, 1, highest_wins=True)[0])
    assert not np.array_equal(W, geo_ref.graph(dm, 1, directed=True)[0])
    assert np.array_equal(geo_ref.keys(dm) >> np.uint64(32), geo_ref.ord32(dm)) and geo_ref.ord32(np.float32(-0.0)) == geo_ref.ord32(np.float32(0.0))
    assert (np.diff(geo_ref.ord32(np.array([-np.inf, -1.0, -0.0, 1e-45, 1.0, np.inf], np.float32)).astype(np.int64)) > 0).all()


def test_bound_and_depth():
    assert geo_ref.depth(1) == 0 and geo_ref.depth(128) == 127 and geo_ref.depth(129) == 66 * 3 and geo_ref.depth(1025) == 66 * 17
    assert geo_ref.depth(65, lds_n=1) == 132 and abs(geo_ref.bound(1025) - 1122 * 2.0 ** -24) < 1e-8


# ---------------------------------------------------------------- 5. the Python entry
def test_python_entry_refuses_before_any_library_call(pkg, built_lib, monkeypatch):
    def no_lib():
        raise AssertionError("the library was called")

    monkeypatch.setattr(pkg._lib, "lib", no_lib)
    X = cloud(10)[None]
    for kw in (dict(), dict(n_neighbors=3, radius=1.0)):
        with pytest.raises(ValueError, match="exactly one"):
            pkg.geodesic_distances(X, **kw)
    for k in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="n_neighbors"):
            pkg.geodesic_distances(X, n_neighbors=k)
    for r in (-1.0, float("nan"), -INF):
        with pytest.raises(ValueError, match="radius"):
            pkg.geodesic_distances(X, radius=r)
    with pytest.raises(ValueError, match="parts"):
        pkg.geodesic_distances([X, X], n_neighbors=3)
    with pytest.raises(NotImplementedError, match="float64"):
        pkg.geodesic_distances(X.astype(np.float64), n_neighbors=3)
    with pytest.raises(ValueError, match="square"):
        pkg.geodesic_distances(np.zeros((1, 4, 5), np.float32), n_neighbors=3, distance_matrix=True)
    with pytest.raises(ValueError):
        pkg.geodesic_distances(X[0], n_neighbors=3)
    with pytest.raises(AssertionError, match="library was called"):
        pkg.geodesic_distances(X, radius=0.0)


def test_valid_python_calls_reach_the_device_check(pkg, built_lib):
    X = np.stack([cloud(10), cloud(10, seed=1)])
    for kw in (dict(n_neighbors=3), dict(radius=INF, graph_only=True), dict(n_neighbors=100)):
        with pytest.raises(RuntimeError, match="gfx950"):
            pkg.geodesic_distances(X, **kw)
    with pytest.raises(RuntimeError, match="gfx950"):
        pkg.geodesic_distances(np.ones((2, 10, 10), np.float64), n_neighbors=3, distance_matrix=True)
    M = np.ones((1, 4, 4), np.float32)
    M[0, 1, 2] = np.inf
    with pytest.raises(ValueError, match="NaN or infinity"):
        pkg.geodesic_distances(M, n_neighbors=2, distance_matrix=True)  # host matrices must be finite
    M[0, 1, 2] = -1.0
    with pytest.raises(ValueError, match="not finite and >= 0"):
        pkg.geodesic_distances(M, n_neighbors=2, distance_matrix=True)  # and non-negative: the library's own check


def test_filled():
    g = __import__("importlib").import_module("tda-multimodal_amd").GeodesicDistances()
    g.dist = np.array([[[0, np.inf], [np.inf, 0]]], np.float32)
    f = g.filled(7.5)
    assert f.tolist() == [[[0, 7.5], [7.5, 0]]] and np.isinf(g.dist[0, 0, 1]) and f.dtype == np.float32
    for bad in (INF, float("nan")):
        with pytest.raises(ValueError, match="finite"):
            g.filled(bad)
