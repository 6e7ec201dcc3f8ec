"""CPU tests of the subsample H0 entry and the persistent-homology dimension (no device): the host
plan (csrc/sh0_plan.h) against a Python restatement and every refusal with its code, its message and
its place in the order of checks; the same refusals through tda_subsample_h0 itself, before the
device check; the numpy restatement (sh0_ref.py) pinned to the oracle; the estimator on clouds of
known dimension through sh0_ref alone; and the Python entries' own checks.

tests/sh0_plan_main.cpp includes only sh0_plan.h; it is compiled with g++ under the address and
undefined-behaviour sanitizers and run as a program of its own, one case per line."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import sh0_ref
import side_plan_ref as spr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tda-multimodal_amd", "csrc")
INVALID, UNSUPPORTED, NODEVICE = -1, -2, -5
F32, F64 = spr.F32, spr.F64
GIB4 = 4 << 30
MAX_OUT = 1 << 27


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sh0_plan") / "sh0_plan")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "sh0_plan_main.cpp")], check=True)
    return exe


def run(exe, lines):
    """-> per line ("err", code, message) or ("ok", {field: value})"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("TDA_")}
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


def arr(t):
    """A table: (0,) NULL, (1, ...) present, (2, values ...) -> the mode, the count and the values."""
    return t if t[0] != 2 else (2, len(t) - 1, *t[1:])


def line_of(c):
    xs = (c["args"], c["cap"], c["x"], c["dtype"], c["dev"], c["L"], c["N"], c["D"], c["is_dist"], c["B"], c["m"], c["per_layer"], c["deaths"],
          c["alpha"], *arr(c["idx"]), *arr(c["sizes"]))
    return " ".join(str(x) for x in xs)


BASE = dict(args=1, cap=GIB4, x=1, dtype=F32, dev=0, L=3, N=65, D=3, is_dist=0, B=4, m=5, per_layer=0, deaths=0, alpha=1.0, idx=(1,), sizes=(1, 5))
F64_POINTS = "subsample H0 of float64 point clouds is not supported (pass float32 points or a distance matrix)"
MANY = "subsample H0: more than 2^27 subsamples (L * B) in one call is not supported: split B over several calls"
MANY_DEATHS = "subsample H0: more than 2^27 deaths (L * B * (m - 1)) in one call is not supported: split B over several calls"


# ---------------------------------------------------------------- the restatement
def plan_ref(L, N, D, dtype, is_dist, host_in, B, m, per_layer_idx, want_deaths, alpha=1.0, cap=GIB4):
    """sh0_plan for valid tables (zeros, sizes in range): the refusal by size, or every field."""
    if N > 8192:
        return "err", UNSUPPORTED, "subsample H0: N > 8192 is not supported"
    if m > 8192:
        return "err", UNSUPPORTED, "subsample H0: m > 8192 is not supported"
    if L * B > MAX_OUT:
        return "err", UNSUPPORTED, MANY
    if want_deaths and L * B * (m - 1) > MAX_OUT:
        return "err", UNSUPPORTED, MANY_DEATHS
    idx_layer = B * m * 4 if per_layer_idx else 0
    deaths_layer = B * (m - 1) * 4 if want_deaths else 0
    p, parts = spr.sq_dist(L, N, D, dtype, is_dist, host_in, spr.align(idx_layer) + spr.align(deaths_layer), cap)
    cv = spr.Carve()
    p.update(L=L, N=N, B=B, m=m, is_dist=int(is_dist), per_layer_idx=int(per_layer_idx), want_deaths=int(want_deaths),
             resident=int(N <= 128 and m <= 128), mode=0 if alpha == 1 else 1 if alpha == 2 else 2, Bc=min(B, 65535),
             idx_lstride=B * m if per_layer_idx else 0, d_lstride=B * (m - 1), lds=128 + 6 * m,
             o_E=cv.take(L * B * 8), o_sz=cv.take(B * 4), o_idx=cv.take((p["Lc"] if per_layer_idx else 1) * B * m * 4))
    p["o_deaths"] = cv.take(p["Lc"] * deaths_layer)
    spr.carve_sq(cv, p, parts)
    p["total"] = cv.o
    return "ok", p


def cap_for(Lc, **kw):
    """The smallest cap under which the plan serves Lc layers per chunk (the GPU tests take it from here)."""
    return Lc * plan_ref(cap=GIB4, **kw)[1]["per_layer"]


# ---------------------------------------------------------------- 1. the plan against the restatement
GRID_L = (1, 3, 70000)
GRID_N = (1, 2, 128, 129, 8192, 8193)
GRID_M = (1, 128, 129, 8192, 8193)
GRID_B = (1, 65535, 65536)


def test_plan_grid(plan_exe):
    """The whole grid in both table forms, with and without deaths, under the default cap, a cap of one
    layer (Lc = 1) and of two.  The plan reads the first sizes[b] entries of every row before it
    weighs L * B, so a table per layer is given where it has at most 2^27 rows (the others are refused
    by size: test_refusals pins that with a small table)."""
    cases = []
    for L, N, m, B, per_layer, deaths in itertools.product(GRID_L, GRID_N, GRID_M, GRID_B, (0, 1), (0, 1)):
        if per_layer and L * B > MAX_OUT:
            continue
        kw = dict(L=L, N=N, D=3, dtype=F32, is_dist=False, host_in=True, B=B, m=m, per_layer_idx=per_layer, want_deaths=deaths)
        first = plan_ref(**kw)
        caps = (GIB4,) if first[0] == "err" else (GIB4, first[1]["per_layer"], 2 * first[1]["per_layer"], 1)
        cases += [(kw, cap) for cap in caps]
    # the other input forms at the path border: device input, matrices, f64 matrices, the matrix-core distances
    for (N, m), (D, dtype, is_dist, host_in), alpha in itertools.product(((128, 128), (129, 128), (128, 129)),
                                                                       ((64, F32, 0, 1), (3, F32, 0, 0), (3, F32, 1, 1), (3, F64, 1, 0)), (1.0, 2.0, 0.5)):
        cases.append((dict(L=3, N=N, D=D, dtype=dtype, is_dist=bool(is_dist), host_in=bool(host_in), B=7, m=m, per_layer_idx=1, want_deaths=1,
                           alpha=alpha), GIB4))
    lines = [line_of(dict(BASE, cap=cap, dtype=kw["dtype"], dev=1 - kw["host_in"], L=kw["L"], N=kw["N"], D=kw["D"], is_dist=int(kw["is_dist"]),
                          B=kw["B"], m=kw["m"], per_layer=kw["per_layer_idx"], deaths=kw["want_deaths"], alpha=kw.get("alpha", 1.0),
                          sizes=(1, 1))) for kw, cap in cases]
    seen, paths = set(), set()
    for (kw, cap), got in zip(cases, run(plan_exe, lines)):
        want = plan_ref(cap=cap, **kw)
        assert got == want, (kw, cap)
        if got[0] == "err":
            continue
        p, L, N, B, m = got[1], kw["L"], kw["N"], kw["B"], kw["m"]
        Lc = p["Lc"]
        assert 1 <= Lc <= min(L, 65535) and (Lc == L or Lc == 65535 or (Lc + 1) * p["per_layer"] > cap) and (Lc == 1 or Lc * p["per_layer"] <= cap)
        assert 1 <= p["Bc"] <= 65535 and (p["Bc"] == B or B > 65535) and p["lds"] <= 64 * 1024
        assert p["resident"] == int(N <= 128 and m <= 128)
        arrays = [("o_E", L * B * 8), ("o_sz", B * 4), ("o_idx", (Lc if kw["per_layer_idx"] else 1) * B * m * 4),
                  ("o_deaths", Lc * B * (m - 1) * 4 if kw["want_deaths"] else 0), ("o_x", Lc * p["x_layer"] if kw["host_in"] else 0),
                  ("o_dm", Lc * N * N * 4), ("o_rm", Lc * N * 4)]
        end = 0
        for name, nbytes in arrays:
            assert p[name] % 256 == 0 and p[name] >= end, name  # aligned, increasing, not overlapping
            end = p[name] + nbytes
        assert p["total"] % 256 == 0 and p["total"] >= end
        if Lc > 1:  # a chunk's own arrays stay within Lc layers' share of the cap
            assert p["total"] - p["o_idx"] <= Lc * p["per_layer"] + spr.align(B * m * 4)
        seen.add(min(Lc, 2) if Lc < L else "all")
        paths.add((p["resident"], p["mode"]))
    assert seen == {1, 2, "all"} and paths == {(r, k) for r in (0, 1) for k in (0, 1, 2)}


# ---------------------------------------------------------------- 2. the refusals, in the order of the checks
def test_refusals(plan_exe):
    """Case i has wrong what refusal i names and everything the later ones name: it must come back with
    refusal i, so no later check runs before an earlier one.  Then each alone."""
    refusals = [
        (dict(args=0), INVALID, "args is NULL"), (dict(x=0), INVALID, "x is NULL"), (dict(idx=(0,)), INVALID, "idx is NULL"),
        (dict(sizes=(0,)), INVALID, "sizes is NULL"), (dict(L=0), INVALID, "L must be >= 1"), (dict(N=0), INVALID, "N must be >= 1"),
        (dict(D=0), INVALID, "D must be >= 1"), (dict(dtype=-1), INVALID, "dtype must be TDA_F32 or TDA_F64"),
        (dict(B=0), INVALID, "B must be >= 1"), (dict(m=0), INVALID, "m must be >= 1"),
        (dict(sizes=(1, 0)), INVALID, "sizes[0] = 0 is outside [1, m = 5]"),
        (dict(idx=(2, 0, 0, 65, *([0] * 17))), INVALID, "idx[2] = 65 is outside [0, N = 65)"),
        (dict(alpha="nan"), INVALID, "alpha must be finite and > 0"),
        (dict(N=8193), UNSUPPORTED, "subsample H0: N > 8192 is not supported"),
        (dict(m=8193), UNSUPPORTED, "subsample H0: m > 8192 is not supported"),
        (dict(L=1 << 20, B=129), UNSUPPORTED, MANY),
        (dict(L=1 << 12, B=1 << 12, m=10, deaths=1), UNSUPPORTED, MANY_DEATHS),
        (dict(dtype=F64), UNSUPPORTED, F64_POINTS)]
    lines = []
    for i in range(len(refusals)):
        c = dict(BASE)
        for wrong, _, _ in reversed(refusals[i:]):
            c.update(wrong)
        if i >= 10:  # the tables of the sizes the later refusals set, wrong where this one says
            c["sizes"] = (1, 0) if i == 10 else (1, min(c["m"], 5))
            c["idx"] = (2, 0, 0, c["N"], *([0] * 17)) if i == 11 else (1,)  # the plan stops at the first bad index
        lines.append(line_of(c))
    lines += [line_of(dict(BASE, **wrong)) for wrong, _, _ in refusals]
    got = run(plan_exe, lines + [line_of(BASE)])
    assert got[-1][0] == "ok", got[-1]
    want = [("err", code, msg) for _, code, msg in refusals]
    want_chain = list(want)
    want_chain[10] = ("err", INVALID, "sizes[0] = 0 is outside [1, m = 8193]")  # m as the later refusals set it
    want_chain[11] = ("err", INVALID, "idx[2] = 8193 is outside [0, N = 8193)")
    assert got[:len(refusals)] == want_chain
    assert got[len(refusals):-1] == want


def test_refusal_edges(plan_exe):
    table = [0] * 20
    cases = [
        (dict(sizes=(2, 5, 5, 6, 5)), ("err", INVALID, "sizes[2] = 6 is outside [1, m = 5]")),
        (dict(sizes=(2, 5, -1, 5, 5)), ("err", INVALID, "sizes[1] = -1 is outside [1, m = 5]")),
        # an index is weighed only among the first sizes[b] entries of its row
        (dict(idx=(2, *table[:13], 65, *table[14:]), sizes=(2, 5, 5, 3, 5)), "ok"),
        (dict(idx=(2, *table[:13], 65, *table[14:]), sizes=(2, 5, 5, 4, 5)), ("err", INVALID, "idx[13] = 65 is outside [0, N = 65)")),
        (dict(idx=(2, *table[:10], -1, *table[11:])), ("err", INVALID, "idx[10] = -1 is outside [0, N = 65)")),
        (dict(idx=(2, *table[:4], -7, *table[5:]), sizes=(1, 4)), "ok"),
        # a table per layer is scanned whole, with the shared sizes
        (dict(per_layer=1, idx=(2, *([0] * 45), 65, *([0] * 14))), ("err", INVALID, "idx[45] = 65 is outside [0, N = 65)")),
        (dict(per_layer=0, idx=(2, *([0] * 45), 65, *([0] * 14))), "ok"),
        (dict(alpha=0.0), ("err", INVALID, "alpha must be finite and > 0")), (dict(alpha=-1.0), ("err", INVALID, "alpha must be finite and > 0")),
        (dict(alpha="inf"), ("err", INVALID, "alpha must be finite and > 0")), (dict(alpha=1e-300), "ok"), (dict(alpha=3.7), "ok"),
        # the limits themselves
        (dict(N=8192, m=8192, B=1, sizes=(1, 8192)), "ok"), (dict(L=1 << 20, B=128, m=1, sizes=(1, 1)), "ok"),
        (dict(L=1 << 12, B=1 << 12, m=9, deaths=1, sizes=(1, 1)), "ok"), (dict(L=1 << 12, B=1 << 12, m=10, deaths=0, sizes=(1, 1)), "ok"),
        (dict(dtype=F64, is_dist=1, D=0), "ok"),
    ]
    got = run(plan_exe, [line_of(dict(BASE, **wrong)) for wrong, _ in cases])
    for (wrong, want), g in zip(cases, got):
        assert (g[0] if want == "ok" else g) == want, (wrong, g)


# ---------------------------------------------------------------- 3. the boundary of the library
A_FIELDS = ["x", "dtype", "x_on_device", "L", "N", "D", "is_dist", "device", "stream", "B", "m", "idx_per_layer", "idx", "sizes", "alpha", "want_deaths"]
R_FIELDS = ["L", "N", "B", "m", "E", "deaths", "device", "device_ms"]


def test_structs_match_header_layout(pkg, tmp_path):
    lb = pkg._lib
    fmt = " ".join(["%zu"] * (2 + len(A_FIELDS) + len(R_FIELDS)))
    args = ", ".join(["sizeof(tda_subsample_h0_args)"] + [f"offsetof(tda_subsample_h0_args, {f})" for f in A_FIELDS]
                     + ["sizeof(tda_subsample_h0_result)"] + [f"offsetof(tda_subsample_h0_result, {f})" for f in R_FIELDS])
    src = tmp_path / "sh0layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tda_rips.h"\n'
                   f'int main(void){{printf("{fmt}\\n", {args}); return 0;}}\n')
    exe = tmp_path / "sh0layout"
    subprocess.run(["gcc", "-I", lb.INCLUDE, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    A, R = lb.SubsampleH0Args, lb.SubsampleH0Result
    assert got == ([ctypes.sizeof(A)] + [getattr(A, f).offset for f in A_FIELDS] + [ctypes.sizeof(R)] + [getattr(R, f).offset for f in R_FIELDS])


def test_constants_match_sources(pkg):
    import re

    lb = pkg._lib
    hdr = open(os.path.join(lb.INCLUDE, "tda_rips.h")).read()
    shift = re.search(r"#define TDA_SH0_MAX_OUT \((\d+)ll << (\d+)\)", hdr)
    assert shift and int(shift.group(1)) << int(shift.group(2)) == lb.TDA_SH0_MAX_OUT == MAX_OUT
    ker = open(os.path.join(lb.CSRC, "sh0_kernels.h")).read()
    assert "constexpr int kSh0LdsN = kRsLdsN;" in ker and lb.TDA_SH0_LDS_N == lb.TDA_RS_LDS_N
    assert int(re.search(r"constexpr int kSh0LdsM = (\d+);", ker).group(1)) == lb.TDA_SH0_LDS_M == 128  # two positions per lane of a wave
    assert int(re.search(r"constexpr int kSh0Head = (\d+);", ker).group(1)) == 128
    plan = open(os.path.join(lb.CSRC, "sh0_plan.h")).read()
    for name, value in (("kSideSh0LdsN", lb.TDA_SH0_LDS_N), ("kSideSh0LdsM", lb.TDA_SH0_LDS_M), ("kSideSh0PerBlock", 16)):
        assert int(re.search(rf"constexpr int {name} = (\d+);", plan).group(1)) == value


def test_symbols_exported_and_abi_version_unchanged(pkg, built_lib):
    lib = ctypes.CDLL(built_lib)
    assert pkg.SUBSAMPLE_H0_EXPORTS == ("tda_subsample_h0", "tda_subsample_h0_free")
    assert all(hasattr(lib, s) for s in pkg.SUBSAMPLE_H0_EXPORTS) and not set(pkg.SUBSAMPLE_H0_EXPORTS) & set(pkg.EXPORTS)
    hdr = open(os.path.join(pkg._lib.INCLUDE, "tda_rips.h")).read()
    assert all(f" {s}(" in hdr for s in pkg.SUBSAMPLE_H0_EXPORTS)
    assert pkg.lib().tda_version() == 8  # symbols added only: no existing struct changed


def test_library_refuses_before_the_device_check(pkg, built_lib):
    """Every refusal of the plan through tda_subsample_h0 itself: they come before need_device, so
    they come back here, where there is no device; a valid call gets as far as TDA_E_NODEVICE."""
    L = pkg.lib()
    lb = pkg._lib
    res = ctypes.POINTER(lb.SubsampleH0Result)()
    X = np.zeros((2, 6, 3), np.float32)
    idx = np.array([[0, 1, 5], [2, 2, 3]], np.int32)  # (B = 2, m = 3)
    sizes = np.array([3, 2], np.int32)
    big = np.zeros(8193, np.int32)
    ones = np.ones(129, np.int32)
    zeros = np.zeros(129 * 4, np.int32)
    s34, s02, s1, s33 = (np.array(v, np.int32) for v in ([3, 4], [0, 2], [1], [3, 3]))  # kept alive: the calls take addresses

    def call(**kw):
        a = lb.SubsampleH0Args()
        a.x, a.dtype, a.L, a.N, a.D, a.B, a.m, a.idx, a.sizes, a.alpha = X.ctypes.data, lb.TDA_F32, 2, 6, 3, 2, 3, idx.ctypes.data, sizes.ctypes.data, 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.tda_subsample_h0(ctypes.byref(a), ctypes.byref(res))
        assert not res  # no result on failure
        return rc, L.tda_last_error()

    assert L.tda_subsample_h0(None, ctypes.byref(res)) == INVALID and b"args is NULL" in L.tda_last_error()
    assert L.tda_subsample_h0(ctypes.byref(lb.SubsampleH0Args()), None) == INVALID and b"out is NULL" in L.tda_last_error()
    for kw, code, msg in [
            (dict(x=None), INVALID, b"x is NULL"), (dict(idx=None), INVALID, b"idx is NULL"), (dict(sizes=None), INVALID, b"sizes is NULL"),
            (dict(L=0), INVALID, b"L must be"), (dict(N=0), INVALID, b"N must be"), (dict(D=0), INVALID, b"D must be"), (dict(dtype=5), INVALID, b"dtype"),
            (dict(B=0), INVALID, b"B must be"), (dict(B=-3), INVALID, b"B must be"), (dict(m=0), INVALID, b"m must be"),
            (dict(sizes=s34.ctypes.data), INVALID, b"sizes[1] = 4 is outside [1, m = 3]"),
            (dict(sizes=s02.ctypes.data), INVALID, b"sizes[0] = 0 is outside [1, m = 3]"),
            (dict(N=5), INVALID, b"idx[2] = 5 is outside [0, N = 5)"),
            (dict(alpha=0.0), INVALID, b"alpha must be finite"), (dict(alpha=float("nan")), INVALID, b"alpha must be finite"),
            (dict(alpha=float("inf")), INVALID, b"alpha must be finite"), (dict(alpha=-2.0), INVALID, b"alpha must be finite"),
            (dict(N=8193), UNSUPPORTED, b"N > 8192"),
            (dict(idx=big.ctypes.data, B=1, m=8193, sizes=s1.ctypes.data), UNSUPPORTED, b"m > 8192"),
            (dict(idx=zeros.ctypes.data, L=2 ** 20, B=129, m=4, sizes=ones.ctypes.data), UNSUPPORTED, b"2^27 subsamples"),  # x is not read
            (dict(idx=zeros.ctypes.data, L=2 ** 20, B=64, m=4, sizes=ones.ctypes.data, want_deaths=1), UNSUPPORTED, b"2^27 deaths"),
            (dict(idx=zeros.ctypes.data, L=2 ** 20, B=64, m=4, sizes=ones.ctypes.data), NODEVICE, b"gfx950"),  # without them the same sizes pass
            (dict(dtype=lb.TDA_F64), UNSUPPORTED, b"float64")]:
        rc, err = call(**kw)
        assert rc == code and msg in err, (kw, rc, err)
    # entries past sizes[b] are not read: row 1 holds a bad index at position 2, sizes[1] = 2
    bad_tail = np.array([[0, 1, 5], [2, 2, 99]], np.int32)
    assert call(idx=bad_tail.ctypes.data)[0] == NODEVICE
    assert call(idx=bad_tail.ctypes.data, sizes=s33.ctypes.data)[0] == INVALID
    # the order: INVALID before UNSUPPORTED, sizes before the table, the table before alpha
    assert b"sizes[0]" in call(sizes=s02.ctypes.data, N=5, alpha=0.0, dtype=lb.TDA_F64)[1]
    assert b"idx[2]" in call(N=5, alpha=0.0, dtype=lb.TDA_F64)[1] and b"alpha" in call(alpha=0.0, dtype=lb.TDA_F64)[1]
    # valid arguments get as far as the device check: f32 points, f64 matrices, a table per layer, the deaths, another alpha
    rc, err = call()
    assert rc == NODEVICE and b"gfx950" in err
    M = np.zeros((2, 6, 6), np.float64)
    per = np.stack([idx, idx])
    assert call(x=M.ctypes.data, dtype=lb.TDA_F64, is_dist=1, D=6)[0] == NODEVICE
    assert call(idx=per.ctypes.data, idx_per_layer=1, want_deaths=1, alpha=0.5)[0] == NODEVICE
    assert call(N=8192)[0] == NODEVICE
    L.tda_subsample_h0_free(None)  # a no-op


# ---------------------------------------------------------------- 4. sh0_ref pinned to the oracle
def lattice():
    i, j = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")
    return np.stack([i.ravel(), j.ravel()], 1).astype(np.float32)


def duplicated():
    base = np.random.default_rng(5).standard_normal((20, 3)).astype(np.float32)
    return np.concatenate([base, base])  # every point twice: 20 zero distances off the diagonal


def test_ref_equals_the_oracle_h0(oracle, ref_clouds):
    """The sorted deaths of the full-cloud subsample are the finite H0 deaths of the oracle, as f32 bits,
    on the 32 reference clouds and on the tie-heavy ones; E at alpha = 1 is the sequential sum."""
    clouds = [np.ascontiguousarray(ref_clouds[l], dtype=np.float32) for l in range(32)] + [lattice(), duplicated()]
    for k, X in enumerate(clouds):
        dm = oracle.distances(X)
        n = len(X)
        want = np.asarray(oracle.rips(X, maxdim=0)["dgms"][0], dtype=np.float64)[:, 1]
        want = np.sort(want[np.isfinite(want)]).astype(np.float32)
        for order in (np.arange(n), np.arange(n)[::-1], np.random.default_rng(k).permutation(n)):
            E, d = sh0_ref.prim(dm, order, 1.0)
            assert d.dtype == np.float32 and len(d) == n - 1
            # ripser (and the oracle) drop the bars of zero length: a duplicate's death at 0 is a death here, no bar there
            assert np.sort(d[d > 0]).tobytes() == want.tobytes() and np.count_nonzero(d == 0) == (20 if k == 33 else 0), k
            acc = 0.0
            for w in d:
                acc += float(w)
            assert E == acc
            E2, d2 = sh0_ref.prim(dm, order, 2.0)
            assert d2.tobytes() == d.tobytes() and E2 == sum_in_order(float(w) * float(w) for w in d)
    dm = oracle.distances(lattice())
    assert set(sh0_ref.prim(dm, np.arange(36))[1].tolist()) == {1.0}  # the lattice's tree: 35 unit edges
    E, d = sh0_ref.prim(oracle.distances(duplicated()), np.arange(40))
    assert np.count_nonzero(d == 0.0) == 20  # every duplicate joins at distance 0
    E1, d1 = sh0_ref.prim(dm, [7])
    assert E1 == 0.0 and len(d1) == 0  # one position: no deaths
    E3, d3 = sh0_ref.prim(dm, [3, 3, 3])
    assert E3 == 0.0 and d3.tolist() == [0.0, 0.0]


def sum_in_order(xs):
    acc = 0.0
    for x in xs:
        acc += x
    return acc


def test_ref_tie_rule_is_the_lowest_position():
    dm = np.array([[0, 1, 1, 1], [1, 0, 1, 1], [1, 1, 0, 1], [1, 1, 1, 0]], np.float32) * np.float32(0.1)
    dm[0, 3] = dm[3, 0] = np.float32(0.05)
    # from position 0: position 3 first (0.05), then the tie of 1 and 2 at 0.1 goes to position 1
    E, d = sh0_ref.prim(dm, [0, 1, 2, 3])
    assert d.tolist() == [np.float32(0.05), np.float32(0.1), np.float32(0.1)]
    assert E == (float(np.float32(0.05)) + float(np.float32(0.1))) + float(np.float32(0.1))


# ---------------------------------------------------------------- 5. the estimator on known shapes
@pytest.mark.parametrize("d,lo,hi", [(1, 0.9, 1.15), (2, 1.7, 2.3), (3, 2.5, 3.3)])
def test_estimator_on_uniform_cubes(d, lo, hi):
    """256 uniform points of the unit d-cube, default sizes, 8 trials, alpha = 1, through sh0_ref alone.
    Sanity bands on the estimator, not accuracy claims (the restatement gave 1.012-1.030, 1.928-1.966
    and 2.794-2.934)."""
    for s in range(4):
        X = np.random.default_rng(s).random((256, d)).astype(np.float32)
        (dim, slope, _), E, idx, sz = sh0_ref.ph_dimension(sh0_ref.distances(X))
        assert lo <= dim <= hi, (d, s, dim)
        assert 0.0 <= slope < 1.0 and E.shape == (1, 80) and sorted(set(sz.tolist())) == sh0_ref.default_sizes(256).tolist()


# ---------------------------------------------------------------- 6. the Python entries
def test_subsample_indices(pkg):
    idx, sz = pkg.subsample_indices(36, [9, 36, 18], 3, seed=4)
    assert idx.dtype == np.int32 and sz.dtype == np.int32 and idx.shape == (9, 36) and idx.flags.c_contiguous
    assert sz.tolist() == [9, 9, 9, 36, 36, 36, 18, 18, 18]  # sizes in the given order, then trials
    again = pkg.subsample_indices(36, [9, 36, 18], 3, seed=4)
    assert idx.tobytes() == again[0].tobytes() and sz.tobytes() == again[1].tobytes()
    assert idx.tobytes() != pkg.subsample_indices(36, [9, 36, 18], 3, seed=5)[0].tobytes()
    for b, n in enumerate(sz.tolist()):
        assert len(set(idx[b, :n].tolist())) == n and idx[b, :n].min() >= 0 and idx[b, :n].max() < 36  # without repetition
        assert not idx[b, n:].any()  # padded with 0
    assert sorted(idx[3].tolist()) == list(range(36))
    # the draw order of the contract, restated
    ridx, rsz = sh0_ref.subsample_indices(36, [9, 36, 18], 3, seed=4)
    assert idx.tobytes() == ridx.tobytes() and sz.tobytes() == rsz.tobytes()
    rng = np.random.default_rng(4)
    assert idx[0, :9].tolist() == rng.permutation(36)[:9].tolist() and idx[1, :9].tolist() == rng.permutation(36)[:9].tolist()
    for bad in (dict(N=0, sizes=[1], n_trials=1), dict(N=4, sizes=[], n_trials=1), dict(N=4, sizes=[5], n_trials=1), dict(N=4, sizes=[0], n_trials=1),
                dict(N=4, sizes=[2], n_trials=0), dict(N=4, sizes=[2.5], n_trials=1)):
        with pytest.raises(ValueError):
            pkg.subsample_indices(**bad)


def test_default_sizes(pkg):
    for N in (256, 36, 324, 2048, 9, 8):
        assert pkg.phdim.default_sizes(N).tolist() == sh0_ref.default_sizes(N).tolist()
    assert pkg.phdim.default_sizes(256).tolist() == [64, 85, 107, 128, 149, 171, 192, 213, 235, 256]
    assert pkg.phdim.default_sizes(2).tolist() == [2] and pkg.phdim.default_sizes(4).tolist() == [2, 3, 4] and not len(pkg.phdim.default_sizes(1))


def test_python_entries_refuse_before_any_library_call(pkg, built_lib, monkeypatch):
    def no_lib():
        raise AssertionError("the library was called")

    monkeypatch.setattr(pkg._lib, "lib", no_lib)
    X = np.random.default_rng(0).standard_normal((2, 10, 3)).astype(np.float32)
    idx, sz = pkg.subsample_indices(10, [5, 10], 2)
    for al in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            pkg.ph_dimension(X, alpha=al)
        with pytest.raises(ValueError, match="alpha"):
            pkg.h0_subsamples(X, idx, sz, alpha=al)
    for nt in (0, -1, 2.5, None):
        with pytest.raises(ValueError, match="n_trials"):
            pkg.ph_dimension(X, n_trials=nt)
    with pytest.raises(ValueError, match="two distinct"):
        pkg.ph_dimension(X, sizes=[5, 5])
    with pytest.raises(ValueError, match="two distinct"):
        pkg.ph_dimension(X[:, :2])  # N = 2: the default sizes are [2]
    with pytest.raises(ValueError, match="two distinct"):
        pkg.ph_dimension(X, idx=idx, sizes=np.full(4, 5))
    with pytest.raises(ValueError, match="sizes"):
        pkg.ph_dimension(X, sizes=[5, 11])  # above N
    entries = (lambda Y, t, s=None, **kw: pkg.ph_dimension(Y, idx=t, sizes=s, **kw), pkg.h0_subsamples)
    bad_idx = (idx[0], idx[None, None], np.zeros((0, 3), np.int32), np.stack([idx] * 3), idx.astype(np.float32), idx + 10, idx - 1)
    for fn in entries:
        for t in bad_idx:
            with pytest.raises(ValueError, match="idx"):
                fn(X, t)
        for s in (np.array([5, 5, 10]), np.array([5, 5, 10, 11]), np.array([0, 5, 10, 10]), np.array([5.0, 5.0, 10.0, 10.0]), sz[None]):
            with pytest.raises(ValueError, match="sizes"):
                fn(X, idx, s)
        with pytest.raises(ValueError, match="parts"):
            fn([X, X], idx, sz)
        with pytest.raises(NotImplementedError, match="float64"):
            fn(X.astype(np.float64), idx, sz)
        with pytest.raises(ValueError, match="square"):
            fn(np.zeros((1, 4, 5), np.float32), np.zeros((2, 3), np.int32), np.array([2, 3]), distance_matrix=True)
        with pytest.raises(ValueError):
            fn(X[0], idx, sz)
    # what is never read is not weighed: a bad index past sizes[b] passes the table check (and reaches the library)
    tail = idx.copy()
    tail[0, 7] = 99
    with pytest.raises(AssertionError, match="library was called"):
        pkg.h0_subsamples(X, tail, sz)


def test_valid_python_calls_reach_the_device_check(pkg, built_lib):
    X = np.random.default_rng(0).standard_normal((2, 10, 3)).astype(np.float32)
    idx, sz = pkg.subsample_indices(10, [5, 10], 2)
    with pytest.raises(RuntimeError, match="gfx950"):
        pkg.ph_dimension(X)
    with pytest.raises(RuntimeError, match="gfx950"):
        pkg.h0_subsamples(X, idx, sz, deaths=True)
    with pytest.raises(RuntimeError, match="gfx950"):
        pkg.h0_subsamples(np.zeros((2, 10, 10), np.float64), np.stack([idx, idx]).astype(np.int64), sz, alpha=0.5, distance_matrix=True)
    M = np.zeros((1, 4, 4), np.float32)
    M[0, 1, 2] = np.inf
    with pytest.raises(ValueError, match="NaN or infinity"):
        pkg.h0_subsamples(M, np.zeros((1, 4), np.int32), distance_matrix=True)  # host matrices must be finite
