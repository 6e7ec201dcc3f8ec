"""CPU tests of the permutation test's boundary (no device): the ctypes mirrors of tda_perm_args /
tda_perm_result have the header's layout, the constants agree with the sources, every bad argument
comes back with its documented code and no result before any device work, the label tables and the
p-value rule are what hypothesis.py documents, the Python entries refuse what they do not support
before any library call, and the numpy restatement stays within the documented bound of the plain
formula."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import perm_ref as pr


def test_perm_structs_match_header_layout(pkg, tmp_path):
    lb = pkg._lib
    a_fields = ["w", "obs", "lab", "S", "B", "G", "device", "reserved"]
    r_fields = ["S", "B", "t_obs", "null", "count", "pvalue", "device", "device_ms"]
    fmt = " ".join(["%zu"] * (2 + len(a_fields) + len(r_fields)))
    args = ", ".join(["sizeof(tda_perm_args)"] + [f"offsetof(tda_perm_args, {f})" for f in a_fields]
                     + ["sizeof(tda_perm_result)"] + [f"offsetof(tda_perm_result, {f})" for f in r_fields])
    src = tmp_path / "playout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tda_rips.h"\n'
                   f'int main(void){{printf("{fmt}\\n", {args}); return 0;}}\n')
    exe = tmp_path / "playout"
    subprocess.run(["gcc", "-I", lb.INCLUDE, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    A, R = lb.PermArgs, lb.PermResult
    assert got == ([ctypes.sizeof(A)] + [getattr(A, f).offset for f in a_fields]
                   + [ctypes.sizeof(R)] + [getattr(R, f).offset for f in r_fields])


def test_perm_constants_match_sources(pkg):
    lb = pkg._lib
    hdr = open(os.path.join(lb.INCLUDE, "tda_rips.h")).read()
    assert int(re.search(r"#define TDA_PERM_MAX_S (\d+)", hdr).group(1)) == lb.TDA_PERM_MAX_S == 2048
    assert int(re.search(r"#define TDA_PERM_MAX_GROUPS (\d+)", hdr).group(1)) == lb.TDA_PERM_MAX_GROUPS == 64
    shift = re.search(r"#define TDA_PERM_MAX_TABLE \((\d+)ll << (\d+)\)", hdr)
    assert int(shift.group(1)) << int(shift.group(2)) == lb.TDA_PERM_MAX_TABLE == 2 ** 27
    ker = open(os.path.join(lb.CSRC, "perm_kernels.h")).read()
    host = open(os.path.join(lb.CSRC, "perm_host.h")).read()
    lds_s = int(re.search(r"constexpr int kPermLdsS = (\d+);", ker).group(1))
    assert lds_s == lb.TDA_PERM_LDS_S
    assert int(re.search(r"constexpr int kPermMaxS = (\d+);", ker).group(1)) == lb.TDA_PERM_MAX_S
    assert int(re.search(r"constexpr int kPermR = (\d+);", ker).group(1)) == lb.TDA_PERM_ROWS
    m = re.search(r"constexpr size_t kPermLdsBytes = (\d+) \* 1024;", host)
    lds_bytes = int(m.group(1)) * 1024
    assert lds_s ** 2 * 8 <= lds_bytes < (lds_s + 1) ** 2 * 8  # the largest tile in the LDS the host asks for
    assert lds_bytes <= 160 * 1024  # of a CU's 160 KiB
    # a launch's rows keep the tiled grid within 65535
    plan = open(os.path.join(lb.CSRC, "side_plan.h")).read()  # the chunk is part of the host plan; perm_host.h ties kSidePermR to kPermR
    chunk = re.search(r"constexpr size_t kPermChunkRows = \(size_t\)(\d+) \* kSidePermR;", plan)
    assert int(chunk.group(1)) <= 65535
    assert int(re.search(r"constexpr int kSidePermR = (\d+);", plan).group(1)) == lb.TDA_PERM_ROWS
    assert "kSidePermR == kPermR" in host


def test_perm_symbols_exported_and_abi_version_unchanged(pkg, built_lib):
    lib = ctypes.CDLL(built_lib)
    assert hasattr(lib, "tda_permutation_test") and hasattr(lib, "tda_perm_free")
    assert {"tda_permutation_test", "tda_perm_free"} <= set(pkg.EXPORTS)
    assert pkg.lib().tda_version() == 8  # symbols added only: no existing struct changed
    assert {"permutation_test", "diagram_permutation_test", "label_permutations"} <= set(pkg.__all__)


def _sym(S, seed=0):
    rng = np.random.default_rng(seed)
    A = rng.random((S, S))
    W = A + A.T
    np.fill_diagonal(W, 0.0)
    return W


def test_perm_invalid_arguments_rejected_before_device(pkg, built_lib):
    L = pkg.lib()
    lb = pkg._lib
    res = ctypes.POINTER(lb.PermResult)()
    S, B, G = 6, 3, 2
    W = _sym(S)
    obs = np.array([0, 0, 1, 1, 1, 0], np.uint8)
    lab = np.stack([obs, obs[::-1], np.roll(obs, 1)]).copy()

    def call(**kw):
        a = lb.PermArgs()
        a.w, a.obs, a.lab, a.S, a.B, a.G = W.ctypes.data, obs.ctypes.data, lab.ctypes.data, S, B, G
        for k, v in kw.items():
            setattr(a, k, v.ctypes.data if isinstance(v, np.ndarray) else v)
        rc = L.tda_permutation_test(ctypes.byref(a), ctypes.byref(res))
        assert not res  # no result on failure
        return rc

    def err():
        return L.tda_last_error()

    # NULL pointers
    assert L.tda_permutation_test(None, ctypes.byref(res)) == -1
    assert call(w=None) == -1 and b"w is NULL" in err()
    assert call(obs=None) == -1 and b"obs is NULL" in err()
    assert call(lab=None) == -1 and b"lab is NULL" in err()
    assert L.tda_permutation_test(ctypes.byref(lb.PermArgs()), None) == -1 and b"out is NULL" in err()
    # counts
    assert call(S=1) == -1 and b"S must be" in err()
    assert call(S=0) == -1 and call(S=-4) == -1
    assert call(B=0) == -1 and b"B must be" in err()
    assert call(B=-1) == -1
    assert call(G=1) == -1 and b"G must be" in err()
    assert call(G=0) == -1
    assert call(reserved=1) == -1 and b"reserved" in err()
    # INVALID comes before UNSUPPORTED
    assert call(S=4096, B=0) == -1 and call(G=65, reserved=2) == -1
    # unsupported sizes, refused before w, obs or the table is read
    assert call(S=2049) == -2 and b"S > 2048" in err()
    assert call(G=65) == -2 and b"G > 64" in err()
    assert call(B=2 ** 27 // S + 1) == -2 and b"2^27" in err() and b"split B" in err()
    # the matrix
    for bad, what in ((np.nan, b"not finite"), (np.inf, b"not finite"), (-1.0, b"not finite and >= 0")):
        V = W.copy()
        V[2, 4] = V[4, 2] = bad
        assert call(w=V) == -1 and b"w[2][4]" in err() and what in err()
    V = W.copy()
    V[3, 3] = 1e-300
    assert call(w=V) == -1 and b"w[3][3]" in err() and b"diagonal" in err()
    V[3, 3] = -0.0
    assert call(w=V) == -1 and b"w[3][3]" in err() and b"diagonal" in err()  # -0.0 is not +0.0
    V = W.copy()
    V[1, 5] = np.nextafter(V[5, 1], 2.0)
    assert call(w=V) == -1 and b"w[1][5] and w[5][1] differ" in err()
    # the observed labels
    o = obs.copy()
    o[4] = 2
    assert call(obs=o) == -1 and b"obs[4] = 2 is outside [0, G = 2)" in err()
    o = np.array([0, 1, 1, 1, 1, 1], np.uint8)
    assert call(obs=o) == -1 and b"group 0 has 1 members" in err()
    o = np.array([0, 0, 0, 0, 0, 0], np.uint8)
    assert call(obs=o) == -1 and b"group 1 has 0 members" in err()
    assert call(G=3) == -1 and b"group 2 has 0 members" in err()
    # the table: a row with another histogram, a code >= G among them
    t = lab.copy()
    t[1, 0] = 1 - t[1, 0]
    assert call(lab=t) == -1 and b"lab[1]" in err() and b"histogram" in err()
    t = lab.copy()
    t[2, 3] = 7
    assert call(lab=t) == -1 and b"lab[2]" in err()
    assert call(lab=t, B=2) == -5  # the table ends before it
    # valid arguments get as far as the device check
    assert call() == -5 and b"gfx950" in err()
    L.tda_perm_free(None)  # a no-op


def test_perm_size_limits_exact(pkg, built_lib):
    """S = 2048 and B * S = 2^27 are served (as far as the device check), S = 2049 and
    B * S = 2^27 + S are not."""
    L = pkg.lib()
    lb = pkg._lib
    res = ctypes.POINTER(lb.PermResult)()
    S = 2048
    W = np.zeros((S, S))
    obs = (np.arange(S) % 2).astype(np.uint8)
    Bmax = 2 ** 27 // S
    lab = np.tile(obs, (Bmax, 1))

    def call(S_, B_):
        a = lb.PermArgs()
        a.w, a.obs, a.lab, a.S, a.B, a.G = W.ctypes.data, obs.ctypes.data, lab.ctypes.data, S_, B_, 2
        rc = L.tda_permutation_test(ctypes.byref(a), ctypes.byref(res))
        assert not res
        return rc

    assert call(2048, 4) == -5
    assert call(2049, 4) == -2 and b"S > 2048" in L.tda_last_error()
    assert Bmax * S == 2 ** 27
    assert call(2048, Bmax) == -5
    assert call(2048, Bmax + 1) == -2 and b"2^27" in L.tda_last_error()


def test_label_permutations(pkg):
    labels = ["clean"] * 5 + ["adv"] * 3 + ["noise"] * 4
    a, b = pkg.label_permutations(labels, 40, seed=3), pkg.label_permutations(labels, 40, seed=3)
    assert a.dtype == np.uint8 and a.shape == (40, 12) and a.flags.c_contiguous
    assert a.tobytes() == b.tobytes()  # the same seed: the same bits
    assert a.tobytes() != pkg.label_permutations(labels, 40, seed=4).tobytes()
    codes = np.unique(labels, return_inverse=True)[1]
    hist = np.bincount(codes, minlength=3)
    assert hist.tolist() == [3, 5, 4]  # np.unique order: adv, clean, noise
    assert all(np.bincount(r, minlength=3).tolist() == hist.tolist() for r in a)  # every row has the label histogram
    assert len({r.tobytes() for r in a}) > 1
    tiled = np.tile(codes.astype(np.uint8), (40, 1))
    assert a.tobytes() == np.random.default_rng(3).permuted(tiled, axis=1).tobytes()  # the documented draw
    for bad in (0, -1, 2.5, None, True):
        with pytest.raises(ValueError, match="B must"):
            pkg.label_permutations(labels, bad)
    with pytest.raises(ValueError, match="labels"):
        pkg.label_permutations([], 3)


def test_pvalue_rule(pkg):
    pv = pkg.hypothesis.pvalue_from_null
    assert pv([3.0, 1.0, 2.0, 5.0], 2.0) == (2, 3 / 5)  # <=: a tie counts
    assert pv([3.0, 4.0], 2.0) == (0, 1 / 3)  # never 0
    assert pv([1.0, 1.0, 1.0], 1.0) == (3, 1.0)
    assert pv([np.nextafter(1.0, 2.0)], 1.0) == (0, 0.5) and pv([np.nextafter(1.0, 0.0)], 1.0) == (1, 1.0)  # one ulp decides
    null = np.arange(9999, dtype=np.float64)
    c, p = pv(null, 499.0)
    assert c == 500 and p == np.float64(501) / np.float64(10000)  # one float64 division
    # the restatement applies the same rule
    W = _sym(8)
    obs = np.array([0, 0, 0, 1, 1, 1, 1, 1], np.uint8)
    lab = np.random.default_rng(0).permuted(np.tile(obs, (50, 1)), axis=1)
    t, nl, cnt, pval = pr.permutation_test(W, obs, lab, 2)
    assert (cnt, pval) == pv(nl, t)


def test_python_entries_refuse_before_any_library_call(pkg, monkeypatch):
    def no_lib():
        raise AssertionError("the library was called")

    monkeypatch.setattr(pkg._lib, "lib", no_lib)
    D = _sym(6)
    labels = [0, 0, 0, 1, 1, 1]
    pt = pkg.permutation_test
    with pytest.raises(ValueError, match="square"):
        pt(D[:, :5], labels)
    with pytest.raises(ValueError, match="square"):
        pt(D[0], labels)
    with pytest.raises(ValueError, match="labels"):
        pt(D, labels[:5])
    with pytest.raises(ValueError, match="labels"):
        pt(D, labels + [1])
    for q in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="q must"):
            pt(D, labels, q=q)
    bad = D.copy()
    bad[1, 2] = bad[2, 1] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        pt(bad, labels)
    bad[1, 2] = bad[2, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        pt(bad, labels)
    big = D * 1e200
    with pytest.raises(ValueError, match="non-finite"):
        pt(big, labels, q=2.0)  # W = D ** q overflows
    for B in (0, -2, 2.5, None):
        with pytest.raises(ValueError, match="B must"):
            pt(D, labels, B=B)
    for perms in (np.zeros((0, 6), np.uint8), np.zeros((3, 5), np.uint8), np.zeros(6, np.uint8), np.zeros((2, 6)), np.full((2, 6), 2), np.full((2, 6), -1)):
        with pytest.raises(ValueError, match="permutations"):
            pt(D, labels, permutations=perms)
    with pytest.raises(NotImplementedError, match="groups"):
        pt(_sym(130), np.arange(130) // 2)  # 65 groups
    with pytest.raises(ValueError, match="metric"):
        pkg.diagram_permutation_test([np.zeros((0, 2))] * 6, labels, metric="euclidean")


def test_valid_python_call_reaches_the_device_check(pkg, built_lib):
    with pytest.raises(RuntimeError, match="gfx950"):
        pkg.permutation_test(_sym(6), list("aaabbb"), B=5)
    with pytest.raises(ValueError, match="at least 2"):
        pkg.permutation_test(_sym(6), list("aaaaab"), B=5)  # the library's own refusal, as a ValueError


def test_diagram_permutation_test_routing(pkg, monkeypatch):
    """One call to the metric's matrix entry with its own arguments, then permutation_test on what
    it returned with the rest."""
    hy = pkg.hypothesis
    calls = []
    D = _sym(6)

    def entry(name):
        def f(dgms, **kw):
            calls.append((name, dgms, kw))
            return D
        return f

    for name in ("sliced_wasserstein_matrix", "bottleneck_matrix", "wasserstein_matrix", "heat_matrix"):
        monkeypatch.setattr(hy.diagrams, name, entry(name))
    seen = []
    monkeypatch.setattr(hy, "permutation_test", lambda D_, labels, **kw: seen.append((D_, labels, kw)) or "result")
    dg, labels = [object()] * 6, list("aaabbb")
    assert hy.diagram_permutation_test(dg, labels) == "result"  # the default metric
    assert calls.pop() == ("wasserstein_matrix", dg, dict(device=0, dim=1))
    assert hy.diagram_permutation_test(dg, labels, metric="bottleneck", dim=0, device=2, B=99, q=2.0) == "result"
    assert calls.pop() == ("bottleneck_matrix", dg, dict(device=2, dim=0))
    assert seen[-1][0] is D and seen[-1][1] is labels and seen[-1][2] == dict(device=2, B=99, q=2.0)
    hy.diagram_permutation_test(dg, labels, metric="sliced_wasserstein", M=20, seed=5, return_null=True)
    assert calls.pop() == ("sliced_wasserstein_matrix", dg, dict(M=20, device=0, dim=1))
    assert seen[-1][2] == dict(device=0, seed=5, return_null=True)
    hy.diagram_permutation_test(dg, labels, metric="heat", sigma=0.7, permutations="table")
    assert calls.pop() == ("heat_matrix", dg, dict(sigma=0.7, device=0, dim=1))
    assert seen[-1][2] == dict(device=0, permutations="table")
    assert not calls and len(seen) == 4


def test_restatement_within_the_bound_of_the_plain_formula():
    """|T - T_exact| <= S u T + 7 u T (tda_rips.h), T_exact by fsum.  The plain form's own error is
    at most 3 u T (a correctly rounded sum and a division per group, a correctly rounded total);
    the derivation's (n_max + 3 + ceil(S / 64)) u T leaves more than that below S + 7 at these
    shapes (n_max <= S - 4)."""
    rng = np.random.default_rng(5)
    for S, sizes in ((8, (4, 4)), (65, (30, 35)), (200, (120, 76, 4)), (384, (380, 4))):
        W = _sym(S, seed=S) * 3.7
        obs = np.repeat(np.arange(len(sizes)), sizes).astype(np.uint8)
        lab = rng.permuted(np.tile(obs, (6, 1)), axis=1)
        c = pr.weights(obs, len(sizes))
        T = pr.statistics(W, np.vstack([obs[None], lab]), c)
        for row, t in zip(np.vstack([obs[None], lab]), T):
            exact = pr.plain(W, row)
            assert abs(t - exact) <= pr.bound(S, exact), (S, t, exact)


def test_restatement_depends_on_the_partition_only():
    S = 12
    W = _sym(S, seed=1)
    obs = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2], np.uint8)
    c = pr.weights(obs, 3)
    swapped = np.stack([obs, (obs + 1) % 3, (obs + 2) % 3, 2 - obs])  # equal groups: any renaming of the codes
    T = pr.statistics(W, swapped, c)
    assert len({t.tobytes() for t in T}) == 1
    assert pr.same_partition(swapped, obs).all()
    other = np.roll(obs, 1)
    other[[0, 1]] = other[[1, 0]]
    assert not pr.same_partition(other, obs)[0]
