"""The host plans of the entries beside the persistence pipeline (csrc/side_plan.h) against the Python
restatement of the host files they came from (side_plan_ref.py), and every refusal of the five
validators with its code, its message and its place in the order of checks (CPU).

tests/side_plan_main.cpp includes only side_plan.h; it is compiled with g++ under the address and
undefined-behaviour sanitizers and run as a program of its own, one case per line."""
import itertools
import os
import subprocess

import pytest

import dist_ref
import side_plan_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tda-multimodal_amd", "csrc")
INVALID, UNSUPPORTED = -1, -2
F32, F64 = ref.F32, ref.F64
GIB4 = 4 << 30


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("side_plan") / "side_plan")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "side_plan_main.cpp")], check=True)
    return exe


def run(exe, lines, env=None):
    """-> per line ("err", code, message) or ("ok", {field: value})"""
    e = {k: v for k, v in os.environ.items() if not k.startswith("TDA_")}
    if env:
        e.update(env, TDA_TEST_OVERRIDES="1")
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=e)
    assert r.returncode == 0, r.stderr[-2000:]  # a sanitizer report ends the program with a non-zero status
    out = []
    for line in r.stdout.splitlines():
        head = line.split(" ", 2)
        if head[0] == "err":
            out.append(("err", int(head[1]), head[2]))
        else:
            assert head[0] == "ok"
            out.append(("ok", {k: (float.fromhex(v) if k.startswith("cw") else int(v)) for k, v in (t.split("=") for t in line.split()[1:])}))
    assert len(out) == len(lines)
    return out


def words(*xs):
    return " ".join(str(int(x)) if isinstance(x, bool) else str(x) for x in xs)


# ---------------------------------------------------------------- the case lines of side_plan_main.cpp
def arr(t):
    """A pointer: (0,) NULL, (1,) present, (2, values ...) -> the mode, the count and the values."""
    return t if t[0] != 2 else (2, len(t) - 1, *t[1:])


def greedy_line(c):
    return words("greedy", c["args"], c["cap"], c["x"], c["dtype"], c["dev"], c["L"], c["N"], c["D"], c["is_dist"], c["k"], c["want_dp"])


def resample_line(c):
    return words("resample", c["args"], c["cap"], c["x"], c["dtype"], c["dev"], c["L"], c["N"], c["D"], c["is_dist"], c["B"], c["m"], c["per_layer"],
                 *arr(c["idx"]))


def perm_line(c):
    return words("perm", c["args"], c["S"], c["B"], c["G"], c["reserved"], *arr(c["w"]), *arr(c["obs"]), *arr(c["lab"]))


def ed_line(c):
    return words("ed", c["args"], c["out"], c["x"], c["dtype"], c["dev"], c["B"], c["N"], c["D"])


def spectral_line(c):
    return words(c["what"], c["args"], c["out"], c["x"], c["dtype"], c["dev"], c["B"], c["S"], c["D"], c["W"], c["n_alpha"], c["eps"], *arr(c["alphas"]))


def umap_line(c):
    return words("umap", c["args"], c["x"], c["out"], c["dtype"], c["dev"], c["L"], c["N"], c["D"], c["metric"], c["k"], c["c"], c["epochs"],
                 c["init"], c["neg"], c["a"], c["b"])


def transform_line(c):
    return words("transform", c["args"], c["xt"], c["emb"], c["y"], c["out"], c["dtype"], c["dev"], c["L"], c["M"], c["N"], c["D"], c["metric"],
                 c["k"], c["c"], c["epochs"], c["neg"], c["a"], c["b"])


GREEDY = dict(args=1, cap=GIB4, x=1, dtype=F32, dev=0, L=3, N=65, D=3, is_dist=0, k=16, want_dp=1)
RESAMPLE = dict(args=1, cap=GIB4, x=1, dtype=F32, dev=0, L=3, N=65, D=3, is_dist=0, B=4, m=5, per_layer=0, idx=(1,))
PERM_W = [0.0, 1.0, 2.0, 3.0, 1.0, 0.0, 4.0, 5.0, 2.0, 4.0, 0.0, 6.0, 3.0, 5.0, 6.0, 0.0]
PERM = dict(args=1, S=4, B=2, G=2, reserved=0, w=(2, *PERM_W), obs=(2, 0, 0, 1, 1), lab=(2, 0, 1, 0, 1, 1, 1, 0, 0))
ED = dict(args=1, out=1, x=1, dtype=F32, dev=0, B=2, N=10, D=7)
SPECTRAL = dict(what="entropy", args=1, out=1, x=1, dtype=F32, dev=0, B=2, S=10, D=7, W=0, n_alpha=2, eps=1e-10, alphas=(2, 0.5, 2.0))
UMAP = dict(args=1, x=1, out=1, dtype=F32, dev=0, L=2, N=50, D=5, metric=0, k=15, c=2, epochs=10, init=0, neg=5, a=1.5, b=0.9)
TRANSFORM = dict(args=1, xt=1, emb=1, y=1, out=1, dtype=F32, dev=0, L=2, M=7, N=50, D=5, metric=0, k=15, c=2, epochs=10, neg=5, a=1.5, b=0.9)


# ---------------------------------------------------------------- 1. the plans against the restatement
GRID_N = (1, 2, 64, 65, 144, 145, 1024, 8192)  # 8193 is refused (test_refusals_*): no plan to compare
GRID_D = (1, 3, 31, 32, 64, 4096)
GRID_L = (1, 2, 65535, 65536, 100000)


def sq_grid():
    """(N, D, dtype, is_dist, host_in) of the grid; float64 points are refused, so f64 goes with matrices only."""
    for N, D, dtype, is_dist, host_in in itertools.product(GRID_N, GRID_D, (F32, F64), (0, 1), (0, 1)):
        if dtype == F64 and not is_dist:
            continue
        yield N, D, dtype, is_dist, host_in


def caps_of(per_layer):
    return (1, per_layer, per_layer - 1, 2 * per_layer, GIB4)


def check_chunks_and_carve(p, cap, arrays):
    """What the issue of side_plan.h requires of every plan with a chunk of layers.  arrays: (offset
    field, bytes) in carve order."""
    L, Lc = p["L"], p["Lc"]
    assert 1 <= Lc <= 65535
    chunks = [(l0, min(Lc, L - l0)) for l0 in range(0, L, Lc)] if L // Lc < 1000 else None
    if chunks is not None:  # the loop of the entries covers 0 .. L once
        assert chunks[0][0] == 0 and sum(lc for _, lc in chunks) == L
        assert all(a + n == b for (a, n), (b, _) in zip(chunks, chunks[1:])) and all(1 <= lc <= Lc for _, lc in chunks)
    else:
        assert (L + Lc - 1) // Lc * Lc >= L > ((L + Lc - 1) // Lc - 1) * Lc
    if Lc > 1:
        assert Lc * p["per_layer"] <= cap
    assert Lc == L or Lc == 65535 or (Lc + 1) * p["per_layer"] > cap  # and it is the largest such count
    end = 0
    for name, nbytes in arrays:
        assert p[name] % 256 == 0 and p[name] >= end, name  # aligned, increasing, not overlapping
        end = p[name] + nbytes
    assert p["total"] % 256 == 0 and p["total"] >= end


def sq_arrays(p, N, host_in):
    sp = p["dsplit"] if p["gram_layer"] or p["dsplit"] > 1 else 0
    Lc = p["Lc"]
    return [("o_x", Lc * p["x_layer"] if host_in else 0), ("o_dm", Lc * N * N * 4), ("o_rm", Lc * N * 4), ("o_gp", Lc * sp * N * N * 8),
            ("o_np", Lc * sp * N * 8)]


def test_greedy_plan_grid(plan_exe):
    cases = []
    for (N, D, dtype, is_dist, host_in), want_dp, L in itertools.product(sq_grid(), (0, 1), GRID_L):
        k = max(1, N // 3)
        kw = dict(L=L, N=N, D=D, dtype=dtype, is_dist=is_dist, host_in=host_in, k=k, want_dp=want_dp)
        for cap in caps_of(ref.greedy(**kw)["per_layer"]):
            cases.append((kw, cap))
    lines = [greedy_line(dict(GREEDY, cap=cap, dtype=kw["dtype"], dev=1 - kw["host_in"], L=kw["L"], N=kw["N"], D=kw["D"], is_dist=kw["is_dist"],
                              k=kw["k"], want_dp=kw["want_dp"])) for kw, cap in cases]
    seen = set()
    for (kw, cap), got in zip(cases, run(plan_exe, lines)):
        assert got == ("ok", ref.greedy(cap=cap, **kw)), (kw, cap)
        p, L, N, k = got[1], kw["L"], kw["N"], kw["k"]
        check_chunks_and_carve(p, cap, [("o_idx", L * k * 8), ("o_lam", L * k * 4), *sq_arrays(p, N, kw["host_in"]),
                                        ("o_dp", p["Lc"] * k * N * 4 if kw["want_dp"] else 0)])
        seen.add(min(p["Lc"], 3) if p["Lc"] < L else "all")
    assert seen == {1, 2, 3, "all"}  # one layer, two, many, and the whole call in one chunk


def test_resample_plan_grid(plan_exe):
    cases = []
    for (N, D, dtype, is_dist, host_in), per_layer, L in itertools.product(sq_grid(), (0, 1), GRID_L):
        B, m = (2, 3) if L <= 2 else (1, 2)  # the plan scans the table: a small one at the large L
        kw = dict(L=L, N=N, D=D, dtype=dtype, is_dist=is_dist, host_in=host_in, B=B, m=m, per_layer_idx=per_layer)
        for cap in caps_of(ref.resample(**kw)["per_layer"]):
            cases.append((kw, cap))
    lines = [resample_line(dict(RESAMPLE, cap=cap, dtype=kw["dtype"], dev=1 - kw["host_in"], L=kw["L"], N=kw["N"], D=kw["D"], is_dist=kw["is_dist"],
                                B=kw["B"], m=kw["m"], per_layer=kw["per_layer_idx"])) for kw, cap in cases]
    for (kw, cap), got in zip(cases, run(plan_exe, lines)):
        assert got == ("ok", ref.resample(cap=cap, **kw)), (kw, cap)
        p, L, N, B, m = got[1], kw["L"], kw["N"], kw["B"], kw["m"]
        check_chunks_and_carve(p, cap, [("o_h", L * B * 4), ("o_idx", (p["Lc"] if kw["per_layer_idx"] else 1) * B * m * 4),
                                        *sq_arrays(p, N, kw["host_in"])])


def test_ws_cap_knob_and_distance_selection(plan_exe):
    """The cap the entries pass: TDA_GREEDY_WS_BYTES, or TDA_SIDE_WS_BYTES (at least 1) behind the gate
    of the test knobs.  And the restatement's distance selection is the library's, on dist_ref's cases."""
    for value, want in ((None, GIB4), ("1", 1), ("0", 1), ("123456789012", 123456789012)):
        assert run(plan_exe, ["cap 1"], {"TDA_SIDE_WS_BYTES": value} if value else None) == [("ok", {"cap": want})]
    r = subprocess.run([plan_exe], input="cap 1\n", capture_output=True, text=True, env={"TDA_SIDE_WS_BYTES": "77"})  # no gate
    assert r.stdout.split() == ["ok", f"cap={GIB4}"]
    for n, d, dt, env, want in dist_ref.CASES:
        if not env:
            assert ref.dist_select(n, d, F64 if dt == dist_ref.F64 else F32, False) == want, (n, d)


def test_perm_plan(plan_exe):
    sizes = [(4, 2), (128, 3), (129, 1)]
    cases, lines = [], []
    for S, B in sizes:
        obs = [i % 2 for i in range(S)] if S > 4 else [0, 0, 1, 1]
        w = [0.0 if i == j else float(1 + min(i, j) + max(i, j)) for i in range(S) for j in range(S)]
        lab = (obs[::-1] + obs) * B
        cases.append((S, B, obs))
        lines.append(perm_line(dict(PERM, S=S, B=B, w=(2, *w), obs=(2, *obs), lab=(2, *lab[:B * S]))))
    for env, kw in (({}, {}), ({"TDA_PERM_CHUNK": "5"}, dict(chunk_env=5)), ({"TDA_PERM_CHUNK": "0"}, dict(chunk_env=0)),
                    ({"TDA_PERM_CHUNK": "99999999"}, dict(chunk_env=99999999)), ({"TDA_PERM_TILED": "1"}, dict(tiled_env=True))):
        for (S, B, obs), got in zip(cases, run(plan_exe, lines, env)):
            assert got == ("ok", ref.perm(S, B, obs, 2, **kw)), (S, B, env)
    got = run(plan_exe, [perm_line(dict(PERM, G=3, obs=(2, 0, 0, 1, 1, 2, 2, 2), S=7, B=1, lab=(2, 2, 2, 2, 1, 1, 0, 0),
                                        w=(2, *[0.0 if i == j else 1.0 for i in range(7) for j in range(7)])))])[0]
    assert got[0] == "ok" and [got[1][f"cw{g}"] for g in range(3)] == [0.25, 0.25, 1.0 / 12.0]
    assert [r[1]["resident"] for r in run(plan_exe, lines)] == [1, 1, 0]  # S = 128 is the last resident one


def test_spectral_plans(plan_exe):
    cases, lines = [], []
    for B, N, D, dtype, dev in itertools.product((1, 3), (1, 7, 128, 129, 1024, 5000), (1, 7, 1024, 4096), (F32, F64), (0, 1)):
        if min(N, D) > 1024:
            continue
        cases.append(ref.ed_job(B, N, D, dtype, dev))
        lines.append(ed_line(dict(ED, B=B, N=N, D=D, dtype=dtype, dev=dev)))
        for W, what in itertools.product((0, 1, 3, 7, N, N + 5), ("windows", "entropy")):
            if W == 0 and what == "windows":
                continue
            n_alpha = 3 if what == "entropy" else 0
            cases.append(ref.spectral(B, N, D, dtype, dev, W, n_alpha or 1))
            lines.append(spectral_line(dict(SPECTRAL, what=what, B=B, S=N, D=D, dtype=dtype, dev=dev, W=W, n_alpha=n_alpha,
                                            alphas=(2, 0.5, 1.0, 3.0) if n_alpha else (0,))))
    got = run(plan_exe, lines)
    for want, g, line in zip(cases, got, lines):
        assert g == ("ok", want), line
    staged = [g[1] for g in got if g[1]["stage"]]
    assert staged and all(j["src_rows"] > j["keep_rows"] and j["keep_rows"] % j["N"] == 0 and j["o_g"] > 0 for j in staged)


def test_umap_plans(plan_exe):
    cases, lines = [], []
    for L, N, D, dtype, dev, k, c, init in itertools.product((1, 3), (2, 50, 1600, 2048, 2049, 4095), (1, 32, 4096), (F32, F64), (0, 1), (2, 15, 64),
                                                             (1, 2, 8), (0, 1)):
        if k > N or N * c * 12 > ref.UMAP_LDS:
            continue
        cases.append(ref.umap(L, N, D, dtype, dev, k, c, init == 0))
        lines.append(umap_line(dict(UMAP, L=L, N=N, D=D, dtype=dtype, dev=dev, k=k, c=c, init=init)))
    got = run(plan_exe, lines)
    for want, g, line in zip(cases, got, lines):
        assert g == ("ok", want), line
    assert {g[1]["spectral"] for g in got} == {0, 1} and all(g[1]["sgd_lds"] <= ref.UMAP_LDS and g[1]["spec_lds"] > 0 for g in got)
    cases, lines = [], []
    for L, M, N, D, dtype, dev, k, c in itertools.product((1, 3), (1, 7, 192), (2, 50, 4797, 8000), (1, 32), (F32, F64), (0, 1), (2, 64), (1, 8)):
        if k > N or ref.transform_lds(M, N, c) > ref.UMAP_LDS:
            continue
        cases.append(ref.transform(L, M, N, D, dtype, dev, k, c))
        lines.append(transform_line(dict(TRANSFORM, L=L, M=M, N=N, D=D, dtype=dtype, dev=dev, k=k, c=c)))
    got = run(plan_exe, lines)
    assert len(cases) > 100
    for want, g, line in zip(cases, got, lines):
        assert g == ("ok", want), line


# ---------------------------------------------------------------- 2. the refusals, in the order of the checks
def check_order(plan_exe, base, line_of, refusals):
    """refusals: (what is wrong, code, message) in the order the entry checks.  Case i has wrong what
    refusal i names and everything the later ones name (where two touch one field, the earlier wins):
    it must come back with refusal i, so no later check runs before an earlier one."""
    lines = []
    for i in range(len(refusals)):
        c = dict(base)
        for wrong, _, _ in reversed(refusals[i:]):
            c.update(wrong)
        lines.append(line_of(c))
    lines += [line_of(dict(base, **wrong)) for wrong, _, _ in refusals]  # and each alone
    got = run(plan_exe, lines + [line_of(base)])
    assert got[-1][0] == "ok", got[-1]
    want = [("err", code, msg) for _, code, msg in refusals]
    assert got[:-1] == want + want


F64_POINTS = " of float64 point clouds is not supported (pass float32 points or a distance matrix)"
DTYPE = "dtype must be TDA_F32 or TDA_F64"


def test_refusals_greedy(plan_exe):
    check_order(plan_exe, GREEDY, greedy_line, [
        (dict(args=0), INVALID, "args is NULL"), (dict(x=0), INVALID, "x is NULL"), (dict(L=0), INVALID, "L must be >= 1"),
        (dict(N=0), INVALID, "N must be >= 1"), (dict(D=0), INVALID, "D must be >= 1"), (dict(dtype=2), INVALID, DTYPE),
        (dict(k=0), INVALID, "n_perm must be in [1, N]"), (dict(N=8193, k=8193), UNSUPPORTED, "greedy subsampling: N > 8192 is not supported"),
        (dict(dtype=F64), UNSUPPORTED, "greedy subsampling" + F64_POINTS)])
    got = run(plan_exe, [greedy_line(dict(GREEDY, k=66)), greedy_line(dict(GREEDY, k=65)), greedy_line(dict(GREEDY, N=8192)),
                         greedy_line(dict(GREEDY, is_dist=1, D=0, dtype=F64))])
    assert got[0] == ("err", INVALID, "n_perm must be in [1, N]") and [g[0] for g in got[1:]] == ["ok"] * 3


def test_refusals_resample(plan_exe):
    many = "resampling: more than 2^27 resamples (L * B) in one call is not supported: split B over several calls"
    check_order(plan_exe, RESAMPLE, resample_line, [
        (dict(args=0), INVALID, "args is NULL"), (dict(x=0), INVALID, "x is NULL"), (dict(idx=(0,)), INVALID, "idx is NULL"),
        (dict(L=0), INVALID, "L must be >= 1"), (dict(N=0), INVALID, "N must be >= 1"), (dict(D=0), INVALID, "D must be >= 1"),
        (dict(dtype=-1), INVALID, DTYPE), (dict(B=0), INVALID, "B must be >= 1"), (dict(m=0), INVALID, "m must be >= 1"),
        (dict(N=8193), UNSUPPORTED, "resampling: N > 8192 is not supported"), (dict(m=8193), UNSUPPORTED, "resampling: m > 8192 is not supported"),
        (dict(dtype=F64), UNSUPPORTED, "resampling" + F64_POINTS), (dict(L=1 << 20, B=129), UNSUPPORTED, many)])
    table = [0] * 20
    table[13] = 65
    low = list(table)
    low[13], low[7] = 64, -1
    got = run(plan_exe, [resample_line(dict(RESAMPLE, idx=(2, *table))), resample_line(dict(RESAMPLE, idx=(2, *low))),
                         resample_line(dict(RESAMPLE, L=1 << 20, B=128, m=1)), resample_line(dict(RESAMPLE, N=8192, m=8192, B=1)),
                         resample_line(dict(RESAMPLE, per_layer=1, idx=(2, *([0] * 59), 65)))])
    assert got[0] == ("err", INVALID, "idx[13] = 65 is outside [0, N = 65)") and got[1] == ("err", INVALID, "idx[7] = -1 is outside [0, N = 65)")
    assert got[2][0] == "ok" and got[3][0] == "ok"  # L * B = 2^27, N = m = 8192: the limits themselves
    assert got[4] == ("err", INVALID, "idx[59] = 65 is outside [0, N = 65)")  # a table per layer is scanned whole


def test_refusals_perm(plan_exe):
    big = "permutation test: a label table of more than 2^27 entries (B * S) is not supported: split B over several calls"
    check_order(plan_exe, PERM, perm_line, [
        (dict(args=0), INVALID, "args is NULL"), (dict(w=(0,)), INVALID, "w is NULL"), (dict(obs=(0,)), INVALID, "obs is NULL"),
        (dict(lab=(0,)), INVALID, "lab is NULL"), (dict(S=1), INVALID, "S must be >= 2"), (dict(B=0), INVALID, "B must be >= 1"),
        (dict(G=1), INVALID, "G must be >= 2"), (dict(reserved=1), INVALID, "reserved must be 0"),
        (dict(S=2049, w=(1,), obs=(1,), lab=(1,)), UNSUPPORTED, "permutation test: S > 2048 is not supported"),
        (dict(G=65), UNSUPPORTED, "permutation test: G > 64 is not supported"),
        (dict(S=2048, B=65537, w=(1,), obs=(1,), lab=(1,)), UNSUPPORTED, big)])

    def w_with(**at):
        w = list(PERM_W)
        for k, v in at.items():
            w[int(k[1:])] = v
        return (2, *w)

    scans = [
        (dict(w=w_with(_6="nan", _9="nan")), "w[1][2] = nan is not finite and >= 0"),
        (dict(w=w_with(_6="-1.0", _9="-1.0")), "w[1][2] = -1.000000 is not finite and >= 0"),
        (dict(w=w_with(_6="inf", _9="inf")), "w[1][2] = inf is not finite and >= 0"),
        (dict(w=w_with(_10="-0.0")), "w[2][2] = -0.000000: the diagonal must be +0.0"),
        (dict(w=w_with(_10="0.5")), "w[2][2] = 0.500000: the diagonal must be +0.0"),
        (dict(w=w_with(_7="5.5")), "w[1][3] and w[3][1] differ: w must be symmetric bit for bit"),
        (dict(obs=(2, 0, 0, 1, 2)), "obs[3] = 2 is outside [0, G = 2)"),
        (dict(obs=(2, 0, 0, 0, 1)), "group 1 has 1 members: every group needs at least 2"),
        (dict(lab=(2, 0, 1, 0, 1, 1, 1, 1, 0)), "lab[1] is not a permutation of obs (its label histogram differs)"),
    ]
    got = run(plan_exe, [perm_line(dict(PERM, **wrong)) for wrong, _ in scans])
    assert got == [("err", INVALID, msg) for _, msg in scans]
    # the scans in their order: w before obs before lab
    both = run(plan_exe, [perm_line(dict(PERM, w=w_with(_7="5.5"), obs=(2, 0, 0, 1, 2), lab=(2, 0, 0, 0, 0, 1, 1, 1, 1))),
                          perm_line(dict(PERM, obs=(2, 0, 0, 1, 2), lab=(2, 0, 0, 0, 0, 1, 1, 1, 1)))])
    assert both[0][2].startswith("w[1][3]") and both[1][2].startswith("obs[3]")
    # B * S = 2^27 is accepted (the zero-filled obs then fails a later check), S = 2048 and G = 64 as well
    edge = run(plan_exe, [perm_line(dict(PERM, S=2048, B=65536, G=64, w=(1,), obs=(1,), lab=(1,)))])
    assert edge == [("err", INVALID, "group 1 has 0 members: every group needs at least 2")]


def test_refusals_spectral(plan_exe):
    head = [(dict(args=0), INVALID, "args and out are required"), (dict(out=0), INVALID, "args and out are required")]
    x_dtype = [(dict(x=0), INVALID, "x is NULL"), (dict(dtype=5), INVALID, DTYPE)]
    check_order(plan_exe, ED, ed_line, head + [(dict(B=0), INVALID, "need B, N, D >= 1")] + x_dtype + [
        (dict(N=1025, D=1025), UNSUPPORTED, "effective dimensionality: min(N, D) <= 1024 is supported")])
    got = run(plan_exe, [ed_line(dict(ED, N=0)), ed_line(dict(ED, D=0)), ed_line(dict(ED, N=1024, D=9000)), ed_line(dict(ED, N=9000, D=1024)),
                         ed_line(dict(ED, N=8193, D=8193))])
    assert got[0] == got[1] == ("err", INVALID, "need B, N, D >= 1") and got[2][0] == got[3][0] == "ok"
    assert got[4] == ("err", UNSUPPORTED, "effective dimensionality: min(N, D) <= 1024 is supported")
    sizes = (dict(S=0), INVALID, "need B, S, D >= 1")
    check_order(plan_exe, SPECTRAL, spectral_line, head + [sizes] + x_dtype + [
        (dict(W=-1), INVALID, "n_windows must be positive"), (dict(S=1025, D=1025), UNSUPPORTED, "matrix entropy: min(N, D) <= 1024 is supported"),
        (dict(n_alpha=17, alphas=(1,)), INVALID, "matrix entropy: 1 .. 16 orders per call"), (dict(alphas=(0,)), INVALID, "alphas is NULL"),
        (dict(eps="nan"), INVALID, "matrix entropy: eps must be >= 0"),
        (dict(alphas=(2, 0.5, 0.0)), INVALID, "matrix entropy: every order alpha must be finite and > 0")])
    windows = dict(SPECTRAL, what="windows", W=2, n_alpha=0, alphas=(0,))
    check_order(plan_exe, windows, spectral_line, head + [sizes] + x_dtype + [
        (dict(W=0), INVALID, "n_windows must be positive"),
        (dict(S=2050, D=1025), UNSUPPORTED, "windowed effective dimensionality: min(N, D) <= 1024 is supported")])
    got = run(plan_exe, [spectral_line(dict(SPECTRAL, n_alpha=0, alphas=(1,))), spectral_line(dict(SPECTRAL, eps=-1e-300)),
                         spectral_line(dict(SPECTRAL, alphas=(2, "inf", 1.0))), spectral_line(dict(SPECTRAL, alphas=(2, 1.0, "nan"))),
                         spectral_line(dict(SPECTRAL, n_alpha=16, alphas=(2, *([1.5] * 16)))), spectral_line(dict(SPECTRAL, eps=0.0)),
                         spectral_line(dict(SPECTRAL, S=2048, D=1025, W=2))])
    assert got[0] == ("err", INVALID, "matrix entropy: 1 .. 16 orders per call") and got[1] == ("err", INVALID, "matrix entropy: eps must be >= 0")
    assert got[2] == got[3] == ("err", INVALID, "matrix entropy: every order alpha must be finite and > 0")
    assert [g[0] for g in got[4:]] == ["ok"] * 3  # 16 orders, eps = 0, windows of exactly 1024 rows


def test_refusals_umap(plan_exe):
    metric = (dict(metric=2), UNSUPPORTED, "metric must be 'euclidean' or 'cosine'")
    knn = (dict(k=1), INVALID, "n_neighbors must be in [2, min(64, N)]")
    comp = (dict(c=0), INVALID, "n_components must be in [1, 8]")
    sgd = [(dict(epochs=0), INVALID, "n_epochs >= 1, negative_sample_rate >= 0"), (dict(a=0.0), INVALID, "a, b must be positive")]
    fit_lds = "UMAP: N * n_components too large for LDS"
    check_order(plan_exe, UMAP, umap_line, [
        (dict(args=0), INVALID, "args is NULL"), (dict(x=0), INVALID, "x and out are required"), (dict(N=1), INVALID, "need L >= 1, N >= 2, D >= 1"),
        (dict(dtype=3), INVALID, DTYPE), metric, (dict(N=4096), UNSUPPORTED, "UMAP: N < 4096 (umap-learn's exact small-data regime) is supported"),
        knn, comp, (dict(N=1601, c=8), UNSUPPORTED, fit_lds)] + sgd)
    got = run(plan_exe, [umap_line(dict(UMAP, **w)) for w in (
        dict(out=0), dict(L=0), dict(D=0), dict(k=65, N=100), dict(k=51), dict(c=9), dict(neg=-1), dict(b="nan"), dict(b=-1.0),
        dict(N=4095, c=1), dict(N=1600, c=8), dict(k=64, N=64), dict(k=50), dict(metric=1), dict(neg=0))])
    assert [g[2] for g in got[:9]] == ["x and out are required", "need L >= 1, N >= 2, D >= 1", "need L >= 1, N >= 2, D >= 1", knn[2], knn[2], comp[2],
                                       sgd[0][2], sgd[1][2], sgd[1][2]]
    assert [g[0] for g in got[9:]] == ["ok"] * 6  # N = 4095, the largest N * c in LDS, k = 64 = N, k = N, cosine, no negative samples
    ptrs = "x_train, emb_train, y and out are required"
    t_lds = "UMAP transform: (M, N) * n_components too large for LDS"
    check_order(plan_exe, TRANSFORM, transform_line, [
        (dict(args=0), INVALID, "args is NULL"), (dict(emb=0), INVALID, ptrs), (dict(M=0), INVALID, "need L >= 1, M >= 1, N >= 2, D >= 1"),
        (dict(dtype=3), INVALID, DTYPE), metric, (dict(N=8000, M=193), UNSUPPORTED, "UMAP transform: N + M <= 8192 (exact small-data regime) is supported"),
        knn, comp, (dict(N=4798, M=1, c=8), UNSUPPORTED, t_lds)] + sgd)
    got = run(plan_exe, [transform_line(dict(TRANSFORM, **w)) for w in (
        dict(xt=0), dict(y=0), dict(out=0), dict(L=0), dict(N=1), dict(D=0), dict(k=51), dict(N=8000, M=192, c=1), dict(N=4797, M=1, c=8))])
    assert [g[2] for g in got[:7]] == [ptrs] * 3 + ["need L >= 1, M >= 1, N >= 2, D >= 1"] * 3 + [knn[2]]
    assert [g[0] for g in got[7:]] == ["ok"] * 2  # N + M = 8192 and the largest (M, N) * c in LDS
