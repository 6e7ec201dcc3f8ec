"""CPU tests of the Frechet mean of persistence diagrams: the host plan (csrc/fm_plan.h) against a
numpy restatement, the reference tests/fm_ref.py against brute force, and the reference's own runs.
The entry's device side is not in the library (known limits), so nothing here loads it.

tests/fm_plan_main.cpp includes only fm_plan.h; it is compiled with g++ under the address and
undefined-behaviour sanitizers and run once per test as a program of its own, over text cases."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import fm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tda-multimodal_amd", "csrc")
INVALID, UNSUPPORTED = -1, -2
E0 = np.zeros((0, 2))
LIMITS = (64, 256, 512)


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fm_plan") / "fm_plan")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "fm_plan_main.cpp")], check=True)
    return exe


def diagrams(sizes, seed=0, junk=()):
    """offsets and points of diagrams of the given numbers of finite rows; diagram s in `junk` also
    gets three non-finite rows (at its start, in its middle and at its end)."""
    rng = np.random.default_rng(seed)
    rows, off = [], [0]
    for s, n in enumerate(sizes):
        b = rng.uniform(0, 5, n)
        d = np.stack([b, b + rng.uniform(0.1, 5, n)], 1)
        if s in junk:
            d = np.concatenate([[[np.nan, 1.0]], d[:n // 2], [[0.5, np.inf]], d[n // 2:], [[-np.inf, np.inf]]])
        rows.append(d)
        off.append(off[-1] + len(d))
    return off, np.concatenate(rows) if rows else E0


def nums(a):
    return [repr(float(x)) for x in np.asarray(a, np.float64).ravel()]


def run(exe, cases):
    """cases: dicts of off, pts and optionally S, init (an index or an (n, 2) array, None: NULL,
    "negative": init_n = -1, "null4": NULL with init_n = 4), max_iter, flags, reserved, or "null" -> per case ("err", code, message)
    or ("ok", {...})"""
    text = []
    for c in cases:
        if c == "null":
            text.append("null")
            continue
        off, pts, init = c["off"], c["pts"], c.get("init", 0)
        S = c.get("S", len(off) - 1 if off is not None else 0)
        t = ["fm", S]
        t += ["null"] if off is None else list(off)[:max(S, 0) + 1]  # the driver reads max(S, 0) + 1 offsets
        t += [-1] if pts is None else [len(pts), *nums(pts)]
        if isinstance(init, (int, np.integer)):
            t += [init, 0]
        elif init is None:
            t += [-1, -1]
        elif isinstance(init, str):
            t += [-1, -3 if init == "null4" else -2]
        else:
            t += [-1, len(init), *nums(init)]
        t += [c.get("max_iter", 100), c.get("flags", 0), c.get("reserved", 0)]
        text.append(" ".join(map(str, t)))
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]  # a sanitizer report ends the program with a non-zero status
    lines, out = r.stdout.split("\n"), []
    while lines and lines[0]:
        head = lines.pop(0).split(" ", 2)
        if head[0] == "err":
            out.append(("err", int(head[1]), head[2]))
            continue
        assert head[0] == "ok"
        S, K0, n_max, cls = (int(x) for x in (head[1] + " " + head[2]).split())
        got = {"S": S, "K0": K0, "n_max": n_max, "cls": cls}
        for name in ("off", "pts", "y0"):
            f = lines.pop(0).split()
            assert f[0] == name
            got[name] = [int(x) for x in f[1:]] if name == "off" else [float.fromhex(x) for x in f[1:]]
        out.append(("ok", got))
    assert len(out) == len(cases)
    return out


def expected(c):
    """The plan restated in numpy (the argument checks are listed where they are tested): the finite
    rows kept, the start the finite rows of diagram `init` or of the given array, the class of the
    first step the first limit that holds max(K0, n_max)."""
    off, pts, init = c["off"], E0 if c["pts"] is None else np.asarray(c["pts"], np.float64).reshape(-1, 2), c.get("init", 0)
    S = len(off) - 1
    fin = np.isfinite(pts).all(1)
    cnt = [int(fin[off[s]:off[s + 1]].sum()) for s in range(S)]
    if max(cnt) > 512:
        return "err", UNSUPPORTED, "frechet mean: a diagram with more than 512 finite points is not supported"
    if isinstance(init, (int, np.integer)):
        y0 = pts[off[init]:off[init + 1]][fin[off[init]:off[init + 1]]]
    else:
        y0 = E0 if init is None else fm_ref.finite_points(init)
        if len(y0) > 512:
            return "err", UNSUPPORTED, "frechet mean: a start with more than 512 finite points is not supported"
    n = max(len(y0), max(cnt))
    return "ok", {"S": S, "K0": len(y0), "n_max": max(cnt), "cls": int(np.searchsorted(LIMITS, n, side="left")),
                  "off": np.concatenate([[0], np.cumsum(cnt)]).tolist(), "pts": pts[:off[S]][fin[:off[S]]].ravel().tolist(), "y0": y0.ravel().tolist()}


def check(exe, cases):
    got = run(exe, cases)
    exp = [expected(c) for c in cases]
    for g, e, c in zip(got, exp, cases):
        assert g == e, (c["off"], c.get("init", 0))
        if g[0] == "ok":  # == takes -0.0 for 0.0: the rows are kept bit for bit
            assert all(np.array(g[1][k]).tobytes() == np.array(e[1][k]).tobytes() for k in ("pts", "y0"))
    return exp


def test_plan_drops_non_finite_rows_and_takes_the_start(plan_exe):
    nan, inf = np.nan, np.inf
    pts = [[0, 1], [nan, 1], [0, nan], [1, 2], [inf, 3], [1, inf], [-inf, 0], [0, -inf], [2, 3], [nan, inf],  # diagram 0: 3 finite
           [0, inf], [nan, nan], [-inf, inf],  # diagram 1: empty after the filter
           [4, 5]]
    off = [0, 10, 13, 13, 14]  # diagram 2 has no rows at all
    start = [[0.5, inf], [1, 2], [nan, 0], [-0.0, 3.5]]
    pts[0][0] = -0.0  # a sign bit in a diagram's row as well
    exp = check(plan_exe, [dict(off=off, pts=pts, init=i) for i in (0, 1, 2, 3)] + [dict(off=off, pts=pts, init=start), dict(off=off, pts=pts, init=None)])
    assert exp[0][1]["off"] == [0, 3, 3, 3, 4] and exp[0][1]["pts"] == [0, 1, 1, 2, 2, 3, 4, 5]
    assert [e[1]["y0"] for e in exp] == [[0, 1, 1, 2, 2, 3], [], [], [4, 5], [1, 2, -0.0, 3.5], []]
    off, pts = diagrams([40, 25, 0, 130], seed=3, junk=(0, 2, 3))
    exp = check(plan_exe, [dict(off=off, pts=pts, init=i) for i in range(4)])
    assert [e[1]["K0"] for e in exp] == [40, 25, 0, 130] and {e[1]["cls"] for e in exp} == {1}


def test_plan_empty_diagrams_and_a_single_one(plan_exe):
    exp = check(plan_exe, [dict(off=[0, 0, 0], pts=E0), dict(off=[0, 0], pts=E0), dict(off=[0, 0], pts=None, init=None)])
    assert all(e[1]["K0"] == 0 and e[1]["n_max"] == 0 and e[1]["cls"] == 0 for e in exp)
    off, pts = diagrams([7], seed=1, junk=(0,))
    (_, one), = check(plan_exe, [dict(off=off, pts=pts)])
    assert one["S"] == 1 and one["K0"] == 7 and one["y0"] == one["pts"]


def test_plan_class_limits(plan_exe):
    """Counts exactly at 64 / 65 / 256 / 257 / 512 / 513, in a diagram or in the start; the non-finite rows do not count."""
    cases, want = [], []
    for n, cls in ((64, 0), (65, 1), (256, 1), (257, 2), (512, 2)):
        off, pts = diagrams([3, n], seed=n, junk=(1,))
        cases += [dict(off=off, pts=pts, init=0), dict(off=off, pts=pts, init=1)]  # by the largest diagram, whatever the start
        off2, pts2 = diagrams([3, 5], seed=n)
        cases.append(dict(off=off2, pts=pts2, init=pts[off[1]:off[2]]))  # by the start
        want += [cls] * 3
    exp = check(plan_exe, cases)
    assert [e[1]["cls"] for e in exp] == want
    off, pts = diagrams([3, 513], seed=513, junk=(1,))
    off2, pts2 = diagrams([3, 5], seed=2)
    exp = check(plan_exe, [dict(off=off, pts=pts), dict(off=off2, pts=pts2, init=pts[off[1]:off[2]])])
    assert [e[0] for e in exp] == ["err", "err"] and "diagram" in exp[0][2] and "start" in exp[1][2]
    # the class of a later step, from (K, max n_j), and the layout of G: (S, K) row-major
    r = subprocess.run([plan_exe], input="".join(f"cls {K} {n}\n" for K, n in ((0, 0), (64, 1), (1, 64), (65, 64), (3, 256), (257, 9), (512, 512), (513, 2), (2, 513))),
                       capture_output=True, text=True, check=True)
    assert r.stdout.split("\n")[:-1] == ["cls 0 0", "cls 0 192", "cls 0 3", "cls 1 195", "cls 1 9", "cls 2 771", "cls 2 1536", "cls -1 1539", "cls -1 6"]


def test_plan_refusals_in_their_order(plan_exe):
    off, pts = diagrams([3, 4, 5], seed=5)
    good = dict(off=off, pts=pts)
    many = [0] * 4098
    cases = [
        ("null", INVALID, "args is NULL"),
        (dict(good, S=-1), INVALID, "S must be >= 0"),
        (dict(good, off=None, S=3), INVALID, "offsets is NULL"),
        (dict(good, reserved=1), INVALID, "reserved must be 0"),
        (dict(good, flags=2), INVALID, "flags holds an unknown bit"),
        (dict(good, flags=-1), INVALID, "flags holds an unknown bit"),
        (dict(good, max_iter=0), INVALID, "max_iter must be >= 1"),
        (dict(good, max_iter=1025), UNSUPPORTED, "frechet mean: max_iter > 1024 is not supported"),
        (dict(off=[0], pts=E0, S=0), INVALID, "S must be >= 1"),
        (dict(off=many, pts=E0, init=None), UNSUPPORTED, "frechet mean: more than 4096 diagrams in one call is not supported"),
        (dict(good, off=[1, 3, 7, 12]), INVALID, "offsets[0] must be 0"),
        (dict(good, off=[0, 7, 3, 12]), INVALID, "offsets must be non-decreasing"),
        (dict(good, pts=None), INVALID, "points is NULL"),
        (dict(good, init=3), INVALID, "init_index must be -1 or in [0, S)"),
        (dict(good, init=-2), INVALID, "init_index must be -1 or in [0, S)"),
        (dict(good, init="negative"), INVALID, "init_n must be >= 0"),
        (dict(good, init="null4"), INVALID, "init_points is NULL"),
        # the checks in their order: each bad call also carries the later faults
        (dict(good, reserved=1, flags=2, max_iter=0, off=[1, 3, 7, 12], init=9), INVALID, "reserved must be 0"),
        (dict(good, flags=2, max_iter=0, off=[1, 3, 7, 12], init=9), INVALID, "flags holds an unknown bit"),
        (dict(good, max_iter=1025, off=[1, 3, 7, 12], init=9), UNSUPPORTED, "frechet mean: max_iter > 1024 is not supported"),
        (dict(good, off=[1, 3, 7, 12], init=9), INVALID, "offsets[0] must be 0"),
    ]
    assert run(plan_exe, [c for c, _, _ in cases]) == [("err", code, m) for _, code, m in cases]
    # at the limits: accepted
    ok = run(plan_exe, [dict(good, max_iter=1), dict(good, max_iter=1024, flags=1), dict(off=many[:4097], pts=E0, init=None)])
    assert [o[0] for o in ok] == ["ok"] * 3 and ok[2][1]["S"] == 4096


# ---------------------------------------------------------------- the reference against brute force
def partial_matchings(K, n):
    """Every map of K points into n others or -1, injective on its hits."""
    for m in itertools.product(range(-1, n), repeat=K):
        hit = [x for x in m if x >= 0]
        if len(set(hit)) == len(hit):
            yield np.array(m, np.int64).reshape(K)


@pytest.mark.parametrize("seed", range(3))
def test_reference_solver_against_all_partial_matchings(seed):
    rng = np.random.default_rng(seed)
    for K in range(5):
        for n in range(5):
            b, c = rng.uniform(0, 2, K), rng.uniform(0, 2, n)
            Y, X = np.stack([b, b + rng.uniform(1e-3, 2, K)], 1), np.stack([c, c + rng.uniform(1e-3, 2, n)], 1)
            best = min(fm_ref.check_matching(Y, X, m) for m in partial_matchings(K, n))
            got = fm_ref.check_matching(Y, X, fm_ref.solve(Y, X))
            assert abs(got - best) <= fm_ref.bound(Y, X), (K, n)
            assert fm_ref.cost_f64(Y, X, fm_ref.solve(Y, X)) == pytest.approx(float(best), rel=1e-14, abs=1e-300)


def test_reference_update_is_the_minimiser():
    """The point of k partners among S diagrams does not lose to its 8 neighbours at +-1e-6 in
    sum |y - x|^2 + (S - k) dist^2(y, diagonal), evaluated in longdouble."""
    ld = np.longdouble
    rng = np.random.default_rng(4)

    def objective(y, P, S):
        return sum((ld(y[0]) - ld(p[0])) ** 2 + (ld(y[1]) - ld(p[1])) ** 2 for p in P) + (S - len(P)) * (ld(y[1]) - ld(y[0])) ** 2 / 2

    for S, k in ((1, 1), (2, 1), (3, 2), (4, 4), (7, 3), (128, 1), (128, 77)):
        b = rng.uniform(0, 5, k)
        P = np.stack([b, b + rng.uniform(1e-3, 5, k)], 1)
        Xs = [P[j:j + 1] if j < k else E0 for j in range(S)]
        Yn = fm_ref.update(P[:1], Xs, [np.array([0 if j < k else -1]) for j in range(S)])
        assert Yn.shape == (1, 2)
        y = Yn[0]
        f0 = objective(y, P, S)
        for db, dd in itertools.product((-1e-6, 0.0, 1e-6), repeat=2):
            assert f0 <= objective((y[0] + db, y[1] + dd), P, S) or (db == 0.0 and dd == 0.0)
    # the order of the next diagram: survivors in their order (a point without a partner is dropped), then the points no y took by (j, i)
    Y = np.array([[0.0, 1.0], [5.0, 6.0], [2.0, 4.0]])
    Xs = [np.array([[0.0, 2.0], [9.0, 10.0]]), np.array([[2.0, 6.0], [7.0, 8.0], [0.0, 4.0]])]
    Yn = fm_ref.update(Y, Xs, [np.array([0, -1, -1]), np.array([2, -1, 0])])
    assert Yn.tolist() == [[0.0, 3.0], [3.0, 5.0], [9.25, 9.75], [7.25, 7.75]]


def seeded(n, seed):
    rng = np.random.default_rng(seed)
    b = rng.uniform(0.0, 5.0, n)
    return np.stack([b, b + rng.uniform(1e-3, 5.0, n)], 1)


@pytest.mark.parametrize("name", ("S4", "S8x20"))
def test_reference_run_converges_and_its_energy_never_rises(name):
    Xs = [seeded(n, 10 + n) for n in (5, 7, 6, 3)] if name == "S4" else [seeded(20, 30 + j) for j in range(8)]
    Y, converged, energy = fm_ref.run(Xs, max_iter=10)
    assert converged and len(energy) <= 10
    # the same steps once more, for each step's summation bound (fm_ref.energy_bound, from the step's own K_j and costs)
    Yt, tol = Xs[0], []
    for E in energy:
        Yn, Et, G = fm_ref.step(Yt, Xs)
        assert Et == E
        tol.append(fm_ref.energy_bound(Yt, Xs, G))
        Yt = Yn
    assert Yt.tobytes() == Y.tobytes()
    for i in range(len(energy) - 1):
        assert energy[i + 1] <= energy[i] + tol[i] + tol[i + 1]
    Y2, E2, _ = fm_ref.step(Y, Xs)
    assert Y2.tobytes() == Y.tobytes() and E2 == energy[-1]
