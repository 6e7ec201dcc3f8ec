"""CPU side of test_distance_paths.py: the kernel selection of every case is
pinned through tda_debug_dist_plan (host only), and the checker itself is
checked -- the oracle's sequential-k Gram form must stay inside dist_ref.bound
of the longdouble truth on every case input, and must be exact on the integer
grid.  If the oracle ever exceeds the bound, the bound is wrong, not a kernel."""
import ctypes

import numpy as np
import pytest

import dist_ref
from dist_ref import CASES, case_id, plan


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_path_table(pkg, built_lib, monkeypatch, case):
    n, d, dtype, env, want = case
    for k in ("TDA_DIST", "TDA_DIST_SPLIT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert plan(pkg, n, d, dtype) == want
    # every slice holds at least one K chunk
    assert want[1] <= max(1, -(-d // 32))


def test_path_hook_gate_and_arguments(pkg, built_lib, monkeypatch):
    """The overrides count only behind TDA_TEST_OVERRIDES=1; bad arguments are refused."""
    monkeypatch.setenv("TDA_DIST", "scalar")
    monkeypatch.setenv("TDA_DIST_SPLIT", "5")
    assert plan(pkg, 40, 1050, np.float32) == (0, 1, 0)
    monkeypatch.setenv("TDA_DIST", "tiles")
    assert plan(pkg, 40, 1050, np.float32) == (1, 5, 0)
    monkeypatch.setenv("TDA_TEST_OVERRIDES", "0")
    assert plan(pkg, 40, 1050, np.float32) == (1, 4, 1)
    L = pkg.lib()
    m = ctypes.c_int32()
    assert L.tda_debug_dist_plan(0, 8, 0, ctypes.byref(m), ctypes.byref(m), ctypes.byref(m)) == -1
    assert L.tda_debug_dist_plan(8, 8, 2, ctypes.byref(m), ctypes.byref(m), ctypes.byref(m)) == -1
    assert L.tda_debug_dist_plan(8, 8, 0, None, ctypes.byref(m), ctypes.byref(m)) == -1


SHAPES = sorted({(n, d, np.dtype(dt).name) for n, d, dt, _, _ in CASES})


@pytest.mark.parametrize("n,d,dtype", SHAPES, ids=[f"n{n}_d{d}_{t}" for n, d, t in SHAPES])
def test_oracle_within_bound_and_exact_on_grid(oracle, n, d, dtype):
    X = dist_ref.layers(n, d, np.dtype(dtype).type)
    worst = 0.0
    for l in range(3):
        t = dist_ref.truth(X[l])
        assert np.array_equal(t, t.T) and np.all(np.diag(t) == 0)
        got = oracle.distances(X[l])
        worst = max(worst, dist_ref.ratio(got, t, dist_ref.bound(X[l], t)))
        if l == 1:
            t1 = t
    print(f"oracle err/bound n{n} d{d} {dtype}: {worst:.3f}")
    assert worst <= 1.0
    assert t1[4, 5] == 0 and 0 < t1[4, 7] < 0.1
    exp = dist_ref.grid_expected(X[2])
    assert np.array_equal(oracle.distances(X[2]).view(np.uint32), exp.view(np.uint32))
    # the grid's truth agrees with the exact integers
    assert np.max(np.abs(dist_ref.truth(X[2]).astype(np.float64) - exp)) <= 2 * dist_ref.U32 * float(exp.max())
