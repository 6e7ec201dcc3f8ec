"""Every launch path of the distance stage (dist_select, csrc/rips_plan.h) against
a longdouble truth with a derived bound (tests/dist_ref.py), the oracle, the
exact integer grid, and persistence on the matrix actually returned.

One ripser_batch call per case: 3 layers (dist_ref.layers), maxdim 1,
want_dist (f64 cases: want_dist64 too).  The path each case was written for is
checked through tda_debug_dist_plan first, so a change to dist_select cannot
quietly move a case to another kernel."""
import functools

import numpy as np
import pytest

import dist_ref
from dist_ref import CASES, case_id, plan
from test_gpu_parity import TOL, assert_same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pkg, built_lib):
    import torch

    torch.cuda.init()  # torch's HIP runtime first, as in test_gpu_parity.py
    assert pkg.lib().tda_device_ok(0) == 1, "no gfx950 device visible"
    return pkg


@functools.lru_cache(maxsize=None)
def reference(n, d, dtype_name):
    """Input, truth and bounds of a shape, computed once and shared (read-only)."""
    X = dist_ref.layers(n, d, np.dtype(dtype_name).type)
    t = [dist_ref.truth(X[l]) for l in range(3)]
    b = [dist_ref.bound(X[l], t[l]) for l in range(3)]
    b64 = [dist_ref.bound64(X[l], t[l]) for l in range(3)] if X.dtype == np.float64 else None
    for a in [X] + t + b + (b64 or []):
        a.setflags(write=False)
    return X, t, b, b64


def set_env(monkeypatch, env):
    for k in ("TDA_DIST", "TDA_DIST_SPLIT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def check_layers(res, X, t, b, b64, oracle, tag):
    """Assertions 1 to 5 of a batch result; returns (largest err/bound, duplicate pair's value)."""
    f64 = X.dtype == np.float64
    worst = 0.0
    for l in range(3):
        got = res[l].dist
        # 3. shape of the matrix
        assert got.dtype == np.float32 and np.all(np.isfinite(got)), (tag, l)
        assert np.array_equal(got, got.T) and np.all(np.diag(got) == 0), (tag, l)
        # 1. the truth
        r = dist_ref.ratio(got, t[l], b[l])
        worst = max(worst, r)
        assert r <= 1.0, (tag, l, r)
        # 2. the oracle (layer 1: the oracle's sequential sums give the duplicate pair exactly 0,
        # the Gram form in another order need not -- assertion 1 covers it)
        if l != 1:
            ref = oracle.distances(X[l])
            rel = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.maximum(1.0, ref.astype(np.float64))
            assert rel.max() <= TOL, (tag, l, float(rel.max()))
            same = np.mean(got.view(np.uint32) == ref.view(np.uint32))
            assert same > 0.9, (tag, l, same)
        if l == 2:
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (tag, "grid vs oracle")
            assert np.array_equal(got.view(np.uint32), dist_ref.grid_expected(X[2]).view(np.uint32)), (tag, "grid vs exact")
        # 4. persistence (threshold from the row maxima, edge count, H0, H1) on the matrix returned
        assert_same(res[l], oracle.rips_dm(got, 1), 1, f"{tag} l{l}")
        # 5. the f64 matrix
        if f64:
            g64 = res[l].dist64
            assert g64 is not None and g64.dtype == np.float64 and np.all(np.isfinite(g64)), (tag, l)
            assert np.array_equal(g64, g64.T) and np.all(np.diag(g64) == 0), (tag, l)
            r64 = dist_ref.ratio(g64, t[l], b64[l])
            assert r64 <= 1.0, (tag, l, r64)
            assert np.array_equal(got.view(np.uint32), g64.astype(np.float32).view(np.uint32)), (tag, l)
    return worst, float(res[1].dist[4, 5])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_distance_path(gpu, oracle, monkeypatch, case):
    n, d, dtype, env, want = case
    tag = case_id(case)
    set_env(monkeypatch, env)
    assert plan(gpu, n, d, dtype) == want, tag
    X, t, b, b64 = reference(n, d, np.dtype(dtype).name)
    f64 = X.dtype == np.float64
    res = gpu.ripser_batch(X, maxdim=1, want_dist=True, want_dist64=f64)
    worst, dup = check_layers(res, X, t, b, b64, oracle, tag)
    print(f"{tag}: path (mfma, dsplit, gram_layer) = {want}, max err/bound = {worst:.3f}, dist(4, 5) of layer 1 = {dup:.3e}, "
          f"dist(4, 7) = {float(res[1].dist[4, 7]):.6e} (truth {float(t[1][4, 7]):.6e})")
    # 6. layer stride of the partial buffers: layer 1 alone returns the bits it has inside the batch
    one = gpu.ripser_batch(X[1:2], maxdim=1, want_dist=True, want_dist64=f64)[0]
    assert np.array_equal(one.dist.view(np.uint32), res[1].dist.view(np.uint32)), tag
    if f64:
        assert np.array_equal(one.dist64.view(np.uint64), res[1].dist64.view(np.uint64)), tag


@pytest.mark.parametrize("n,d,dtype,forced", [(40, 1050, np.float32, {"TDA_DIST_SPLIT": "5"}),
                                              (40, 1050, np.float32, {"TDA_DIST": "tiles"}),
                                              (65, 260, np.float64, {"TDA_DIST_SPLIT": "7"})])
def test_forced_plan_is_not_replayed_for_another(gpu, oracle, monkeypatch, n, d, dtype, forced):
    """Two calls of one (L, N, D) that differ only in TDA_DIST_SPLIT / TDA_DIST=tiles have different
    partial-buffer sizes, hence different workspace offsets: a captured graph of one must not be
    replayed for the other.  The forced (larger) plan runs first, so the workspace does not grow
    (and drop its graphs) in between; every call is checked in full."""
    X, t, b, b64 = reference(n, d, np.dtype(dtype).name)
    f64 = X.dtype == np.float64
    bits = {}
    for step, env in enumerate((forced, {}, forced, {})):
        set_env(monkeypatch, env)
        res = gpu.ripser_batch(X, maxdim=1, want_dist=True, want_dist64=f64)
        check_layers(res, X, t, b, b64, oracle, f"n{n}_d{d} step {step} {env}")
        key = bool(env)
        cur = np.stack([res[l].dist for l in range(3)]).view(np.uint32)
        assert key not in bits or np.array_equal(bits[key], cur), (step, env)
        bits[key] = cur
