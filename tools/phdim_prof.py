"""Times ph_dimension against what a user could do without tda_subsample_h0: one
ripser_batch(X, maxdim=0, want_dist=True) call for the library's distance matrices, then the minimum
spanning tree of every subsample on the host (scipy.sparse.csgraph.minimum_spanning_tree where scipy
imports, else the numpy Prim of tests/sh0_ref.py; the numpy Prim is timed as a second baseline either way).

Workloads: the 32 committed N = 36 layers, 4 Gaussian layers of N = 324, 1 layer of N = 2048; default
sizes, n_trials = 8.  Before any timing the deaths of every subsample are compared bit for bit with
tests/sh0_ref.py, and the host baseline's sorted MST weights with the sorted deaths.  Then two
warm-up rounds and RUNS timed rounds, the two sides alternated; the table gives the median and
(min .. max) of the wall time of each side and of the entry's device_ms.  Needs a gfx950 device.

    python tools/phdim_prof.py [--runs 7] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sh0_ref  # noqa: E402

try:
    from scipy.sparse.csgraph import minimum_spanning_tree
except ImportError:
    minimum_spanning_tree = None


def host_mst_weights(dm, pts, numpy_prim=False):
    """Sorted MST weights of one subsample (f32 values)."""
    if minimum_spanning_tree is None or numpy_prim:
        return np.sort(sh0_ref.prim(dm, pts)[1])
    pts = np.unique(pts)  # scipy reads a zero as no edge: coincident positions are merged (they die at 0)
    w = minimum_spanning_tree(dm[np.ix_(pts, pts)].astype(np.float64)).data
    return np.sort(w.astype(np.float32))


def baseline(pkg, X, idx, sz, numpy_prim=False):
    """The parent commit's route: distances from the pipeline, every MST on the host. -> E (L, B)"""
    res = pkg.ripser_batch(X, maxdim=0, want_dist=True)
    E = np.zeros((len(res), len(sz)))
    for l, r in enumerate(res):
        for b, n in enumerate(sz.tolist()):
            E[l, b] = host_mst_weights(r.dist, idx[b, :n], numpy_prim).astype(np.float64).sum()
    return E


def summary(ts):
    ts = np.asarray(ts)
    return f"{np.median(ts):.2f} ({ts.min():.2f} .. {ts.max():.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("tda-multimodal_amd")
    if pkg.lib().tda_device_ok(0) != 1:
        raise SystemExit("no gfx950 device at ordinal 0")
    z = np.load(os.path.join(ROOT, "tests", "golden", "reference_clouds.npz"))
    rng = np.random.default_rng(0)
    loads = [("32 x N=36 (committed layers)", np.stack([z[f"layer_{l}"] for l in range(32)]).astype(np.float32)),
             ("4 x N=324 (Gaussian, D=3)", rng.standard_normal((4, 324, 3)).astype(np.float32)),
             ("1 x N=2048 (Gaussian, D=3)", rng.standard_normal((1, 2048, 3)).astype(np.float32))]
    rows = []
    for name, X in loads:
        L, N = X.shape[0], X.shape[1]
        idx, sz = pkg.subsample_indices(N, pkg.phdim.default_sizes(N), 8, 0)
        # values first: deaths bit for bit against the restatement, the baseline's weights against the sorted deaths
        dm = np.stack([r.dist for r in pkg.ripser_batch(X, maxdim=0, want_dist=True)])
        E, D = pkg.h0_subsamples(X, idx, sz, deaths=True)
        for l in range(L):
            for b, n in enumerate(sz.tolist()):
                Er, dr = sh0_ref.prim(dm[l], idx[b, :n])
                assert D[l][b].astype(np.float32).tobytes() == dr.tobytes() and E[l, b] == Er, (name, l, b)
                w = host_mst_weights(dm[l], idx[b, :n])
                assert np.sort(dr[dr > 0]).tobytes() == w[w > 0].tobytes(), (name, l, b)
        t_new, t_old, t_np, t_dev = [], [], [], []
        for it in range(2 + a.runs):
            t0 = time.perf_counter()
            ph = pkg.ph_dimension(X)
            t1 = time.perf_counter()
            baseline(pkg, X, idx, sz)
            t2 = time.perf_counter()
            baseline(pkg, X, idx, sz, numpy_prim=True)
            t3 = time.perf_counter()
            print(f"{name}: round {it}: {(t1 - t0) * 1e3:.2f} {(t2 - t1) * 1e3:.2f} {(t3 - t2) * 1e3:.2f} ms", flush=True)
            if it >= 2:
                t_new.append((t1 - t0) * 1e3), t_old.append((t2 - t1) * 1e3), t_np.append((t3 - t2) * 1e3), t_dev.append(ph.device_ms)
        rows.append(dict(workload=name, B=int(len(sz)), ph_dimension_ms=summary(t_new), device_ms=summary(t_dev), host_mst_ms=summary(t_old),
                         host_numpy_prim_ms=summary(t_np), ratio=float(np.median(t_old) / np.median(t_new)),
                         ratio_numpy_prim=float(np.median(t_np) / np.median(t_new)), dimension=[float(v) for v in ph.dimension[:4]]))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(host_mst="scipy" if minimum_spanning_tree is not None else "sh0_ref (numpy Prim)", runs=a.runs, rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
