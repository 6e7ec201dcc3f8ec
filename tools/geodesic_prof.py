"""Measure geodesic_distances against what the library allowed before it: the layers' distance
matrices read back (ripser_batch(X, maxdim=0, want_dist=True)) and scipy's shortest_path per layer on
the host, both as Dijkstra on the sparse graph (method="D") and as Floyd-Warshall on the dense one
(method="FW").

The results are checked against tests/geo_ref.py first.  Then 7 rounds after 2 warm-ups, the sides
alternated within a round; median (min .. max) of the call's wall time, the entry's device_ms and
the ratios.  For the blocked closure the achieved min-plus operations per second stand beside the
f32 vector peak.  One min-plus operation is one addition and one minimum.  The count is what the
schedule performs: per round one closure of the diagonal tile, T - 1 row products and T (T - 1) / 2
products of the rest, T (T + 1) / 2 tiles of 64^3 operations each, over T = ceil(N / 64) rounds (the
mirror tiles are stored, not computed; the pad's share is counted, as it is performed).

    python tools/geodesic_prof.py [--out FILE]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

WORKLOADS = [("32 x 36", 32, 36), ("4 x 324", 4, 324), ("1 x 2048", 1, 2048)]
K = 6
ROUNDS, WARMUP = 7, 2
# MI355X: 157.3 TFLOP/s of f32 vector arithmetic counts a fused multiply-add as two operations.  An addition or a
# minimum fills the slot of one FMA, so the most the same pipes can give of them is half that figure per second.
F32_VECTOR_SLOTS = 157.3e12 / 2


def fmt(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import geo_ref
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import shortest_path

    pkg = importlib.import_module("tda-multimodal_amd")
    rows = []
    for name, L, N in WORKLOADS:
        X = np.stack([np.random.default_rng(100 * N + l).standard_normal((N, 3)).astype(np.float32) for l in range(L)])

        def ours():
            t = time.perf_counter()
            g = pkg.geodesic_distances(X, n_neighbors=K)
            return (time.perf_counter() - t) * 1e3, g

        def host(method):
            t = time.perf_counter()
            dm = [r.dist for r in pkg.ripser_batch(X, maxdim=0, want_dist=True)]
            t_dm = (time.perf_counter() - t) * 1e3
            out = []
            for d in dm:
                W, _ = geo_ref.graph(d, K)
                if method == "D":
                    fin = np.isfinite(W) & ~np.eye(N, dtype=bool)
                    r_, c_ = np.nonzero(fin)
                    out.append(shortest_path(csr_matrix((W[r_, c_].astype(np.float64), (r_, c_)), shape=(N, N)), method="D", directed=False))
                else:
                    out.append(shortest_path(np.where(np.isfinite(W), W, 0.0).astype(np.float64), method="FW", directed=False))
            return (time.perf_counter() - t) * 1e3, t_dm, out

        # correctness first: the graph bit for bit, the closure within the header's bound
        _, g = ours()
        dm = pkg.geodesic_distances(X, radius=float("inf"), graph_only=True).dist
        Wg = pkg.geodesic_distances(X, n_neighbors=K, graph_only=True).dist
        for l in range(L):
            W, G, nc, ne = geo_ref.geodesic(dm[l], K)
            assert Wg[l].tobytes() == W.tobytes() and g.n_components[l] == nc and g.n_edges[l] == ne
            fin = np.isfinite(G) & (G > 0)
            assert np.array_equal(np.isinf(g.dist[l]), np.isinf(G))
            assert (np.abs(g.dist[l].astype(np.float64)[fin] - G[fin]) <= geo_ref.bound(N) * G[fin]).all()
        wall, dev, hD, hFW = [], [], [], []
        for r in range(WARMUP + ROUNDS):
            w, g = ours()
            d = host("D")[0]
            f = host("FW")[0] if N <= 324 or r >= WARMUP + ROUNDS - 3 else None  # dense FW at N = 2048 takes seconds: 3 rounds
            if r >= WARMUP:
                wall.append(w), dev.append(g.device_ms), hD.append(d)
                if f is not None:
                    hFW.append(f)
        row = dict(workload=name, k=K, wall_ms=fmt(wall), device_ms=fmt(dev), host_dijkstra_ms=fmt(hD), host_fw_ms=fmt(hFW),
                   ratio_dijkstra=statistics.median(hD) / statistics.median(wall), ratio_fw=statistics.median(hFW) / statistics.median(wall))
        if N > geo_ref.LDS_N:
            T = -(-N // 64)
            ops = L * T * (T * (T + 1) // 2) * 64 ** 3  # T rounds of 1 + (T - 1) + T (T - 1) / 2 tiles, 64^3 each
            row["minplus_per_s"] = ops / (statistics.median(dev) * 1e-3)
            row["of_f32_vector_peak"] = row["minplus_per_s"] * 2 / F32_VECTOR_SLOTS  # a min-plus operation takes two slots
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
