"""Time fisher_matrix (one GPU call) beside heat_kernel_matrix on the same diagrams and the
numpy float64 restatement tests/pf_ref.py on the same host, in one run.

Workloads (seeded diagrams, sigma 1.0 for fisher and 0.4 for heat):
  sweep64    128 diagrams of 64 points: 8,128 pairs;
  sweep1024  128 diagrams of 1024 points (the limit): the same pairs;
  pair1024   2 diagrams of 1024 points: 1 pair.

GPU side, for both entries: 3 warm-up calls, then 10 timed; ``device_ms`` is the library's HIP
events around upload, kernels and download, wall the host clock around the Python entry (numpy
in, matrix out; the call ends in a stream synchronise); median and spread (min .. max) in ms.
exp_per_s counts the exponentials of the call over the median device time: 4 (n1 + n2)^2 per
pair for fisher, 2 n1 n2 per evaluation (the pairs and the selfs) for heat.
``device_ratio_to_heat`` stands beside ``exp_ratio_to_heat``.  CPU side, as context: the
restatement on one core, timed on at most 4 of the call's pairs and scaled to all of them
(``numpy_pairs_timed`` says how many were run), and the largest difference of those pairs'
affinities from the GPU's beside their bound.

Usage: python tools/fisher_prof.py [--workloads sweep64,sweep1024,pair1024] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP, TIMED = 3, 10
WORKLOADS = {"sweep64": (128, 64), "sweep1024": (128, 1024), "pair1024": (2, 1024)}  # diagrams, points
SIGMA, HEAT_SIGMA = 1.0, 0.4
NUMPY_PAIRS = 4


def seeded(n_diagrams, n_points, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_diagrams):
        b = rng.uniform(0.0, 5.0, n_points)
        out.append(np.stack([b, b + rng.uniform(1e-3, 5.0, n_points)], 1))
    return out


def timed(fn):
    """(last result, device ms, wall ms) of WARMUP + TIMED calls of fn() -> (result, device_ms); the timed ones kept."""
    dev, wall = [], []
    for i in range(WARMUP + TIMED):
        t0 = time.perf_counter()
        out, ms = fn()
        t1 = time.perf_counter()
        if i >= WARMUP:
            dev.append(ms)
            wall.append((t1 - t0) * 1e3)
    return out, dev, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--workloads", default="sweep64,sweep1024,pair1024")
    args = ap.parse_args()
    import pf_ref

    pkg = importlib.import_module("tda-multimodal_amd")
    if pkg.lib().tda_device_ok(0) != 1:
        raise SystemExit("fisher_prof: no gfx950 device; nothing is measured without one")
    rows = []
    stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}  # noqa: E731
    for name in args.workloads.split(","):
        if name not in WORKLOADS:
            raise SystemExit(f"unknown workload {name}")
        S, n = WORKLOADS[name]
        dgms = seeded(S, n, n)
        D, dev, wall = timed(lambda: pkg.fisher_matrix(dgms, SIGMA, return_time=True))
        _, hdev, hwall = timed(lambda: pkg.heat_kernel_matrix(dgms, HEAT_SIGMA, return_time=True))
        pairs = S * (S - 1) // 2
        exps, hexps = pairs * 4 * (2 * n) ** 2, 2 * (pairs + S) * n * n
        some = [(i, i + 1) for i in range(min(S - 1, NUMPY_PAIRS))]
        t0 = time.perf_counter()
        ref = [pf_ref.affinity_of(*pf_ref.sums(dgms[i], dgms[j], SIGMA)) for i, j in some]
        numpy_ms = (time.perf_counter() - t0) * 1e3 * pairs / len(some)
        diff = max(abs(r - np.cos(D[i, j])) for r, (i, j) in zip(ref, some))  # the affinity back from the distance: context only
        med, hmed = statistics.median(dev), statistics.median(hdev)
        row = {"workload": name, "diagrams": S, "points_per_diagram": n, "sigma": SIGMA, "pairs": pairs, "exp": exps,
               "device_ms": stat(dev), "wall_ms": stat(wall), "exp_per_s": exps / (med * 1e-3),
               "heat": {"sigma": HEAT_SIGMA, "evaluations": pairs + S, "exp": hexps, "device_ms": stat(hdev), "wall_ms": stat(hwall),
                        "exp_per_s": hexps / (hmed * 1e-3)},
               "device_ratio_to_heat": med / hmed, "exp_ratio_to_heat": exps / hexps,
               "numpy_wall_ms_scaled": numpy_ms, "numpy_pairs_timed": len(some), "numpy_exp_per_s": exps / (numpy_ms * 1e-3),
               "max_abs_affinity_diff_vs_float64_restatement": float(diff), "bound_of_one_pair": pf_ref.bound(n, n)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
