"""Time heat_kernel_matrix (one GPU call) against the numpy float64 restatement
tests/hk_ref.py restatement_k on the same host, in one run.

Workloads (seeded diagrams, sigma 0.4):
  sweep64    128 diagrams of 64 points: 8,128 pairs and 128 selfs;
  sweep1024  128 diagrams of 1024 points: the same pairs;
  pair4096   2 diagrams of 4096 points (the limit): 1 pair and 2 selfs.

GPU side: 3 warm-up calls, then 10 timed; ``device_ms`` is the library's HIP
events around upload, kernels and download, wall the host clock around the
Python entry (numpy in, matrix out; the call ends in a stream synchronise);
median and spread (min .. max) in ms.  exp_per_s counts the two exponentials of
every term of every evaluation of the call (P + S of them) over the median
device time.  CPU side, as context: the restatement on one core, timed on at
most 8 of the call's evaluations and scaled to all of them by their terms
(``numpy_evaluations_timed`` says how many were run), and the largest difference
of those evaluations from the GPU's values beside their bound.

Usage: python tools/heat_prof.py [--workloads sweep64,sweep1024,pair4096] [--out FILE.json]
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
WORKLOADS = {"sweep64": (128, 64), "sweep1024": (128, 1024), "pair4096": (2, 4096)}  # diagrams, points
SIGMA = 0.4
NUMPY_EVALUATIONS = 8


def seeded(n_diagrams, n_points, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_diagrams):
        b = rng.uniform(0.0, 5.0, n_points)
        out.append(np.stack([b, b + rng.uniform(1e-3, 5.0, n_points)], 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--workloads", default="sweep64,sweep1024,pair4096")
    args = ap.parse_args()
    import hk_ref

    pkg = importlib.import_module("tda-multimodal_amd")
    if pkg.lib().tda_device_ok(0) != 1:
        raise SystemExit("heat_prof: no gfx950 device; nothing is measured without one")
    rows = []
    for name in args.workloads.split(","):
        if name not in WORKLOADS:
            raise SystemExit(f"unknown workload {name}")
        S, n = WORKLOADS[name]
        dgms = seeded(S, n, n)
        dev, wall = [], []
        for i in range(WARMUP + TIMED):
            t0 = time.perf_counter()
            K, ms = pkg.heat_kernel_matrix(dgms, SIGMA, return_time=True)
            t1 = time.perf_counter()
            if i >= WARMUP:
                dev.append(ms)
                wall.append((t1 - t0) * 1e3)
        stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}  # noqa: E731
        evaluations = S * (S - 1) // 2 + S
        exps = 2 * evaluations * n * n
        some = [(0, 0)] + [(i, i + 1) for i in range(min(S - 1, NUMPY_EVALUATIONS - 1))]
        t0 = time.perf_counter()
        ref = [hk_ref.restatement_k(dgms[i], dgms[j], SIGMA) for i, j in some]
        numpy_ms = (time.perf_counter() - t0) * 1e3 * evaluations / len(some)
        diff = max(abs(r - K[i, j]) for r, (i, j) in zip(ref, some))
        row = {"workload": name, "diagrams": S, "points_per_diagram": n, "sigma": SIGMA, "evaluations": evaluations, "exp": exps,
               "device_ms": stat(dev), "wall_ms": stat(wall), "exp_per_s": exps / (statistics.median(dev) * 1e-3),
               "numpy_wall_ms_scaled": numpy_ms, "numpy_evaluations_timed": len(some), "numpy_exp_per_s": exps / (numpy_ms * 1e-3),
               "max_abs_diff_vs_float64_restatement": float(diff), "bound_of_one_evaluation": hk_ref.bound_k(n, n, SIGMA)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
