"""Time persistence_landscapes and persistence_images (one GPU call each) against
the numpy restatements tests/pl_ref.py and tests/pi_ref.py on the same host, in
one run.

Workloads (seeded diagrams; landscape depth 10 x 500 steps, image 32 x 32, sigma 0.25):
  rand20     128 diagrams of 20 points (the size of a sweep's H1 diagrams);
  rand1024   32 diagrams of 1024 points;
  rand4096   8 diagrams of 4096 points (the limit).

GPU side: 3 warm-up calls, then 10 timed; ``device_ms`` is the library's HIP
events around upload, kernels and download, wall the host clock around the
Python entry (numpy in, array out; the call ends in a stream synchronise);
median and spread (min .. max) in ms.  CPU side: the restatement once, one core,
as context and not as a competitor: pl_ref sorts every tent per grid value,
pi_ref.restatement calls libm's erf from Python.  The landscape is compared
bit for bit with its restatement; the image's largest difference from the
float64 restatement is reported (the tests hold it to the 40-digit reference).

Usage: python tools/vectorize_prof.py [--workloads rand20,rand1024,rand4096] [--out FILE.json]
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
WORKLOADS = {"rand20": (128, 20), "rand1024": (32, 1024), "rand4096": (8, 4096)}  # diagrams, points
DEPTH, STEPS, RES, SIGMA = 10, 500, (32, 32), 0.25
RANGE = (0.0, 10.0), (0.0, 5.0)


def seeded(n_diagrams, n_points, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_diagrams):
        b = rng.uniform(0.0, 5.0, n_points)
        out.append(np.stack([b, b + rng.uniform(1e-3, 5.0, n_points)], 1))
    return out


def timed(fn):
    dev, wall = [], []
    for i in range(WARMUP + TIMED):
        t0 = time.perf_counter()
        out, ms = fn()
        t1 = time.perf_counter()
        if i >= WARMUP:
            dev.append(ms)
            wall.append((t1 - t0) * 1e3)
    stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}  # noqa: E731
    return out, stat(dev), stat(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--workloads", default="rand20,rand1024,rand4096")
    args = ap.parse_args()
    import pi_ref
    import pl_ref

    pkg = importlib.import_module("tda-multimodal_amd")
    if pkg.lib().tda_device_ok(0) != 1:
        raise SystemExit("vectorize_prof: no gfx950 device; nothing is measured without one")
    rows = []
    for name in args.workloads.split(","):
        if name not in WORKLOADS:
            raise SystemExit(f"unknown workload {name}")
        S, n = WORKLOADS[name]
        dgms = seeded(S, n, n)
        (pl, grid), pl_dev, pl_wall = timed(lambda: (lambda o, g, ms: ((o, g), ms))(*pkg.persistence_landscapes(
            dgms, num_steps=STEPS, depth=DEPTH, return_grid=True, return_time=True)))
        t0 = time.perf_counter()
        ref = pl_ref.landscapes(dgms, grid, DEPTH)
        pl_ref_ms = (time.perf_counter() - t0) * 1e3
        im, pi_dev, pi_wall = timed(lambda: pkg.persistence_images(dgms, RANGE[0], RANGE[1], RES, SIGMA, return_time=True))
        xe, ye = np.linspace(*RANGE[0], RES[0] + 1), np.linspace(*RANGE[1], RES[1] + 1)
        t0 = time.perf_counter()
        ref_im = np.stack([pi_ref.restatement(D, xe, ye, SIGMA) for D in dgms])
        pi_ref_ms = (time.perf_counter() - t0) * 1e3
        row = {
            "workload": name, "diagrams": S, "points_per_diagram": n,
            "landscape": {"depth": DEPTH, "steps": STEPS, "device_ms": pl_dev, "wall_ms": pl_wall, "numpy_wall_ms": pl_ref_ms,
                          "equals_restatement": bool(np.array_equal(pl, ref))},
            "image": {"resolution": list(RES), "sigma": SIGMA, "device_ms": pi_dev, "wall_ms": pi_wall, "numpy_wall_ms": pi_ref_ms,
                      "max_abs_diff_vs_float64_restatement": float(np.abs(im - ref_im).max()),
                      "bound_of_first_diagram": pi_ref.bound(dgms[0])},
        }
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
