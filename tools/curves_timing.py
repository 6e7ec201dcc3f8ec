"""Time persistence_curves (one GPU call) against the numpy restatement tests/pc_ref.py and,
for the tent kernel, against persistence_landscapes(depth=1) on the same input: the closest entry
that existed before the curves, with the same O(n G) tents per diagram.

Shapes (seeded diagrams, diagrams x points x grid values):
  sweep32     32 x 40 x 100      one sweep's H1 diagrams;
  sweep4096   4096 x 40 x 100    128 sweeps in one call;
  large       128 x 4096 x 4096  the point limit on the longest grid.

Two curves per shape: "betti" (indicator, no coefficients) and "silhouette" (tent, coefficients
d - b, normalised).  GPU side: 3 warm-up calls, then 10 timed; ``device_ms`` is the library's HIP
events around upload, kernels and download, wall the host clock around the Python entry (numpy
in, array out; the call ends in a stream synchronise); median and spread (min .. max) in ms.  CPU
side: pc_ref once, one core, as context: a Python loop over the points.  On the large shape
pc_ref runs on the first REF_DIAGRAMS diagrams only and the row says so (``numpy_diagrams``).
Every GPU result is compared bit for bit with what pc_ref computed.

Usage: python tools/curves_timing.py [--shapes sweep32,sweep4096,large] [--out FILE.json]
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
SHAPES = {"sweep32": (32, 40, 100), "sweep4096": (4096, 40, 100), "large": (128, 4096, 4096)}  # diagrams, points, grid values
REF_DIAGRAMS = 8  # of the large shape


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
    ap.add_argument("--shapes", default="sweep32,sweep4096,large")
    args = ap.parse_args()
    import pc_ref

    pkg = importlib.import_module("tda-multimodal_amd")
    if pkg.lib().tda_device_ok(0) != 1:
        raise SystemExit("curves_timing: no gfx950 device; nothing is measured without one")
    rows = []
    for name in args.shapes.split(","):
        if name not in SHAPES:
            raise SystemExit(f"unknown shape {name}")
        S, n, G = SHAPES[name]
        dgms = seeded(S, n, n + S)
        allp = np.concatenate(dgms)
        lo, hi = float(allp[:, 0].min()), float(allp[:, 1].max())
        grid = np.linspace(lo, hi, G)
        life = [D[:, 1] - D[:, 0] for D in dgms]
        n_ref = S if name != "large" else REF_DIAGRAMS
        row = {"shape": name, "diagrams": S, "points_per_diagram": n, "grid_values": G, "numpy_diagrams": n_ref}
        for curve, kw in (("betti", dict(coef=None, kernel="indicator", normalize=False)),
                          ("silhouette", dict(coef=life, kernel="tent", normalize=True))):
            out, dev, wall = timed(lambda: pkg.persistence_curves(dgms, grid, return_time=True, **kw))
            t0 = time.perf_counter()
            ref = pc_ref.curves(dgms[:n_ref], grid, None if kw["coef"] is None else life[:n_ref], kernel=kw["kernel"], normalize=kw["normalize"])
            ref_ms = (time.perf_counter() - t0) * 1e3
            row[curve] = {"device_ms": dev, "wall_ms": wall, "numpy_wall_ms": ref_ms, "equals_restatement": bool(np.array_equal(out[:n_ref], ref))}
        _, dev, wall = timed(lambda: pkg.persistence_landscapes(dgms, lo, hi, G, 1, return_time=True))
        row["landscape_depth1"] = {"device_ms": dev, "wall_ms": wall}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
