"""Time tda_matrix_entropy against torch doing the reference's formula on the
same GPU, in one run.

Per shape: 2 warm-up calls, then 7 timed calls of each side, alternating,
timed with HIP events on the caller's stream (the library call orders itself
after that stream and synchronises before it returns, so the interval between
the two events is the whole call); median and spread (min .. max) in ms.  The
input is a device tensor for both sides.  The torch side restates
metrics.py:344-399 (float32 matmul, linalg.eigvalsh, the entropy) once per
order; the library evaluates all orders in one call.

Usage: python tools/spectral_prof.py [--shapes 0,1,2] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((32, 36, 4096), (32, 144, 4096), (8, 1024, 4096))
ALPHAS = (0.5, 1.0, 2.0)
WARMUP, TIMED = 2, 7


def torch_entropy(z, alpha, eps=1e-10):
    import torch

    k = torch.matmul(z, z.transpose(-2, -1))
    lam = torch.clamp(torch.linalg.eigvalsh(k), min=0)
    p = lam / (lam.sum(-1) + eps).unsqueeze(-1)
    if abs(alpha - 1.0) < eps:
        return -torch.sum(torch.xlogy(p, p), dim=-1)
    return torch.log(torch.sum(torch.pow(p, alpha), dim=-1)) / (1.0 - alpha)


def timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="0,1,2", help="indices into SHAPES, e.g. 2 for the HBM Jacobi shape alone")
    args = ap.parse_args()
    shapes = [SHAPES[int(i)] for i in args.shapes.split(",")]
    import torch

    pkg = importlib.import_module("tda-multimodal_amd")
    if not torch.cuda.is_available() or pkg.lib().tda_device_ok(0) != 1:
        raise SystemExit("spectral_prof: no gfx950 device; nothing is measured without one")
    rows = []
    for shape in shapes:
        g = torch.Generator(device="cpu").manual_seed(shape[1])
        z = torch.randn(shape, generator=g, dtype=torch.float32).to("cuda:0")
        ours = lambda: pkg.matrix_entropy_profile(z, ALPHAS)  # noqa: E731
        ref = lambda: torch.stack([torch_entropy(z, a) for a in ALPHAS], -1)  # noqa: E731
        ref1 = lambda: torch_entropy(z, 1.0)  # noqa: E731
        t = {"lib_profile3": [], "torch_profile3": [], "torch_one_order": []}
        for i in range(WARMUP + TIMED):
            for key, fn in (("lib_profile3", ours), ("torch_profile3", ref), ("torch_one_order", ref1)):
                ms, r = timed(fn)
                if i >= WARMUP:
                    t[key].append(ms)
                if key == "lib_profile3":
                    got = r
                elif key == "torch_profile3":
                    want = r
        dev = float(((got - want).abs() / want.abs().clamp(min=1.0)).max())
        row = {"shape": list(shape), "alphas": list(ALPHAS), "max_rel_dev_vs_torch_f32": dev}
        for key, v in t.items():
            row[key + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
