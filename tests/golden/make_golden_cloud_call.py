"""Regenerate tests/golden/cloud_call_args.json: what every entry that takes point clouds or
distance matrices hands to the library, and what it refuses, for the grid of tests/cloud_call.py
(input forms, options, refusals and their order), recorded with that module's stand-in library.

The file was written once, from the code as it stood before the entries got one input path and
one call path, and pins them to it: regenerating it from later code would pin that code to itself.
Needs _hostviews.so (``__graft_entry__.build()``), no device.

Usage: python tests/golden/make_golden_cloud_call.py
"""
from __future__ import annotations

import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cloud_call  # noqa: E402


def main():
    pkg = importlib.import_module("tda-multimodal_amd")
    real = pkg._lib.lib
    try:
        got = cloud_call.record(pkg, setattr)
    finally:
        pkg._lib.lib = real
    n_calls = sum(len(v["calls"]) for v in got.values())
    kinds = sorted({v["outcome"][0] for v in got.values()})
    print(f"{len(got)} cases, {n_calls} recorded calls, outcomes {kinds}")
    with open(os.path.join(HERE, "cloud_call_args.json"), "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
