"""Golden vectors of the reference's matrix entropy and fixed-window metrics
(run in the build container only): imports /root/reference/metrics.py (torch is
installed here) and evaluates matrix_entropy (metrics.py:344-399) at alpha in
{0.5, 1, 2}, compute_fixed_window_ed (:47-109) and compute_fixed_window_id
(:211-265) on seeded inputs.  The inputs are regenerated in the tests from
`entropy_inputs()` / `window_inputs()` (pinned by a SHA-256); the outputs are
stored in entropy.json, non-finite values as strings.  Nothing of the
reference is copied: only its outputs.

Beside every output the script stores the float64 restatement's value
(tests/spectral_ref.py) and the reference-minus-restatement relative gap
(spectral_ref.rel_gap).  Every strict entropy case -- all of them but N > D at
alpha = 0.5, where the reference's float32 noise eigenvalues go under a square
root -- must be within STRICT_GAP of the restatement, so that the tests' 1e-5
against these goldens is reachable by a correct implementation alone.

Usage: python tests/golden/make_golden_entropy.py
"""
from __future__ import annotations

import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import spectral_ref  # noqa: E402
from make_golden_large import hd_cloud  # noqa: E402

ALPHAS = (0.5, 1.0, 2.0)
STRICT_GAP = 3e-6


def entropy_inputs() -> dict:
    """name -> (..., n, d) float32."""
    rng = np.random.default_rng(11)
    return {
        "act_n36_d4096": np.stack([hd_cloud(36, 4096, 700 + s) for s in range(3)]),  # MFMA Gram, LDS Jacobi
        "gauss_n37_d64": rng.standard_normal((1, 37, 64)).astype(np.float32),  # odd m: the dummy rotation index
        "gauss_n128_d200": rng.standard_normal((1, 128, 200)).astype(np.float32),  # m = kEdLdsMaxM: LDS Jacobi
        "gauss_n129_d200": rng.standard_normal((1, 129, 200)).astype(np.float32),  # m = kEdLdsMaxM + 1: HBM Jacobi
        "gauss_n20_d24": rng.standard_normal((2, 20, 24)).astype(np.float32),  # scalar row Gram
        "gauss_n48_d3": rng.standard_normal((4, 48, 3)).astype(np.float32),  # N > D: column Gram, N - m zero eigenvalues
        "one_row_n1_d5": rng.standard_normal((2, 1, 5)).astype(np.float32),  # m = 1
        "zeros_n10_d10": np.zeros((1, 10, 10), np.float32),  # trace 0
        "lead2x3_n10_d8": rng.standard_normal((2, 3, 10, 8)).astype(np.float32),  # two leading dims
    }


def window_inputs() -> dict:
    """name -> ((batch, seq_len, d) float32, n_windows)."""
    rng = np.random.default_rng(12)
    x50 = rng.standard_normal((3, 50, 16)).astype(np.float32)
    return {
        "s50_d16_w4": (x50, 4),  # remainder 2
        "s48_d64_w4": (rng.standard_normal((2, 48, 64)).astype(np.float32), 4),  # no remainder, MFMA Gram
        "s3_d16_w5": (rng.standard_normal((3, 3, 16)).astype(np.float32), 5),  # the clamp
        "s50_d16_w10": (x50, 10),  # ID all-NaN: windows of 5
        "s64_d8_w2": (rng.standard_normal((2, 64, 8)).astype(np.float32), 2),  # ID defined
    }


def is_strict(X, alpha) -> bool:
    return not (X.shape[-2] > X.shape[-1] and alpha == 0.5)


def sha(X) -> str:
    return hashlib.sha256(np.ascontiguousarray(X).tobytes()).hexdigest()


def enc(v):
    """Floats as they are; non-finite values as strings."""
    v = float(v)
    return v if np.isfinite(v) else str(v)


def dec(v) -> float:
    return float(v)


def _enc_all(a):
    return [enc(v) for v in np.asarray(a, dtype=np.float64).ravel()]


def _gaps(ref, rs):
    return [spectral_ref.rel_gap(a, b, spectral_ref.F32_ULP) for a, b in zip(np.ravel(ref), np.ravel(rs))]


def main():
    import torch

    spec = importlib.util.spec_from_file_location("ref_metrics", "/root/reference/metrics.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    out = {"entropy": {}, "windows": {}}
    for name, X in entropy_inputs().items():
        rec = {"sha": sha(X), "shape": list(X.shape), "alphas": {}}
        for al in ALPHAS:
            ref = m.matrix_entropy(torch.from_numpy(X), al).numpy().astype(np.float64)
            rs = spectral_ref.matrix_entropy(X, al)
            gap = _gaps(ref, rs)
            if is_strict(X, al):
                assert max(gap) <= STRICT_GAP, (name, al, gap)
            rec["alphas"][repr(al)] = {"ref": _enc_all(ref), "restated": _enc_all(rs), "gap": [enc(g) for g in gap],
                                       "strict": is_strict(X, al)}
            print(name, al, _enc_all(ref), "gap", max(gap))
        out["entropy"][name] = rec
    for name, (X, W) in window_inputs().items():
        t = torch.from_numpy(X)
        ed = m.compute_fixed_window_ed(t, W).numpy().astype(np.float64)
        idv = m.compute_fixed_window_id(t, W).numpy().astype(np.float64)
        ed_rs, id_rs = spectral_ref.fixed_window_ed(X, W), spectral_ref.fixed_window_id(X, W)
        assert ed.shape == ed_rs.shape and idv.shape == id_rs.shape, name
        out["windows"][name] = {
            "sha": sha(X), "shape": list(X.shape), "n_windows": W,
            "ed_shape": list(ed.shape), "ed": _enc_all(ed), "ed_restated": _enc_all(ed_rs),
            "ed_gap": [enc(g) for g in _gaps(ed, ed_rs)],
            "id_shape": list(idv.shape), "id": _enc_all(idv), "id_restated": _enc_all(id_rs),
            "id_gap": [enc(g) for g in _gaps(idv, id_rs)],
        }
        print(name, W, "ed gap", max(_gaps(ed, ed_rs)), "id gap", max(_gaps(idv, id_rs)), _enc_all(idv))
    with open(os.path.join(HERE, "entropy.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
