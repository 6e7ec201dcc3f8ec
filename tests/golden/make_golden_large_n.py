"""Regenerate tests/golden/large_n_h0_*.npz: the CPU oracle's H0 of the two-layer clouds of
tests/large_n.py from N = 4096 up, where it is too slow to run in a GPU test (one core: about 5 s a
layer at N = 4096, 15 to 21 s at 8192; four minutes in all), and of the finite-threshold cases.

One file per case, `large_n_h0_<N>.npz` (`..._t.npz` with the threshold of H0_THRESH_CASES).  The
clouds come from the seeds in tests/large_n.py, in the test as here; `sha` (SHA-256 of the input's
bytes) pins them.  Per layer l: `thresh`, `num_edges`, `n_all_pairs`, `checksum` (the order-free hash
of all pairs, zero persistence included) and every emitted finite pair in emission order as
`l<l>__death` (f32), `l<l>__bidx` (the younger component's vertex, i32) and `l<l>__didx` (the edge,
i32); the essential classes as `l<l>__ess` (vertices, i32).  Births are 0.

The conditions tests/test_large_n.py asserts of these inputs are checked here first.

Usage: python tests/golden/make_golden_large_n.py
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import large_n as ln  # noqa: E402


def h0_arrays(X: np.ndarray, res: list) -> dict:
    out = {"sha": np.array(ln.sha(X)),
           "thresh": np.array([r["thresh"] for r in res], np.float32),
           "num_edges": np.array([r["num_edges"] for r in res], np.int64),
           "n_all_pairs": np.array([r["n_all_pairs"][0] for r in res], np.int64),
           "checksum": np.array([r["checksum"][0] for r in res], np.uint64)}
    for l, r in enumerate(res):
        dg, bi, di = r["dgms"][0], r["birth_idx"][0], r["death_idx"][0]
        fin = np.isfinite(dg[:, 1])
        k = int(fin.sum())
        assert fin[:k].all() and not fin[k:].any() and (dg[:, 0] == 0).all() and (di[k:] == -1).all()
        out[f"l{l}__death"] = dg[:k, 1].astype(np.float32)
        out[f"l{l}__bidx"] = bi[:k].astype(np.int32)
        out[f"l{l}__didx"] = di[:k].astype(np.int32)
        out[f"l{l}__ess"] = bi[k:].astype(np.int32)
        assert (out[f"l{l}__death"].astype(np.float64) == dg[:k, 1]).all()
        assert (out[f"l{l}__bidx"] == bi[:k]).all() and (out[f"l{l}__didx"] == di[:k]).all() and (out[f"l{l}__ess"] == bi[k:]).all()
    return out


def main():
    from oracle import oracle

    cases = [(n, 1.0, np.inf) for n in ln.H0_NS if n >= ln.H0_GOLDEN_MIN_N] + list(ln.H0_THRESH_CASES)
    for n, scale, thresh in cases:
        X = ln.h0_layers(n, scale)
        t0 = time.time()
        res = [oracle.rips(X[l], maxdim=0, thresh=thresh) for l in range(X.shape[0])]
        dt = time.time() - t0
        fin = [int(np.isfinite(r["dgms"][0][:, 1]).sum()) for r in res]
        ess = [len(r["dgms"][0]) - f for r, f in zip(res, fin)]
        groups = [ln.equal_death_groups(r["dgms"][0][:, 1]) for r in res]
        zero = res[1]["n_all_pairs"][0] - fin[1]
        print(f"N = {n} scale {scale} thresh {thresh}: {dt:.1f} s; edges {[r['num_edges'] for r in res]}; forest keys "
              f"{[r['n_all_pairs'][0] for r in res]}; finite pairs {fin}; essential {ess}; groups of equal deaths {groups}; "
              f"zero-length forest edges of the lattice layer {zero}", flush=True)
        assert zero >= 1
        if np.isinf(thresh):
            assert groups[1] >= ln.LATTICE_MIN_GROUPS
        else:
            assert min(ess) > 1 and min(fin) >= ln.H0_THRESH_MIN_FINITE
        name = f"large_n_h0_{n}" + ("" if np.isinf(thresh) else "_t")
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **h0_arrays(X, res))


if __name__ == "__main__":
    main()
