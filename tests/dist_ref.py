"""High-precision truth and a derived error bound for the distance stage, the
checker of test_distance_paths*.py.  Plain numpy, no GPU.  Test infrastructure only.

truth(X) is the difference form t_ij = sqrt(sum_k (x_ik - x_jk)^2) in
np.longdouble: no cancellation, so its own error (a few D * 2^-64 * t) is far
below everything bounded here, and equal rows give exactly 0.

What is bounded.  Every distance kernel (and the oracle) evaluates the Gram form
in float64,

    d2 = (-2 g + n_i) + n_j,   g = sum_k x_ik x_jk,   n_i = sum_k x_ik^2,

clamps it at 0 and takes the root; they differ only in the order of the sums
(sequential k, K slices added by k_distance_combine, 4-wide MFMA blocks, two k
halves per row for the norms).  With u32 = 2^-24, u64 = 2^-53, s = t^2:

 1. The sums.  Products of upcast f32 values are exact in f64; for f64 input
    each product is rounded once (or not at all inside an fma).  A sum of D terms
    in ANY order, one rounding per addition, is within gamma_(D+1) * sum|terms| of
    the exact sum (Higham, Accuracy and Stability, section 4.2), gamma_m =
    m u64 / (1 - m u64).  sum_k |x_ik x_jk| <= (n_i + n_j) / 2, so
        |-2 g^ + 2 g| <= gamma_(D+1) (n_i + n_j),
        |n_i^ - n_i| + |n_j^ - n_j| <= gamma_(D+1) (n_i + n_j).
    The two final additions round numbers no larger than 2 (n_i + n_j) (1 + tiny):
    at most 4 u64 (n_i + n_j) together.  In all
        e := |d2^ - s| <= (2 D + 6) u64 (n_i + n_j) (1 + O(D u64)) <= E / 2,
        E := 4 (D + 4) u64 (n_i + n_j),
    i.e. E carries a factor 2 over the first-order error.  Clamping at 0 moves
    d2^ towards s >= 0, never away.
 2. The root of a = max(d2^, 0).
    a < s, e <= s:  t - sqrt(a) = e / (t + sqrt(a)) <= e / t <= E / (2 t).
    a < s, e >  s:  a may clamp to 0, the error is at most t, and 2 t^2 <= E,
                    so t <= E / (2 t) as well.
    a > s:          sqrt(a) - t = e / (sqrt(a) + t) <= e / (2 t) = E / (4 t).
    Always          |sqrt(a) - t| <= sqrt(e) <= sqrt(E / 2): this branch is the
                    smaller one for pairs at or near distance 0 (duplicate rows:
                    t = 0, the kernels return sqrt of the summation noise).
    So |sqrt(a) - t| <= min(E / (2 t), sqrt(E)), with a factor of at least
    sqrt(2) to spare wherever sqrt(a) > t.
 3. The roundings after the sums.  f32 path: d2^ is rounded to f32 (relative
    u32 on the square, u32 / 2 on the root) and the f32 root is correctly rounded
    (u32): 1.5 u32 sqrt(a).  f64 path: the f64 root (u64) is rounded to f32 once
    (u32).  Where sqrt(a) <= t this is below 2 u32 t; where sqrt(a) > t the
    excess 1.5 u32 (sqrt(a) - t) disappears in the spare factor of step 2.

    bound   = 2 u32 t + min(E / (2 t), sqrt(E))        the f32 matrix
    bound64 = 2 u64 t + min(E / (2 t), sqrt(E))        dist64 (one f64 rounding of the root)

Overflow and subnormals are not modelled: the tests' values are O(1) to O(1e3).
"""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
LD = np.longdouble


def truth(X, block_bytes: int = 64 << 20) -> np.ndarray:
    """(N, N) np.longdouble distances of the (N, D) rows of X, difference form,
    in row blocks (an (N, N, D) longdouble array does not fit at N = 200, D = 1050)."""
    X = np.asarray(X)
    n, d = X.shape
    Xl = X.astype(LD)
    out = np.zeros((n, n), dtype=LD)
    rows = max(1, int(block_bytes // (max(1, n * d) * Xl.itemsize)))
    for i0 in range(0, n, rows):
        diff = Xl[i0:i0 + rows, None, :] - Xl[None, :, :]
        out[i0:i0 + rows] = np.sqrt((diff * diff).sum(axis=-1))
    return out


def _spread(X, t) -> np.ndarray:
    """min(E / (2 t), sqrt(E)) per pair, E = 4 (D + 4) u64 (n_i + n_j)."""
    Xl = np.asarray(X).astype(LD)
    d = Xl.shape[1]
    nrm = (Xl * Xl).sum(axis=1)
    E = 4 * (d + 4) * LD(U64) * (nrm[:, None] + nrm[None, :])
    rootE = np.sqrt(E)
    with np.errstate(divide="ignore", invalid="ignore"):
        lin = np.where(t > 0, E / (2 * np.where(t > 0, t, 1)), np.inf)
    return np.minimum(lin, rootE)


def bound(X, t) -> np.ndarray:
    """Per-pair bound on |dist - truth| for the f32 matrix (module docstring)."""
    return 2 * LD(U32) * t + _spread(X, t)


def bound64(X, t) -> np.ndarray:
    """Per-pair bound on |dist64 - truth| for the f64 matrix of f64 points."""
    return 2 * LD(U64) * t + _spread(X, t)


def ratio(got, t, b) -> float:
    """Largest |got - truth| / bound over all pairs (off the diagonal, where the
    bound is positive; the diagonal is asserted to be exactly 0 separately)."""
    n = t.shape[0]
    off = ~np.eye(n, dtype=bool)
    err = np.abs(np.asarray(got).astype(LD) - t)
    assert np.all(b[off] > 0)
    return float((err[off] / b[off]).max())


# ---- the cases of test_distance_paths*.py: (N, D, dtype, environment) -> (mfma, dsplit, gram_layer)
# as tda_debug_dist_plan reports them
F32, F64 = np.float32, np.float64
SCALAR = (0, 1, 0)
CASES = [
    # automatic selection
    (17, 31, F32, {}, SCALAR),                 # below kDistMfmaMinD
    (17, 32, F32, {}, (1, 1, 1)),              # k_gram_layer, one chunk
    (144, 96, F32, {}, (1, 1, 1)),             # k_gram_layer at its largest N, 3 chunks
    (145, 96, F32, {}, (1, 1, 0)),             # f32 tiles unsplit, 3 chunks, 3 x 3 tiles with a 17-row edge
    (145, 257, F32, {}, (1, 2, 0)),            # f32 tiles, 4 + 5 chunks, K tail of 1
    (40, 1050, F32, {}, (1, 4, 1)),            # k_gram_layer, 8 + 8 + 8 + 9 chunks, K tail of 26
    (200, 1050, F32, {}, (1, 3, 0)),           # f32 tiles, 3 slices
    (65, 260, F64, {}, (1, 2, 0)),             # f64 tiles split, one off-diagonal tile
    (129, 160, F64, {}, (1, 1, 0)),            # f64 tiles unsplit, 5 chunks
    # forced
    (63, 100, F32, {"TDA_DIST": "tiles"}, (1, 1, 0)),                         # tile kernel below 144
    (130, 224, F32, {"TDA_DIST": "tiles", "TDA_DIST_SPLIT": "3"}, (1, 3, 0)),  # 2 + 2 + 3 chunks
    (40, 1050, F32, {"TDA_DIST_SPLIT": "5"}, (1, 5, 1)),
    (65, 260, F64, {"TDA_DIST_SPLIT": "7"}, (1, 7, 0)),                       # 9 chunks in 7 slices
    (145, 257, F32, {"TDA_DIST": "scalar"}, SCALAR),                          # scalar kernel, large D, K tail
    (145, 257, F64, {"TDA_DIST": "scalar"}, SCALAR),
]


def plan(pkg, n, d, dtype):
    """(mfma, dsplit, gram_layer) of (n, d) points under the current environment (host only)."""
    import ctypes

    m, s, g = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = pkg.lib().tda_debug_dist_plan(n, d, 1 if np.dtype(dtype) == np.float64 else 0, ctypes.byref(m), ctypes.byref(s), ctypes.byref(g))
    assert rc == 0
    return m.value, s.value, g.value


def case_id(case) -> str:
    n, d, dt, env, _ = case
    return f"n{n}_d{d}_{np.dtype(dt).name}" + "".join(f"_{k[4:].lower()}={v}" for k, v in sorted(env.items()))


GRID_MAX = 8  # layer 2: integer coordinates in [-GRID_MAX, GRID_MAX]


def layers(n: int, d: int, dtype) -> np.ndarray:
    """The (3, n, d) input of a case.  Layer 0: hd_cloud (offset, heavy-tailed
    features: real cancellation in the Gram form).  Layer 1: hd_cloud of another
    seed with row 5 = row 4 (exact duplicate), row 7 = row 4 + 1e-3 (near
    duplicate), row 9 = 0.  Layer 2: integers in [-8, 8]: every product and sum is
    exact in any order."""
    from golden.make_golden_large import hd_cloud

    seed = 1000 + 7 * n + d
    X = np.empty((3, n, d), dtype=dtype)
    X[0] = hd_cloud(n, d, seed)
    X[1] = hd_cloud(n, d, seed + 1)
    X[1, 5] = X[1, 4]
    X[1, 7] = X[1, 4] + dtype(1e-3)
    X[1, 9] = 0
    X[2] = np.random.default_rng(seed + 2).integers(-GRID_MAX, GRID_MAX + 1, (n, d))
    return X


def grid_expected(G) -> np.ndarray:
    """Correctly rounded f32 sqrt of the exact integer squared distances of a grid layer.
    d2 <= D * (2 * GRID_MAX)^2 < 2^24 for the D used here, so np.float32(d2) is exact;
    on the f64 path sqrt in f64 followed by one rounding to f32 gives the same value
    (double rounding is innocuous for sqrt when 53 >= 2 * 24 + 2)."""
    Gi = np.asarray(G).astype(np.int64)
    assert np.array_equal(Gi, G) and Gi.shape[1] * (2 * GRID_MAX) ** 2 < 2 ** 24
    sq = (Gi * Gi).sum(axis=1)
    d2 = sq[:, None] + sq[None, :] - 2 * (Gi @ Gi.T)
    return np.sqrt(d2.astype(np.float32))
