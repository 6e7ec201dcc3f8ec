"""CPU references of the heat (persistence scale-space) kernel (include/tda_dgm.h
tda_heat_kernel) and the accuracy bounds the header derives; test infrastructure only.

    c8      = 1 / (8 sigma),  cn = 1 / (8 pi sigma)        float64, as the library forms them
    t(p,q)  = exp(-c8 r2(p,q)) - exp(-c8 m2(p,q))
    k(F,G)  = cn * sum_p sum_q t(p,q)
    heat    = sqrt(max(0, (k(F,F) + k(G,G)) - 2 k(F,G)))

exact_k is the value of these formulas on the float64 inputs, c8 and cn in mpmath at 40
digits (small diagrams).  ld_k is the same in np.longdouble, in row chunks, for the large
sizes: 64-bit significands, so each term carries some 2^-63 against the (2 E + 8 + D) 2^-53
the bound allows per term; tests/test_heat_cpu.py checks that it stays below 1 / 16 of the
bound."""
import mpmath
import numpy as np

U = 2.0 ** -53
EXP_ULP = 3  # E: the OpenCL conformance bound of double exp (tda_dgm.h says why this one)
ROWS, CHUNK = 64, 256  # the rows and columns of a part (csrc/dgm_plan.h)
EIGHT_PI = 25.132741228718345908
LD = np.longdouble


def constants(sigma: float):
    """(c8, cn) as float64, rounded as the header says."""
    sigma = np.float64(sigma)
    return float(np.float64(1.0) / (np.float64(8.0) * sigma)), float(np.float64(1.0) / (np.float64(EIGHT_PI) * sigma))


def finite_points(D) -> np.ndarray:
    D = np.asarray(D, dtype=np.float64).reshape(-1, 2)
    return D[np.isfinite(D).all(axis=1)]


def depth(n1: int, n2: int) -> int:
    """tda_dgm.h: D(n1, n2), n1 >= n2."""
    parts = -(-n1 // ROWS) * -(-n2 // CHUNK)
    return min(n2, CHUNK) + 12 + -(-parts // 64)


def C(n1: int, n2: int) -> int:
    """tda_dgm.h: C(n1, n2) = n1 n2 (2 E + 8 + D(n1, n2)), the counts in the canonical orientation."""
    n1, n2 = max(n1, n2), min(n1, n2)
    return n1 * n2 * (2 * EXP_ULP + 8 + depth(n1, n2))


def bound_k(n1: int, n2: int, sigma: float) -> float:
    """Bound 3: C(n1, n2) u cn."""
    return C(n1, n2) * U * constants(sigma)[1]


def bound_d2(n1: int, n2: int, sigma: float, self1: float, self2: float, kern: float) -> float:
    """The header's B2, the bound on the squared distance before the clamp."""
    cn = constants(sigma)[1]
    return (C(n1, n1) + C(n2, n2) + 2 * C(n1, n2)) * U * cn + 2 * U * (abs(self1) + abs(self2) + 2 * abs(kern))


def exact_k(F, G, sigma: float):
    """k(F, G) as an mpf at 40 digits."""
    F, G = finite_points(F), finite_points(G)
    c8, cn = constants(sigma)
    with mpmath.workdps(40):
        c8, cn = mpmath.mpf(c8), mpmath.mpf(cn)
        G_ = [(mpmath.mpf(float(b)), mpmath.mpf(float(d))) for b, d in G]
        total = mpmath.mpf(0)
        for b, d in F:
            b, d = mpmath.mpf(float(b)), mpmath.mpf(float(d))
            total += mpmath.fsum(mpmath.exp(-c8 * ((b - x) ** 2 + (d - y) ** 2)) - mpmath.exp(-c8 * ((b - y) ** 2 + (d - x) ** 2)) for x, y in G_)
        return cn * total


def ld_k(F, G, sigma: float, block: int = 1 << 20):
    """k(F, G) in np.longdouble, in chunks of rows of F."""
    F, G = finite_points(F).astype(LD), finite_points(G).astype(LD)
    c8, cn = (LD(c) for c in constants(sigma))
    total = LD(0)
    if len(F) and len(G):
        rows = max(1, block // len(G))
        for i0 in range(0, len(F), rows):
            b, d = F[i0:i0 + rows, 0:1], F[i0:i0 + rows, 1:2]
            r2 = (b - G[None, :, 0]) ** 2 + (d - G[None, :, 1]) ** 2
            m2 = (b - G[None, :, 1]) ** 2 + (d - G[None, :, 0]) ** 2
            total += (np.exp(-c8 * r2) - np.exp(-c8 * m2)).sum(dtype=LD)
    return cn * total


def restatement_k(F, G, sigma: float) -> float:
    """The same in plain numpy float64 (context for the bound, and the profiler's CPU figure)."""
    F, G = finite_points(F), finite_points(G)
    c8, cn = constants(sigma)
    if not (len(F) and len(G)):
        return 0.0
    b, d = F[:, 0:1], F[:, 1:2]
    r2 = (b - G[None, :, 0]) ** 2 + (d - G[None, :, 1]) ** 2
    m2 = (b - G[None, :, 1]) ** 2 + (d - G[None, :, 0]) ** 2
    return float(cn * (np.exp(-c8 * r2) - np.exp(-c8 * m2)).sum())


def to_mpf(x):
    """A longdouble as an mpf, exactly (two float64 pieces)."""
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(LD(x) - LD(hi)))


def d2(self1, self2, kern):
    """(k(F,F) + k(G,G)) - 2 k(F,G) in the arithmetic of its arguments (mpf or longdouble), unclamped."""
    return (self1 + self2) - 2 * kern
