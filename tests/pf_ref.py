"""CPU references of the persistence Fisher distance (include/tda_dgm.h tda_persistence_fisher)
and the accuracy bounds the header derives; test infrastructure only.

    c2       = 1 / (2 sigma sigma)                       float64, as the library forms it
    U        = F, pi(G);  V = G, pi(F);  Z = U then V    pi(b, d) = (m, m), m = (b + d) * 0.5
    e(z, w)  = +0.0 if -c2 r2 < -708 else exp(-c2 r2)
    rhoU(z)  = sum_{w in U} e(z, w);  rhoV(z) likewise
    a, b, h  = sum_z rhoU, sum_z rhoV, sum_z sqrt(rhoU rhoV)
    fisher   = arccos(min(1, h / sqrt(a b)))

restatement is the same in numpy float64 in the header's order of operations and of sums: a
Python loop over the sources, vectorised over z only, then the two butterflies.  It differs
from the device by the exponential alone (numpy's against the device's), so it sits well
inside the bound.  exact is the value of the formulas, cut included, on the float64 inputs and
c2 in mpmath at 50 digits (small diagrams)."""
import mpmath
import numpy as np

U_ = 2.0 ** -53
EXP_ULP = 3  # E: the OpenCL conformance bound of double exp (tda_dgm.h says why this one)
CUT = 708
LANES, CHUNK = 64, 128  # TDA_PF_LANES (enters the order of the sums), TDA_PF_CHUNK (does not)
MAX_POINTS = 1024
T = 6 * CUT + 2 * EXP_ULP + 2


def c2_of(sigma: float) -> float:
    """c2 as float64, rounded as the header says."""
    sigma = np.float64(sigma)
    return float(np.float64(1.0) / (np.float64(2.0) * (sigma * sigma)))


def finite_points(D) -> np.ndarray:
    D = np.asarray(D, dtype=np.float64).reshape(-1, 2)
    return D[np.isfinite(D).all(axis=1)]


def R(n1: int, n2: int) -> int:
    """tda_dgm.h: R(n1, n2) = T + (n1 + n2)."""
    return T + n1 + n2


def bound(n1: int, n2: int) -> float:
    """tda_dgm.h: B(n1, n2) = (2 R + 30) u + 3 (n1 + n2) 2^-510, on the affinity."""
    return (2 * R(n1, n2) + 30) * U_ + 3 * (n1 + n2) * 2.0 ** -510


def bound_dist(affinity: float, B: float) -> float:
    """The header's bound on the distance, from the computed affinity and B."""
    return float(np.arccos(max(-1.0, affinity - B)) - np.arccos(min(1.0, affinity + B)) + 4 * U_)


def orient(F, G):
    """The canonical orientation of dgm_orient: the longer diagram first and, at equal counts, the
    one whose finite points come first lexicographically.  Returns (F, G, swapped)."""
    F, G = finite_points(F), finite_points(G)
    swap = len(G) > len(F)
    if len(F) == len(G):
        a, b = F.ravel(), G.ravel()
        d = np.flatnonzero((a != b) | (np.signbit(a) != np.signbit(b)))
        if len(d):
            k = d[0]
            swap = bool(b[k] < a[k] or (b[k] == a[k] and np.signbit(b[k]) and not np.signbit(a[k])))
    return (G, F, True) if swap else (F, G, False)


def proj(P):
    m = (P[:, 0] + P[:, 1]) * 0.5
    return np.stack([m, m], 1)


def supports(F, G):
    """(U, V) of two arrays of finite points, in the header's order."""
    return np.concatenate([F, proj(G)]), np.concatenate([G, proj(F)])


def butterfly(v):
    """(parts, 64) -> (parts,): lanes l and l ^ 1, then l ^ 2, ... l ^ 32, every lane ending with the same bits."""
    lane = np.arange(LANES)
    for m in (1, 2, 4, 8, 16, 32):
        v = v + v[:, lane ^ m]
    assert (v == v[:, :1]).all()
    return v[:, 0]


def sums(F, G, sigma: float):
    """(a, b, h) of the pair as named, in the header's order (the pair is oriented first and a, b
    are exchanged back)."""
    F, G, swapped = orient(F, G)
    M = len(F) + len(G)
    if M == 0:
        return 0.0, 0.0, 0.0
    nc2 = -c2_of(sigma)
    Us, Vs = supports(F, G)
    Z = np.concatenate([Us, Vs])
    zb, zd = Z[:, 0], Z[:, 1]
    rho = []
    with np.errstate(over="ignore", under="ignore"):
        for S_ in (Us, Vs):
            acc = np.zeros(2 * M)
            for wb, wd in S_:
                db, dd = zb - wb, zd - wd
                t = nc2 * (db * db + dd * dd)
                keep = ~(t < -float(CUT))
                e = np.zeros(2 * M)
                e[keep] = np.exp(t[keep])
                acc = acc + e
            rho.append(acc)
    parts = -(-2 * M // LANES)
    out = []
    for v in (rho[0], rho[1], np.sqrt(rho[0] * rho[1])):
        lanes = np.zeros(parts * LANES)
        lanes[:2 * M] = v
        per_part = np.zeros(LANES)
        per_part[:parts] = butterfly(lanes.reshape(parts, LANES))
        out.append(float(butterfly(per_part[None])[0]))
    a, b, h = out
    return (b, a, h) if swapped else (a, b, h)


def affinity_of(a: float, b: float, h: float) -> float:
    """min(1, h / sqrt(a b)) in the host's order; 1 for two empty diagrams."""
    if not a > 0.0:
        return 1.0
    q = np.float64(h) / np.sqrt(np.float64(a) * np.float64(b))
    return float(q if q < 1.0 else 1.0)


def restatement(F, G, sigma: float) -> float:
    """fisher in the header's order; +0.0 for two empty diagrams."""
    a, b, h = sums(F, G, sigma)
    return float(np.arccos(affinity_of(a, b, h))) if a > 0.0 else 0.0


def exact(F, G, sigma: float):
    """(affinity, fisher) as mpf at 50 digits: the formulas, the cut included, on the float64 inputs and c2
    (the projections pi rounded as the header rounds them: they are inputs of the sums).  Must be
    called, and its result used, inside mpmath.workdps(50)."""
    F, G = finite_points(F), finite_points(G)
    if len(F) + len(G) == 0:
        return mpmath.mpf(1), mpmath.mpf(0)
    c2 = mpmath.mpf(c2_of(sigma))
    Us, Vs = ([(mpmath.mpf(float(x)), mpmath.mpf(float(y))) for x, y in S_] for S_ in supports(F, G))

    def rho(z, S_):
        tot = mpmath.mpf(0)
        for w in S_:
            t = -c2 * ((z[0] - w[0]) ** 2 + (z[1] - w[1]) ** 2)
            if not t < -CUT:
                tot += mpmath.exp(t)
        return tot

    a = b = h = mpmath.mpf(0)
    for z in Us + Vs:
        ru, rv = rho(z, Us), rho(z, Vs)
        a, b, h = a + ru, b + rv, h + mpmath.sqrt(ru * rv)
    aff = min(mpmath.mpf(1), h / mpmath.sqrt(a * b))
    return aff, mpmath.acos(aff)
