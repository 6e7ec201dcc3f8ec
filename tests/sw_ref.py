"""float64 numpy restatement of the sliced Wasserstein distance between two
persistence diagrams (Carriere, Cuturi, Oudot 2017), the checker of
test_sliced_wasserstein*.py.  Written from the definition:

    drop the points with a non-finite coordinate
    pi(p)   = ((b + d) / 2, (b + d) / 2)
    theta_i = -pi/2 + i * (pi / M),  u_i = (cos theta_i, sin theta_i),  i = 0 .. M-1
    V1_i    = {p . u_i : p in A} u {pi(q) . u_i : q in B}
    V2_i    = {q . u_i : q in B} u {pi(p) . u_i : p in A}
    SW(A,B) = (1/pi) * sum_i (pi/M) * sum_k |sort(V1_i)[k] - sort(V2_i)[k]|

with the directions added in increasing i.  Test infrastructure only."""
import math

import numpy as np


def finite_points(D) -> np.ndarray:
    D = np.asarray(D, dtype=np.float64).reshape(-1, 2)
    return D[np.isfinite(D).all(axis=1)]


def sliced_wasserstein(A, B, M: int = 50) -> float:
    A, B = finite_points(A), finite_points(B)
    mA, mB = (A[:, 0] + A[:, 1]) / 2, (B[:, 0] + B[:, 1]) / 2
    total = 0.0
    for i in range(M):
        th = -math.pi / 2 + i * (math.pi / M)
        c, s = math.cos(th), math.sin(th)
        V1 = np.concatenate([A[:, 0] * c + A[:, 1] * s, mB * c + mB * s])
        V2 = np.concatenate([B[:, 0] * c + B[:, 1] * s, mA * c + mA * s])
        total += (math.pi / M) * float(np.abs(np.sort(V1) - np.sort(V2)).sum())
    return total / math.pi


def matrix(dgms, M: int = 50, other=None) -> np.ndarray:
    other = dgms if other is None else other
    return np.array([[sliced_wasserstein(a, b, M) for b in other] for a in dgms], dtype=np.float64).reshape(len(dgms), len(other))


def bound(A, B) -> float:
    """64 * eps * n * xmax: each projected value is two products and a sum of
    numbers bounded by xmax (a few eps * xmax of error, more where one side
    contracts to fma), each |a - b| term doubles that, n terms are added, and
    the average over directions does not grow it."""
    A, B = finite_points(A), finite_points(B)
    n = len(A) + len(B)
    xmax = max([0.0] + [float(np.abs(X).max()) for X in (A, B) if len(X)])
    return 64 * 2.0 ** -52 * n * xmax
