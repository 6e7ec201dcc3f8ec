"""numpy restatement of tda_permutation_test (include/tda_rips.h), in the header's exact order of
operations, and a plain float64 form of the same statistic (Robinson and Turner's formula by
boolean masks and math.fsum) to hold it against.

numpy's elementwise float64 `+` and `*` are single correctly rounded operations, never fused, so
the restatement below gives the bits the header defines."""
import math

import numpy as np

U = 2.0 ** -53


def weights(obs, G):
    """c_g = 1 / (2 n_g (n_g - 1)): one rounded division by the exact product."""
    n = np.bincount(np.asarray(obs, dtype=np.int64), minlength=G).astype(np.float64)
    return np.float64(1.0) / (2.0 * n * (n - 1.0))


def statistics(W, lab, c):
    """T of every row of the (B, S) label table: (B,) float64."""
    W = np.asarray(W, dtype=np.float64)
    lab = np.atleast_2d(np.asarray(lab))
    B, S = lab.shape
    col = np.zeros((B, S))
    for i in range(S):  # ascending i, one rounded addition each; an unselected i adds +0.0
        col = col + np.where(lab[:, i, None] == lab, W[i], 0.0)
    t = np.asarray(c, dtype=np.float64)[lab] * col  # one rounded product
    lanes = np.zeros((B, 64))
    for j in range(S):  # lane j % 64 takes j, j + 64, ... in ascending order
        lanes[:, j % 64] = lanes[:, j % 64] + t[:, j]
    for m in (1, 2, 4, 8, 16, 32):  # lane k adds lane k ^ m
        lanes = lanes + lanes[:, np.arange(64) ^ m]
    return lanes[:, 0].copy()


def permutation_test(W, obs, lab, G):
    """(t_obs, null (B,), count, pvalue) as the library returns them."""
    obs = np.asarray(obs)
    c = weights(obs, G)
    t_obs = statistics(W, obs[None], c)[0]
    null = statistics(W, lab, c)
    count = int(np.count_nonzero(null <= t_obs))
    return t_obs, null, count, float(np.float64(1 + count) / np.float64(len(null) + 1))


def plain(W, labels):
    """sigma^2 = sum_g 1 / (2 n_g (n_g - 1)) sum_{i, j in g} W[i, j], every group's sum exact (fsum)."""
    W = np.asarray(W, dtype=np.float64)
    labels = np.asarray(labels)
    total = []
    for g in np.unique(labels):
        m = labels == g
        n = int(m.sum())
        total.append(math.fsum(W[np.ix_(m, m)].ravel()) / (2 * n * (n - 1)))
    return math.fsum(total)


def bound(S, T):
    """The documented accuracy bound S u T + 7 u T (tda_rips.h; for S <= 384)."""
    return (S + 7) * U * T


def same_partition(a, b):
    """True where the labellings a and b (1-d, or rows of 2-d tables) split the diagrams into the same sets."""
    a, b = np.atleast_2d(np.asarray(a)), np.atleast_2d(np.asarray(b))
    return ((a[:, :, None] == a[:, None, :]) == (b[:, :, None] == b[:, None, :])).all(axis=(1, 2))
