"""The numpy restatement of tda_geodesic (include/tda_rips.h): the 64-bit keys and their tie rule, the
union graph, W; then G* by scipy's shortest_path on the float64 copy of W and the component count
by connected_components; the plan (csrc/geo_plan.h) and the header's bound.  Nothing here imports
the package."""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components, shortest_path

import side_plan_ref as spr

LDS_N, TILE, MAX_N, MAX_OUT = 128, 64, 8192, 1 << 28
U = 2.0 ** -24


def ord32(w):
    """sh0_ord: an unsigned integer ordered as the f32 values are, -0.0 as +0.0."""
    u = np.ascontiguousarray(w, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, 0, u)
    return np.where(u >> 31 != 0, u ^ 0xFFFFFFFF, u ^ 0x80000000).astype(np.uint64)


def keys(dm):
    """key[i][j] = ord(dm[i][j]) << 32 | j."""
    n = dm.shape[0]
    return (ord32(dm) << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :]


def row_order(dm, highest_wins=False):
    """Per row, the columns j != i by ascending key (the keys of a row are distinct), then i itself.
    `highest_wins` restates a wrong tie rule (the index reversed in the key), for the mutation records."""
    n = dm.shape[0]
    low = np.arange(n, dtype=np.uint64)
    key = (ord32(dm) << np.uint64(32)) | (low[::-1] if highest_wins else low)[None, :]
    key[np.arange(n), np.arange(n)] = np.uint64(2 ** 64 - 1)  # above every key: ord(NaN) at most 2^32 - 1, an index below 2^32 - 1
    return np.argsort(key, axis=1, kind="stable")


def neighbours(dm, k, highest_wins=False, order=None):
    """(N, N) bool: j is one of row i's min(k, N - 1) columns j != i of smallest key."""
    n = dm.shape[0]
    order = row_order(dm, highest_wins) if order is None else order
    nb = np.zeros((n, n), dtype=bool)
    nb[np.arange(n)[:, None], order[:, :min(k, n - 1)]] = True
    return nb


def graph(dm, n_neighbors=None, radius=None, directed=False, highest_wins=False, order=None):
    """One layer's W (f32: dm on an edge, +inf elsewhere, 0 on the diagonal) and its undirected edge
    count.  `directed` (no union) and `highest_wins` restate two wrong definitions, for the
    mutation records."""
    dm = np.asarray(dm, dtype=np.float32)
    n = dm.shape[0]
    if n_neighbors is not None:
        nb = neighbours(dm, n_neighbors, highest_wins, order)
        edge = nb if directed else nb | nb.T
    else:
        edge = dm.astype(np.float64) <= float(radius)
    edge = edge & ~np.eye(n, dtype=bool)
    W = np.where(edge, dm, np.float32(np.inf)).astype(np.float32)
    W[np.arange(n), np.arange(n)] = 0.0
    return W, int(np.count_nonzero(np.triu(edge | edge.T, 1)))


def closure(W):
    """G* (float64, exact up to scipy's float64 sums) and the number of components."""
    n = W.shape[0]
    finite = np.isfinite(W) & ~np.eye(n, dtype=bool)
    rows, cols = np.nonzero(finite)
    # explicit entries: an edge of weight 0 (duplicated points) is an edge, not a missing one
    g = csr_matrix((W[rows, cols].astype(np.float64), (rows, cols)), shape=(n, n))
    G = shortest_path(g, method="D", directed=False) if n > 1 else np.zeros((1, 1))
    ncomp = connected_components(g, directed=False)[0]
    return G, int(ncomp)


def closure_resident(W):
    """The resident schedule in numpy f32, step for step: the ascending-k loop in place (row k and column
    k are unchanged by step k, so a whole-matrix update is the kernel's).  min is exact and f32 addition
    is the device's, so the result is the kernel's bit for bit."""
    G = np.array(W, dtype=np.float32)
    for k in range(G.shape[0]):
        G = np.minimum(G, G[:, k:k + 1] + G[k:k + 1, :])
    return G


def closure_blocked(W):
    """The blocked schedule in numpy f32, step for step: per round the diagonal tile by the loop, the row
    tiles as min(old, closed (x) old) and their mirrors, then every other tile as min(old, row^T (x) row).
    The matrix is padded to a multiple of 64 with +inf (what the kernels read beyond N)."""
    n = W.shape[0]
    T = (n + TILE - 1) // TILE
    G = np.full((T * TILE, T * TILE), np.inf, dtype=np.float32)
    G[:n, :n] = W

    def product(C, A, B):  # C[r][c] = min(C[r][c], min over k of A[k][r] + B[k][c])
        for k in range(TILE):
            C = np.minimum(C, A[k, :, None] + B[k, None, :])
        return C

    sl = [slice(t * TILE, (t + 1) * TILE) for t in range(T)]
    for t in range(T):
        G[sl[t], sl[t]] = closure_resident(G[sl[t], sl[t]])
        D = G[sl[t], sl[t]].copy()
        for j in range(T):
            if j != t:
                G[sl[t], sl[j]] = product(G[sl[t], sl[j]], D, G[sl[t], sl[j]].copy())
                G[sl[j], sl[t]] = G[sl[t], sl[j]].T
        for i in range(T):
            for j in range(i, T):
                if i != t and j != t:
                    G[sl[i], sl[j]] = product(G[sl[i], sl[j]], G[sl[t], sl[i]], G[sl[t], sl[j]])
                    G[sl[j], sl[i]] = G[sl[i], sl[j]].T
    return G[:n, :n].copy()


def geodesic(dm, n_neighbors=None, radius=None, order=None):
    W, ne = graph(dm, n_neighbors, radius, order=order)
    G, nc = closure(W)
    return W, G, nc, ne


def depth(N, lds_n=LDS_N):
    """c of the header's bound for the schedule that serves N."""
    return max(N - 1, 0) if N <= lds_n else (TILE + 2) * ((N + TILE - 1) // TILE)


def bound(N, lds_n=LDS_N):
    return (1.0 + U) ** depth(N, lds_n) - 1.0


def plan(L, N, D, dtype, is_dist, host_in, n_neighbors, graph_only=0, cap=spr.WS_BYTES, lds_n=None):
    """geo_plan for valid arguments: the refusal by size, or every field."""
    if N > MAX_N:
        return "err", -2, "geodesic distances: N > 8192 is not supported"
    if L * N * N > MAX_OUT:
        return "err", -2, "geodesic distances: more than 2^28 values (L * N * N) in one call is not supported: split L over several calls"
    knn = n_neighbors >= 1
    p, parts = spr.sq_dist(L, N, D, dtype, is_dist, host_in, N * 8 if knn else 0, cap)
    lim = LDS_N if lds_n is None else min(LDS_N, max(1, lds_n))
    resident = N <= lim
    tiles = 0 if resident else (N + TILE - 1) // TILE
    cv = spr.Carve()
    p.update(L=L, N=N, is_dist=int(is_dist), knn=int(knn), graph_only=int(graph_only), resident=int(resident), k=min(n_neighbors, N - 1) if knn else 0,
             lds_n=lim, tiles=tiles, padded=tiles * TILE, lds_select=MAX_N * 4 + 32, lds_resident=LDS_N * LDS_N * 4, lds_diag=TILE * TILE * 4,
             lds_product=2 * TILE * TILE * 4, o_ne=cv.take(L * 8), o_nc=cv.take(L * 4))
    p["o_thr"] = cv.take(p["Lc"] * N * 8 if knn else 0)
    spr.carve_sq(cv, p, parts)
    p["total"] = cv.o
    return "ok", p


def cap_for(Lc, **kw):
    """The smallest cap under which the plan serves Lc layers per chunk."""
    return Lc * plan(**kw)[1]["per_layer"]
