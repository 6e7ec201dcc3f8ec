"""The host arithmetic of the entries beside the persistence pipeline, restated in Python from the
host files as they stood before csrc/side_plan.h (greedy_host.h, resample_host.h, perm_host.h,
ed_host.h, umap_host.h): the per-layer sum and the chunk of layers, every offset and total, the edge
capacities, the LDS sizes, the window split, the group weights and the choice of the resident kernel.
Only successful plans are restated; the refusals are listed case by case in test_side_plan_cpu.py.
The GPU tests take from here the caps that give a wanted chunk of layers."""
F32, F64 = 0, 1
WS_BYTES = 4 << 30       # TDA_GREEDY_WS_BYTES
PERM_CHUNK = 65535 * 8   # rows of the label table per launch
PERM_LDS_S = 128         # the resident kernel's largest S
UMAP_LDS = 150 * 1024


def align(x, a=256):
    return (x + a - 1) // a * a


class Carve:
    """Consecutive 256-byte-aligned offsets."""

    def __init__(self):
        self.o = 0

    def take(self, nbytes):
        r, self.o = self.o, align(self.o + nbytes)
        return r


def dist_select(N, D, dtype, is_dist):
    """rips_plan.h's DistSel without test knobs: (mfma, dsplit, gram_layer)."""
    if is_dist or D < 32:
        return 0, 1, 0
    chunks = (D + 31) // 32
    if dtype == F32 and N <= 144:
        return 1, min(16, max(1, chunks // 8)), 1
    nt = (N + 63) // 64
    tiles = nt * (nt + 1) // 2 * 32
    return 1, min(min(8, max(1, (768 + tiles - 1) // tiles)), max(1, chunks // 4)), 0


def sq_dist(L, N, D, dtype, is_dist, host_in, own, cap):
    """The distance stage of a chunk of layers: what both greedy and resampling computed inline."""
    esz = 8 if dtype == F64 else 4
    x_layer = N * (N if is_dist else D) * esz
    mfma, sp, gl = dist_select(N, D, dtype, is_dist)
    partials = gl or sp > 1
    parts = [x_layer if host_in else 0, N * N * 4, N * 4, sp * N * N * 8 if partials else 0, sp * N * 8 if partials else 0, own]
    per_layer = sum(align(b) for b in parts)
    Lc = min(L, 65535, max(1, cap // per_layer))
    return dict(x_layer=x_layer, per_layer=per_layer, Lc=Lc, mfma=mfma, dsplit=sp, gram_layer=gl), parts


def carve_sq(cv, p, parts):
    for name, b in zip(("o_x", "o_dm", "o_rm", "o_gp", "o_np"), parts):
        p[name] = cv.take(p["Lc"] * b)


def greedy(L, N, D, dtype, is_dist, host_in, k, want_dp, cap=WS_BYTES):
    p, parts = sq_dist(L, N, D, dtype, is_dist, host_in, k * N * 4 if want_dp else 0, cap)
    cv = Carve()
    p.update(L=L, N=N, k=k, is_dist=int(is_dist), want_dp=int(want_dp), o_idx=cv.take(L * k * 8), o_lam=cv.take(L * k * 4))
    carve_sq(cv, p, parts)
    p["o_dp"] = cv.take(p["Lc"] * k * N * 4 if want_dp else 0)
    p.update(total=cv.o, sub_bytes=L * k * k * 4)
    return p


def resample(L, N, D, dtype, is_dist, host_in, B, m, per_layer_idx, cap=WS_BYTES):
    p, parts = sq_dist(L, N, D, dtype, is_dist, host_in, B * m * 4 if per_layer_idx else 0, cap)
    cv = Carve()
    p.update(L=L, N=N, B=B, m=m, is_dist=int(is_dist), per_layer_idx=int(per_layer_idx), Bc=min(B, 65535),
             idx_lstride=B * m if per_layer_idx else 0, o_h=cv.take(L * B * 4), o_idx=cv.take((p["Lc"] if per_layer_idx else 1) * B * m * 4))
    carve_sq(cv, p, parts)
    p["total"] = cv.o
    return p


def cap_for(plan, Lc, **kw):
    """The smallest cap under which `plan` (greedy or resample) serves Lc layers per chunk."""
    return Lc * plan(cap=WS_BYTES, **kw)["per_layer"]


def perm(S, B, obs, G, chunk_env=None, tiled_env=False):
    cv = Carve()
    p = dict(S=S, B=B, rows=B + 1, chunk=PERM_CHUNK if chunk_env is None else min(PERM_CHUNK, max(1, chunk_env)),
             resident=int(S <= PERM_LDS_S and not tiled_env), o_w=cv.take(S * S * 8), o_c=cv.take(64 * 8), o_out=cv.take((B + 1) * 8),
             o_lab=cv.take((B + 1) * S))
    p["total"] = cv.o
    for g in range(G):
        n = sum(1 for c in obs if c == g)
        p[f"cw{g}"] = 1.0 / float(2 * n * (n - 1))
    return p


def ed_job(B, N, D, dtype, on_device, per_item=1, src=(0, 0, 0)):
    esz = 8 if dtype == F64 else 4
    m, stage = min(N, D), src[0] > 0
    cv = Carve()
    p = dict(B=B, N=N, D=D, src_items=src[0], src_rows=src[1], keep_rows=src[2], per_item=per_item, m=m, esz=esz,
             o_x=cv.take(0 if on_device and not stage else B * N * D * esz), o_g=cv.take(B * m * m * 8), stage=int(stage))
    p.update(total=cv.o, n_out=B * per_item, pinned=4 * B * per_item)
    return p


def spectral(B, S, D, dtype, on_device, n_windows, per_item=1):
    """The window split of metrics.py:61-96."""
    W = min(n_windows, S)
    rows = S // W if W else S
    src = (B, S, W * rows) if W and S % W else (0, 0, 0)
    return ed_job(B * max(W, 1), rows, D, dtype, on_device, per_item, src)


def umap(L, N, D, dtype, on_device, k, c, spectral_init=True):
    esz = 8 if dtype == F64 else 4
    ecap = align(2 * N * k, 64)
    cv = Carve()
    p = dict(L=L, N=N, D=D, k=k, c=c, esz=esz, ecap=ecap)
    sizes = [("o_x", 0 if on_device else L * N * D * esz), ("o_dist", L * N * N * 4), ("o_rmax", L * N * 4), ("o_kd", L * N * k * 4),
             ("o_ki", L * N * k * 4), ("o_P", L * N * N * 4), ("o_S", L * N * N * 4), ("o_smax", L * 4), ("o_ne", L * 4), ("o_head", L * ecap * 4),
             ("o_tail", L * ecap * 4), ("o_eps", L * ecap * 8), ("o_nxt", L * ecap * 8), ("o_nxn", L * ecap * 8), ("o_deg", L * N * 4),
             ("o_emb", L * N * c * 4)]
    for name, b in sizes:
        p[name] = cv.take(b)
    spec_lds = (2 * (c + 3) + 1) * N * 4
    p.update(total=cv.o, spec_lds=spec_lds, spectral=int(spectral_init and N <= 2048 and spec_lds <= UMAP_LDS),
             sgd_lds=align(4 * N * c, 16) + 8 * N * c)
    return p


def transform_lds(M, N, c):
    return align(4 * M * c, 16) + 8 * M * c + 4 * N * c


def transform(L, M, N, D, dtype, on_device, k, c):
    esz = 8 if dtype == F64 else 4
    NM, ecap = N + M, M * k
    cv = Carve()
    p = dict(L=L, M=M, N=N, D=D, NM=NM, k=k, c=c, esz=esz, ecap=ecap)
    sizes = [("o_xt", 0 if on_device else N * D * esz), ("o_y", 0 if on_device else L * M * D * esz), ("o_z", L * NM * D * esz),
             ("o_dist", L * NM * NM * 4), ("o_rmax", L * NM * 4), ("o_kd", L * M * k * 4), ("o_ki", L * M * k * 4), ("o_val", L * M * k * 4),
             ("o_eps", L * ecap * 8), ("o_nxt", L * ecap * 8), ("o_nxn", L * ecap * 8), ("o_temb", N * c * 4), ("o_emb", L * M * c * 4)]
    for name, b in sizes:
        p[name] = cv.take(b)
    p.update(total=cv.o, lds=transform_lds(M, N, c), tw=N * D * esz // 4, lw=M * D * esz // 4)
    return p
