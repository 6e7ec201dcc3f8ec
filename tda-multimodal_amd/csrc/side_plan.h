// side_plan.h -- the host plans of the entries that take clouds or tables beside the persistence pipeline:
// greedy_plan (tda_greedy_perm), resample_plan (tda_resample), perm_plan (tda_permutation_test), ed_plan /
// spectral_plan / entropy_plan (the three spectral metrics) and umap_plan / umap_transform_plan.  A plan is
// the entry's argument checks, in the order the entry has always made them, then every size the call needs:
// the chunk of layers, the byte offset of every array in the entry's workspace (aux_ws.h), the total, the
// dynamic-LDS sizes.  Plain C++, no HIP: a plan returns an error code and leaves its message in `msg`
// (tests/side_plan_main.cpp runs them with a host compiler alone, tests/test_side_plan_cpu.py pins them).
// The kernels' limits are restated here as kSide*; the host file of each entry asserts that they are the
// kernels' own.
#pragma once
#include <cmath>
#include <string>

#include "../../include/tda_umap.h"
#include "rips_plan.h"

namespace tda {

constexpr int64_t kSideMaxN = 8192;          // greedy (kGpMaxQ * kGpT), resampling (N and m)
constexpr int kSidePermLdsS = 128;           // kPermLdsS: the resident kernel's largest S
constexpr int kSidePermR = 8;                // kPermR: labellings served by a tiled workgroup
constexpr size_t kPermChunkRows = (size_t)65535 * kSidePermR;  // rows of the table per launch (TDA_PERM_CHUNK overrides it in tests)
constexpr int kSideEdMaxM = 1024;            // kEdMaxM
constexpr int kSideEdMaxAlpha = 16;          // kEdMaxAlpha
constexpr int kSideUmapMaxK = 64;            // kUmapMaxK
constexpr int kSideUmapMaxC = 8;             // kUmapMaxC
constexpr int64_t kSideUmapSpecMaxN = 2048;  // kUmapSpecMaxN
constexpr size_t kSideUmapLds = 150 * 1024;  // dynamic LDS a UMAP layout kernel may be launched with

// The cap of a chunk of layers' device bytes: TDA_GREEDY_WS_BYTES, or TDA_SIDE_WS_BYTES (tests: bytes, at least 1)
inline size_t side_ws_cap() {
    if (const char* e = test_env("TDA_SIDE_WS_BYTES")) return std::max<size_t>(1, strtoull(e, nullptr, 10));
    return (size_t)TDA_GREEDY_WS_BYTES;
}

// ---------------------------------------------------------------- the shared head
inline int side_bad(std::string& msg, int code, const std::string& m) { return msg = m, code; }

template <typename Args>
inline int side_check_x(const Args* a, std::string& msg) {
    if (!a) return side_bad(msg, TDA_E_INVALID, "args is NULL");
    if (!a->x) return side_bad(msg, TDA_E_INVALID, "x is NULL");
    return 0;
}
inline int side_check_dtype(int dtype, std::string& msg) {
    return dtype != TDA_F32 && dtype != TDA_F64 ? side_bad(msg, TDA_E_INVALID, "dtype must be TDA_F32 or TDA_F64") : 0;
}
// (L, N, D) points or (L, N, N) distances of greedy and resampling
template <typename Args>
inline int side_check_cloud(const Args* a, std::string& msg) {
    if (a->L < 1) return side_bad(msg, TDA_E_INVALID, "L must be >= 1");
    if (a->N < 1) return side_bad(msg, TDA_E_INVALID, "N must be >= 1");
    if (!a->is_dist && a->D < 1) return side_bad(msg, TDA_E_INVALID, "D must be >= 1");
    return side_check_dtype(a->dtype, msg);
}
// sklearn's row-wise and full-matrix float64 distances disagree: no exact contract (`what` of the entry)
template <typename Args>
inline int side_check_f64_points(const Args* a, const char* what, std::string& msg) {
    if (!a->is_dist && a->dtype == TDA_F64)
        return side_bad(msg, TDA_E_UNSUPPORTED, std::string(what) + " of float64 point clouds is not supported (pass float32 points or a distance matrix)");
    return 0;
}

// ---------------------------------------------------------------- the distance stage of a chunk of layers
// The (Lc, N, N) f32 matrices of Lc layers at a time with what their kernels need: the staged input, the
// row maxima and the K slices' partial Grams and norms.  Lc is the largest count whose bytes (with `own`,
// the entry's own bytes per layer) stay within cap, one layer at least, 65535 (a grid dimension) at most.
struct SqDistPlan {
    size_t N = 0, x_layer = 0, per_layer = 0, Lc = 0;
    bool host_in = false;
    DistSel sel;
    size_t o_x = 0, o_dm = 0, o_rm = 0, o_gp = 0, o_np = 0;
    size_t gp_layer() const { return sel.partials() ? (size_t)sel.dsplit * N * N * 8 : 0; }
    size_t np_layer() const { return sel.partials() ? (size_t)sel.dsplit * N * 8 : 0; }
    // the five arrays, after whatever the entry has carved
    void carve(Carve& cv) {
        o_x = cv.take(host_in ? Lc * x_layer : 0), o_dm = cv.take(Lc * N * N * 4), o_rm = cv.take(Lc * N * 4);
        o_gp = cv.take(Lc * gp_layer()), o_np = cv.take(Lc * np_layer());
    }
};
inline SqDistPlan sq_dist_plan(size_t L, size_t N, int64_t D, int dtype, bool is_dist, bool host_in, size_t own, size_t cap) {
    SqDistPlan p;
    p.N = N, p.host_in = host_in;
    p.x_layer = N * (is_dist ? N : (size_t)D) * (dtype == TDA_F64 ? 8 : 4);
    p.sel = dist_select(N, D, dtype, is_dist);
    for (size_t bytes : {host_in ? p.x_layer : 0, N * N * 4, N * 4, p.gp_layer(), p.np_layer(), own}) p.per_layer += align_up(bytes, 256);
    p.Lc = std::min<size_t>(std::min<size_t>(L, 65535), std::max<size_t>(1, cap / p.per_layer));
    return p;
}

// ---------------------------------------------------------------- tda_greedy_perm
struct GreedyPlan {
    size_t L = 0, N = 0, k = 0;
    bool is_dist = false, want_dp = false;
    SqDistPlan sq;
    size_t o_idx = 0, o_lam = 0, o_dp = 0, total = 0;
    size_t sub_bytes = 0;  // the result's own device buffer: the (L, k, k) landmark matrices
};
inline int greedy_plan(const tda_greedy_args* a, size_t cap, GreedyPlan& p, std::string& msg) {
    if (int rc = side_check_x(a, msg)) return rc;
    if (int rc = side_check_cloud(a, msg)) return rc;
    if (a->n_perm < 1 || (int64_t)a->n_perm > a->N) return side_bad(msg, TDA_E_INVALID, "n_perm must be in [1, N]");
    if (a->N > kSideMaxN) return side_bad(msg, TDA_E_UNSUPPORTED, "greedy subsampling: N > 8192 is not supported");
    if (int rc = side_check_f64_points(a, "greedy subsampling", msg)) return rc;
    p.L = (size_t)a->L, p.N = (size_t)a->N, p.k = (size_t)a->n_perm;
    p.is_dist = a->is_dist != 0, p.want_dp = a->want_dperm2all != 0;
    p.sq = sq_dist_plan(p.L, p.N, a->D, a->dtype, p.is_dist, !a->x_on_device, p.want_dp ? p.k * p.N * 4 : 0, cap);
    Carve cv;
    p.o_idx = cv.take(p.L * p.k * 8), p.o_lam = cv.take(p.L * p.k * 4);
    p.sq.carve(cv);
    p.o_dp = cv.take(p.want_dp ? p.sq.Lc * p.k * p.N * 4 : 0);
    p.total = cv.o;
    p.sub_bytes = p.L * p.k * p.k * 4;
    return 0;
}

// ---------------------------------------------------------------- tda_resample
struct ResamplePlan {
    size_t L = 0, N = 0, B = 0, m = 0;
    bool is_dist = false, per_layer_idx = false;
    size_t Bc = 0;           // resamples per launch: grid dimensions stay <= 65535
    size_t idx_lstride = 0;  // the table's entries per layer (0: one table for every layer)
    SqDistPlan sq;
    size_t o_h = 0, o_idx = 0, total = 0;
};
inline int resample_plan(const tda_resample_args* a, size_t cap, ResamplePlan& p, std::string& msg) {
    if (int rc = side_check_x(a, msg)) return rc;
    if (!a->idx) return side_bad(msg, TDA_E_INVALID, "idx is NULL");
    if (int rc = side_check_cloud(a, msg)) return rc;
    if (a->B < 1) return side_bad(msg, TDA_E_INVALID, "B must be >= 1");
    if (a->m < 1) return side_bad(msg, TDA_E_INVALID, "m must be >= 1");
    if (a->N > kSideMaxN) return side_bad(msg, TDA_E_UNSUPPORTED, "resampling: N > 8192 is not supported");
    if (a->m > kSideMaxN) return side_bad(msg, TDA_E_UNSUPPORTED, "resampling: m > 8192 is not supported");
    if (int rc = side_check_f64_points(a, "resampling", msg)) return rc;
    if ((unsigned __int128)a->L * (uint64_t)a->B > (uint64_t)TDA_RESAMPLE_MAX_OUT)
        return side_bad(msg, TDA_E_UNSUPPORTED, "resampling: more than 2^27 resamples (L * B) in one call is not supported: split B over several calls");
    p.L = (size_t)a->L, p.N = (size_t)a->N, p.B = (size_t)a->B, p.m = (size_t)a->m;
    p.is_dist = a->is_dist != 0, p.per_layer_idx = a->idx_per_layer != 0;
    const size_t n_idx = (p.per_layer_idx ? p.L : 1) * p.B * p.m;
    for (size_t e = 0; e < n_idx; ++e)
        if (a->idx[e] < 0 || a->idx[e] >= a->N)
            return side_bad(msg, TDA_E_INVALID,
                            "idx[" + std::to_string(e) + "] = " + std::to_string(a->idx[e]) + " is outside [0, N = " + std::to_string(a->N) + ")");
    p.sq = sq_dist_plan(p.L, p.N, a->D, a->dtype, p.is_dist, !a->x_on_device, p.per_layer_idx ? p.B * p.m * 4 : 0, cap);
    p.Bc = std::min<size_t>(p.B, 65535);
    p.idx_lstride = p.per_layer_idx ? p.B * p.m : 0;
    Carve cv;
    p.o_h = cv.take(p.L * p.B * 4), p.o_idx = cv.take((p.per_layer_idx ? p.sq.Lc : 1) * p.B * p.m * 4);
    p.sq.carve(cv);
    p.total = cv.o;
    return 0;
}

// ---------------------------------------------------------------- tda_permutation_test
struct PermPlan {
    size_t S = 0, B = 0, rows = 0;         // rows: the B relabellings, then the observed one
    double cw[TDA_PERM_MAX_GROUPS] = {};   // cw[g] = 1 / (2 n_g (n_g - 1))
    size_t chunk = 0;                      // rows of the table per launch
    bool resident = false;                 // k_perm_resident (w in LDS) instead of k_perm_tiled
    size_t o_w = 0, o_c = 0, o_out = 0, o_lab = 0, total = 0;
};
inline int perm_plan(const tda_perm_args* a, PermPlan& p, std::string& msg) {
    if (!a) return side_bad(msg, TDA_E_INVALID, "args is NULL");
    if (!a->w) return side_bad(msg, TDA_E_INVALID, "w is NULL");
    if (!a->obs) return side_bad(msg, TDA_E_INVALID, "obs is NULL");
    if (!a->lab) return side_bad(msg, TDA_E_INVALID, "lab is NULL");
    if (a->S < 2) return side_bad(msg, TDA_E_INVALID, "S must be >= 2");
    if (a->B < 1) return side_bad(msg, TDA_E_INVALID, "B must be >= 1");
    if (a->G < 2) return side_bad(msg, TDA_E_INVALID, "G must be >= 2");
    if (a->reserved != 0) return side_bad(msg, TDA_E_INVALID, "reserved must be 0");
    if (a->S > TDA_PERM_MAX_S) return side_bad(msg, TDA_E_UNSUPPORTED, "permutation test: S > 2048 is not supported");
    if (a->G > TDA_PERM_MAX_GROUPS) return side_bad(msg, TDA_E_UNSUPPORTED, "permutation test: G > 64 is not supported");
    if ((unsigned __int128)a->B * (uint64_t)a->S > (uint64_t)TDA_PERM_MAX_TABLE)
        return side_bad(msg, TDA_E_UNSUPPORTED, "permutation test: a label table of more than 2^27 entries (B * S) is not supported: split B over several calls");
    const size_t S = (size_t)a->S, B = (size_t)a->B, G = (size_t)a->G;
    auto at = [&](size_t i, size_t j) { return "w[" + std::to_string(i) + "][" + std::to_string(j) + "]"; };
    for (size_t i = 0; i < S; ++i)
        for (size_t j = 0; j < S; ++j) {
            const double v = a->w[i * S + j];
            uint64_t bits, tb;
            memcpy(&bits, &v, 8);
            if (!std::isfinite(v) || v < 0.0) return side_bad(msg, TDA_E_INVALID, at(i, j) + " = " + std::to_string(v) + " is not finite and >= 0");
            if (i == j && bits != 0) return side_bad(msg, TDA_E_INVALID, at(i, j) + " = " + std::to_string(v) + ": the diagonal must be +0.0");
            memcpy(&tb, &a->w[j * S + i], 8);
            if (bits != tb) return side_bad(msg, TDA_E_INVALID, at(i, j) + " and " + at(j, i) + " differ: w must be symmetric bit for bit");
        }
    size_t hist[256] = {};
    for (size_t i = 0; i < S; ++i) {
        if (a->obs[i] >= G)
            return side_bad(msg, TDA_E_INVALID, "obs[" + std::to_string(i) + "] = " + std::to_string((int)a->obs[i]) + " is outside [0, G = " + std::to_string(G) + ")");
        ++hist[a->obs[i]];
    }
    for (size_t g = 0; g < G; ++g)
        if (hist[g] < 2)
            return side_bad(msg, TDA_E_INVALID, "group " + std::to_string(g) + " has " + std::to_string(hist[g]) + " members: every group needs at least 2");
    for (size_t b = 0; b < B; ++b) {
        size_t h[256] = {};
        const uint8_t* row = a->lab + b * S;
        for (size_t i = 0; i < S; ++i) ++h[row[i]];
        if (memcmp(h, hist, sizeof h))
            return side_bad(msg, TDA_E_INVALID, "lab[" + std::to_string(b) + "] is not a permutation of obs (its label histogram differs)");
    }
    for (size_t g = 0; g < G; ++g) p.cw[g] = 1.0 / (double)(2 * hist[g] * (hist[g] - 1));  // the product is exact: one rounding
    p.S = S, p.B = B, p.rows = B + 1;
    p.chunk = kPermChunkRows;
    if (const char* e = test_env("TDA_PERM_CHUNK")) p.chunk = std::min<size_t>(kPermChunkRows, std::max<size_t>(1, strtoull(e, nullptr, 10)));
    p.resident = S <= (size_t)kSidePermLdsS && !test_env_is("TDA_PERM_TILED", "1");
    Carve cv;
    p.o_w = cv.take(S * S * 8), p.o_c = cv.take(sizeof p.cw), p.o_out = cv.take(p.rows * 8), p.o_lab = cv.take(p.rows * S);
    p.total = cv.o;
    return 0;
}

// ---------------------------------------------------------------- the spectral metrics
// One call's work, validated: B matrices of N x D.  src_items > 0: the B matrices are the windows of
// src_items items of src_rows rows each, of which only the first keep_rows are used (a remainder is
// dropped), so the kept rows are staged with one 2-D copy; otherwise x already is (B, N, D).
struct EdJob {
    const void* x;
    int32_t dtype, x_on_device;
    int64_t B, N, D;
    int64_t src_items, src_rows, keep_rows;
    int32_t device;
    void* stream;
    // the workspace: the staged input (0 bytes when it is read in place), the f64 Gram matrices; the pinned result
    int64_t per_item = 1, m = 0;  // floats per matrix; min(N, D), the side of a Gram matrix
    size_t esz = 0, o_x = 0, o_g = 0, total = 0, n_out = 0, pinned = 0;
    bool stage() const { return src_items > 0; }
};
inline void ed_layout(EdJob& j, int64_t per_item) {
    j.per_item = per_item, j.m = std::min(j.N, j.D), j.esz = j.dtype == TDA_F64 ? 8 : 4;
    Carve cv;
    j.o_x = cv.take(j.x_on_device && !j.stage() ? 0 : (size_t)j.B * j.N * j.D * j.esz), j.o_g = cv.take((size_t)j.B * j.m * j.m * 8);
    j.total = cv.o;
    j.n_out = (size_t)(j.B * per_item);
    j.pinned = sizeof(float) * j.n_out;
}
// the shape limits of the Gram and Jacobi kernels, shared by the three entries
inline int ed_check_shape(const char* what, int64_t N, int64_t D, std::string& msg) {
    if (std::min(N, D) > kSideEdMaxM) return side_bad(msg, TDA_E_UNSUPPORTED, std::string(what) + ": min(N, D) <= 1024 is supported");
    if (N > 8192 && N <= D) return side_bad(msg, TDA_E_UNSUPPORTED, std::string(what) + ": N <= 8192");
    return 0;
}
// the head of the three entries: `rows` is the entry's row count (N or S), `sizes` its own wording of the size check
template <typename Args>
inline int ed_check_head(const Args* a, const float* out, int64_t Args::*rows, const char* sizes, std::string& msg) {
    if (!a || !out) return side_bad(msg, TDA_E_INVALID, "args and out are required");
    if (a->B < 1 || a->*rows < 1 || a->D < 1) return side_bad(msg, TDA_E_INVALID, sizes);
    if (!a->x) return side_bad(msg, TDA_E_INVALID, "x is NULL");
    return side_check_dtype(a->dtype, msg);
}
inline int ed_plan(const tda_ed_args* a, const float* out, EdJob& j, std::string& msg) {
    if (int rc = ed_check_head(a, out, &tda_ed_args::N, "need B, N, D >= 1", msg)) return rc;
    if (int rc = ed_check_shape("effective dimensionality", a->N, a->D, msg)) return rc;
    j = EdJob{a->x, a->dtype, a->x_on_device, a->B, a->N, a->D, 0, 0, 0, a->device, a->stream};
    ed_layout(j, 1);
    return 0;
}
// tda_spectral_args -> the job, one float per matrix: the window split of metrics.py:61-96
inline int spectral_plan(const char* what, const tda_spectral_args* a, const float* out, bool need_windows, EdJob& j, std::string& msg) {
    if (int rc = ed_check_head(a, out, &tda_spectral_args::S, "need B, S, D >= 1", msg)) return rc;
    if (a->n_windows < 0 || (need_windows && a->n_windows == 0)) return side_bad(msg, TDA_E_INVALID, "n_windows must be positive");
    const int64_t W = std::min(a->n_windows, a->S);  // more windows than rows: each row is its own window
    const int64_t rows = W ? a->S / W : a->S;
    j = EdJob{a->x, a->dtype, a->x_on_device, a->B * std::max<int64_t>(W, 1), rows, a->D, 0, 0, 0, a->device, a->stream};
    if (W && a->S % W) j.src_items = a->B, j.src_rows = a->S, j.keep_rows = W * rows;
    if (int rc = ed_check_shape(what, rows, a->D, msg)) return rc;
    ed_layout(j, 1);
    return 0;
}
// tda_matrix_entropy: the job, then its orders (n_alpha floats per matrix)
inline int entropy_plan(const tda_spectral_args* a, const float* out, EdJob& j, std::string& msg) {
    if (int rc = spectral_plan("matrix entropy", a, out, false, j, msg)) return rc;
    if (a->n_alpha < 1 || a->n_alpha > kSideEdMaxAlpha) return side_bad(msg, TDA_E_INVALID, "matrix entropy: 1 .. 16 orders per call");
    if (!a->alphas) return side_bad(msg, TDA_E_INVALID, "alphas is NULL");
    if (!(a->eps >= 0.0)) return side_bad(msg, TDA_E_INVALID, "matrix entropy: eps must be >= 0");
    for (int i = 0; i < a->n_alpha; ++i)  // order <= 0 counts the zero eigenvalues of the N x N Gram matrix, which the reference's f32 noise decides
        if (!(a->alphas[i] > 0.0) || !std::isfinite(a->alphas[i])) return side_bad(msg, TDA_E_INVALID, "matrix entropy: every order alpha must be finite and > 0");
    ed_layout(j, a->n_alpha);
    return 0;
}

// ---------------------------------------------------------------- UMAP: fit and transform
// the checks the two entries share, in three runs (their own size limits stand between them)
template <typename Args>
inline int umap_check_kind(const Args* a, std::string& msg) {
    if (int rc = side_check_dtype(a->dtype, msg)) return rc;
    if (a->metric != TDA_UMAP_EUCLIDEAN && a->metric != TDA_UMAP_COSINE) return side_bad(msg, TDA_E_UNSUPPORTED, "metric must be 'euclidean' or 'cosine'");
    return 0;
}
template <typename Args>
inline int umap_check_knn(const Args* a, std::string& msg) {
    if (a->n_neighbors < 2 || a->n_neighbors > kSideUmapMaxK || a->n_neighbors > a->N)
        return side_bad(msg, TDA_E_INVALID, "n_neighbors must be in [2, min(64, N)]");
    if (a->n_components < 1 || a->n_components > kSideUmapMaxC) return side_bad(msg, TDA_E_INVALID, "n_components must be in [1, 8]");
    return 0;
}
template <typename Args>
inline int umap_check_sgd(const Args* a, std::string& msg) {
    if (a->n_epochs < 1 || a->negative_sample_rate < 0) return side_bad(msg, TDA_E_INVALID, "n_epochs >= 1, negative_sample_rate >= 0");
    if (!(a->a > 0.0f) || !(a->b > 0.0f)) return side_bad(msg, TDA_E_INVALID, "a, b must be positive");
    return 0;
}

struct UmapPlan {
    size_t L = 0, N = 0, D = 0, k = 0, c = 0, esz = 0;
    uint64_t ecap = 0;  // edges of a layer at most
    size_t o_x = 0, o_dist = 0, o_rmax = 0, o_kd = 0, o_ki = 0, o_P = 0, o_S = 0, o_smax = 0, o_ne = 0, o_head = 0, o_tail = 0, o_eps = 0,
           o_nxt = 0, o_nxn = 0, o_deg = 0, o_emb = 0, total = 0;
    bool spectral = false;               // the spectral layout (else random init)
    size_t spec_lds = 0, sgd_lds = 0;    // dynamic LDS of k_umap_spectral (when spectral) and k_umap_sgd
};
inline int umap_plan(const tda_umap_args* a, UmapPlan& p, std::string& msg) {
    if (!a) return side_bad(msg, TDA_E_INVALID, "args is NULL");
    if (!a->x || !a->out) return side_bad(msg, TDA_E_INVALID, "x and out are required");
    if (a->L < 1 || a->N < 2 || a->D < 1) return side_bad(msg, TDA_E_INVALID, "need L >= 1, N >= 2, D >= 1");
    if (int rc = umap_check_kind(a, msg)) return rc;
    if (a->N >= 4096) return side_bad(msg, TDA_E_UNSUPPORTED, "UMAP: N < 4096 (umap-learn's exact small-data regime) is supported");
    if (int rc = umap_check_knn(a, msg)) return rc;
    if ((size_t)a->N * a->n_components * 12 > kSideUmapLds) return side_bad(msg, TDA_E_UNSUPPORTED, "UMAP: N * n_components too large for LDS");
    if (int rc = umap_check_sgd(a, msg)) return rc;
    const size_t L = p.L = (size_t)a->L, N = p.N = (size_t)a->N, D = p.D = (size_t)a->D, k = p.k = (size_t)a->n_neighbors, c = p.c = (size_t)a->n_components;
    const size_t esz = p.esz = a->dtype == TDA_F64 ? 8 : 4;
    const uint64_t ecap = p.ecap = align_up(2 * N * k, 64);
    Carve cv;
    p.o_x = cv.take(a->x_on_device ? 0 : L * N * D * esz), p.o_dist = cv.take(L * N * N * 4), p.o_rmax = cv.take(L * N * 4);
    p.o_kd = cv.take(L * N * k * 4), p.o_ki = cv.take(L * N * k * 4), p.o_P = cv.take(L * N * N * 4), p.o_S = cv.take(L * N * N * 4);
    p.o_smax = cv.take(L * 4), p.o_ne = cv.take(L * 4), p.o_head = cv.take(L * ecap * 4), p.o_tail = cv.take(L * ecap * 4);
    p.o_eps = cv.take(L * ecap * 8), p.o_nxt = cv.take(L * ecap * 8), p.o_nxn = cv.take(L * ecap * 8), p.o_deg = cv.take(L * N * 4);
    p.o_emb = cv.take(L * N * c * 4);
    p.total = cv.o;
    p.spec_lds = (2 * (c + 3) + 1) * N * 4;
    p.spectral = a->init == TDA_UMAP_INIT_SPECTRAL && (int64_t)N <= kSideUmapSpecMaxN && p.spec_lds <= kSideUmapLds;
    p.sgd_lds = align_up(4 * N * c, 16) + 8 * N * c;
    return 0;
}

struct UmapTransformPlan {
    size_t L = 0, M = 0, N = 0, D = 0, NM = 0, k = 0, c = 0, esz = 0;
    uint64_t ecap = 0;
    size_t o_xt = 0, o_y = 0, o_z = 0, o_dist = 0, o_rmax = 0, o_kd = 0, o_ki = 0, o_val = 0, o_eps = 0, o_nxt = 0, o_nxn = 0, o_temb = 0,
           o_emb = 0, total = 0;
    size_t lds = 0;          // dynamic LDS of k_umap_transform
    uint64_t tw = 0, lw = 0;  // 32-bit words of the training points and of one batch of new points
};
inline int umap_transform_plan(const tda_umap_transform_args* a, UmapTransformPlan& p, std::string& msg) {
    if (!a) return side_bad(msg, TDA_E_INVALID, "args is NULL");
    if (!a->x_train || !a->emb_train || !a->y || !a->out) return side_bad(msg, TDA_E_INVALID, "x_train, emb_train, y and out are required");
    if (a->L < 1 || a->M < 1 || a->N < 2 || a->D < 1) return side_bad(msg, TDA_E_INVALID, "need L >= 1, M >= 1, N >= 2, D >= 1");
    if (int rc = umap_check_kind(a, msg)) return rc;
    if (a->N + a->M > 8192) return side_bad(msg, TDA_E_UNSUPPORTED, "UMAP transform: N + M <= 8192 (exact small-data regime) is supported");
    if (int rc = umap_check_knn(a, msg)) return rc;
    const size_t L = p.L = (size_t)a->L, M = p.M = (size_t)a->M, N = p.N = (size_t)a->N, D = p.D = (size_t)a->D, NM = p.NM = N + M;
    const size_t k = p.k = (size_t)a->n_neighbors, c = p.c = (size_t)a->n_components;
    p.lds = align_up(4 * M * c, 16) + 8 * M * c + 4 * N * c;
    if (p.lds > kSideUmapLds) return side_bad(msg, TDA_E_UNSUPPORTED, "UMAP transform: (M, N) * n_components too large for LDS");
    if (int rc = umap_check_sgd(a, msg)) return rc;
    const size_t esz = p.esz = a->dtype == TDA_F64 ? 8 : 4;
    const uint64_t ecap = p.ecap = (uint64_t)M * k;
    Carve cv;
    p.o_xt = cv.take(a->x_on_device ? 0 : N * D * esz), p.o_y = cv.take(a->x_on_device ? 0 : L * M * D * esz), p.o_z = cv.take(L * NM * D * esz);
    p.o_dist = cv.take(L * NM * NM * 4), p.o_rmax = cv.take(L * NM * 4), p.o_kd = cv.take(L * M * k * 4), p.o_ki = cv.take(L * M * k * 4);
    p.o_val = cv.take(L * M * k * 4), p.o_eps = cv.take(L * ecap * 8), p.o_nxt = cv.take(L * ecap * 8), p.o_nxn = cv.take(L * ecap * 8);
    p.o_temb = cv.take(N * c * 4), p.o_emb = cv.take(L * M * c * 4);
    p.total = cv.o;
    p.tw = (uint64_t)N * D * esz / 4, p.lw = (uint64_t)M * D * esz / 4;
    return 0;
}

}  // namespace tda
