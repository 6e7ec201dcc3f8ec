// geo_plan.h -- the host plan of tda_geodesic (include/tda_rips.h): the argument checks in the
// header's order, each with its message, then every size the call needs: the distance stage of a
// chunk of layers (side_plan.h's SqDistPlan), which graph is built, which closure runs (resident in
// LDS, or blocked over 64 x 64 tiles), the tile count and the padded size of the blocked path, the
// LDS bytes of each kernel, the byte offset of every array in the resampling family's workspace and
// the total.  The counts of all L layers sit beside the chunk of layers; the rows' thresholds are
// chunked with the layers.  Plain C++, no HIP: tests/geo_plan_main.cpp prints a plan with a host
// compiler alone and tests/test_shortest_paths_cpu.py pins it.  The kernels' constants are restated
// here as kSideGeo*; geo_host.h asserts that they are the kernels' own.
#pragma once
#include "side_plan.h"

namespace tda {

constexpr int kSideGeoLdsN = 128;  // kGeoLdsN: the resident closure's largest N (its matrix in 64 KiB of static LDS)
constexpr int kSideGeoTile = 64;   // kGeoTile: the side of a tile of the blocked closure
constexpr int kSideGeoT = 256;     // kGeoT: threads of a workgroup, every kernel

struct GeoPlan {
    size_t L = 0, N = 0;
    bool is_dist = false, knn = false, graph_only = false;
    bool resident = false;  // the LDS-resident closure (else the blocked one)
    size_t k = 0;           // kNN: neighbours per row, min(n_neighbors, N - 1)
    size_t lds_n = 0;       // the resident limit in force (TDA_GEO_LDS_N can only lower it, in tests)
    size_t tiles = 0;       // blocked: tiles per side, and so rounds
    // Descriptive only, nothing reads the next five: there is no padded copy (a tile reads +inf and stores
    // nothing beyond N) and every kernel's LDS is static, so no launch is given a size.
    size_t padded = 0;      // blocked: tiles * 64, the side of the matrix the tiles cover
    size_t lds_select = 0, lds_resident = 0, lds_diag = 0, lds_product = 0;  // static LDS of the four kernels that use any
    SqDistPlan sq;
    size_t o_ne = 0, o_nc = 0, o_thr = 0, total = 0;
};

// the resident limit: kSideGeoLdsN, or TDA_GEO_LDS_N (tests: at least 1, never above the kernel's)
inline size_t geo_lds_n() {
    if (const char* e = test_env("TDA_GEO_LDS_N")) return std::min<size_t>(kSideGeoLdsN, std::max<size_t>(1, strtoull(e, nullptr, 10)));
    return kSideGeoLdsN;
}

inline int geo_plan(const tda_geodesic_args* a, size_t cap, GeoPlan& p, std::string& msg) {
    if (int rc = side_check_x(a, msg)) return rc;
    if (int rc = side_check_cloud(a, msg)) return rc;
    if (a->n_neighbors < 0) return side_bad(msg, TDA_E_INVALID, "n_neighbors must be >= 1 (0: not given)");
    if (std::isnan(a->radius)) return side_bad(msg, TDA_E_INVALID, "radius is NaN");
    if (a->n_neighbors >= 1 && a->radius >= 0.0) return side_bad(msg, TDA_E_INVALID, "give n_neighbors or radius, not both");
    if (a->n_neighbors == 0 && !(a->radius >= 0.0)) return side_bad(msg, TDA_E_INVALID, "give n_neighbors >= 1 or radius >= 0");
    if (a->N > kSideMaxN) return side_bad(msg, TDA_E_UNSUPPORTED, "geodesic distances: N > 8192 is not supported");
    if ((unsigned __int128)a->L * (uint64_t)a->N * (uint64_t)a->N > (uint64_t)TDA_GEO_MAX_OUT)
        return side_bad(msg, TDA_E_UNSUPPORTED, "geodesic distances: more than 2^28 values (L * N * N) in one call is not supported: split L over several calls");
    if (int rc = side_check_f64_points(a, "geodesic distances", msg)) return rc;
    const size_t L = (size_t)a->L, N = (size_t)a->N;
    if (a->is_dist && !a->x_on_device)
        for (size_t e = 0; e < L * N * N; ++e) {
            const double v = a->dtype == TDA_F64 ? ((const double*)a->x)[e] : (double)((const float*)a->x)[e];
            if (!std::isfinite(v) || v < 0.0)
                return side_bad(msg, TDA_E_INVALID,
                                "x[" + std::to_string(e / (N * N)) + "][" + std::to_string(e / N % N) + "][" + std::to_string(e % N) + "] = " +
                                    std::to_string(v) + " is not finite and >= 0");
        }
    p.L = L, p.N = N;
    p.is_dist = a->is_dist != 0, p.knn = a->n_neighbors >= 1, p.graph_only = a->graph_only != 0;
    p.k = p.knn ? std::min<size_t>((size_t)a->n_neighbors, N - 1) : 0;
    p.lds_n = geo_lds_n();
    p.resident = N <= p.lds_n;
    p.tiles = p.resident ? 0 : (N + kSideGeoTile - 1) / kSideGeoTile;
    p.padded = p.tiles * kSideGeoTile;
    p.lds_select = (size_t)kSideMaxN * 4 + 2 * (kSideGeoT / 64) * 4;
    p.lds_resident = (size_t)kSideGeoLdsN * kSideGeoLdsN * 4;
    p.lds_diag = (size_t)kSideGeoTile * kSideGeoTile * 4;
    p.lds_product = 2 * p.lds_diag;
    p.sq = sq_dist_plan(L, N, a->D, a->dtype, p.is_dist, !a->x_on_device, p.knn ? N * 8 : 0, cap);
    Carve cv;
    p.o_ne = cv.take(L * 8), p.o_nc = cv.take(L * 4), p.o_thr = cv.take(p.knn ? p.sq.Lc * N * 8 : 0);
    p.sq.carve(cv);
    p.total = cv.o;
    return 0;
}

}  // namespace tda
