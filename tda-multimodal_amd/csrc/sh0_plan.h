// sh0_plan.h -- the host plan of tda_subsample_h0 (include/tda_rips.h): the argument checks in the
// header's order, each with its message, then every size the call needs: the distance stage of a
// chunk of layers (side_plan.h's SqDistPlan), the subsamples per launch, which of k_subsample_h0's
// two paths runs, the dynamic LDS of the global path, the byte offset of every array in the
// resampling family's workspace and the total.  The whole (L, B) result, the sizes and a shared
// table sit beside the chunk of layers, as in ResamplePlan; a table per layer and the deaths are
// chunked with the layers.  Plain C++, no HIP: tests/sh0_plan_main.cpp prints a plan with a host
// compiler alone and tests/test_subsample_h0_cpu.py pins it.  The kernel's limits are restated here
// as kSideSh0*; sh0_host.h asserts that they are the kernel's own.
#pragma once
#include "side_plan.h"

namespace tda {

constexpr int kSideSh0LdsN = 128;      // kSh0LdsN: the resident path's largest N (its matrix in 64 KiB of LDS)
constexpr int kSideSh0LdsM = 128;      // kSh0LdsM: and its largest row length (two keys per lane)
constexpr int kSideSh0PerBlock = 16;   // kSh0PerBlock: subsamples served by a resident workgroup
constexpr size_t kSideSh0Head = 128;   // kSh0Head: the block argmin's partials in front of the global path's keys

struct Sh0Plan {
    size_t L = 0, N = 0, B = 0, m = 0;
    bool is_dist = false, per_layer_idx = false, want_deaths = false;
    bool resident = false;   // the LDS-resident path (else one workgroup per subsample and layer)
    int mode = 0;            // term(w): 0 w, 1 w * w, 2 pow(w, alpha)
    size_t Bc = 0;           // subsamples per launch: grid dimensions stay <= 65535
    size_t idx_lstride = 0;  // the table's entries per layer (0: one table for every layer)
    size_t d_lstride = 0;    // the deaths' entries per layer
    size_t lds = 0;          // dynamic LDS of the global path: the head, m f32 keys, m u16 points
    SqDistPlan sq;
    size_t o_E = 0, o_sz = 0, o_idx = 0, o_deaths = 0, total = 0;
};

inline int sh0_plan(const tda_subsample_h0_args* a, size_t cap, Sh0Plan& p, std::string& msg) {
    if (int rc = side_check_x(a, msg)) return rc;
    if (!a->idx) return side_bad(msg, TDA_E_INVALID, "idx is NULL");
    if (!a->sizes) return side_bad(msg, TDA_E_INVALID, "sizes is NULL");
    if (int rc = side_check_cloud(a, msg)) return rc;
    if (a->B < 1) return side_bad(msg, TDA_E_INVALID, "B must be >= 1");
    if (a->m < 1) return side_bad(msg, TDA_E_INVALID, "m must be >= 1");
    const size_t B = (size_t)a->B, m = (size_t)a->m, layers = a->idx_per_layer ? (size_t)a->L : 1;
    for (size_t b = 0; b < B; ++b)
        if (a->sizes[b] < 1 || a->sizes[b] > a->m)
            return side_bad(msg, TDA_E_INVALID,
                            "sizes[" + std::to_string(b) + "] = " + std::to_string(a->sizes[b]) + " is outside [1, m = " + std::to_string(a->m) + "]");
    for (size_t r = 0; r < layers * B; ++r) {  // the first sizes[b] entries of every row; the rest is never read
        const size_t e0 = r * m, s = (size_t)a->sizes[r % B];
        for (size_t e = e0; e < e0 + s; ++e)
            if (a->idx[e] < 0 || a->idx[e] >= a->N)
                return side_bad(msg, TDA_E_INVALID,
                                "idx[" + std::to_string(e) + "] = " + std::to_string(a->idx[e]) + " is outside [0, N = " + std::to_string(a->N) + ")");
    }
    if (!std::isfinite(a->alpha) || !(a->alpha > 0.0)) return side_bad(msg, TDA_E_INVALID, "alpha must be finite and > 0");
    if (a->N > kSideMaxN) return side_bad(msg, TDA_E_UNSUPPORTED, "subsample H0: N > 8192 is not supported");
    if (a->m > kSideMaxN) return side_bad(msg, TDA_E_UNSUPPORTED, "subsample H0: m > 8192 is not supported");
    if ((unsigned __int128)a->L * (uint64_t)a->B > (uint64_t)TDA_SH0_MAX_OUT)
        return side_bad(msg, TDA_E_UNSUPPORTED, "subsample H0: more than 2^27 subsamples (L * B) in one call is not supported: split B over several calls");
    if (a->want_deaths && (unsigned __int128)a->L * (uint64_t)a->B * (uint64_t)(a->m - 1) > (uint64_t)TDA_SH0_MAX_OUT)
        return side_bad(msg, TDA_E_UNSUPPORTED,
                        "subsample H0: more than 2^27 deaths (L * B * (m - 1)) in one call is not supported: split B over several calls");
    if (int rc = side_check_f64_points(a, "subsample H0", msg)) return rc;
    p.L = (size_t)a->L, p.N = (size_t)a->N, p.B = B, p.m = m;
    p.is_dist = a->is_dist != 0, p.per_layer_idx = a->idx_per_layer != 0, p.want_deaths = a->want_deaths != 0;
    p.resident = p.N <= (size_t)kSideSh0LdsN && m <= (size_t)kSideSh0LdsM;
    p.mode = a->alpha == 1.0 ? 0 : a->alpha == 2.0 ? 1 : 2;
    p.Bc = std::min<size_t>(B, 65535);
    p.idx_lstride = p.per_layer_idx ? B * m : 0;
    p.d_lstride = B * (m - 1);
    p.lds = kSideSh0Head + 6 * m;
    const size_t idx_layer = p.per_layer_idx ? B * m * 4 : 0, deaths_layer = p.want_deaths ? p.d_lstride * 4 : 0;
    p.sq = sq_dist_plan(p.L, p.N, a->D, a->dtype, p.is_dist, !a->x_on_device, align_up(idx_layer, 256) + align_up(deaths_layer, 256), cap);
    Carve cv;
    p.o_E = cv.take(p.L * B * 8), p.o_sz = cv.take(B * 4), p.o_idx = cv.take((p.per_layer_idx ? p.sq.Lc : 1) * B * m * 4);
    p.o_deaths = cv.take(p.sq.Lc * deaths_layer);
    p.sq.carve(cv);
    p.total = cv.o;
    return 0;
}

}  // namespace tda
