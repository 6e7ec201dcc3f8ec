// fm_plan.h -- the host plan of the Frechet mean of diagrams (include/tda_dgm.h tda_fm_args), beside
// dgm_plan.h and in its style: plain C++, no HIP; fm_plan returns an error code and leaves its
// message in `msg` (tests/fm_plan_main.cpp runs it with a host compiler alone).  The checks run in
// the order the header documents.  The entry's device side is not in the library yet (DESIGN.md
// 6.29), so nothing in rips.hip includes this file.
#pragma once
#include "dgm_plan.h"

namespace tda {

constexpr int kFmClassN[kPairClasses] = {64, 256, TDA_FM_MAX_POINTS};  // max(K, max_j n_j) at most; also the workgroup size

struct FmPlan {
    std::vector<double> pts;   // (total finite, 2): the diagrams' finite points
    std::vector<int64_t> off;  // [S + 1] into pts
    std::vector<double> y0;    // (K0, 2): the finite points of the start
    int64_t S = 0;
    int K0 = 0;     // points of the start
    int n_max = 0;  // the largest diagram of the call
};

// the class of a step whose candidate holds K points: the first whose limit holds max(K, n_max), or -1
inline int fm_class(int K, int n_max) {
    const int n = std::max(K, n_max);
    for (int c = 0; c < kPairClasses; ++c)
        if (n <= kFmClassN[c]) return c;
    return -1;
}

// G of a step: (S, K) row-major, the mate of column y in diagram j at j * K + y; its entries at the largest K
inline size_t fm_g_entries(int64_t S, int K) { return (size_t)S * (size_t)K; }

inline int fm_plan(const tda_fm_args* a, FmPlan& fp, std::string& msg) {
    auto bad = [&](int code, const char* m) { return msg = m, code; };
    if (int rc = dgm_check_head(a, msg)) return rc;
    if (a->reserved != 0) return bad(TDA_E_INVALID, "reserved must be 0");
    if (a->flags & ~TDA_FM_WANT_MATCHING) return bad(TDA_E_INVALID, "flags holds an unknown bit");
    if (a->max_iter < 1) return bad(TDA_E_INVALID, "max_iter must be >= 1");
    if (a->max_iter > TDA_FM_MAX_ITER) return bad(TDA_E_UNSUPPORTED, "frechet mean: max_iter > 1024 is not supported");
    if (a->S < 1) return bad(TDA_E_INVALID, "S must be >= 1");
    if (a->S > TDA_FM_MAX_DIAGRAMS) return bad(TDA_E_UNSUPPORTED, "frechet mean: more than 4096 diagrams in one call is not supported");
    if (int rc = dgm_check_layout(a->points, a->offsets, a->S, nullptr, 0, "frechet mean", msg)) return rc;
    if (a->init_index < -1 || a->init_index >= a->S) return bad(TDA_E_INVALID, "init_index must be -1 or in [0, S)");
    if (a->init_index == -1) {
        if (a->init_n < 0) return bad(TDA_E_INVALID, "init_n must be >= 0");
        if (a->init_n > 0 && !a->init_points) return bad(TDA_E_INVALID, "init_points is NULL");
    }
    fp.S = a->S;
    dgm_gather_points(a->points, a->offsets, a->S, fp.pts, fp.off);
    for (int64_t s = 0; s < a->S; ++s) {
        const int64_t n = fp.off[s + 1] - fp.off[s];
        if (n > TDA_FM_MAX_POINTS) return bad(TDA_E_UNSUPPORTED, "frechet mean: a diagram with more than 512 finite points is not supported");
        fp.n_max = std::max(fp.n_max, (int)n);
    }
    if (a->init_index >= 0) {
        fp.y0.assign(fp.pts.begin() + 2 * fp.off[a->init_index], fp.pts.begin() + 2 * fp.off[a->init_index + 1]);
    } else {
        const int64_t one[2] = {0, a->init_n};
        std::vector<int64_t> yoff;
        dgm_gather_points(a->init_points, one, 1, fp.y0, yoff);
        if (yoff[1] > TDA_FM_MAX_POINTS) return bad(TDA_E_UNSUPPORTED, "frechet mean: a start with more than 512 finite points is not supported");
    }
    fp.K0 = (int)(fp.y0.size() / 2);
    return 0;
}

}  // namespace tda
