// dgm_plan.h -- the host plans of the eight entries of include/tda_dgm.h, one per entry: sw_plan, bn_plan
// and ws_plan (PairPlan: the layout checks, the finite points and the pair list, the pairs sorted into size
// classes and, for tda_wasserstein, oriented canonically), hk_plan (HkPlan: the work list of
// tda_heat_kernel), pf_plan (PfPlan: that of tda_persistence_fisher) and pl_plan / pi_plan / pc_plan (VecPlan: per
// diagram, at the end), each with the size classes
// of its launches.  Plain C++, no HIP: a plan returns an error code and leaves its message in `msg`
// (tests/dgm_plan_main.cpp, ws_plan_main.cpp, hk_plan_main.cpp, pf_plan_main.cpp, vec_plan_main.cpp and pc_plan_main.cpp run
// them with a host compiler alone).  The checks of a plan run in the order its entry has always made them.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tda_dgm.h"

namespace tda {

constexpr int kPairClasses = 3;

// what the device reads, laid out on the host: one upload
struct PairPlan {
    std::vector<double> pts;     // (total finite, 2)
    std::vector<int64_t> off;    // [S + 1] into pts
    std::vector<int32_t> pairs;  // (P, 2)
    std::vector<int32_t> order;  // [P]: pair ids, class 0 first, ascending within a class
    int64_t cls_cnt[kPairClasses] = {};
    int cls_n[kPairClasses] = {};  // the largest size of the class
    int64_t P = 0;
};

// the first three checks of a pair entry, before its own (M, reserved, flags, sigma)
template <typename Args>
inline int dgm_check_head(const Args* a, std::string& msg) {
    if (!a) return msg = "args is NULL", TDA_E_INVALID;
    if (a->S < 0) return msg = "S must be >= 0", TDA_E_INVALID;
    if (!a->offsets) return msg = "offsets is NULL", TDA_E_INVALID;
    return 0;
}

// The layout checks every entry of tda_dgm.h shares, in the order tda_sliced_wasserstein has always made them
// (S >= 0 and offsets != NULL are checked by the caller first, with its own checks in between).
inline int dgm_check_layout(const double* points, const int64_t* offsets, int64_t S, const int32_t* pairs, int64_t P, const char* what,
                            std::string& msg) {
    auto bad = [&](int code, const std::string& m) { return msg = m, code; };
    if (offsets[0] != 0) return bad(TDA_E_INVALID, "offsets[0] must be 0");
    for (int64_t s = 0; s < S; ++s)
        if (offsets[s + 1] < offsets[s]) return bad(TDA_E_INVALID, "offsets must be non-decreasing");
    if (offsets[S] > 0 && !points) return bad(TDA_E_INVALID, "points is NULL");
    if (pairs && P < 0) return bad(TDA_E_INVALID, "P must be >= 0");
    if (S > TDA_SW_MAX_WORK) return bad(TDA_E_UNSUPPORTED, std::string(what) + ": too many diagrams in one call");
    return 0;
}

// pts / off: the finite points of the S diagrams (the essential classes dropped) with their row boundaries
inline void dgm_gather_points(const double* points, const int64_t* offsets, int64_t S, std::vector<double>& pts, std::vector<int64_t>& off) {
    off.assign((size_t)S + 1, 0);
    pts.reserve((size_t)offsets[S] * 2);
    for (int64_t s = 0; s < S; ++s) {
        for (int64_t r = offsets[s]; r < offsets[s + 1]; ++r) {
            const double b = points[2 * r], d = points[2 * r + 1];
            if (!std::isfinite(b) || !std::isfinite(d)) continue;  // the essential classes
            pts.push_back(b);
            pts.push_back(d);
        }
        off[s + 1] = (int64_t)(pts.size() / 2);
    }
}

// pl.pts / off: dgm_gather_points; pl.pairs / P: the P pairs, copied and index-checked or, for pairs == NULL, every i < j in
// row-major order.  offsets is valid (dgm_check_layout).
inline int dgm_gather(const double* points, const int64_t* offsets, int64_t S, const int32_t* pairs, int64_t P, PairPlan& pl,
                      std::string& msg) {
    pl.P = P;
    dgm_gather_points(points, offsets, S, pl.pts, pl.off);
    pl.pairs.resize((size_t)P * 2);
    if (pairs) {
        for (int64_t q = 0; q < 2 * P; ++q) {
            if (pairs[q] < 0 || pairs[q] >= S) return msg = "pairs holds an index outside [0, S)", TDA_E_INVALID;
            pl.pairs[q] = pairs[q];
        }
    } else {
        size_t q = 0;
        for (int32_t i = 0; i < S; ++i)
            for (int32_t j = i + 1; j < S; ++j) {
                pl.pairs[q++] = i;
                pl.pairs[q++] = j;
            }
    }
    return 0;
}

// What a pair entry does after its own argument checks: the layout, P (every i < j without a list),
// the limit of a call's work (P and P * per_pair at most 2^27, else `too_many`), the points and the pairs.
template <typename Args>
inline int dgm_pairs(const Args* a, const char* what, int64_t per_pair, const char* too_many, PairPlan& pl, std::string& msg) {
    if (int rc = dgm_check_layout(a->points, a->offsets, a->S, a->pairs, a->P, what, msg)) return rc;
    const int64_t P = a->pairs ? a->P : a->S * (a->S - 1) / 2;
    if (P > TDA_SW_MAX_WORK || P * per_pair > TDA_SW_MAX_WORK) return msg = too_many, TDA_E_UNSUPPORTED;
    return dgm_gather(a->points, a->offsets, a->S, a->pairs, P, pl, msg);
}

// The counting sort of every plan: item x of size size_of(x) belongs to the first class whose limit
// holds it (limits ascending); order lists the items class 0 first, ascending within a class, and
// cls_n is the largest size of each class.  False at the first item larger than the last limit.
template <int C, typename SizeOf>
inline bool dgm_sort_classes(int64_t count, SizeOf&& size_of, const int (&limits)[C], std::vector<int32_t>& order, int64_t (&cls_cnt)[C],
                             int (&cls_n)[C]) {
    std::vector<uint8_t> cls((size_t)count);
    for (int64_t x = 0; x < count; ++x) {
        const int64_t n = size_of(x);
        if (n > limits[C - 1]) return false;
        int c = 0;
        while (n > limits[c]) ++c;
        cls[x] = (uint8_t)c;
        cls_cnt[c]++;
        cls_n[c] = std::max(cls_n[c], (int)n);
    }
    order.resize((size_t)count);
    int64_t at[C], sum = 0;
    for (int c = 0; c < C; ++c) {
        at[c] = sum;
        sum += cls_cnt[c];
    }
    for (int64_t x = 0; x < count; ++x) order[at[cls[x]]++] = (int32_t)x;
    return true;
}

enum class PairSize { kSum, kMax };  // a pair's size: n1 + n2 or max(n1, n2) finite points

// Sorts the gathered pairs into classes: class c holds the pairs of size <= limits[c] (ascending;
// the last one is the limit of a call: a larger pair is TDA_E_UNSUPPORTED with `too_large`).
inline int dgm_classify(PairPlan& pl, PairSize measure, const int (&limits)[kPairClasses], const char* too_large, std::string& msg) {
    auto size_of = [&](int64_t p) {
        const int32_t i = pl.pairs[2 * p], j = pl.pairs[2 * p + 1];
        const int64_t n1 = pl.off[i + 1] - pl.off[i], n2 = pl.off[j + 1] - pl.off[j];
        return measure == PairSize::kSum ? n1 + n2 : std::max(n1, n2);
    };
    if (!dgm_sort_classes(pl.P, size_of, limits, pl.order, pl.cls_cnt, pl.cls_n)) return msg = too_large, TDA_E_UNSUPPORTED;
    return 0;
}

// Orients every gathered pair canonically, for a kernel that has to see the same input for (i, j) and
// (j, i): the diagram with more finite points first and, at equal counts, the one whose finite points
// (b0, d0, b1, d1, ...) come first lexicographically (by value, -0 below +0, so that equal means the
// same bits).  swapped[p] = 1 where the two entries of pair p in pl.pairs were exchanged.
inline void dgm_orient(PairPlan& pl, std::vector<uint8_t>& swapped) {
    auto key = [](double x) {  // finite doubles as integers in the order of their values
        uint64_t b;
        std::memcpy(&b, &x, 8);
        return b >> 63 ? ~b : b | (uint64_t)1 << 63;
    };
    swapped.assign((size_t)pl.P, 0);
    for (int64_t p = 0; p < pl.P; ++p) {
        const int32_t i = pl.pairs[2 * p], j = pl.pairs[2 * p + 1];
        const int64_t n1 = pl.off[i + 1] - pl.off[i], n2 = pl.off[j + 1] - pl.off[j];
        bool swap = n2 > n1;
        if (n1 == n2 && i != j) {
            const double *a = pl.pts.data() + 2 * pl.off[i], *b = pl.pts.data() + 2 * pl.off[j];
            for (int64_t k = 0; k < 2 * n1; ++k)
                if (key(a[k]) != key(b[k])) {
                    swap = key(b[k]) < key(a[k]);
                    break;
                }
        }
        if (swap) {
            std::swap(pl.pairs[2 * p], pl.pairs[2 * p + 1]);
            swapped[p] = 1;
        }
    }
}

// ---------------------------------------------------------------- the three distances
// Size classes: what a class means for a launch is told where the launch is (dgm_host.h, bn_host.h, ws_host.h).

struct SwClass {
    int npow_max, threads, dirs_per_wg;  // next_pow2(n1 + n2) at most
};
constexpr SwClass kSwClasses[kPairClasses] = {{128, 64, 8}, {1024, 256, 1}, {TDA_SW_MAX_POINTS, 1024, 1}};
constexpr int kBnClassN[kPairClasses] = {64, 256, TDA_BN_MAX_POINTS};  // max(n1, n2) at most; also the workgroup size
constexpr int kWsClassN[kPairClasses] = {64, 256, TDA_WS_MAX_POINTS};  // max(n1, n2) at most; also the workgroup size

inline int sw_plan(const tda_sw_args* a, PairPlan& pl, std::string& msg) {
    auto bad = [&](int code, const char* m) { return msg = m, code; };
    if (int rc = dgm_check_head(a, msg)) return rc;
    if (a->M < 1) return bad(TDA_E_INVALID, "M must be >= 1");
    if (a->M > TDA_SW_MAX_DIRECTIONS) return bad(TDA_E_UNSUPPORTED, "sliced Wasserstein: M > 1024 directions is not supported");
    if (int rc = dgm_pairs(a, "sliced Wasserstein", a->M, "sliced Wasserstein: P * M > 2^27 in one call is not supported (split the pairs)", pl, msg))
        return rc;
    const int limits[kPairClasses] = {kSwClasses[0].npow_max, kSwClasses[1].npow_max, kSwClasses[2].npow_max};
    return dgm_classify(pl, PairSize::kSum, limits, "sliced Wasserstein: a pair of diagrams with more than 4096 finite points together is not supported",
                        msg);
}

inline int bn_plan(const tda_bn_args* a, PairPlan& pl, std::string& msg) {
    if (int rc = dgm_check_head(a, msg)) return rc;
    if (a->reserved != 0) return msg = "reserved must be 0", TDA_E_INVALID;
    if (int rc = dgm_pairs(a, "bottleneck", 1, "bottleneck: more than 2^27 pairs in one call is not supported (split the pairs)", pl, msg)) return rc;
    return dgm_classify(pl, PairSize::kMax, kBnClassN, "bottleneck: a diagram with more than 512 finite points is not supported", msg);
}

// the pairs oriented (swapped[p]: pair p was exchanged) and, with the matching, moff [P + 1]: where
// the mates of each pair's first diagram (as oriented) start in the device's match array
struct WsPlan {
    PairPlan pl;
    std::vector<uint8_t> swapped;
    std::vector<int64_t> moff;
};

inline int ws_plan(const tda_ws_args* a, WsPlan& wp, std::string& msg) {
    if (int rc = dgm_check_head(a, msg)) return rc;
    if (a->flags & ~TDA_WS_WANT_MATCHING) return msg = "flags holds an unknown bit", TDA_E_INVALID;
    PairPlan& pl = wp.pl;
    if (int rc = dgm_pairs(a, "wasserstein", 1, "wasserstein: more than 2^27 pairs in one call is not supported (split the pairs)", pl, msg)) return rc;
    if (int rc = dgm_classify(pl, PairSize::kMax, kWsClassN, "wasserstein: a diagram with more than 512 finite points is not supported", msg)) return rc;
    dgm_orient(pl, wp.swapped);
    if (a->flags & TDA_WS_WANT_MATCHING) {
        wp.moff.assign((size_t)pl.P + 1, 0);
        for (int64_t p = 0; p < pl.P; ++p) wp.moff[p + 1] = wp.moff[p] + (pl.off[pl.pairs[2 * p] + 1] - pl.off[pl.pairs[2 * p]]);
        if (wp.moff[pl.P] > TDA_SW_MAX_WORK)
            return msg = "wasserstein: a matching of more than 2^27 entries in one call is not supported (split the pairs)", TDA_E_UNSUPPORTED;
    }
    return 0;
}

// ---------------------------------------------------------------- the heat kernel (tda_heat_kernel)
// The work list of a call: its P pairs and then the S self pairs (s, s), every one oriented
// canonically (dgm_orient) and cut into parts of kHkRows rows of the first diagram by kHkChunk
// columns of the second (tda_dgm.h gives the order of the sum that these two constants fix).

constexpr int kHkRows = 64;     // rows of a part: one per lane of the part's wave
constexpr int kHkChunk = 256;   // columns of a part: the points staged in LDS
constexpr int kHkClassN[kPairClasses] = {kHkRows, 512, TDA_HK_MAX_POINTS};  // max(n1, n2) at most

struct HkPlan {
    PairPlan pl;                    // pl.P = P + S evaluations; pl.pairs oriented
    std::vector<int64_t> part_off;  // [P + S + 1] into the parts, in the order of pl.pairs
    int cls_parts[kPairClasses] = {};  // the largest number of parts of an evaluation of the class
    int64_t P = 0, S = 0;           // the caller's pairs and diagrams
    double c8 = 0.0, cn = 0.0;
};

inline int64_t hk_parts(int64_t n1, int64_t n2) { return ((n1 + kHkRows - 1) / kHkRows) * ((n2 + kHkChunk - 1) / kHkChunk); }

inline int hk_plan(const tda_hk_args* a, HkPlan& hp, std::string& msg) {
    auto bad = [&](int code, const char* m) { return msg = m, code; };
    if (int rc = dgm_check_head(a, msg)) return rc;
    if (a->reserved != 0) return bad(TDA_E_INVALID, "reserved must be 0");
    if (!std::isfinite(a->sigma) || !(a->sigma > 0.0)) return bad(TDA_E_INVALID, "sigma must be finite and > 0");
    hp.c8 = 1.0 / (8.0 * a->sigma);  // 8 sigma is exact (or overflows: c8 = 0, refused below)
    hp.cn = 1.0 / (25.132741228718345908 * a->sigma);  // 8 pi, rounded
    if (!std::isnormal(hp.c8) || !std::isnormal(hp.cn))
        return bad(TDA_E_INVALID, "sigma: 1 / (8 sigma) and 1 / (8 pi sigma) must be finite normal numbers");
    PairPlan& pl = hp.pl;
    if (int rc = dgm_pairs(a, "heat kernel", 1, "heat kernel: more than 2^27 pairs in one call is not supported (split the pairs)", pl, msg)) return rc;
    const int64_t P = hp.P = pl.P;
    hp.S = a->S;
    for (int64_t s = 0; s < a->S; ++s) {  // every diagram has a self, named by a pair or not
        if (pl.off[s + 1] - pl.off[s] > TDA_HK_MAX_POINTS)
            return bad(TDA_E_UNSUPPORTED, "heat kernel: a diagram with more than 4096 finite points is not supported");
        pl.pairs.push_back((int32_t)s);
        pl.pairs.push_back((int32_t)s);
    }
    pl.P = P + a->S;
    if (int rc = dgm_classify(pl, PairSize::kMax, kHkClassN, "heat kernel: a diagram with more than 4096 finite points is not supported", msg))
        return rc;
    std::vector<uint8_t> swapped;
    dgm_orient(pl, swapped);  // k and heat are symmetric: nothing to turn back
    hp.part_off.assign((size_t)pl.P + 1, 0);
    for (int64_t w = 0; w < pl.P; ++w) {
        const int32_t i = pl.pairs[2 * w], j = pl.pairs[2 * w + 1];
        const int64_t n1 = pl.off[i + 1] - pl.off[i], n2 = pl.off[j + 1] - pl.off[j];
        const int64_t parts = hk_parts(n1, n2);
        hp.part_off[w + 1] = hp.part_off[w] + parts;
        int c = 0;
        while (std::max(n1, n2) > kHkClassN[c]) ++c;
        hp.cls_parts[c] = std::max(hp.cls_parts[c], (int)parts);
    }
    if (hp.part_off[pl.P] > TDA_SW_MAX_WORK)
        return bad(TDA_E_UNSUPPORTED, "heat kernel: more than 2^27 parts of 64 x 256 terms in one call is not supported (split the pairs)");
    return 0;
}

// ---------------------------------------------------------------- the persistence Fisher distance (tda_persistence_fisher)
// The work list of a call: its P pairs and nothing else (no selfs), every one oriented canonically
// (dgm_orient; swapped[p] tells which, so that a and b go back to the diagrams as the caller named
// them) and cut into parts of kPfLanes evaluation points of Z = U then V (tda_dgm.h gives the order
// of the sums that this constant fixes; kPfChunk only sizes the staging of the sources).

constexpr int kPfLanes = TDA_PF_LANES;  // evaluation points of a part: one per lane of the part's wave
constexpr int kPfChunk = TDA_PF_CHUNK;  // sources of U and of V staged in LDS at a time
constexpr int kPfClassM[kPairClasses] = {64, 512, 2 * TDA_PF_MAX_POINTS};  // n1 + n2 at most: 2, 16 and 64 parts

struct PfPlan {
    PairPlan pl;                    // pl.pairs oriented
    std::vector<uint8_t> swapped;   // [P]
    std::vector<int64_t> part_off;  // [P + 1] into the parts, in the order of pl.pairs
    int cls_parts[kPairClasses] = {};  // the largest number of parts of a pair of the class
    double c2 = 0.0;
};

inline int64_t pf_parts(int64_t n1, int64_t n2) { return (2 * (n1 + n2) + kPfLanes - 1) / kPfLanes; }

inline int pf_plan(const tda_pf_args* a, PfPlan& fp, std::string& msg) {
    auto bad = [&](int code, const char* m) { return msg = m, code; };
    if (int rc = dgm_check_head(a, msg)) return rc;
    if (a->reserved != 0) return bad(TDA_E_INVALID, "reserved must be 0");
    if (!std::isfinite(a->sigma) || !(a->sigma > 0.0)) return bad(TDA_E_INVALID, "sigma must be finite and > 0");
    const double s2 = a->sigma * a->sigma;  // rounded; 2 s2 is exact (or overflows: c2 = 0, refused below)
    fp.c2 = 1.0 / (2.0 * s2);
    if (!std::isnormal(fp.c2)) return bad(TDA_E_INVALID, "sigma: 1 / (2 sigma^2) must be a finite normal number");
    PairPlan& pl = fp.pl;
    if (int rc = dgm_pairs(a, "persistence Fisher", 1, "persistence Fisher: more than 2^27 pairs in one call is not supported (split the pairs)", pl, msg))
        return rc;
    for (int64_t q = 0; q < 2 * pl.P; ++q) {  // only a diagram that a pair names is measured
        const int32_t s = pl.pairs[q];
        if (pl.off[s + 1] - pl.off[s] > TDA_PF_MAX_POINTS)
            return bad(TDA_E_UNSUPPORTED, "persistence Fisher: a diagram with more than 1024 finite points is not supported");
    }
    if (int rc = dgm_classify(pl, PairSize::kSum, kPfClassM, "persistence Fisher: a diagram with more than 1024 finite points is not supported", msg))
        return rc;
    dgm_orient(pl, fp.swapped);
    fp.part_off.assign((size_t)pl.P + 1, 0);
    for (int64_t w = 0; w < pl.P; ++w) {
        const int32_t i = pl.pairs[2 * w], j = pl.pairs[2 * w + 1];
        const int64_t n1 = pl.off[i + 1] - pl.off[i], n2 = pl.off[j + 1] - pl.off[j];
        const int64_t parts = pf_parts(n1, n2);
        fp.part_off[w + 1] = fp.part_off[w] + parts;
        int c = 0;
        while (n1 + n2 > kPfClassM[c]) ++c;
        fp.cls_parts[c] = std::max(fp.cls_parts[c], (int)parts);
    }
    if (fp.part_off[pl.P] > TDA_SW_MAX_WORK)
        return bad(TDA_E_UNSUPPORTED, "persistence Fisher: more than 2^27 parts of 64 evaluation points in one call is not supported (split the pairs)");
    return 0;
}

// ---------------------------------------------------------------- the vectorisations (tda_landscape, tda_persistence_image)
// One plan per call, per diagram and not per pair: the finite points, the diagrams sorted into size
// classes by their number n of finite points, and for the image the points as (birth, persistence)
// with their weights.

constexpr int kVecClasses = 4;
constexpr int kVecClassN[kVecClasses] = {64, 256, 1024, TDA_VEC_MAX_POINTS};  // n at most

struct VecPlan {
    std::vector<double> pts;     // (total finite, 2): (b, d); after pi_weights (b, pi)
    std::vector<double> wgt;     // [total finite] the image's weights (pi_weights)
    std::vector<int64_t> off;    // [S + 1] into pts
    std::vector<int32_t> order;  // [S]: diagram ids, class 0 first, ascending within a class
    int64_t cls_cnt[kVecClasses] = {};
    int cls_n[kVecClasses] = {};  // the largest n of the class
    int64_t S = 0;
};

// the layout checks of a per-diagram entry; `what` names the entry in the messages
inline int vec_check(const double* points, const int64_t* offsets, int64_t S, const char* what, std::string& msg) {
    if (S < 0) return msg = "S must be >= 0", TDA_E_INVALID;
    if (!offsets) return msg = "offsets is NULL", TDA_E_INVALID;
    return dgm_check_layout(points, offsets, S, nullptr, 0, what, msg);
}

// the gathered diagrams (pl.off) sorted into the size classes
inline int vec_classify(const char* what, VecPlan& pl, std::string& msg) {
    if (!dgm_sort_classes(pl.S, [&](int64_t s) { return pl.off[s + 1] - pl.off[s]; }, kVecClassN, pl.order, pl.cls_cnt, pl.cls_n))
        return msg = std::string(what) + ": a diagram with more than 4096 finite points is not supported", TDA_E_UNSUPPORTED;
    return 0;
}

// the layout checks, the finite points and the classes
inline int vec_gather(const double* points, const int64_t* offsets, int64_t S, const char* what, VecPlan& pl, std::string& msg) {
    if (int rc = vec_check(points, offsets, S, what, msg)) return rc;
    pl.S = S;
    dgm_gather_points(points, offsets, S, pl.pts, pl.off);
    return vec_classify(what, pl, msg);
}

inline int pl_plan(const tda_pl_args* a, VecPlan& pl, std::string& msg) {
    auto bad = [&](int code, const char* m) { return msg = m, code; };
    if (!a) return bad(TDA_E_INVALID, "args is NULL");
    if (a->reserved != 0) return bad(TDA_E_INVALID, "reserved must be 0");
    if (a->K < 1) return bad(TDA_E_INVALID, "K must be >= 1");
    if (a->G < 1) return bad(TDA_E_INVALID, "G must be >= 1");
    if (!a->grid) return bad(TDA_E_INVALID, "grid is NULL");
    if (a->K > TDA_PL_MAX_DEPTH) return bad(TDA_E_UNSUPPORTED, "landscape: K > 64 is not supported");
    if (a->G > TDA_PL_MAX_STEPS) return bad(TDA_E_UNSUPPORTED, "landscape: G > 4096 grid values is not supported");
    for (int32_t g = 0; g < a->G; ++g)
        if (!std::isfinite(a->grid[g])) return bad(TDA_E_INVALID, "grid holds a non-finite value");
    if (int rc = vec_gather(a->points, a->offsets, a->S, "landscape", pl, msg)) return rc;
    if (a->S * ((int64_t)a->K * a->G) > TDA_VEC_MAX_OUT)
        return bad(TDA_E_UNSUPPORTED, "landscape: S * K * G > 2^24 values in one call is not supported (split the diagrams)");
    return 0;
}

// (b, d) -> (b, pi = d - b) in place, and the weights: pi^power for pi > 0 (1 for power 0, pi for power 1), else 0
inline void pi_weights(VecPlan& pl, double power) {
    const size_t n = pl.pts.size() / 2;
    pl.wgt.resize(n);
    for (size_t p = 0; p < n; ++p) {
        const double pi = pl.pts[2 * p + 1] - pl.pts[2 * p];
        pl.pts[2 * p + 1] = pi;
        pl.wgt[p] = !(pi > 0.0) ? 0.0 : power == 0.0 ? 1.0 : power == 1.0 ? pi : std::pow(pi, power);
    }
}

inline int pi_plan(const tda_pi_args* a, VecPlan& pl, std::string& msg) {
    auto bad = [&](int code, const char* m) { return msg = m, code; };
    if (!a) return bad(TDA_E_INVALID, "args is NULL");
    if (a->reserved != 0) return bad(TDA_E_INVALID, "reserved must be 0");
    if (a->W < 1 || a->H < 1) return bad(TDA_E_INVALID, "W and H must be >= 1");
    if (!a->x_edges || !a->y_edges) return bad(TDA_E_INVALID, "x_edges or y_edges is NULL");
    if (!std::isfinite(a->sigma) || !(a->sigma > 0.0)) return bad(TDA_E_INVALID, "sigma must be finite and > 0");
    if (!std::isfinite(a->weight_power) || a->weight_power < 0.0) return bad(TDA_E_INVALID, "weight_power must be finite and >= 0");
    if (a->W > TDA_PI_MAX_PIXELS || a->H > TDA_PI_MAX_PIXELS)
        return bad(TDA_E_UNSUPPORTED, "persistence image: more than 256 pixels per axis is not supported");
    for (int axis = 0; axis < 2; ++axis) {
        const double* e = axis ? a->y_edges : a->x_edges;
        const int32_t n = axis ? a->H : a->W;
        for (int32_t i = 0; i <= n; ++i)
            if (!std::isfinite(e[i])) return bad(TDA_E_INVALID, "the edges hold a non-finite value");
        for (int32_t i = 0; i < n; ++i)
            if (!(e[i] < e[i + 1])) return bad(TDA_E_INVALID, "the edges must be strictly increasing");
    }
    if (int rc = vec_gather(a->points, a->offsets, a->S, "persistence image", pl, msg)) return rc;
    if (a->S * ((int64_t)a->W * a->H) > TDA_VEC_MAX_OUT)
        return bad(TDA_E_UNSUPPORTED, "persistence image: S * W * H > 2^24 values in one call is not supported (split the diagrams)");
    pi_weights(pl, a->weight_power);
    return 0;
}

// ---------------------------------------------------------------- persistence curves (tda_persistence_curve)
// A VecPlan whose rows are the kept rows (with TDA_PC_KEEP_ESSENTIAL also those with d = +inf), wgt
// their coefficients (empty for coef == NULL), and W the divisor of every diagram.  The launches
// (pc_host.h): class 0 of the plan (n <= kPcPackN) packed, one diagram per wave; the classes
// above it together, one diagram per workgroup with its rows in chunks of kPcChunk.

constexpr int kPcPackN = kVecClassN[0];  // a packed diagram's rows at most: one row per lane when staged
constexpr int kPcChunk = 1024;           // rows of a chunked workgroup's LDS

struct PcPlan {
    VecPlan v;
    std::vector<double> W;  // [S]: the row-order sum of the kept coefficients, or the number of kept rows
};

inline int pc_plan(const tda_pc_args* a, PcPlan& pp, std::string& msg) {
    auto bad = [&](int code, const char* m) { return msg = m, code; };
    if (!a) return bad(TDA_E_INVALID, "args is NULL");
    if (a->reserved != 0) return bad(TDA_E_INVALID, "reserved must be 0");
    if (a->kernel != TDA_PC_INDICATOR && a->kernel != TDA_PC_TENT) return bad(TDA_E_INVALID, "kernel must be TDA_PC_INDICATOR or TDA_PC_TENT");
    if (a->flags & ~(TDA_PC_NORMALIZE | TDA_PC_KEEP_ESSENTIAL)) return bad(TDA_E_INVALID, "flags holds an unknown bit");
    const bool essential = a->flags & TDA_PC_KEEP_ESSENTIAL;
    if (essential && a->kernel == TDA_PC_TENT) return bad(TDA_E_INVALID, "TDA_PC_KEEP_ESSENTIAL needs the indicator kernel: a tent has no value on an essential row");
    if (a->G < 1) return bad(TDA_E_INVALID, "G must be >= 1");
    if (!a->grid) return bad(TDA_E_INVALID, "grid is NULL");
    if (a->G > TDA_PL_MAX_STEPS) return bad(TDA_E_UNSUPPORTED, "persistence curve: G > 4096 grid values is not supported");
    for (int32_t g = 0; g < a->G; ++g)
        if (!std::isfinite(a->grid[g])) return bad(TDA_E_INVALID, "grid holds a non-finite value");
    if (int rc = vec_check(a->points, a->offsets, a->S, "persistence curve", msg)) return rc;
    VecPlan& pl = pp.v;
    pl.S = a->S;
    pl.off.assign((size_t)a->S + 1, 0);
    pp.W.assign((size_t)a->S, 0.0);
    for (int64_t s = 0; s < a->S; ++s) {
        double w = 0.0;
        for (int64_t r = a->offsets[s]; r < a->offsets[s + 1]; ++r) {
            const double b = a->points[2 * r], d = a->points[2 * r + 1];
            if (!std::isfinite(b) || !(std::isfinite(d) || (essential && d > 0.0 && std::isinf(d)))) continue;
            pl.pts.push_back(b);
            pl.pts.push_back(d);
            if (a->coef) {
                if (!std::isfinite(a->coef[r])) return bad(TDA_E_INVALID, "coef holds a non-finite value on a kept row");
                pl.wgt.push_back(a->coef[r]);
                w = w + a->coef[r];
            }
        }
        pl.off[s + 1] = (int64_t)(pl.pts.size() / 2);
        pp.W[s] = a->coef ? w : (double)(pl.off[s + 1] - pl.off[s]);
    }
    if (int rc = vec_classify("persistence curve", pl, msg)) return rc;
    if (a->S * (int64_t)a->G > TDA_VEC_MAX_OUT)
        return bad(TDA_E_UNSUPPORTED, "persistence curve: S * G > 2^24 values in one call is not supported (split the diagrams)");
    return 0;
}

}  // namespace tda
