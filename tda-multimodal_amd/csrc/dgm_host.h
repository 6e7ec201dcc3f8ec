// dgm_host.h -- host side of tda_sliced_wasserstein (include/tda_dgm.h), part of
// rips.hip's translation unit (shares its error state and device checks).
//
// One call: drop the non-finite points on the host, sort the pairs into three
// size classes, upload everything in one copy, launch k_sw_pairs once per
// non-empty class and k_sw_sum once, copy the P distances back (the plan:
// dgm_plan.h; the workspace: aux_ws.h).
//
// Size classes (npow = next_pow2(n1 + n2) of a pair): a launch has one
// workgroup size and one dynamic-LDS size, and both should fit the pair.
//   npow <= 128:   64 threads (one wave: the barriers cost nothing), 8
//                  directions per workgroup -- a direction is a few hundred
//                  compare-exchanges, so the copy of the points into LDS and
//                  the workgroup's dispatch are shared among 8 of them;
//   npow <= 1024:  256 threads, 1 direction per workgroup;
//   npow <= 4096:  1024 threads, 1 direction per workgroup.
// From 256 points on a direction's sort moves a hundred times the bytes of the
// point copy through LDS, so one direction per workgroup costs nothing and
// gives a single large pair M workgroups to spread over the CUs.  The class
// only sets the launch shape: the values do not depend on it (dgm_kernels.h).
#pragma once
#include "../../include/tda_dgm.h"
#include "dgm_kernels.h"
#include "dgm_plan.h"

namespace {

static_assert(kSwMaxN == TDA_SW_MAX_POINTS && kSwMaxM == TDA_SW_MAX_DIRECTIONS, "tda_dgm.h and dgm_kernels.h disagree");

struct SwClass {
    int npow_max, threads, dirs_per_wg;
};
constexpr SwClass kSwClasses[3] = {{128, 64, 8}, {1024, 256, 1}, {kSwMaxN, 1024, 1}};

// one result type for both distances: the public structs have the same layout but are distinct types
template <typename Pub>
struct DgmResultImpl {
    Pub pub = {};
    std::unique_ptr<double[]> dist;
    explicit DgmResultImpl(int64_t P) : dist(new double[std::max<int64_t>(P, 1)]) {
        pub.P = P;
        pub.dist = dist.get();
    }
};
template <typename Pub>
void dgm_free(Pub* r) {
    delete reinterpret_cast<DgmResultImpl<Pub>*>(r);  // pub is the first member; NULL is a no-op
}

// the plan's four arrays at the head of a call's buffer (carved first, in this order), packed for one upload
struct PlanAt {
    size_t pts, off, pairs, order;
    PlanAt(const PairPlan& pl, Carve& cv)
        : pts(cv.take(pl.pts.size() * 8)), off(cv.take(pl.off.size() * 8)), pairs(cv.take(pl.pairs.size() * 4)),
          order(cv.take(pl.order.size() * 4)) {}
    void pack(const PairPlan& pl, char* up) const {
        if (!pl.pts.empty()) std::memcpy(up + pts, pl.pts.data(), pl.pts.size() * 8);
        std::memcpy(up + off, pl.off.data(), pl.off.size() * 8);
        std::memcpy(up + pairs, pl.pairs.data(), pl.pairs.size() * 4);
        std::memcpy(up + order, pl.order.data(), pl.order.size() * 4);
    }
};

int sw_plan(const tda_sw_args* a, PairPlan& pl) {
    if (!a) return fail(TDA_E_INVALID, "args is NULL");
    if (a->S < 0) return fail(TDA_E_INVALID, "S must be >= 0");
    if (!a->offsets) return fail(TDA_E_INVALID, "offsets is NULL");
    if (a->M < 1) return fail(TDA_E_INVALID, "M must be >= 1");
    if (a->M > kSwMaxM) return fail(TDA_E_UNSUPPORTED, "sliced Wasserstein: M > 1024 directions is not supported");
    std::string msg;
    if (int rc = dgm_check_layout(a->points, a->offsets, a->S, a->pairs, a->P, "sliced Wasserstein", msg)) return fail(rc, msg);
    const int64_t P = a->pairs ? a->P : a->S * (a->S - 1) / 2;
    if (P > TDA_SW_MAX_WORK || P * a->M > TDA_SW_MAX_WORK) return fail(TDA_E_UNSUPPORTED, "sliced Wasserstein: P * M > 2^27 in one call is not supported (split the pairs)");
    if (int rc = dgm_gather(a->points, a->offsets, a->S, a->pairs, P, pl, msg)) return fail(rc, msg);
    const int limits[kPairClasses] = {kSwClasses[0].npow_max, kSwClasses[1].npow_max, kSwClasses[2].npow_max};
    if (int rc = dgm_classify(pl, PairSize::kSum, limits,
                              "sliced Wasserstein: a pair of diagrams with more than 4096 finite points together is not supported", msg))
        return fail(rc, msg);
    return 0;
}

}  // namespace

extern "C" int tda_sliced_wasserstein(const tda_sw_args* a, tda_sw_result** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    PairPlan pl;
    if (int rc = sw_plan(a, pl)) return rc;
    if (!tda_device_ok(a->device)) return fail(TDA_E_NODEVICE, "no gfx950 device at ordinal " + std::to_string(a->device));
    const size_t P = (size_t)pl.P, M = (size_t)a->M;
    std::unique_ptr<DgmResultImpl<tda_sw_result>> R(new DgmResultImpl<tda_sw_result>(pl.P));
    if (P == 0) {  // nothing to launch
        *out = &R.release()->pub;
        return 0;
    }

    // the direction table, computed here once so that host and device use the same directions
    std::vector<double> dirs(2 * M);
    const double pi = 3.14159265358979323846, step = pi / (double)a->M;
    for (size_t i = 0; i < M; ++i) {
        const double th = -pi / 2 + (double)i * step;
        dirs[2 * i] = std::cos(th);
        dirs[2 * i + 1] = std::sin(th);
    }

    Carve cv;
    const PlanAt at(pl, cv);
    const size_t o_dirs = cv.take(dirs.size() * 8);
    const size_t up_bytes = cv.o;  // the uploaded part
    const size_t o_part = cv.take(P * M * 8), o_dist = cv.take(P * 8);
    std::vector<char> up(up_bytes);
    at.pack(pl, up.data());
    std::memcpy(up.data() + o_dirs, dirs.data(), dirs.size() * 8);

    AuxWs& w = aux_ws(kAuxSw, a->device);
    std::lock_guard<std::mutex> guard(w.mu);
    if (int rc = aux_open(w, 2)) return rc;
    if (int rc = aux_lds_attr(w, (const void*)k_sw_pairs, sw_lds_bytes(kSwMaxN, kSwMaxN))) return rc;
    if (int rc = aux_reserve(w, cv.o)) return rc;
    hipStream_t s = w.stream;
    double* part = (double*)(w.buf + o_part);
    double* dist = (double*)(w.buf + o_dist);
    HIPC(hipEventRecord(w.ev[0], s));
    HIPC(hipMemcpyAsync(w.buf, up.data(), up_bytes, hipMemcpyHostToDevice, s));
    int64_t first = 0;
    for (int c = 0; c < kPairClasses; ++c) {
        const int64_t cnt = pl.cls_cnt[c];
        if (!cnt) continue;
        const SwClass& k = kSwClasses[c];
        const int n = pl.cls_n[c];
        const size_t lds = sw_lds_bytes(n, (int)next_pow2((uint64_t)std::max(n, 1)));
        const unsigned chunks = (unsigned)((a->M + k.dirs_per_wg - 1) / k.dirs_per_wg);
        hipLaunchKernelGGL(k_sw_pairs, dim3((unsigned)cnt, chunks), dim3(k.threads), lds, s, (const double*)(w.buf + at.pts),
                           (const int64_t*)(w.buf + at.off), (const int32_t*)(w.buf + at.pairs),
                           (const int32_t*)(w.buf + at.order) + first, (const double*)(w.buf + o_dirs), (int)a->M, k.dirs_per_wg, part);
        HIPC(hipGetLastError());
        first += cnt;
    }
    hipLaunchKernelGGL(k_sw_sum, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, (const double*)part, (int64_t)P, (int)a->M, dist);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(R->dist.get(), dist, P * 8, hipMemcpyDeviceToHost, s));
    HIPC(hipEventRecord(w.ev[1], s));
    HIPC(hipStreamSynchronize(s));
    float ms = 0.0f;
    HIPC(hipEventElapsedTime(&ms, w.ev[0], w.ev[1]));
    R->pub.device_ms = ms;
    *out = &R.release()->pub;
    return 0;
}

extern "C" void tda_sw_free(tda_sw_result* r) { dgm_free(r); }
