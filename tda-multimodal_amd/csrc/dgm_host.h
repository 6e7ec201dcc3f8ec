// dgm_host.h -- host side of tda_sliced_wasserstein (include/tda_dgm.h), part of
// rips.hip's translation unit (shares its error state and device checks).
//
// One call: drop the non-finite points on the host, sort the pairs into three
// size classes, upload everything in one copy, launch k_sw_pairs once per
// non-empty class and k_sw_sum once, copy the P distances back (the plan and
// the classes' numbers: dgm_plan.h; the frame of the call: dgm_call.h).
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
#include "dgm_call.h"
#include "dgm_kernels.h"

namespace {

static_assert(kSwMaxN == TDA_SW_MAX_POINTS && kSwMaxM == TDA_SW_MAX_DIRECTIONS, "tda_dgm.h and dgm_kernels.h disagree");
static_assert(kSwClasses[kPairClasses - 1].npow_max == kSwMaxN, "dgm_plan.h and dgm_kernels.h disagree");

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

}  // namespace

extern "C" int tda_sliced_wasserstein(const tda_sw_args* a, tda_sw_result** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    PairPlan pl;
    std::string msg;
    if (int rc = sw_plan(a, pl, msg)) return fail(rc, msg);
    if (!tda_device_ok(a->device)) return fail(TDA_E_NODEVICE, "no gfx950 device at ordinal " + std::to_string(a->device));
    const size_t P = (size_t)pl.P, M = (size_t)a->M;
    std::unique_ptr<DgmResultImpl<tda_sw_result>> R(new DgmResultImpl<tda_sw_result>(pl.P));
    if (P == 0) return dgm_return(R, out);  // nothing to launch

    // the direction table, computed here once so that host and device use the same directions
    std::vector<double> dirs(2 * M);
    const double pi = 3.14159265358979323846, step = pi / (double)a->M;
    for (size_t i = 0; i < M; ++i) {
        const double th = -pi / 2 + (double)i * step;
        dirs[2 * i] = std::cos(th);
        dirs[2 * i + 1] = std::sin(th);
    }

    DgmCall call;
    const PairAt at(call, pl);
    const size_t o_dirs = call.upload(dirs);
    const size_t o_part = call.device(P * M * 8), o_dist = call.device(P * 8);
    if (int rc = call.begin(kAuxSw, a->device, (const void*)k_sw_pairs, sw_lds_bytes(kSwMaxN, kSwMaxN))) return rc;
    hipStream_t s = call.stream();
    double* part = call.at<double>(o_part);
    int64_t first = 0;
    for (int c = 0; c < kPairClasses; ++c) {
        const int64_t cnt = pl.cls_cnt[c];
        if (!cnt) continue;
        const SwClass& k = kSwClasses[c];
        const int n = pl.cls_n[c];
        const size_t lds = sw_lds_bytes(n, (int)next_pow2((uint64_t)std::max(n, 1)));
        const unsigned chunks = (unsigned)((a->M + k.dirs_per_wg - 1) / k.dirs_per_wg);
        hipLaunchKernelGGL(k_sw_pairs, dim3((unsigned)cnt, chunks), dim3(k.threads), lds, s, call.at<const double>(at.pts),
                           call.at<const int64_t>(at.off), call.at<const int32_t>(at.pairs), call.at<const int32_t>(at.order) + first,
                           call.at<const double>(o_dirs), (int)a->M, k.dirs_per_wg, part);
        HIPC(hipGetLastError());
        first += cnt;
    }
    hipLaunchKernelGGL(k_sw_sum, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, (const double*)part, (int64_t)P, (int)a->M,
                       call.at<double>(o_dist));
    HIPC(hipGetLastError());
    if (int rc = call.end(R->dist.get(), o_dist, P * 8)) return rc;
    return dgm_return(R, out, call.ms);
}

extern "C" void tda_sw_free(tda_sw_result* r) { dgm_free(r); }
