// bn_host.h -- host side of tda_bottleneck (include/tda_dgm.h), part of rips.hip's
// translation unit (shares its error state and device checks; the plan and the
// classes' limits are dgm_plan.h's, the frame of the call dgm_call.h's, the
// result type dgm_host.h's).
//
// One call, the shape of tda_sliced_wasserstein: drop the non-finite points on
// the host, sort the pairs into size classes, upload everything in one copy,
// launch k_bn_pairs once per non-empty class, copy the P distances back.
//
// Size classes (nm = max(n1, n2) of a pair).  The kernel wants one thread per
// point of the longer diagram (thread y owns row y of the bitmap), so the
// workgroup size follows nm, and the dynamic LDS of a launch is that of the
// class's largest pair, bn_lds_bytes(nm, nm) = 48 nm + 8 nm ceil(nm / 64) + 328:
//   nm <= 64:   64 threads, at most  3.8 KiB: one wave, so the barriers cost
//               nothing, one bitmap word per row, and some 40 workgroups fit a
//               CU's 160 KiB -- the wave slots, not LDS, bound the occupancy.
//               The sweep's H1 diagrams (a few to a few dozen points) live here;
//   nm <= 256:  256 threads, at most 20.3 KiB: 7 workgroups per CU by LDS, 8 by
//               wave slots;
//   nm <= 512:  512 threads, at most 56.3 KiB (the bitmap is 32 KiB of it): 2
//               workgroups per CU, below the 64 KiB a launch gets without
//               asking for more.
// A pair is searched by one workgroup whatever its class, and the value is the
// smallest feasible candidate cost, which no launch shape can change
// (bn_kernels.h).
#pragma once
#include "../../include/tda_dgm.h"
#include "bn_kernels.h"
#include "dgm_call.h"

namespace {

static_assert(kBnMaxN == TDA_BN_MAX_POINTS && kBnClassN[kPairClasses - 1] == kBnMaxN, "tda_dgm.h, dgm_plan.h and bn_kernels.h disagree");
static_assert(bn_lds_bytes(kBnMaxN, kBnMaxN) <= 64 * 1024, "k_bn_pairs would need hipFuncAttributeMaxDynamicSharedMemorySize");

}  // namespace

extern "C" int tda_bottleneck(const tda_bn_args* a, tda_bn_result** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    PairPlan pl;
    std::string msg;
    if (int rc = bn_plan(a, pl, msg)) return fail(rc, msg);
    if (!tda_device_ok(a->device)) return fail(TDA_E_NODEVICE, "no gfx950 device at ordinal " + std::to_string(a->device));
    const size_t P = (size_t)pl.P;
    std::unique_ptr<DgmResultImpl<tda_bn_result>> R(new DgmResultImpl<tda_bn_result>(pl.P));
    if (P == 0) return dgm_return(R, out);  // nothing to launch

    DgmCall call;
    const PairAt at(call, pl);
    const size_t o_dist = call.device(P * 8);
    if (int rc = call.begin(kAuxBn, a->device)) return rc;
    int64_t first = 0;
    for (int c = 0; c < kPairClasses; ++c) {
        const int64_t cnt = pl.cls_cnt[c];
        if (!cnt) continue;
        hipLaunchKernelGGL(k_bn_pairs, dim3((unsigned)cnt), dim3(kBnClassN[c]), bn_lds_bytes(pl.cls_n[c], pl.cls_n[c]), call.stream(),
                           call.at<const double>(at.pts), call.at<const int64_t>(at.off), call.at<const int32_t>(at.pairs),
                           call.at<const int32_t>(at.order) + first, call.at<double>(o_dist));
        HIPC(hipGetLastError());
        first += cnt;
    }
    if (int rc = call.end(R->dist.get(), o_dist, P * 8)) return rc;
    // no cost is a NaN (the coordinates are finite), so a NaN is the kernel's word for "a loop bound was hit"
    for (size_t p = 0; p < P; ++p)
        if (std::isnan(R->dist[p]))
            return fail(TDA_E_CAPACITY, "bottleneck: the matching of pair " + std::to_string(p) + " ran into a loop bound (internal error)");
    return dgm_return(R, out, call.ms);
}

extern "C" void tda_bn_free(tda_bn_result* r) { dgm_free(r); }
