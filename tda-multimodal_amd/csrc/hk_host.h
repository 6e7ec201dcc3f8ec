// hk_host.h -- host side of tda_heat_kernel (include/tda_dgm.h), part of rips.hip's
// translation unit (shares its error state and device checks; the plan is dgm_plan.h's
// HkPlan, the frame of the call dgm_call.h's).
//
// One call, the shape of the distance entries: drop the non-finite points on the host, add
// the S self pairs to the P pairs, orient every evaluation canonically and sort them into
// size classes, upload everything in one copy, launch k_hk_parts once per non-empty class
// and k_hk_sum once (each in slices of 2^24 evaluations, the launch's grid limit), copy the
// P + S kernel values back in one copy, and form the distances on the host.
//
// Size classes (the larger count of an evaluation): <= 64 (one part), <= 512 (at most 16),
// <= 4096 (at most 1024).  A class's grid is (its evaluations, the parts of its largest
// one); a workgroup beyond its evaluation's parts returns after the loads that tell it so.
// A sweep of like-sized diagrams therefore carries few idle workgroups; a class of mixed
// sizes does not (one 4096 x 4096 pair among many 600 x 600 ones gives each of those about
// 1000 idle workgroups): the price of a grid without a per-part lookup table.  The class
// sets nothing else: block size, LDS and the order of the sum are the same everywhere
// (hk_kernels.h).
// The parts (8 bytes each, at most 2^27 per call) live in the workspace buffer.
#pragma once
#include "../../include/tda_dgm.h"
#include "dgm_call.h"
#include "hk_kernels.h"

namespace {

static_assert(kHkMaxN == TDA_HK_MAX_POINTS && kHkClassN[kPairClasses - 1] == kHkMaxN, "tda_dgm.h, dgm_plan.h and hk_kernels.h disagree");

constexpr int64_t kHkGridX = 1ll << 24;  // evaluations per launch: 2^24 workgroups of 64 (k_hk_parts) or 2^22 of 256 (k_hk_sum)

struct HkResultImpl {
    tda_hk_result pub = {};
    std::vector<double> kern, dist;  // kern: [P] and then self [S], as downloaded
};

}  // namespace

extern "C" int tda_heat_kernel(const tda_hk_args* a, tda_hk_result** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    HkPlan hp;
    std::string msg;
    if (int rc = hk_plan(a, hp, msg)) return fail(rc, msg);
    if (!tda_device_ok(a->device)) return fail(TDA_E_NODEVICE, "no gfx950 device at ordinal " + std::to_string(a->device));
    const PairPlan& pl = hp.pl;
    const size_t P = (size_t)hp.P, W = (size_t)pl.P;
    std::unique_ptr<HkResultImpl> R(new HkResultImpl());
    R->kern.assign(std::max<size_t>(W, 1), 0.0);
    R->dist.assign(std::max<size_t>(P, 1), 0.0);
    R->pub.P = hp.P;
    R->pub.kern = R->kern.data();
    R->pub.self = R->kern.data() + P;
    R->pub.dist = R->dist.data();
    if (W == 0) return dgm_return(R, out);  // no diagram: nothing to launch

    DgmCall call;
    const PairAt at(call, pl);
    const size_t o_poff = call.upload(hp.part_off);
    const size_t o_part = call.device((size_t)hp.part_off[W] * 8), o_kern = call.device(W * 8);
    if (int rc = call.begin(kAuxHk, a->device)) return rc;
    hipStream_t s = call.stream();
    const int64_t* poff = call.at<const int64_t>(o_poff);
    double* part = call.at<double>(o_part);
    // a launch's grid x times its block size has to stay below 2^32 threads: at most kHkGridX evaluations per launch
    int64_t first = 0;
    for (int c = 0; c < kPairClasses; ++c) {
        const int64_t cnt = pl.cls_cnt[c];
        if (hp.cls_parts[c])  // a class of empty evaluations has nothing to add up
            for (int64_t at0 = 0; at0 < cnt; at0 += kHkGridX) {
                hipLaunchKernelGGL(k_hk_parts, dim3((unsigned)std::min(cnt - at0, kHkGridX), (unsigned)hp.cls_parts[c]), dim3(kHkRows), 0, s,
                                   call.at<const double>(at.pts), call.at<const int64_t>(at.off), call.at<const int32_t>(at.pairs),
                                   call.at<const int32_t>(at.order) + first + at0, poff, -hp.c8, part);
                HIPC(hipGetLastError());
            }
        first += cnt;
    }
    constexpr int64_t per_block = kHkSumThreads / 64;
    for (int64_t w0 = 0; w0 < (int64_t)W; w0 += kHkGridX) {
        const int64_t n = std::min((int64_t)W - w0, kHkGridX);
        hipLaunchKernelGGL(k_hk_sum, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(kHkSumThreads), 0, s, (const double*)part, poff, w0,
                           w0 + n, hp.cn, call.at<double>(o_kern));
        HIPC(hipGetLastError());
    }
    if (int rc = call.end(R->kern.data(), o_kern, W * 8)) return rc;
    const double* self = R->kern.data() + P;
    for (size_t p = 0; p < P; ++p) {  // the header's order of operations; the sum of the two selfs is commutative
        const double q = (self[pl.pairs[2 * p]] + self[pl.pairs[2 * p + 1]]) - 2.0 * R->kern[p];
        R->dist[p] = q > 0.0 ? std::sqrt(q) : 0.0;
    }
    return dgm_return(R, out, call.ms);
}

extern "C" void tda_hk_free(tda_hk_result* r) {
    delete reinterpret_cast<HkResultImpl*>(r);  // pub is the first member; NULL is a no-op
}
