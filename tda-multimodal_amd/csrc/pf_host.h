// pf_host.h -- host side of tda_persistence_fisher (include/tda_dgm.h), part of rips.hip's
// translation unit (shares its error state and device checks; the plan is dgm_plan.h's
// PfPlan, the frame of the call dgm_call.h's).
//
// One call, the shape of tda_heat_kernel's without the selfs: drop the non-finite points on the
// host, orient every pair canonically and sort the pairs into size classes, upload everything in
// one copy, launch k_pf_parts once per non-empty class and k_pf_sum once (each in slices of 2^24
// pairs, the launch's grid limit), copy the three sums of every pair back in one copy, and form
// the distances on the host.
//
// Size classes (n1 + n2 of a pair): <= 64 (at most 2 parts), <= 512 (at most 16), <= 2048 (at
// most 64).  A class's grid is (its pairs, the parts of its largest one); a workgroup beyond its
// pair's parts returns after the loads that tell it so.  The class sets nothing else: block
// size, LDS and the order of the sums are the same everywhere (pf_kernels.h).
// The parts (24 bytes each, at most 2^27 per call) live in the workspace buffer.
#pragma once
#include "../../include/tda_dgm.h"
#include "dgm_call.h"
#include "pf_kernels.h"

namespace {

static_assert(kPfMaxN == TDA_PF_MAX_POINTS && kPfClassM[kPairClasses - 1] == 2 * kPfMaxN, "tda_dgm.h, dgm_plan.h and pf_kernels.h disagree");

constexpr int64_t kPfGridX = 1ll << 24;  // pairs per launch: 2^24 workgroups of 64 (k_pf_parts) or 2^22 of 256 (k_pf_sum)

struct PfResultImpl {
    tda_pf_result pub = {};
    std::vector<double> sums;  // [P][3] as downloaded: a, b, h of the oriented pair
    std::vector<double> a, b, h, dist;
};

}  // namespace

extern "C" int tda_persistence_fisher(const tda_pf_args* a, tda_pf_result** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    PfPlan fp;
    std::string msg;
    if (int rc = pf_plan(a, fp, msg)) return fail(rc, msg);
    if (!tda_device_ok(a->device)) return fail(TDA_E_NODEVICE, "no gfx950 device at ordinal " + std::to_string(a->device));
    const PairPlan& pl = fp.pl;
    const size_t P = (size_t)pl.P;
    std::unique_ptr<PfResultImpl> R(new PfResultImpl());
    R->sums.assign(3 * std::max<size_t>(P, 1), 0.0);
    for (std::vector<double>* v : {&R->a, &R->b, &R->h, &R->dist}) v->assign(std::max<size_t>(P, 1), 0.0);
    R->pub.P = pl.P;
    R->pub.a = R->a.data();
    R->pub.b = R->b.data();
    R->pub.h = R->h.data();
    R->pub.dist = R->dist.data();
    if (P == 0) return dgm_return(R, out);  // no pair: nothing to launch

    DgmCall call;
    const PairAt at(call, pl);
    const size_t o_poff = call.upload(fp.part_off);
    const size_t o_part = call.device((size_t)fp.part_off[P] * 24), o_sums = call.device(P * 24);
    if (int rc = call.begin(kAuxPf, a->device)) return rc;
    hipStream_t s = call.stream();
    const int64_t* poff = call.at<const int64_t>(o_poff);
    double* part = call.at<double>(o_part);
    // a launch's grid x times its block size has to stay below 2^32 threads: at most kPfGridX pairs per launch
    int64_t first = 0;
    for (int c = 0; c < kPairClasses; ++c) {
        const int64_t cnt = pl.cls_cnt[c];
        if (fp.cls_parts[c])  // a class of pairs of two empty diagrams has nothing to add up
            for (int64_t at0 = 0; at0 < cnt; at0 += kPfGridX) {
                hipLaunchKernelGGL(k_pf_parts, dim3((unsigned)std::min(cnt - at0, kPfGridX), (unsigned)fp.cls_parts[c]), dim3(kPfLanes), 0, s,
                                   call.at<const double>(at.pts), call.at<const int64_t>(at.off), call.at<const int32_t>(at.pairs),
                                   call.at<const int32_t>(at.order) + first + at0, poff, -fp.c2, part);
                HIPC(hipGetLastError());
            }
        first += cnt;
    }
    constexpr int64_t per_block = kPfSumThreads / 64;
    for (int64_t w0 = 0; w0 < (int64_t)P; w0 += kPfGridX) {
        const int64_t n = std::min((int64_t)P - w0, kPfGridX);
        hipLaunchKernelGGL(k_pf_sum, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(kPfSumThreads), 0, s, (const double*)part, poff, w0,
                           w0 + n, call.at<double>(o_sums));
        HIPC(hipGetLastError());
    }
    if (int rc = call.end(R->sums.data(), o_sums, P * 24)) return rc;
    for (size_t p = 0; p < P; ++p) {  // the header's order of operations
        const double sa = R->sums[3 * p], sb = R->sums[3 * p + 1], sh = R->sums[3 * p + 2];
        R->a[p] = fp.swapped[p] ? sb : sa;  // back to the diagrams as the caller named them
        R->b[p] = fp.swapped[p] ? sa : sb;
        R->h[p] = sh;
        if (sa > 0.0) {  // else two empty diagrams: +0.0
            const double q = sh / std::sqrt(sa * sb);
            R->dist[p] = std::acos(q < 1.0 ? q : 1.0);
        }
    }
    return dgm_return(R, out, call.ms);
}

extern "C" void tda_persistence_fisher_free(tda_pf_result* r) {
    delete reinterpret_cast<PfResultImpl*>(r);  // pub is the first member; NULL is a no-op
}
