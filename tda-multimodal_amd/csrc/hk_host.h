// hk_host.h -- host side of tda_heat_kernel (include/tda_dgm.h), part of rips.hip's
// translation unit (shares its error state and device checks; the plan is dgm_plan.h's
// HkPlan, the upload's layout dgm_host.h's, the workspace aux_ws.h's).
//
// One call, the shape of the distance entries: drop the non-finite points on the host, add
// the S self pairs to the P pairs, orient every evaluation canonically and sort them into
// size classes, upload everything in one copy, launch k_hk_parts once per non-empty class
// and k_hk_sum once (each in slices of 2^24 evaluations, the launch's grid limit), copy the P + S kernel values back in one copy, and form the distances
// on the host.
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
    if (W == 0) {  // no diagram: nothing to launch
        R->pub.kern = R->pub.self = R->kern.data();
        R->pub.dist = R->dist.data();
        *out = &R.release()->pub;
        return 0;
    }

    Carve cv;
    const PlanAt at(pl, cv);
    const size_t o_poff = cv.take(hp.part_off.size() * 8);
    const size_t up_bytes = cv.o;  // the uploaded part
    const size_t o_part = cv.take((size_t)hp.part_off[W] * 8), o_kern = cv.take(W * 8);
    std::vector<char> up(up_bytes);
    at.pack(pl, up.data());
    std::memcpy(up.data() + o_poff, hp.part_off.data(), hp.part_off.size() * 8);

    AuxWs& w = aux_ws(kAuxHk, a->device);
    std::lock_guard<std::mutex> guard(w.mu);
    if (int rc = aux_open(w, 2)) return rc;
    if (int rc = aux_reserve(w, cv.o)) return rc;
    hipStream_t s = w.stream;
    const int64_t* poff = (const int64_t*)(w.buf + o_poff);
    double* part = (double*)(w.buf + o_part);
    double* kern = (double*)(w.buf + o_kern);
    HIPC(hipEventRecord(w.ev[0], s));
    HIPC(hipMemcpyAsync(w.buf, up.data(), up_bytes, hipMemcpyHostToDevice, s));
    // a launch's grid x times its block size has to stay below 2^32 threads: at most kHkGridX evaluations per launch
    int64_t first = 0;
    for (int c = 0; c < kPairClasses; ++c) {
        const int64_t cnt = pl.cls_cnt[c];
        if (hp.cls_parts[c])  // a class of empty evaluations has nothing to add up
            for (int64_t at0 = 0; at0 < cnt; at0 += kHkGridX) {
                hipLaunchKernelGGL(k_hk_parts, dim3((unsigned)std::min(cnt - at0, kHkGridX), (unsigned)hp.cls_parts[c]), dim3(kHkRows), 0, s,
                                   (const double*)(w.buf + at.pts), (const int64_t*)(w.buf + at.off), (const int32_t*)(w.buf + at.pairs),
                                   (const int32_t*)(w.buf + at.order) + first + at0, poff, -hp.c8, part);
                HIPC(hipGetLastError());
            }
        first += cnt;
    }
    constexpr int64_t per_block = kHkSumThreads / 64;
    for (int64_t w0 = 0; w0 < (int64_t)W; w0 += kHkGridX) {
        const int64_t n = std::min((int64_t)W - w0, kHkGridX);
        hipLaunchKernelGGL(k_hk_sum, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(kHkSumThreads), 0, s, (const double*)part, poff, w0,
                           w0 + n, hp.cn, kern);
        HIPC(hipGetLastError());
    }
    HIPC(hipMemcpyAsync(R->kern.data(), kern, W * 8, hipMemcpyDeviceToHost, s));
    HIPC(hipEventRecord(w.ev[1], s));
    HIPC(hipStreamSynchronize(s));
    float ms = 0.0f;
    HIPC(hipEventElapsedTime(&ms, w.ev[0], w.ev[1]));
    const double* self = R->kern.data() + P;
    for (size_t p = 0; p < P; ++p) {  // the header's order of operations; the sum of the two selfs is commutative
        const double q = (self[pl.pairs[2 * p]] + self[pl.pairs[2 * p + 1]]) - 2.0 * R->kern[p];
        R->dist[p] = q > 0.0 ? std::sqrt(q) : 0.0;
    }
    R->pub.kern = R->kern.data();
    R->pub.self = self;
    R->pub.dist = R->dist.data();
    R->pub.device_ms = ms;
    *out = &R.release()->pub;
    return 0;
}

extern "C" void tda_hk_free(tda_hk_result* r) {
    delete reinterpret_cast<HkResultImpl*>(r);  // pub is the first member; NULL is a no-op
}
