// bn_host.h -- host side of tda_bottleneck (include/tda_dgm.h), part of rips.hip's
// translation unit (shares its error state and device checks; the plan is
// dgm_plan.h's, the result type and the upload's layout dgm_host.h's).
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

namespace {

static_assert(kBnMaxN == TDA_BN_MAX_POINTS, "tda_dgm.h and bn_kernels.h disagree");

constexpr int kBnClassN[kPairClasses] = {64, 256, kBnMaxN};  // nm at most; also the workgroup size
static_assert(bn_lds_bytes(kBnMaxN, kBnMaxN) <= 64 * 1024, "k_bn_pairs would need hipFuncAttributeMaxDynamicSharedMemorySize");

int bn_plan(const tda_bn_args* a, PairPlan& pl) {
    if (!a) return fail(TDA_E_INVALID, "args is NULL");
    if (a->S < 0) return fail(TDA_E_INVALID, "S must be >= 0");
    if (!a->offsets) return fail(TDA_E_INVALID, "offsets is NULL");
    if (a->reserved != 0) return fail(TDA_E_INVALID, "reserved must be 0");
    std::string msg;
    if (int rc = dgm_check_layout(a->points, a->offsets, a->S, a->pairs, a->P, "bottleneck", msg)) return fail(rc, msg);
    const int64_t P = a->pairs ? a->P : a->S * (a->S - 1) / 2;
    if (P > TDA_SW_MAX_WORK) return fail(TDA_E_UNSUPPORTED, "bottleneck: more than 2^27 pairs in one call is not supported (split the pairs)");
    if (int rc = dgm_gather(a->points, a->offsets, a->S, a->pairs, P, pl, msg)) return fail(rc, msg);
    if (int rc = dgm_classify(pl, PairSize::kMax, kBnClassN, "bottleneck: a diagram with more than 512 finite points is not supported", msg))
        return fail(rc, msg);
    return 0;
}

}  // namespace

extern "C" int tda_bottleneck(const tda_bn_args* a, tda_bn_result** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    PairPlan pl;
    if (int rc = bn_plan(a, pl)) return rc;
    if (!tda_device_ok(a->device)) return fail(TDA_E_NODEVICE, "no gfx950 device at ordinal " + std::to_string(a->device));
    const size_t P = (size_t)pl.P;
    std::unique_ptr<DgmResultImpl<tda_bn_result>> R(new DgmResultImpl<tda_bn_result>(pl.P));
    if (P == 0) {  // nothing to launch
        *out = &R.release()->pub;
        return 0;
    }

    Carve cv;
    const PlanAt at(pl, cv);
    const size_t up_bytes = cv.o;  // the uploaded part
    const size_t o_dist = cv.take(P * 8);
    std::vector<char> up(up_bytes);
    at.pack(pl, up.data());

    AuxWs& w = aux_ws(kAuxBn, a->device);
    std::lock_guard<std::mutex> guard(w.mu);
    if (int rc = aux_open(w, 2)) return rc;
    if (int rc = aux_reserve(w, cv.o)) return rc;
    hipStream_t s = w.stream;
    double* dist = (double*)(w.buf + o_dist);
    HIPC(hipEventRecord(w.ev[0], s));
    HIPC(hipMemcpyAsync(w.buf, up.data(), up_bytes, hipMemcpyHostToDevice, s));
    int64_t first = 0;
    for (int c = 0; c < kPairClasses; ++c) {
        const int64_t cnt = pl.cls_cnt[c];
        if (!cnt) continue;
        hipLaunchKernelGGL(k_bn_pairs, dim3((unsigned)cnt), dim3(kBnClassN[c]), bn_lds_bytes(pl.cls_n[c], pl.cls_n[c]), s,
                           (const double*)(w.buf + at.pts), (const int64_t*)(w.buf + at.off), (const int32_t*)(w.buf + at.pairs),
                           (const int32_t*)(w.buf + at.order) + first, dist);
        HIPC(hipGetLastError());
        first += cnt;
    }
    HIPC(hipMemcpyAsync(R->dist.get(), dist, P * 8, hipMemcpyDeviceToHost, s));
    HIPC(hipEventRecord(w.ev[1], s));
    HIPC(hipStreamSynchronize(s));
    float ms = 0.0f;
    HIPC(hipEventElapsedTime(&ms, w.ev[0], w.ev[1]));
    // no cost is a NaN (the coordinates are finite), so a NaN is the kernel's word for "a loop bound was hit"
    for (size_t p = 0; p < P; ++p)
        if (std::isnan(R->dist[p]))
            return fail(TDA_E_CAPACITY, "bottleneck: the matching of pair " + std::to_string(p) + " ran into a loop bound (internal error)");
    R->pub.device_ms = ms;
    *out = &R.release()->pub;
    return 0;
}

extern "C" void tda_bn_free(tda_bn_result* r) { dgm_free(r); }
