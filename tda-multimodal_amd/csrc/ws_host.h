// ws_host.h -- host side of tda_wasserstein (include/tda_dgm.h), part of rips.hip's
// translation unit (shares its error state and device checks; the plan and the
// classes' limits are dgm_plan.h's, the frame of the call dgm_call.h's).
//
// One call, the shape of tda_bottleneck: drop the non-finite points on the host,
// orient every pair canonically (dgm_orient: the kernel sees the same input for
// (i, j) and (j, i)), sort the pairs into size classes, upload everything in one
// copy, launch k_ws_pairs once per non-empty class, copy the results back in one
// copy: the P distances and, with TDA_WS_WANT_MATCHING, the mates of every pair's
// first diagram (as oriented), which the host turns into the caller's orientation.
//
// Size classes (nm = max(n1, n2) of a pair).  Thread j owns column j, a point of
// the longer diagram, so the workgroup size follows nm, and the dynamic LDS of a
// launch is that of the class's largest pair, ws_lds_bytes(nm, nm) = 60 nm + 200:
//   nm <= 64:   64 threads, at most  3.9 KiB: one wave, so the barrier of a scan
//               step costs nothing, and the wave slots, not LDS, bound the
//               occupancy.  The sweep's H1 diagrams live here;
//   nm <= 256:  256 threads, at most 15.2 KiB: 8 workgroups per CU by wave slots,
//               10 by LDS;
//   nm <= 512:  512 threads, at most 30.2 KiB: 4 workgroups per CU by wave slots,
//               5 by LDS, below the 64 KiB a launch gets without asking for more.
// A pair is solved by one workgroup whatever its class, and the scan's choices
// depend on distances and column indices alone (ws_kernels.h), so the class only
// sets the launch shape.
#pragma once
#include "../../include/tda_dgm.h"
#include "dgm_call.h"
#include "ws_kernels.h"

namespace {

static_assert(kWsMaxN == TDA_WS_MAX_POINTS && kWsClassN[kPairClasses - 1] == kWsMaxN, "tda_dgm.h, dgm_plan.h and ws_kernels.h disagree");
static_assert(ws_lds_bytes(kWsMaxN, kWsMaxN) <= 64 * 1024, "k_ws_pairs would need hipFuncAttributeMaxDynamicSharedMemorySize");

struct WsResultImpl {
    tda_ws_result pub = {};
    std::vector<double> dist;
    std::vector<int64_t> match_off;
    std::vector<int32_t> match;
};

}  // namespace

extern "C" int tda_wasserstein(const tda_ws_args* a, tda_ws_result** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    WsPlan wp;
    std::string msg;
    if (int rc = ws_plan(a, wp, msg)) return fail(rc, msg);
    if (!tda_device_ok(a->device)) return fail(TDA_E_NODEVICE, "no gfx950 device at ordinal " + std::to_string(a->device));
    const PairPlan& pl = wp.pl;
    const std::vector<uint8_t>& swapped = wp.swapped;
    const std::vector<int64_t>& moff = wp.moff;
    const size_t P = (size_t)pl.P;
    const bool want = a->flags & TDA_WS_WANT_MATCHING;
    std::unique_ptr<WsResultImpl> R(new WsResultImpl());
    R->pub.P = pl.P;
    R->dist.assign(std::max<size_t>(P, 1), 0.0);
    R->pub.dist = R->dist.data();
    if (want) {
        R->match_off.assign(P + 1, 0);
        R->pub.match_off = R->match_off.data();
        R->match.assign(1, -1);  // never NULL with the flag
        R->pub.match = R->match.data();
    }
    if (P == 0) return dgm_return(R, out);  // nothing to launch

    DgmCall call;
    const PairAt at(call, pl);
    const size_t o_moff = want ? call.upload(moff) : 0;
    const size_t o_dist = call.device(P * 8);
    const size_t n_match = want ? (size_t)moff[P] : 0;
    const size_t o_match = want ? call.device(n_match * 4) : 0;
    const size_t down_bytes = want ? o_match + n_match * 4 - o_dist : P * 8;  // the downloaded part: dist, then match
    std::vector<char> down(down_bytes);
    if (int rc = call.begin(kAuxWs, a->device)) return rc;
    int64_t first = 0;
    for (int c = 0; c < kPairClasses; ++c) {
        const int64_t cnt = pl.cls_cnt[c];
        if (!cnt) continue;
        hipLaunchKernelGGL(k_ws_pairs, dim3((unsigned)cnt), dim3(kWsClassN[c]), ws_lds_bytes(pl.cls_n[c], pl.cls_n[c]), call.stream(),
                           call.at<const double>(at.pts), call.at<const int64_t>(at.off), call.at<const int32_t>(at.pairs),
                           call.at<const int32_t>(at.order) + first, call.at<double>(o_dist),
                           want ? call.at<const int64_t>(o_moff) : nullptr, want ? call.at<int32_t>(o_match) : nullptr);
        HIPC(hipGetLastError());
        first += cnt;
    }
    if (int rc = call.end(down.data(), o_dist, down_bytes)) return rc;
    std::memcpy(R->dist.data(), down.data(), P * 8);
    // no sum of costs is a NaN (the coordinates are finite), so a NaN is the kernel's word for "a loop bound was hit"
    for (size_t p = 0; p < P; ++p)
        if (std::isnan(R->dist[p]))
            return fail(TDA_E_CAPACITY, "wasserstein: the solver of pair " + std::to_string(p) + " ran into a loop bound (internal error)");
    if (want) {
        // the caller's orientation: the device's entries are the mates of the oriented pair's first diagram
        const int32_t* dev = (const int32_t*)(down.data() + (o_match - o_dist));
        for (size_t p = 0; p < P; ++p) {
            const int32_t i = pl.pairs[2 * p], j = pl.pairs[2 * p + 1];  // as oriented
            const int64_t nc = pl.off[i + 1] - pl.off[i], nr = pl.off[j + 1] - pl.off[j];
            R->match_off[p + 1] = R->match_off[p] + (swapped[p] ? nr : nc);
        }
        R->match.assign(std::max<size_t>((size_t)R->match_off[P], 1), -1);
        for (size_t p = 0; p < P; ++p) {
            const int32_t i = pl.pairs[2 * p], j = pl.pairs[2 * p + 1];
            const int64_t nc = pl.off[i + 1] - pl.off[i], nr = pl.off[j + 1] - pl.off[j];
            const int32_t* m = dev + moff[p];
            int32_t* o = R->match.data() + R->match_off[p];
            for (int64_t k = 0; k < nc; ++k) {
                if (m[k] < -1 || m[k] >= nr)
                    return fail(TDA_E_CAPACITY, "wasserstein: the matching of pair " + std::to_string(p) + " is not one (internal error)");
                if (!swapped[p])
                    o[k] = m[k];
                else if (m[k] >= 0)
                    o[m[k]] = (int32_t)k;  // the map inverted: the caller's first diagram is the oriented pair's second
            }
        }
        R->pub.match = R->match.data();
    }
    return dgm_return(R, out, call.ms);
}

extern "C" void tda_ws_free(tda_ws_result* r) {
    delete reinterpret_cast<WsResultImpl*>(r);  // pub is the first member; NULL is a no-op
}
