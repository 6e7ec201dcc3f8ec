// resample_host.h -- host side of tda_resample (include/tda_rips.h), part of rips.hip's
// translation unit (shares its error state, device checks and the distance kernel selection of
// the persistence entry).
//
// One call, the structure of tda_greedy_perm: per chunk of layers (resample_plan, side_plan.h), the
// (Lc, N, N) f32 distance matrices (enqueue_chunk_distances), then per chunk of resamples
// k_resample_hausdorff.  The workspace, its stream and its mutex are per device and this entry's own
// (side_call.h: no slot's stream is used, nothing is captured into a graph).  A chunk's device
// bytes stay within TDA_GREEDY_WS_BYTES (a single layer may exceed it), beside the whole (L, B)
// result and a shared index table; layers and resamples are chunked so that no grid dimension
// exceeds 65535.  The index table is validated on the host (by the plan) before any device work.
#pragma once
#include "resample_kernels.h"

namespace {

struct ResampleResultImpl {
    tda_resample_result pub = {};
    std::unique_ptr<float[]> haus;
};

}  // namespace

extern "C" int tda_resample(const tda_resample_args* a, tda_resample_result** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    ResamplePlan p;
    std::string msg;
    if (int rc = resample_plan(a, side_ws_cap(), p, msg)) return fail(rc, msg);
    if (int rc = need_device(a->device)) return rc;
    const size_t L = p.L, B = p.B, m = p.m, Lc = p.sq.Lc;
    const int n = (int)p.N;

    SideCall call;
    if (int rc = call.open(kAuxResample, a->device, 2)) return rc;
    hipStream_t s = call.stream();
    std::unique_ptr<ResampleResultImpl> R(new ResampleResultImpl());
    R->haus.reset(new float[L * B]);
    if (int rc = call.reserve(p.total)) return rc;
    if (a->x_on_device)
        if (int rc = call.after_caller(a->stream)) return rc;
    float* d_h = call.at<float>(p.o_h);
    int32_t* d_idx = call.at<int32_t>(p.o_idx);
    float* dm = call.at<float>(p.sq.o_dm);
    if (int rc = call.start()) return rc;
    if (!p.per_layer_idx) HIPC(hipMemcpyAsync(d_idx, a->idx, B * m * 4, hipMemcpyHostToDevice, s));
    for (size_t l0 = 0; l0 < L; l0 += Lc) {
        const size_t lc = std::min(Lc, L - l0);
        const auto table = [&]() -> int {  // a table per layer: this chunk's
            if (p.per_layer_idx) HIPC(hipMemcpyAsync(d_idx, a->idx + l0 * B * m, lc * B * m * 4, hipMemcpyHostToDevice, s));
            return 0;
        };
        if (int rc = enqueue_chunk_distances(s, call.buf(), p.sq, (const char*)a->x + l0 * p.sq.x_layer, a->dtype, a->D, p.is_dist, lc, table)) return rc;
        for (size_t b0 = 0; b0 < B; b0 += p.Bc) {
            const size_t bc = std::min(p.Bc, B - b0);
            const int32_t* ix = d_idx + b0 * m;
            float* h = d_h + l0 * B + b0;
            if (n <= kRsLdsN)
                hipLaunchKernelGGL(k_resample_hausdorff<true>, dim3((unsigned)((bc + kRsPerBlock - 1) / kRsPerBlock), (unsigned)lc), dim3(kRsT),
                                   0, s, dm, n, (int)m, (int)bc, ix, p.idx_lstride, h, B);
            else
                hipLaunchKernelGGL(k_resample_hausdorff<false>, dim3((unsigned)bc, (unsigned)lc), dim3(kRsT), 0, s, dm, n, (int)m, (int)bc, ix,
                                   p.idx_lstride, h, B);
            HIPC(hipGetLastError());
        }
    }
    HIPC(hipMemcpyAsync(R->haus.get(), d_h, L * B * 4, hipMemcpyDeviceToHost, s));
    if (int rc = call.finish()) return rc;
    tda_resample_result& r = R->pub;
    r.L = a->L;
    r.N = a->N;
    r.B = a->B;
    r.m = a->m;
    r.hausdorff = R->haus.get();
    r.device = a->device;
    return side_return(R, out, call.ms);
}

extern "C" void tda_resample_free(tda_resample_result* r) { side_free<ResampleResultImpl>(r); }
