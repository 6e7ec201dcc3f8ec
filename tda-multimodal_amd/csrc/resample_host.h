// resample_host.h -- host side of tda_resample (include/tda_rips.h), part of rips.hip's
// translation unit (shares its error state, device checks and the distance kernel selection of
// the persistence entry).
//
// One call, the structure of tda_greedy_perm: per chunk of layers, the (Lc, N, N) f32 distance
// matrices (launch_point_distances, or k_square_dist for distance-matrix input), then per chunk of
// resamples k_resample_hausdorff.  The workspace, its stream and its mutex are per device and this
// entry's own (no slot's stream is used, nothing is captured into a graph).  A chunk's device
// bytes stay within TDA_GREEDY_WS_BYTES (a single layer may exceed it), beside the whole (L, B)
// result and a shared index table; layers and resamples are chunked so that no grid dimension
// exceeds 65535.  The index table is validated on the host before any device work.
#pragma once
#include "resample_kernels.h"

namespace {

struct ResampleResultImpl {
    tda_resample_result pub = {};
    std::unique_ptr<float[]> haus;
};

int resample_validate(const tda_resample_args* a) {
    if (!a) return fail(TDA_E_INVALID, "args is NULL");
    if (!a->x) return fail(TDA_E_INVALID, "x is NULL");
    if (!a->idx) return fail(TDA_E_INVALID, "idx is NULL");
    if (a->L < 1) return fail(TDA_E_INVALID, "L must be >= 1");
    if (a->N < 1) return fail(TDA_E_INVALID, "N must be >= 1");
    if (!a->is_dist && a->D < 1) return fail(TDA_E_INVALID, "D must be >= 1");
    if (a->dtype != TDA_F32 && a->dtype != TDA_F64) return fail(TDA_E_INVALID, "dtype must be TDA_F32 or TDA_F64");
    if (a->B < 1) return fail(TDA_E_INVALID, "B must be >= 1");
    if (a->m < 1) return fail(TDA_E_INVALID, "m must be >= 1");
    if (a->N > 8192) return fail(TDA_E_UNSUPPORTED, "resampling: N > 8192 is not supported");
    if (a->m > 8192) return fail(TDA_E_UNSUPPORTED, "resampling: m > 8192 is not supported");
    if (!a->is_dist && a->dtype == TDA_F64)
        return fail(TDA_E_UNSUPPORTED, "resampling of float64 point clouds is not supported (pass float32 points or a distance matrix)");
    if ((unsigned __int128)a->L * (uint64_t)a->B > (uint64_t)TDA_RESAMPLE_MAX_OUT)
        return fail(TDA_E_UNSUPPORTED, "resampling: more than 2^27 resamples (L * B) in one call is not supported: split B over several calls");
    const size_t n_idx = (size_t)(a->idx_per_layer ? a->L : 1) * (size_t)a->B * (size_t)a->m;
    for (size_t e = 0; e < n_idx; ++e)
        if (a->idx[e] < 0 || a->idx[e] >= a->N)
            return fail(TDA_E_INVALID, "idx[" + std::to_string(e) + "] = " + std::to_string(a->idx[e]) + " is outside [0, N = " +
                                           std::to_string(a->N) + ")");
    return 0;
}

}  // namespace

extern "C" int tda_resample(const tda_resample_args* a, tda_resample_result** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    if (int rc = resample_validate(a)) return rc;
    if (!tda_device_ok(a->device)) return fail(TDA_E_NODEVICE, "no gfx950 device at ordinal " + std::to_string(a->device));
    const size_t L = (size_t)a->L, N = (size_t)a->N, B = (size_t)a->B, m = (size_t)a->m;
    const int n = (int)a->N;
    const bool is_dist = a->is_dist != 0, host_in = !a->x_on_device, per_layer_idx = a->idx_per_layer != 0;
    const size_t esz = a->dtype == TDA_F64 ? 8 : 4;
    const size_t x_layer = N * (is_dist ? N : (size_t)a->D) * esz;
    const DistSel sel = dist_select(N, a->D, a->dtype, is_dist);
    const size_t sp = (size_t)sel.dsplit;

    AuxWs& w = aux_ws(kAuxResample, a->device);
    std::lock_guard<std::mutex> guard(w.mu);
    if (int rc = aux_open(w, 2)) return rc;
    hipStream_t s = w.stream;
    const hipEvent_t ev0 = w.ev[0], ev1 = w.ev[1];

    // chunk of layers: the largest whose workspace stays within the cap (one layer at least)
    size_t per_layer = 0;
    auto add = [&](size_t bytes) { per_layer += align_up(bytes, 256); };
    add(host_in ? x_layer : 0);
    add(N * N * 4);
    add(N * 4);
    add(sel.partials() ? sp * N * N * 8 : 0);
    add(sel.partials() ? sp * N * 8 : 0);
    add(per_layer_idx ? B * m * 4 : 0);
    const size_t Lc = std::min<size_t>(std::min<size_t>(L, 65535), std::max<size_t>(1, (size_t)TDA_GREEDY_WS_BYTES / per_layer));
    const size_t Bc = std::min<size_t>(B, 65535);  // resamples per launch: grid dimensions stay <= 65535
    Carve cv;
    const size_t o_h = cv.take(L * B * 4), o_idx = cv.take((per_layer_idx ? Lc : 1) * B * m * 4);
    const size_t o_x = cv.take(host_in ? Lc * x_layer : 0), o_dm = cv.take(Lc * N * N * 4), o_rm = cv.take(Lc * N * 4);
    const size_t o_gp = cv.take(sel.partials() ? Lc * sp * N * N * 8 : 0), o_np = cv.take(sel.partials() ? Lc * sp * N * 8 : 0);

    std::unique_ptr<ResampleResultImpl> R(new ResampleResultImpl());
    R->haus.reset(new float[L * B]);
    if (int rc = aux_reserve(w, cv.o)) return rc;
    if (a->x_on_device)
        if (int rc = aux_after_caller(w, a->stream)) return rc;
    float* d_h = (float*)(w.buf.p + o_h);
    int32_t* d_idx = (int32_t*)(w.buf.p + o_idx);
    float* dm = (float*)(w.buf.p + o_dm);
    const size_t idx_lstride = per_layer_idx ? B * m : 0;
    HIPC(hipEventRecord(ev0, s));
    if (!per_layer_idx) HIPC(hipMemcpyAsync(d_idx, a->idx, B * m * 4, hipMemcpyHostToDevice, s));
    for (size_t l0 = 0; l0 < L; l0 += Lc) {
        const size_t lc = std::min(Lc, L - l0);
        const void* x = (const char*)a->x + l0 * x_layer;
        if (host_in) {
            HIPC(hipMemcpyAsync(w.buf.p + o_x, x, lc * x_layer, hipMemcpyHostToDevice, s));
            x = w.buf.p + o_x;
        }
        if (per_layer_idx) HIPC(hipMemcpyAsync(d_idx, a->idx + l0 * B * m, lc * B * m * 4, hipMemcpyHostToDevice, s));
        if (!is_dist) {
            HIPC(hipMemsetAsync(w.buf.p + o_rm, 0, lc * N * 4, s));  // the distance kernels fold row maxima in (unused here)
            const DistLaunch dl = {x, a->dtype, n, a->D, (int)lc, sel, dm, (uint32_t*)(w.buf.p + o_rm), (double*)(w.buf.p + o_gp),
                                   (double*)(w.buf.p + o_np), nullptr};
            if (int rc = launch_point_distances(s, dl, [](const char*) { return 0; })) return rc;
        } else {
            const unsigned gx = (unsigned)std::min<uint64_t>(1024, ((uint64_t)N * N + 255) / 256);
            if (a->dtype == TDA_F64)
                hipLaunchKernelGGL(k_square_dist<double>, dim3(gx, (unsigned)lc), dim3(256), 0, s, (const double*)x, n, dm);
            else
                hipLaunchKernelGGL(k_square_dist<float>, dim3(gx, (unsigned)lc), dim3(256), 0, s, (const float*)x, n, dm);
        }
        HIPC(hipGetLastError());
        for (size_t b0 = 0; b0 < B; b0 += Bc) {
            const size_t bc = std::min(Bc, B - b0);
            const int32_t* ix = d_idx + b0 * m;
            float* h = d_h + l0 * B + b0;
            if (n <= kRsLdsN)
                hipLaunchKernelGGL(k_resample_hausdorff<true>, dim3((unsigned)((bc + kRsPerBlock - 1) / kRsPerBlock), (unsigned)lc), dim3(kRsT),
                                   0, s, dm, n, (int)m, (int)bc, ix, idx_lstride, h, B);
            else
                hipLaunchKernelGGL(k_resample_hausdorff<false>, dim3((unsigned)bc, (unsigned)lc), dim3(kRsT), 0, s, dm, n, (int)m, (int)bc, ix,
                                   idx_lstride, h, B);
            HIPC(hipGetLastError());
        }
    }
    HIPC(hipMemcpyAsync(R->haus.get(), d_h, L * B * 4, hipMemcpyDeviceToHost, s));
    HIPC(hipEventRecord(ev1, s));
    HIPC(hipStreamSynchronize(s));
    float ms = 0.0f;
    HIPC(hipEventElapsedTime(&ms, ev0, ev1));
    tda_resample_result& r = R->pub;
    r.L = a->L;
    r.N = a->N;
    r.B = a->B;
    r.m = a->m;
    r.hausdorff = R->haus.get();
    r.device = a->device;
    r.device_ms = ms;
    *out = &R.release()->pub;
    return 0;
}

extern "C" void tda_resample_free(tda_resample_result* r) {
    if (!r) return;
    delete reinterpret_cast<ResampleResultImpl*>(r);  // pub is the first member
}
