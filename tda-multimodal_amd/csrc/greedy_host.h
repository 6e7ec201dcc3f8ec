// greedy_host.h -- host side of tda_greedy_perm (include/tda_rips.h), part of
// rips.hip's translation unit (shares its error state, device checks and the
// distance kernel selection of the persistence entry).
//
// One call: per chunk of layers, the (Lc, N, N) f32 distance matrices
// (launch_point_distances, or k_square_dist for distance-matrix input), then
// k_greedy_perm (one workgroup per layer) and k_gather_landmarks.  The
// workspace, its stream and its mutex are per device and this entry's own (no
// slot's stream is used, nothing is captured into a graph).  A chunk's device
// bytes stay within TDA_GREEDY_WS_BYTES (a single layer may exceed it: N =
// 8192 alone takes 256 MiB for its matrix).
#pragma once
#include "greedy_kernels.h"

namespace {

struct GreedyResultImpl {
    tda_greedy_result pub = {};
    std::unique_ptr<int64_t[]> idx;
    std::unique_ptr<float[]> lam, dperm;
    float* sub_dev = nullptr;
    ~GreedyResultImpl() {
        if (!sub_dev) return;
        ws::AllocScope lock;  // a free synchronises the device: never beside a slot's capture
        (void)hipFree(sub_dev);
    }
};

int greedy_validate(const tda_greedy_args* a) {
    if (!a) return fail(TDA_E_INVALID, "args is NULL");
    if (!a->x) return fail(TDA_E_INVALID, "x is NULL");
    if (a->L < 1) return fail(TDA_E_INVALID, "L must be >= 1");
    if (a->N < 1) return fail(TDA_E_INVALID, "N must be >= 1");
    if (!a->is_dist && a->D < 1) return fail(TDA_E_INVALID, "D must be >= 1");
    if (a->dtype != TDA_F32 && a->dtype != TDA_F64) return fail(TDA_E_INVALID, "dtype must be TDA_F32 or TDA_F64");
    if (a->n_perm < 1 || (int64_t)a->n_perm > a->N) return fail(TDA_E_INVALID, "n_perm must be in [1, N]");
    if (a->N > (int64_t)kGpMaxQ * kGpT) return fail(TDA_E_UNSUPPORTED, "greedy subsampling: N > 8192 is not supported");
    if (!a->is_dist && a->dtype == TDA_F64)
        return fail(TDA_E_UNSUPPORTED, "greedy subsampling of float64 point clouds is not supported (pass float32 points or a distance matrix)");
    return 0;
}

void launch_greedy_perm(hipStream_t s, const float* dm, int L, int n, int k, int64_t* idx, float* lam) {
    if (n <= kGpT) hipLaunchKernelGGL(k_greedy_perm<1>, dim3(L), dim3(kGpT), 0, s, dm, n, k, idx, lam);
    else if (n <= 2 * kGpT) hipLaunchKernelGGL(k_greedy_perm<2>, dim3(L), dim3(kGpT), 0, s, dm, n, k, idx, lam);
    else if (n <= 4 * kGpT) hipLaunchKernelGGL(k_greedy_perm<4>, dim3(L), dim3(kGpT), 0, s, dm, n, k, idx, lam);
    else hipLaunchKernelGGL(k_greedy_perm<kGpMaxQ>, dim3(L), dim3(kGpT), 0, s, dm, n, k, idx, lam);
}

}  // namespace

extern "C" int tda_greedy_perm(const tda_greedy_args* a, tda_greedy_result** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    if (int rc = greedy_validate(a)) return rc;
    if (!tda_device_ok(a->device)) return fail(TDA_E_NODEVICE, "no gfx950 device at ordinal " + std::to_string(a->device));
    const size_t L = (size_t)a->L, N = (size_t)a->N, k = (size_t)a->n_perm;
    const int n = (int)a->N;
    const bool is_dist = a->is_dist != 0, host_in = !a->x_on_device, want_dp = a->want_dperm2all != 0;
    const size_t esz = a->dtype == TDA_F64 ? 8 : 4;
    const size_t x_layer = N * (is_dist ? N : (size_t)a->D) * esz;
    const DistSel sel = dist_select(N, a->D, a->dtype, is_dist);
    const size_t sp = (size_t)sel.dsplit;

    AuxWs& w = aux_ws(kAuxGreedy, a->device);
    std::lock_guard<std::mutex> guard(w.mu);
    if (int rc = aux_open(w, 4)) return rc;
    hipStream_t s = w.stream;
    const hipEvent_t ev0 = w.ev[0], ev1 = w.ev[1], evk0 = w.ev[2], evk1 = w.ev[3];  // the call; k_greedy_perm of a chunk

    // chunk of layers: the largest whose workspace stays within the cap (one layer at least)
    size_t per_layer = 0;
    auto add = [&](size_t bytes) { per_layer += align_up(bytes, 256); };
    add(host_in ? x_layer : 0);
    add(N * N * 4);
    add(N * 4);
    add(sel.partials() ? sp * N * N * 8 : 0);
    add(sel.partials() ? sp * N * 8 : 0);
    add(want_dp ? k * N * 4 : 0);
    const size_t Lc = std::min<size_t>(std::min<size_t>(L, 65535), std::max<size_t>(1, (size_t)TDA_GREEDY_WS_BYTES / per_layer));
    Carve cv;
    const size_t o_idx = cv.take(L * k * 8), o_lam = cv.take(L * k * 4);
    const size_t o_x = cv.take(host_in ? Lc * x_layer : 0), o_dm = cv.take(Lc * N * N * 4), o_rm = cv.take(Lc * N * 4);
    const size_t o_gp = cv.take(sel.partials() ? Lc * sp * N * N * 8 : 0), o_np = cv.take(sel.partials() ? Lc * sp * N * 8 : 0);
    const size_t o_dp = cv.take(want_dp ? Lc * k * N * 4 : 0);

    std::unique_ptr<GreedyResultImpl> R(new GreedyResultImpl());
    R->idx.reset(new int64_t[L * k]);
    R->lam.reset(new float[L * k]);
    if (want_dp) R->dperm.reset(new float[L * k * N]);
    const auto alloc_sub = [&]() -> int {  // the result's own buffer, in the same hold of the allocation scope
        HIPC(hipMalloc((void**)&R->sub_dev, L * k * k * 4));
        return 0;
    };
    if (int rc = aux_reserve(w, cv.o, alloc_sub)) return rc;
    if (a->x_on_device)
        if (int rc = aux_after_caller(w, a->stream)) return rc;
    int64_t* d_idx = (int64_t*)(w.buf.p + o_idx);
    float* d_lam = (float*)(w.buf.p + o_lam);
    float* dm = (float*)(w.buf.p + o_dm);
    float* d_dp = want_dp ? (float*)(w.buf.p + o_dp) : nullptr;
    double select_ms = 0.0;
    HIPC(hipEventRecord(ev0, s));
    for (size_t l0 = 0; l0 < L; l0 += Lc) {
        const size_t lc = std::min(Lc, L - l0);
        const void* x = (const char*)a->x + l0 * x_layer;
        if (host_in) {
            HIPC(hipMemcpyAsync(w.buf.p + o_x, x, lc * x_layer, hipMemcpyHostToDevice, s));
            x = w.buf.p + o_x;
        }
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
        HIPC(hipEventRecord(evk0, s));
        launch_greedy_perm(s, dm, (int)lc, n, (int)k, d_idx + l0 * k, d_lam + l0 * k);
        HIPC(hipGetLastError());
        HIPC(hipEventRecord(evk1, s));
        hipLaunchKernelGGL(k_gather_landmarks, dim3((unsigned)k, (unsigned)lc), dim3(256), 0, s, dm, n, (int)k, d_idx + l0 * k,
                           R->sub_dev + l0 * k * k, d_dp);
        HIPC(hipGetLastError());
        if (want_dp) HIPC(hipMemcpyAsync(R->dperm.get() + l0 * k * N, d_dp, lc * k * N * 4, hipMemcpyDeviceToHost, s));
        if (l0 + lc < L) {  // the next chunk reuses the buffers and the two kernel events
            HIPC(hipStreamSynchronize(s));
            float ms = 0.0f;
            HIPC(hipEventElapsedTime(&ms, evk0, evk1));
            select_ms += ms;
        }
    }
    HIPC(hipMemcpyAsync(R->idx.get(), d_idx, L * k * 8, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(R->lam.get(), d_lam, L * k * 4, hipMemcpyDeviceToHost, s));
    HIPC(hipEventRecord(ev1, s));
    HIPC(hipStreamSynchronize(s));
    float ms = 0.0f;
    HIPC(hipEventElapsedTime(&ms, evk0, evk1));
    select_ms += ms;
    HIPC(hipEventElapsedTime(&ms, ev0, ev1));
    tda_greedy_result& r = R->pub;
    r.L = a->L;
    r.N = a->N;
    r.n_perm = a->n_perm;
    r.idx_perm = R->idx.get();
    r.lambdas = R->lam.get();
    r.dperm2all = want_dp ? R->dperm.get() : nullptr;
    r.sub_dev = R->sub_dev;
    r.device = a->device;
    r.device_ms = ms;
    r.select_ms = select_ms;
    *out = &R.release()->pub;
    return 0;
}

extern "C" void tda_greedy_free(tda_greedy_result* r) {
    if (!r) return;
    delete reinterpret_cast<GreedyResultImpl*>(r);  // pub is the first member
}
