// sh0_host.h -- host side of tda_subsample_h0 (include/tda_rips.h), part of rips.hip's translation
// unit.
//
// One call, the structure of tda_resample line for line: per chunk of layers (sh0_plan, sh0_plan.h),
// the (Lc, N, N) f32 distance matrices (enqueue_chunk_distances), then per chunk of subsamples
// k_subsample_h0.  The entry is of the resampling family: its frame opens on kAuxResample, so it
// shares tda_resample's lock, stream and workspace and the process gains neither a stream nor a
// workspace through it (no slot's stream is used, nothing is captured into a graph).  A chunk's
// device bytes stay within TDA_GREEDY_WS_BYTES (a single layer may exceed it), beside the whole
// (L, B) result, the sizes and a shared index table; the deaths are chunked with the layers and
// read back chunk by chunk.  Sizes and table are validated on the host (by the plan) before any
// device work.
#pragma once
#include "sh0_kernels.h"
#include "sh0_plan.h"

namespace {

static_assert(kSideSh0LdsN == kSh0LdsN && kSideSh0LdsM == kSh0LdsM && kSideSh0PerBlock == kSh0PerBlock && kSideSh0Head == (size_t)kSh0Head,
              "sh0_plan.h and sh0_kernels.h disagree");
static_assert(kSh0Head + 6 * kSideMaxN <= 64 * 1024, "the global path's LDS needs no raised limit");

struct Sh0ResultImpl {
    tda_subsample_h0_result pub = {};
    std::unique_ptr<double[]> E;
    std::unique_ptr<float[]> deaths;
};

template <bool kPow>
void launch_subsample_h0(hipStream_t s, const Sh0Plan& p, size_t bc, size_t lc, const float* dm, const int32_t* ix, const int32_t* sz, double alpha,
                         double* E, float* deaths) {
    const int n = (int)p.N, m = (int)p.m;
    if (p.resident)
        hipLaunchKernelGGL((k_subsample_h0<true, kPow>), dim3((unsigned)((bc + kSh0PerBlock - 1) / kSh0PerBlock), (unsigned)lc), dim3(kSh0T), 0, s, dm,
                           n, m, (int)bc, ix, p.idx_lstride, sz, (int)(p.mode == 1), alpha, E, p.B, deaths, p.d_lstride);
    else
        hipLaunchKernelGGL((k_subsample_h0<false, kPow>), dim3((unsigned)bc, (unsigned)lc), dim3(kSh0T), p.lds, s, dm, n, m, (int)bc, ix,
                           p.idx_lstride, sz, (int)(p.mode == 1), alpha, E, p.B, deaths, p.d_lstride);
}

}  // namespace

extern "C" int tda_subsample_h0(const tda_subsample_h0_args* a, tda_subsample_h0_result** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    Sh0Plan p;
    std::string msg;
    if (int rc = sh0_plan(a, side_ws_cap(), p, msg)) return fail(rc, msg);
    if (int rc = need_device(a->device)) return rc;
    const size_t L = p.L, B = p.B, m = p.m, Lc = p.sq.Lc;

    SideCall call;
    if (int rc = call.open(kAuxResample, a->device, 2)) return rc;
    hipStream_t s = call.stream();
    std::unique_ptr<Sh0ResultImpl> R(new Sh0ResultImpl());
    R->E.reset(new double[L * B]);
    if (p.want_deaths) R->deaths.reset(new float[L * p.d_lstride + 1]);
    if (int rc = call.reserve(p.total)) return rc;
    if (a->x_on_device)
        if (int rc = call.after_caller(a->stream)) return rc;
    double* d_E = call.at<double>(p.o_E);
    int32_t* d_sz = call.at<int32_t>(p.o_sz);
    int32_t* d_idx = call.at<int32_t>(p.o_idx);
    float* d_deaths = p.want_deaths ? call.at<float>(p.o_deaths) : nullptr;
    float* dm = call.at<float>(p.sq.o_dm);
    if (int rc = call.start()) return rc;
    HIPC(hipMemcpyAsync(d_sz, a->sizes, B * 4, hipMemcpyHostToDevice, s));
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
            float* dd = d_deaths ? d_deaths + b0 * (m - 1) : nullptr;
            if (p.mode == 2) launch_subsample_h0<true>(s, p, bc, lc, dm, d_idx + b0 * m, d_sz + b0, a->alpha, d_E + l0 * B + b0, dd);
            else launch_subsample_h0<false>(s, p, bc, lc, dm, d_idx + b0 * m, d_sz + b0, a->alpha, d_E + l0 * B + b0, dd);
            HIPC(hipGetLastError());
        }
        if (p.want_deaths && p.d_lstride)  // the next chunk reuses the buffer: stream order keeps this copy ahead of it
            HIPC(hipMemcpyAsync(R->deaths.get() + l0 * p.d_lstride, d_deaths, lc * p.d_lstride * 4, hipMemcpyDeviceToHost, s));
    }
    HIPC(hipMemcpyAsync(R->E.get(), d_E, L * B * 8, hipMemcpyDeviceToHost, s));
    if (int rc = call.finish()) return rc;
    tda_subsample_h0_result& r = R->pub;
    r.L = a->L;
    r.N = a->N;
    r.B = a->B;
    r.m = a->m;
    r.E = R->E.get();
    r.deaths = p.want_deaths ? R->deaths.get() : nullptr;
    r.device = a->device;
    return side_return(R, out, call.ms);
}

extern "C" void tda_subsample_h0_free(tda_subsample_h0_result* r) { side_free<Sh0ResultImpl>(r); }
