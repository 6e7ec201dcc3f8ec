// ed_host.h -- host side of the spectral metrics (include/tda_rips.h):
// tda_effective_dim, tda_effective_dim_windows and tda_matrix_entropy, part of
// rips.hip's translation unit (shares its error state and device checks).
// The checks and the job of a call (EdJob) are ed_plan / spectral_plan / entropy_plan, side_plan.h.
#pragma once
#include "ed_kernels.h"

namespace {

static_assert(kSideEdMaxM == kEdMaxM && kSideEdMaxAlpha == kEdMaxAlpha, "side_plan.h and ed_kernels.h disagree");

// Gram matrices, Jacobi and the epilogue `epi` (j.per_item floats per matrix) -> out[j.n_out] (host)
template <typename Epi>
int ed_run(const EdJob& j, const Epi& epi, float* out) {
    const int64_t B = j.B, N = j.N, D = j.D, m = j.m;
    if (int rc = need_device(j.device)) return rc;
    SideCall call;
    if (int rc = call.open(kAuxSpectral, j.device)) return rc;
    hipStream_t s = call.stream();
    if (j.x_on_device)
        if (int rc = call.after_caller(j.stream)) return rc;
    if (int rc = call.reserve(j.total)) return rc;
    if (int rc = call.reserve_pinned(j.pinned)) return rc;  // the result
    const void* x = j.x;
    if (j.stage()) {  // the kept rows of every item, packed: they then are (B, N, D)
        const size_t width = (size_t)j.keep_rows * D * j.esz;
        HIPC(hipMemcpy2DAsync(call.at<char>(j.o_x), width, x, (size_t)j.src_rows * D * j.esz, width, (size_t)j.src_items,
                              j.x_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        x = call.at<char>(j.o_x);
    } else if (!j.x_on_device) {
        HIPC(hipMemcpyAsync(call.at<char>(j.o_x), x, (size_t)B * N * D * j.esz, hipMemcpyHostToDevice, s));
        x = call.at<char>(j.o_x);
    }
    double* G = call.at<double>(j.o_g);
    const bool f64 = j.dtype == TDA_F64;
    if (N <= D && D >= kDistMfmaMinD) {  // X X^T on the FP64 matrix cores
        const unsigned nt = (unsigned)((N + kDmT - 1) / kDmT);
        const dim3 gm(nt * (nt + 1) / 2, (unsigned)B);
        if (f64)
            hipLaunchKernelGGL((k_distance_mfma<double, 2>), gm, dim3(256), 0, s, (const double*)x, (int)N, (int)D, (float*)nullptr,
                               (uint32_t*)nullptr, G, (double*)nullptr);
        else
            hipLaunchKernelGGL((k_distance_mfma<float, 2>), gm, dim3(256), 0, s, (const float*)x, (int)N, (int)D, (float*)nullptr,
                               (uint32_t*)nullptr, G, (double*)nullptr);
    } else {
        const unsigned gx = (unsigned)std::min<uint64_t>(1024, ((uint64_t)m * m + 255) / 256);
        if (N <= D) {
            if (f64) hipLaunchKernelGGL(k_gram_rows<double>, dim3(gx, (unsigned)B), dim3(256), 0, s, (const double*)x, (int)N, (int)D, G);
            else hipLaunchKernelGGL(k_gram_rows<float>, dim3(gx, (unsigned)B), dim3(256), 0, s, (const float*)x, (int)N, (int)D, G);
        } else {
            if (f64) hipLaunchKernelGGL(k_gram_cols<double>, dim3(gx, (unsigned)B), dim3(256), 0, s, (const double*)x, (int)N, (int)D, G);
            else hipLaunchKernelGGL(k_gram_cols<float>, dim3(gx, (unsigned)B), dim3(256), 0, s, (const float*)x, (int)N, (int)D, G);
        }
    }
    HIPC(hipGetLastError());
    float* dout = (float*)call.pinned_dev();
    if (m <= kEdLdsMaxM) {
        if (int rc = call.lds_attr((const void*)k_ed_jacobi<true, Epi>, 8 * kEdLdsMaxM * kEdLdsMaxM)) return rc;
        hipLaunchKernelGGL((k_ed_jacobi<true, Epi>), dim3((unsigned)B), dim3(kEdT), (size_t)8 * m * m, s, G, (int)m, epi, dout);
    } else {
        hipLaunchKernelGGL((k_ed_jacobi<false, Epi>), dim3((unsigned)B), dim3(kEdT), 0, s, G, (int)m, epi, dout);
    }
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));
    std::memcpy(out, call.pinned(), j.pinned);
    return 0;
}

}  // namespace

extern "C" int tda_effective_dim(const tda_ed_args* a, float* out) {
    EdJob j;
    std::string msg;
    if (int rc = ed_plan(a, out, j, msg)) return fail(rc, msg);
    return ed_run(j, EdRatio{(int)j.m}, out);
}

extern "C" int tda_effective_dim_windows(const tda_spectral_args* a, float* out) {
    EdJob j;
    std::string msg;
    if (int rc = spectral_plan("windowed effective dimensionality", a, out, true, j, msg)) return fail(rc, msg);
    return ed_run(j, EdRatio{(int)j.m}, out);
}

extern "C" int tda_matrix_entropy(const tda_spectral_args* a, float* out) {
    EdJob j;
    std::string msg;
    if (int rc = entropy_plan(a, out, j, msg)) return fail(rc, msg);
    EdRenyi r{};
    r.n_alpha = a->n_alpha;
    r.eps = a->eps;
    std::copy(a->alphas, a->alphas + a->n_alpha, r.alpha);
    return ed_run(j, r, out);
}
