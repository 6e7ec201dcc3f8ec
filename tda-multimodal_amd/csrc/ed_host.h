// ed_host.h -- host side of the spectral metrics (include/tda_rips.h):
// tda_effective_dim, tda_effective_dim_windows and tda_matrix_entropy, part of
// rips.hip's translation unit (shares its error state and device checks).
#pragma once
#include "ed_kernels.h"

namespace {

// One call's work, validated: B matrices of N x D.  src_items > 0: the B
// matrices are the windows of src_items items of src_rows rows each, of which
// only the first keep_rows are used (a remainder is dropped), so the kept rows
// are staged with one 2-D copy; otherwise x already is (B, N, D).
struct EdJob {
    const void* x;
    int32_t dtype, x_on_device;
    int64_t B, N, D;
    int64_t src_items, src_rows, keep_rows;
    int32_t device;
    void* stream;
};

// the shape limits of the Gram and Jacobi kernels, shared by the three entries
int ed_check_shape(const char* what, int64_t N, int64_t D) {
    if (std::min(N, D) > kEdMaxM) return fail(TDA_E_UNSUPPORTED, std::string(what) + ": min(N, D) <= 1024 is supported");
    if (N > 8192 && N <= D) return fail(TDA_E_UNSUPPORTED, std::string(what) + ": N <= 8192");
    return 0;
}

// Gram matrices, Jacobi and the epilogue `epi` (per_item floats per matrix) -> out[B * per_item] (host)
template <typename Epi>
int ed_run(const EdJob& j, const Epi& epi, int64_t per_item, float* out) {
    const int64_t B = j.B, N = j.N, D = j.D, m = std::min(N, D);
    if (!tda_device_ok(j.device)) return fail(TDA_E_NODEVICE, "no gfx950 device at ordinal " + std::to_string(j.device));
    AuxWs& w = aux_ws(kAuxSpectral, j.device);
    std::lock_guard<std::mutex> guard(w.mu);
    if (int rc = aux_open(w)) return rc;
    hipStream_t s = w.stream;
    if (j.x_on_device)
        if (int rc = aux_after_caller(w, j.stream)) return rc;
    const size_t esz = j.dtype == TDA_F64 ? 8 : 4;
    const bool stage = j.src_items > 0;
    Carve cv;
    const size_t o_x = cv.take(j.x_on_device && !stage ? 0 : (size_t)B * N * D * esz), o_g = cv.take((size_t)B * m * m * 8);
    if (int rc = aux_reserve(w, cv.o)) return rc;
    const size_t n_out = (size_t)(B * per_item);
    if (int rc = aux_reserve_pinned(w, sizeof(float) * n_out)) return rc;  // the result
    const void* x = j.x;
    if (stage) {  // the kept rows of every item, packed: they then are (B, N, D)
        const size_t width = (size_t)j.keep_rows * D * esz;
        HIPC(hipMemcpy2DAsync(w.buf.p + o_x, width, x, (size_t)j.src_rows * D * esz, width, (size_t)j.src_items,
                              j.x_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        x = w.buf.p + o_x;
    } else if (!j.x_on_device) {
        HIPC(hipMemcpyAsync(w.buf.p + o_x, x, (size_t)B * N * D * esz, hipMemcpyHostToDevice, s));
        x = w.buf.p + o_x;
    }
    double* G = (double*)(w.buf.p + o_g);
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
    float* dout = (float*)w.hout.dev;
    if (m <= kEdLdsMaxM) {
        if (int rc = aux_lds_attr(w, (const void*)k_ed_jacobi<true, Epi>, 8 * kEdLdsMaxM * kEdLdsMaxM)) return rc;
        hipLaunchKernelGGL((k_ed_jacobi<true, Epi>), dim3((unsigned)B), dim3(kEdT), (size_t)8 * m * m, s, G, (int)m, epi, dout);
    } else {
        hipLaunchKernelGGL((k_ed_jacobi<false, Epi>), dim3((unsigned)B), dim3(kEdT), 0, s, G, (int)m, epi, dout);
    }
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));
    std::memcpy(out, w.hout.p, sizeof(float) * n_out);
    return 0;
}

// tda_spectral_args -> the job: the window split of metrics.py:61-96
int spectral_job(const char* what, const tda_spectral_args* a, const float* out, bool need_windows, EdJob* j) {
    if (!a || !out) return fail(TDA_E_INVALID, "args and out are required");
    if (a->B < 1 || a->S < 1 || a->D < 1) return fail(TDA_E_INVALID, "need B, S, D >= 1");
    if (!a->x) return fail(TDA_E_INVALID, "x is NULL");
    if (a->dtype != TDA_F32 && a->dtype != TDA_F64) return fail(TDA_E_INVALID, "dtype must be TDA_F32 or TDA_F64");
    if (a->n_windows < 0 || (need_windows && a->n_windows == 0)) return fail(TDA_E_INVALID, "n_windows must be positive");
    const int64_t W = std::min(a->n_windows, a->S);  // more windows than rows: each row is its own window
    const int64_t rows = W ? a->S / W : a->S;
    *j = EdJob{a->x, a->dtype, a->x_on_device, a->B * std::max<int64_t>(W, 1), rows, a->D, 0, 0, 0, a->device, a->stream};
    if (W && a->S % W) j->src_items = a->B, j->src_rows = a->S, j->keep_rows = W * rows;
    return ed_check_shape(what, rows, a->D);
}

}  // namespace

extern "C" int tda_effective_dim(const tda_ed_args* a, float* out) {
    if (!a || !out) return fail(TDA_E_INVALID, "args and out are required");
    if (a->B < 1 || a->N < 1 || a->D < 1) return fail(TDA_E_INVALID, "need B, N, D >= 1");
    if (!a->x) return fail(TDA_E_INVALID, "x is NULL");
    if (a->dtype != TDA_F32 && a->dtype != TDA_F64) return fail(TDA_E_INVALID, "dtype must be TDA_F32 or TDA_F64");
    if (int rc = ed_check_shape("effective dimensionality", a->N, a->D)) return rc;
    const EdJob j{a->x, a->dtype, a->x_on_device, a->B, a->N, a->D, 0, 0, 0, a->device, a->stream};
    return ed_run(j, EdRatio{(int)std::min(a->N, a->D)}, 1, out);
}

extern "C" int tda_effective_dim_windows(const tda_spectral_args* a, float* out) {
    EdJob j;
    if (int rc = spectral_job("windowed effective dimensionality", a, out, true, &j)) return rc;
    return ed_run(j, EdRatio{(int)std::min(j.N, j.D)}, 1, out);
}

extern "C" int tda_matrix_entropy(const tda_spectral_args* a, float* out) {
    EdJob j;
    if (int rc = spectral_job("matrix entropy", a, out, false, &j)) return rc;
    if (a->n_alpha < 1 || a->n_alpha > kEdMaxAlpha) return fail(TDA_E_INVALID, "matrix entropy: 1 .. 16 orders per call");
    if (!a->alphas) return fail(TDA_E_INVALID, "alphas is NULL");
    if (!(a->eps >= 0.0)) return fail(TDA_E_INVALID, "matrix entropy: eps must be >= 0");
    EdRenyi r{};
    r.n_alpha = a->n_alpha;
    r.eps = a->eps;
    for (int i = 0; i < a->n_alpha; ++i) {
        // order <= 0 counts the zero eigenvalues of the N x N Gram matrix, which the reference's f32 noise decides
        if (!(a->alphas[i] > 0.0) || !std::isfinite(a->alphas[i])) return fail(TDA_E_INVALID, "matrix entropy: every order alpha must be finite and > 0");
        r.alpha[i] = a->alphas[i];
    }
    return ed_run(j, r, a->n_alpha, out);
}
