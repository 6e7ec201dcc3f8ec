// umap_host.h -- host side of tda_umap_batch and tda_umap_transform (include/tda_umap.h), part of
// rips.hip's translation unit (shares its error state and device checks).  The checks, every offset
// and the LDS sizes of a call are umap_plan / umap_transform_plan, side_plan.h.
#pragma once
#include "../../include/tda_umap.h"
#include "umap_kernels.h"

namespace {

static_assert(kSideUmapMaxK == kUmapMaxK && kSideUmapMaxC == kUmapMaxC && kSideUmapSpecMaxN == kUmapSpecMaxN, "side_plan.h and umap_kernels.h disagree");

// the UMAP input distances of L clouds of n points (cosine always on the FP64
// matrix cores; euclidean from D >= 32 there too, else the scalar kernel)
void umap_distances(const void* x, int dtype, int metric, int64_t L, int64_t N, int64_t D, float* dist, uint32_t* rmax, hipStream_t s) {
    const unsigned nt = (unsigned)((N + kDmT - 1) / kDmT);
    const dim3 gm(nt * (nt + 1) / 2, (unsigned)L);
    if (metric == TDA_UMAP_COSINE) {
        if (dtype == TDA_F64)
            hipLaunchKernelGGL((k_distance_mfma<double, 1>), gm, dim3(256), 0, s, (const double*)x, (int)N, (int)D, dist, rmax, (double*)nullptr, (double*)nullptr);
        else
            hipLaunchKernelGGL((k_distance_mfma<float, 1>), gm, dim3(256), 0, s, (const float*)x, (int)N, (int)D, dist, rmax, (double*)nullptr, (double*)nullptr);
    } else if (D >= kDistMfmaMinD) {
        if (dtype == TDA_F64)
            hipLaunchKernelGGL((k_distance_mfma<double, 0>), gm, dim3(256), 0, s, (const double*)x, (int)N, (int)D, dist, rmax, (double*)nullptr, (double*)nullptr);
        else
            hipLaunchKernelGGL((k_distance_mfma<float, 0>), gm, dim3(256), 0, s, (const float*)x, (int)N, (int)D, dist, rmax, (double*)nullptr, (double*)nullptr);
    } else {
        const dim3 g((unsigned)((N + 15) / 16), (unsigned)((N + 15) / 16), (unsigned)L);
        if (dtype == TDA_F64)
            hipLaunchKernelGGL(k_distance<double>, g, dim3(256), 0, s, (const double*)x, (int)N, (int)D, dist, rmax);
        else
            hipLaunchKernelGGL(k_distance<float>, g, dim3(256), 0, s, (const float*)x, (int)N, (int)D, dist, rmax);
    }
}

// what both entries hand their kernels: n points per layer of the distance matrices, of which rows qrow0 .. qrow0 + nq - 1
// look for neighbours among the first p.N (the fit's own arrays stay null for the transform)
template <typename Plan>
UmapBufs umap_bufs(const SideCall& call, const Plan& p, size_t n, int n_epochs, size_t qrow0, size_t nq) {
    UmapBufs u = {};
    u.dist = call.at<const float>(p.o_dist);
    u.kd = call.at<float>(p.o_kd);
    u.ki = call.at<int32_t>(p.o_ki);
    u.eps = call.at<double>(p.o_eps);
    u.nxt = call.at<double>(p.o_nxt);
    u.nxn = call.at<double>(p.o_nxn);
    u.emb = call.at<float>(p.o_emb);
    u.ecap = p.ecap;
    u.n = (int)n;
    u.k = (int)p.k;
    u.c = (int)p.c;
    u.n_epochs = n_epochs;
    u.lstride = n * n;
    u.stride = (int)n;
    u.qrow0 = (int)qrow0;
    u.nq = (int)nq;
    u.ncand = (int)p.N;
    return u;
}

}  // namespace

extern "C" int tda_umap_batch(const tda_umap_args* a) {
    UmapPlan p;
    std::string msg;
    if (int rc = umap_plan(a, p, msg)) return fail(rc, msg);
    if (int rc = need_device(a->device)) return rc;
    SideCall call;
    if (int rc = call.open(kAuxUmap, a->device)) return rc;
    const size_t L = p.L, N = p.N;
    if (int rc = call.reserve(p.total)) return rc;
    hipStream_t s = call.stream();
    if (a->x_on_device)
        if (int rc = call.after_caller(a->stream)) return rc;
    const void* x = a->x;
    if (!a->x_on_device) {
        HIPC(hipMemcpyAsync(call.at<char>(p.o_x), a->x, L * N * p.D * p.esz, hipMemcpyHostToDevice, s));
        x = call.at<char>(p.o_x);
    }
    UmapBufs u = umap_bufs(call, p, N, a->n_epochs, 0, N);
    u.P = call.at<float>(p.o_P);
    u.S = call.at<float>(p.o_S);
    u.smax = call.at<uint32_t>(p.o_smax);
    u.head = call.at<int32_t>(p.o_head);
    u.tail = call.at<int32_t>(p.o_tail);
    u.deg = call.at<float>(p.o_deg);
    u.nedge = call.at<uint32_t>(p.o_ne);
    HIPC(hipMemsetAsync(u.P, 0, L * N * N * 4, s));
    HIPC(hipMemsetAsync(u.smax, 0, L * 4, s));
    HIPC(hipMemsetAsync(u.nedge, 0, L * 4, s));
    // distances: Gram tiles on the FP64 matrix cores (cosine always; euclidean from D >= 32, else the scalar kernel)
    umap_distances(x, a->dtype, a->metric, a->L, a->N, a->D, call.at<float>(p.o_dist), call.at<uint32_t>(p.o_rmax), s);
    HIPC(hipGetLastError());
    hipLaunchKernelGGL(k_umap_knn, dim3((unsigned)((N + kUmapKnnT - 1) / kUmapKnnT), (unsigned)L), dim3(kUmapKnnT), 0, s, u);
    HIPC(hipGetLastError());
    hipLaunchKernelGGL(k_umap_smooth, dim3((unsigned)L), dim3(kUmapT), 0, s, u);
    HIPC(hipGetLastError());
    const unsigned gs = (unsigned)std::min<uint64_t>(1024, ((uint64_t)N * N + 255) / 256);
    hipLaunchKernelGGL(k_umap_sym, dim3(gs, (unsigned)L), dim3(256), 0, s, u);
    HIPC(hipGetLastError());
    hipLaunchKernelGGL(k_umap_edges, dim3((unsigned)L), dim3(kUmapT), 0, s, u);
    HIPC(hipGetLastError());
    if (int rc = call.lds_attr((const void*)k_umap_spectral, kSideUmapLds)) return rc;
    if (int rc = call.lds_attr((const void*)k_umap_sgd, kSideUmapLds)) return rc;
    const int spec_iters = test_env("TDA_UMAP_SPEC_ITERS") ? atoi(test_env("TDA_UMAP_SPEC_ITERS")) : 300;
    hipLaunchKernelGGL(k_umap_spectral, dim3((unsigned)L), dim3(kUmapT), p.spectral ? p.spec_lds : 0, s, u, spec_iters, a->seed,
                       p.spectral ? 0 : 1);
    HIPC(hipGetLastError());
    hipLaunchKernelGGL(k_umap_sgd, dim3((unsigned)L), dim3(kUmapT), p.sgd_lds, s, u, (double)a->a, (double)a->b,
                       (double)a->learning_rate, (double)a->repulsion_strength, a->negative_sample_rate, a->seed);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(a->out, u.emb, L * N * p.c * 4, hipMemcpyDeviceToHost, s));
    if (a->graph_out) HIPC(hipMemcpyAsync(a->graph_out, u.S, L * N * N * 4, hipMemcpyDeviceToHost, s));
    std::vector<uint32_t> ne(L);
    HIPC(hipMemcpyAsync(ne.data(), u.nedge, L * 4, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    for (size_t l = 0; l < L; ++l)
        if (ne[l] > p.ecap) return fail(TDA_E_CAPACITY, "UMAP edge list overflow");
    return 0;
}

extern "C" int tda_umap_transform(const tda_umap_transform_args* a) {
    UmapTransformPlan p;
    std::string msg;
    if (int rc = umap_transform_plan(a, p, msg)) return fail(rc, msg);
    if (int rc = need_device(a->device)) return rc;
    SideCall call;
    if (int rc = call.open(kAuxUmap, a->device)) return rc;
    hipStream_t s = call.stream();
    if (a->x_on_device)
        if (int rc = call.after_caller(a->stream)) return rc;
    if (int rc = call.reserve(p.total)) return rc;
    const size_t L = p.L, M = p.M, N = p.N;
    const void* xt = a->x_train;
    const void* y = a->y;
    if (!a->x_on_device) {
        HIPC(hipMemcpyAsync(call.at<char>(p.o_xt), xt, N * p.D * p.esz, hipMemcpyHostToDevice, s));
        HIPC(hipMemcpyAsync(call.at<char>(p.o_y), y, L * M * p.D * p.esz, hipMemcpyHostToDevice, s));
        xt = call.at<char>(p.o_xt);
        y = call.at<char>(p.o_y);
    }
    HIPC(hipMemcpyAsync(call.at<char>(p.o_temb), a->emb_train, N * p.c * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_umap_concat, dim3((unsigned)std::min<uint64_t>(1024, (p.tw + p.lw + 255) / 256), (unsigned)L), dim3(256), 0, s,
                       (const uint32_t*)xt, (const uint32_t*)y, call.at<uint32_t>(p.o_z), p.tw, p.lw);
    HIPC(hipGetLastError());
    umap_distances(call.at<char>(p.o_z), a->dtype, a->metric, a->L, (int64_t)p.NM, a->D, call.at<float>(p.o_dist), call.at<uint32_t>(p.o_rmax), s);
    HIPC(hipGetLastError());
    const UmapBufs u = umap_bufs(call, p, p.NM, a->n_epochs, N, M);
    hipLaunchKernelGGL(k_umap_knn, dim3((unsigned)((M + kUmapKnnT - 1) / kUmapKnnT), (unsigned)L), dim3(kUmapKnnT), 0, s, u);
    HIPC(hipGetLastError());
    if (int rc = call.lds_attr((const void*)k_umap_transform, kSideUmapLds)) return rc;
    hipLaunchKernelGGL(k_umap_transform, dim3((unsigned)L), dim3(kUmapT), p.lds, s, u, call.at<const float>(p.o_temb), (int)N,
                       call.at<float>(p.o_val), (double)a->a, (double)a->b, (double)a->learning_rate, (double)a->repulsion_strength,
                       a->negative_sample_rate, a->seed, a->disconnection);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(a->out, u.emb, L * M * p.c * 4, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    return 0;
}
