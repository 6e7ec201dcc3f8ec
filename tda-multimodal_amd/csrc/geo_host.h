// geo_host.h -- host side of tda_geodesic (include/tda_rips.h), part of rips.hip's translation unit.
//
// One call, the structure of tda_subsample_h0 line for line: per chunk of layers (geo_plan,
// geo_plan.h), the (Lc, N, N) f32 distance matrices (enqueue_chunk_distances), then in place on
// them the graph (k_geo_select for the kNN rows' thresholds, k_geo_graph), the closure
// (k_geo_resident, or per round k_geo_diag and the two k_geo_product launches) and the count of
// components, then the chunk's matrices back to the host.  The entry is of the resampling family:
// its frame opens on kAuxResample, so it shares tda_resample's lock, stream and workspace and the
// process gains neither a stream nor a workspace through it (no slot's stream is used, nothing is
// captured into a graph).  Every kernel's LDS is static and at most 64 KiB: no limit is raised.
#pragma once
#include "geo_kernels.h"
#include "geo_plan.h"

namespace {

static_assert(kSideGeoLdsN == kGeoLdsN && kSideGeoTile == kGeoTile && kSideGeoT == kGeoT && kSideMaxN == kGeoMaxN,
              "geo_plan.h and geo_kernels.h disagree");
static_assert((size_t)kGeoLdsN * kGeoLdsN * 4 <= 64 * 1024 && (size_t)kGeoMaxN * 4 + 64 <= 64 * 1024, "static LDS within 64 KiB");

struct GeoResultImpl {
    tda_geodesic_result pub = {};
    std::unique_ptr<float[]> dist;
    std::unique_ptr<int32_t[]> nc;
    std::unique_ptr<int64_t[]> ne;
};

}  // namespace

extern "C" int tda_geodesic(const tda_geodesic_args* a, tda_geodesic_result** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    GeoPlan p;
    std::string msg;
    if (int rc = geo_plan(a, side_ws_cap(), p, msg)) return fail(rc, msg);
    if (int rc = need_device(a->device)) return rc;
    const size_t L = p.L, N = p.N, Lc = p.sq.Lc;
    const int n = (int)N;

    SideCall call;
    if (int rc = call.open(kAuxResample, a->device, 2)) return rc;
    hipStream_t s = call.stream();
    std::unique_ptr<GeoResultImpl> R(new GeoResultImpl());
    R->dist.reset(new float[L * N * N]);
    R->nc.reset(new int32_t[L]);
    R->ne.reset(new int64_t[L]);
    if (int rc = call.reserve(p.total)) return rc;
    if (a->x_on_device)
        if (int rc = call.after_caller(a->stream)) return rc;
    unsigned long long* d_ne = call.at<unsigned long long>(p.o_ne);
    int* d_nc = call.at<int>(p.o_nc);
    uint64_t* d_thr = p.knn ? call.at<uint64_t>(p.o_thr) : nullptr;
    float* dm = call.at<float>(p.sq.o_dm);
    if (int rc = call.start()) return rc;
    HIPC(hipMemsetAsync(d_ne, 0, L * 8, s));
    HIPC(hipMemsetAsync(d_nc, 0, L * 4, s));
    const unsigned gx = (unsigned)std::min<uint64_t>(1024, ((uint64_t)N * N + kGeoT - 1) / kGeoT);
    for (size_t l0 = 0; l0 < L; l0 += Lc) {
        const size_t lc = std::min(Lc, L - l0);
        if (int rc = enqueue_chunk_distances(s, call.buf(), p.sq, (const char*)a->x + l0 * p.sq.x_layer, a->dtype, a->D, p.is_dist, lc, [] { return 0; }))
            return rc;
        if (p.knn && N >= 2) hipLaunchKernelGGL(k_geo_select, dim3((unsigned)N, (unsigned)lc), dim3(kGeoT), 0, s, dm, n, (int)p.k, d_thr);
        hipLaunchKernelGGL(k_geo_graph, dim3(gx, (unsigned)lc), dim3(kGeoT), 0, s, dm, n, d_thr, a->radius, d_ne + l0);
        if (!p.graph_only) {
            if (p.resident) {
                hipLaunchKernelGGL(k_geo_resident, dim3((unsigned)lc), dim3(kGeoT), 0, s, dm, n);
            } else {
                const unsigned nt = (unsigned)p.tiles;
                for (unsigned kb = 0; kb < nt; ++kb) {
                    hipLaunchKernelGGL(k_geo_diag, dim3((unsigned)lc), dim3(kGeoT), 0, s, dm, n, (int)kb);
                    if (nt == 1) continue;
                    hipLaunchKernelGGL((k_geo_product<false>), dim3(nt - 1, 1, (unsigned)lc), dim3(kGeoT), 0, s, dm, n, (int)kb);
                    hipLaunchKernelGGL((k_geo_product<true>), dim3(nt - 1, nt - 1, (unsigned)lc), dim3(kGeoT), 0, s, dm, n, (int)kb);
                }
            }
            hipLaunchKernelGGL(k_geo_components, dim3((unsigned)((N + 3) / 4), (unsigned)lc), dim3(kGeoT), 0, s, dm, n, d_nc + l0);
        }
        HIPC(hipGetLastError());
        // the next chunk reuses the buffer: stream order keeps this copy ahead of it
        HIPC(hipMemcpyAsync(R->dist.get() + l0 * N * N, dm, lc * N * N * 4, hipMemcpyDeviceToHost, s));
    }
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "n_edges is read back as int64");
    HIPC(hipMemcpyAsync(R->ne.get(), d_ne, L * 8, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(R->nc.get(), d_nc, L * 4, hipMemcpyDeviceToHost, s));
    if (int rc = call.finish()) return rc;
    if (p.graph_only) std::fill(R->nc.get(), R->nc.get() + L, -1);
    tda_geodesic_result& r = R->pub;
    r.L = a->L;
    r.N = a->N;
    r.dist = R->dist.get();
    r.n_components = R->nc.get();
    r.n_edges = R->ne.get();
    r.device = a->device;
    return side_return(R, out, call.ms);
}

extern "C" void tda_geodesic_free(tda_geodesic_result* r) { side_free<GeoResultImpl>(r); }
