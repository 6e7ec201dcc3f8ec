// vec_host.h -- host side of tda_landscape and tda_persistence_image
// (include/tda_dgm.h), part of rips.hip's translation unit (shares its error
// state and device checks; the plan is dgm_plan.h's VecPlan, the workspace
// aux_ws.h's).
//
// One call, the shape of the distance entries: drop the non-finite points on the
// host and sort the diagrams into size classes, upload everything in one copy,
// launch, copy the S * F values back.
//
// tda_landscape launches k_pl_tents once per non-empty size class of n (the
// diagram's finite points); a class sets the registers a lane keeps (PER = the
// class's n / 64 tents) and the launch's dynamic LDS, 16 n bytes for the class's
// largest diagram:
//   n <= 64:    PER 1,   at most  1 KiB;
//   n <= 256:   PER 4,   at most  4 KiB;
//   n <= 1024:  PER 16,  at most 16 KiB;
//   n <= 4096:  PER 64,  at most 64 KiB (two workgroups per CU).
// The values are tents, so no class can change them (vec_kernels.h).
//
// tda_persistence_image launches k_pi_image once for all diagrams: its LDS is the
// two erf tables of a chunk of points (16.8 KiB, static) whatever n is, so there
// is nothing a size class would change.
#pragma once
#include "../../include/tda_dgm.h"
#include "dgm_plan.h"
#include "vec_kernels.h"

namespace {

static_assert(kVecMaxN == TDA_VEC_MAX_POINTS && kPlMaxK == TDA_PL_MAX_DEPTH && kPiMaxPixels == TDA_PI_MAX_PIXELS,
              "tda_dgm.h and vec_kernels.h disagree");
static_assert(kVecClassN[0] == 64 && kVecClassN[1] == 256 && kVecClassN[2] == 1024 && kVecClassN[3] == kVecMaxN,
              "the classes of dgm_plan.h are the PER of k_pl_tents times 64");

// one result type for both entries: the public structs have the same layout but are distinct types
template <typename Pub>
struct VecResultImpl {
    Pub pub = {};
    std::unique_ptr<double[]> values;
    VecResultImpl(int64_t S, int64_t F) : values(new double[(size_t)std::max<int64_t>(S * F, 1)]) {
        pub.S = S;
        pub.F = F;
        pub.values = values.get();
    }
};
template <typename Pub>
void vec_free(Pub* r) {
    delete reinterpret_cast<VecResultImpl<Pub>*>(r);  // pub is the first member; NULL is a no-op
}

void pl_launch(int c, dim3 grid, size_t lds, hipStream_t s, const double* pts, const int64_t* off, const int32_t* order, const double* gridv,
               int G, int K, double* out) {
    switch (c) {
        case 0: hipLaunchKernelGGL(k_pl_tents<1>, grid, dim3(kPlThreads), lds, s, pts, off, order, gridv, G, K, out); break;
        case 1: hipLaunchKernelGGL(k_pl_tents<4>, grid, dim3(kPlThreads), lds, s, pts, off, order, gridv, G, K, out); break;
        case 2: hipLaunchKernelGGL(k_pl_tents<16>, grid, dim3(kPlThreads), lds, s, pts, off, order, gridv, G, K, out); break;
        default: hipLaunchKernelGGL(k_pl_tents<64>, grid, dim3(kPlThreads), lds, s, pts, off, order, gridv, G, K, out); break;
    }
}

}  // namespace

extern "C" int tda_landscape(const tda_pl_args* a, tda_pl_result** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    VecPlan pl;
    std::string msg;
    if (int rc = pl_plan(a, pl, msg)) return fail(rc, msg);
    if (!tda_device_ok(a->device)) return fail(TDA_E_NODEVICE, "no gfx950 device at ordinal " + std::to_string(a->device));
    const size_t S = (size_t)pl.S, G = (size_t)a->G, K = (size_t)a->K;
    std::unique_ptr<VecResultImpl<tda_pl_result>> R(new VecResultImpl<tda_pl_result>(pl.S, (int64_t)(K * G)));
    if (S == 0) {  // nothing to launch
        *out = &R.release()->pub;
        return 0;
    }

    Carve cv;
    const size_t o_pts = cv.take(pl.pts.size() * 8), o_off = cv.take(pl.off.size() * 8), o_order = cv.take(pl.order.size() * 4);
    const size_t o_grid = cv.take(G * 8);
    const size_t up_bytes = cv.o;  // the uploaded part
    const size_t o_out = cv.take(S * K * G * 8);
    std::vector<char> up(up_bytes);
    if (!pl.pts.empty()) std::memcpy(up.data() + o_pts, pl.pts.data(), pl.pts.size() * 8);
    std::memcpy(up.data() + o_off, pl.off.data(), pl.off.size() * 8);
    std::memcpy(up.data() + o_order, pl.order.data(), pl.order.size() * 4);
    std::memcpy(up.data() + o_grid, a->grid, G * 8);

    AuxWs& w = aux_ws(kAuxPl, a->device);
    std::lock_guard<std::mutex> guard(w.mu);
    if (int rc = aux_open(w, 2)) return rc;
    if (int rc = aux_lds_attr(w, (const void*)k_pl_tents<64>, pl_lds_bytes(kVecMaxN))) return rc;
    if (int rc = aux_reserve(w, cv.o)) return rc;
    hipStream_t s = w.stream;
    double* dout = (double*)(w.buf + o_out);
    HIPC(hipEventRecord(w.ev[0], s));
    HIPC(hipMemcpyAsync(w.buf, up.data(), up_bytes, hipMemcpyHostToDevice, s));
    const unsigned tiles = (unsigned)((G + kPlTile - 1) / kPlTile);
    int64_t first = 0;
    for (int c = 0; c < kVecClasses; ++c) {
        const int64_t cnt = pl.cls_cnt[c];
        if (!cnt) continue;
        pl_launch(c, dim3((unsigned)cnt, tiles), pl_lds_bytes(pl.cls_n[c]), s, (const double*)(w.buf + o_pts), (const int64_t*)(w.buf + o_off),
                  (const int32_t*)(w.buf + o_order) + first, (const double*)(w.buf + o_grid), (int)G, (int)K, dout);
        HIPC(hipGetLastError());
        first += cnt;
    }
    HIPC(hipMemcpyAsync(R->values.get(), dout, S * K * G * 8, hipMemcpyDeviceToHost, s));
    HIPC(hipEventRecord(w.ev[1], s));
    HIPC(hipStreamSynchronize(s));
    float ms = 0.0f;
    HIPC(hipEventElapsedTime(&ms, w.ev[0], w.ev[1]));
    R->pub.device_ms = ms;
    *out = &R.release()->pub;
    return 0;
}

extern "C" void tda_pl_free(tda_pl_result* r) { vec_free(r); }

extern "C" int tda_persistence_image(const tda_pi_args* a, tda_pi_result** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    VecPlan pl;
    std::string msg;
    if (int rc = pi_plan(a, pl, msg)) return fail(rc, msg);
    if (!tda_device_ok(a->device)) return fail(TDA_E_NODEVICE, "no gfx950 device at ordinal " + std::to_string(a->device));
    const size_t S = (size_t)pl.S, W = (size_t)a->W, H = (size_t)a->H;
    std::unique_ptr<VecResultImpl<tda_pi_result>> R(new VecResultImpl<tda_pi_result>(pl.S, (int64_t)(W * H)));
    if (S == 0) {  // nothing to launch
        *out = &R.release()->pub;
        return 0;
    }

    Carve cv;
    const size_t o_pts = cv.take(pl.pts.size() * 8), o_wgt = cv.take(pl.wgt.size() * 8), o_off = cv.take(pl.off.size() * 8);
    const size_t o_xe = cv.take((W + 1) * 8), o_ye = cv.take((H + 1) * 8);
    const size_t up_bytes = cv.o;  // the uploaded part
    const size_t o_out = cv.take(S * W * H * 8);
    std::vector<char> up(up_bytes);
    if (!pl.pts.empty()) {
        std::memcpy(up.data() + o_pts, pl.pts.data(), pl.pts.size() * 8);
        std::memcpy(up.data() + o_wgt, pl.wgt.data(), pl.wgt.size() * 8);
    }
    std::memcpy(up.data() + o_off, pl.off.data(), pl.off.size() * 8);
    std::memcpy(up.data() + o_xe, a->x_edges, (W + 1) * 8);
    std::memcpy(up.data() + o_ye, a->y_edges, (H + 1) * 8);
    const double r = 0.70710678118654752440 / a->sigma;  // 1 / (sigma sqrt(2)): a rounded constant, a rounded division

    AuxWs& w = aux_ws(kAuxPi, a->device);
    std::lock_guard<std::mutex> guard(w.mu);
    if (int rc = aux_open(w, 2)) return rc;
    if (int rc = aux_reserve(w, cv.o)) return rc;
    hipStream_t s = w.stream;
    double* dout = (double*)(w.buf + o_out);
    HIPC(hipEventRecord(w.ev[0], s));
    HIPC(hipMemcpyAsync(w.buf, up.data(), up_bytes, hipMemcpyHostToDevice, s));
    const unsigned tiles = (unsigned)(((W + kPiTile - 1) / kPiTile) * ((H + kPiTile - 1) / kPiTile));
    hipLaunchKernelGGL(k_pi_image, dim3((unsigned)S, tiles), dim3(kPiThreads), 0, s, (const double*)(w.buf + o_pts),
                       (const double*)(w.buf + o_wgt), (const int64_t*)(w.buf + o_off), (const double*)(w.buf + o_xe),
                       (const double*)(w.buf + o_ye), (int)W, (int)H, r, dout);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(R->values.get(), dout, S * W * H * 8, hipMemcpyDeviceToHost, s));
    HIPC(hipEventRecord(w.ev[1], s));
    HIPC(hipStreamSynchronize(s));
    float ms = 0.0f;
    HIPC(hipEventElapsedTime(&ms, w.ev[0], w.ev[1]));
    R->pub.device_ms = ms;
    *out = &R.release()->pub;
    return 0;
}

extern "C" void tda_pi_free(tda_pi_result* r) { vec_free(r); }
