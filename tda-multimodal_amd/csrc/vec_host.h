// vec_host.h -- host side of tda_landscape and tda_persistence_image
// (include/tda_dgm.h), part of rips.hip's translation unit (shares its error
// state and device checks; the plan is dgm_plan.h's VecPlan, the frame of the
// call dgm_call.h's).
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
#include "dgm_call.h"
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
    if (S == 0) return dgm_return(R, out);  // nothing to launch

    DgmCall call;
    const size_t o_pts = call.upload(pl.pts), o_off = call.upload(pl.off), o_order = call.upload(pl.order);
    const size_t o_grid = call.upload(a->grid, G * 8);
    const size_t o_out = call.device(S * K * G * 8);
    if (int rc = call.begin(kAuxPl, a->device, (const void*)k_pl_tents<64>, pl_lds_bytes(kVecMaxN))) return rc;
    const unsigned tiles = (unsigned)((G + kPlTile - 1) / kPlTile);
    int64_t first = 0;
    for (int c = 0; c < kVecClasses; ++c) {
        const int64_t cnt = pl.cls_cnt[c];
        if (!cnt) continue;
        pl_launch(c, dim3((unsigned)cnt, tiles), pl_lds_bytes(pl.cls_n[c]), call.stream(), call.at<const double>(o_pts),
                  call.at<const int64_t>(o_off), call.at<const int32_t>(o_order) + first, call.at<const double>(o_grid), (int)G, (int)K,
                  call.at<double>(o_out));
        HIPC(hipGetLastError());
        first += cnt;
    }
    if (int rc = call.end(R->values.get(), o_out, S * K * G * 8)) return rc;
    return dgm_return(R, out, call.ms);
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
    if (S == 0) return dgm_return(R, out);  // nothing to launch

    DgmCall call;
    const size_t o_pts = call.upload(pl.pts), o_wgt = call.upload(pl.wgt), o_off = call.upload(pl.off);
    const size_t o_xe = call.upload(a->x_edges, (W + 1) * 8), o_ye = call.upload(a->y_edges, (H + 1) * 8);
    const size_t o_out = call.device(S * W * H * 8);
    const double r = 0.70710678118654752440 / a->sigma;  // 1 / (sigma sqrt(2)): a rounded constant, a rounded division
    if (int rc = call.begin(kAuxPi, a->device)) return rc;
    const unsigned tiles = (unsigned)(((W + kPiTile - 1) / kPiTile) * ((H + kPiTile - 1) / kPiTile));
    hipLaunchKernelGGL(k_pi_image, dim3((unsigned)S, tiles), dim3(kPiThreads), 0, call.stream(), call.at<const double>(o_pts),
                       call.at<const double>(o_wgt), call.at<const int64_t>(o_off), call.at<const double>(o_xe), call.at<const double>(o_ye),
                       (int)W, (int)H, r, call.at<double>(o_out));
    HIPC(hipGetLastError());
    if (int rc = call.end(R->values.get(), o_out, S * W * H * 8)) return rc;
    return dgm_return(R, out, call.ms);
}

extern "C" void tda_pi_free(tda_pi_result* r) { vec_free(r); }
