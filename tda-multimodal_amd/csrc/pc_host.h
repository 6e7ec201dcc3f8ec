// pc_host.h -- host side of tda_persistence_curve (include/tda_dgm.h), part of rips.hip's
// translation unit (shares its error state and device checks; the plan is dgm_plan.h's PcPlan,
// the frame of the call dgm_call.h's, the result vec_host.h's).
//
// One call, the shape of the landscape's: keep the rows the kernel and the flags ask for, with
// their coefficients and every diagram's divisor W (pc_plan), upload everything in one copy,
// launch, copy the S * G values back.  At most two launches:
//   the plan's class 0 (n <= 64 rows): k_pc_packed, a wave per (diagram, 64 grid values), four
//                                      per workgroup;
//   the classes above it, together:    k_pc_chunked, a workgroup per (diagram, 256 grid values),
//                                      the rows in chunks of 1024 (24 KiB of static LDS).
// Both walk a diagram's rows in row order per grid value (pc_kernels.h), so which of them serves a
// diagram cannot change a bit of its values.
#pragma once
#include "../../include/tda_dgm.h"
#include "dgm_call.h"
#include "pc_kernels.h"
#include "vec_host.h"  // VecResultImpl, vec_free

namespace {

static_assert(kPcPackRows == kPcPackN && kPcRows == kPcChunk, "dgm_plan.h and pc_kernels.h disagree");

struct PcLaunch {
    const double *pts, *coef;
    const int64_t* off;
    const double *W, *grid;
    int G;
    double* out;
};

template <bool TENT, bool COEF>
void pc_launch_as(const PcLaunch& l, hipStream_t st, const int32_t* packed, int64_t n_packed, const int32_t* chunked, int64_t n_chunked) {
    if (n_packed) {
        const int tiles = (l.G + 63) / 64;
        const int64_t items = n_packed * tiles;
        hipLaunchKernelGGL((k_pc_packed<TENT, COEF>), dim3((unsigned)((items + kPcWaves - 1) / kPcWaves)), dim3(kPcThreads), 0, st, l.pts, l.coef,
                           l.off, packed, l.W, l.grid, l.G, tiles, items, l.out);
    }
    if (n_chunked)
        hipLaunchKernelGGL((k_pc_chunked<TENT, COEF>), dim3((unsigned)n_chunked, (unsigned)((l.G + kPcThreads - 1) / kPcThreads)),
                           dim3(kPcThreads), 0, st, l.pts, l.coef, l.off, chunked, l.W, l.grid, l.G, l.out);
}

}  // namespace

extern "C" int tda_persistence_curve(const tda_pc_args* a, tda_pc_result** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    PcPlan pp;
    std::string msg;
    if (int rc = pc_plan(a, pp, msg)) return fail(rc, msg);
    if (!tda_device_ok(a->device)) return fail(TDA_E_NODEVICE, "no gfx950 device at ordinal " + std::to_string(a->device));
    const VecPlan& pl = pp.v;
    const size_t S = (size_t)pl.S, G = (size_t)a->G;
    std::unique_ptr<VecResultImpl<tda_pc_result>> R(new VecResultImpl<tda_pc_result>(pl.S, (int64_t)G));
    if (S == 0) return dgm_return(R, out);  // nothing to launch

    const bool coef = a->coef != nullptr, norm = a->flags & TDA_PC_NORMALIZE;
    DgmCall call;
    const size_t o_pts = call.upload(pl.pts), o_coef = call.upload(pl.wgt), o_off = call.upload(pl.off), o_order = call.upload(pl.order);
    const size_t o_W = call.upload(pp.W), o_grid = call.upload(a->grid, G * 8);
    const size_t o_out = call.device(S * G * 8);
    if (int rc = call.begin(kAuxPc, a->device)) return rc;
    const PcLaunch l = {call.at<const double>(o_pts), coef ? call.at<const double>(o_coef) : nullptr, call.at<const int64_t>(o_off),
                        norm ? call.at<const double>(o_W) : nullptr, call.at<const double>(o_grid), (int)G, call.at<double>(o_out)};
    const int32_t* order = call.at<const int32_t>(o_order);
    const int64_t n_packed = pl.cls_cnt[0], n_chunked = pl.S - n_packed;
    const bool tent = a->kernel == TDA_PC_TENT;
    if (tent && coef) pc_launch_as<true, true>(l, call.stream(), order, n_packed, order + n_packed, n_chunked);
    else if (tent) pc_launch_as<true, false>(l, call.stream(), order, n_packed, order + n_packed, n_chunked);
    else if (coef) pc_launch_as<false, true>(l, call.stream(), order, n_packed, order + n_packed, n_chunked);
    else pc_launch_as<false, false>(l, call.stream(), order, n_packed, order + n_packed, n_chunked);
    HIPC(hipGetLastError());
    if (int rc = call.end(R->values.get(), o_out, S * G * 8)) return rc;
    return dgm_return(R, out, call.ms);
}

extern "C" void tda_pc_free(tda_pc_result* r) { vec_free(r); }
