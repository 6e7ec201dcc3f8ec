// perm_host.h -- host side of tda_permutation_test (include/tda_rips.h), part of rips.hip's
// translation unit (shares its error state and device checks).
//
// One call: everything is validated on the host first (perm_plan, side_plan.h; after which the kernels
// read in bounds by construction), then w, the group weights and the label table go up, the observed labelling as
// one more row of the table (row B), so that it is computed by the same kernel code as the null
// distribution.  The rows are served in chunks of kPermChunkRows, which keeps the tiled grid within
// 65535; S alone picks the kernel.  The B + 1 statistics come back in one copy; the count and the
// p-value are taken on the host.  The workspace, its stream and its mutex are per device and this
// entry's own (kAuxPerm, side_call.h): no slot's stream is used, nothing is captured into a graph and the
// persistence pipeline sees no allocation of this call.
#pragma once
#include "perm_kernels.h"

namespace {

constexpr size_t kPermLdsBytes = 128 * 1024;  // dynamic LDS the resident kernel may be launched with
constexpr unsigned kPermResGrid = 256;        // resident workgroups per launch at most: one per CU of an MI355X
static_assert((size_t)kPermLdsS * kPermLdsS * 8 <= kPermLdsBytes, "the resident tile fits the LDS asked for");
static_assert(kPermMaxS == TDA_PERM_MAX_S, "the tiled kernel's label words cover every supported S");
static_assert(kSidePermLdsS == kPermLdsS && kSidePermR == kPermR, "side_plan.h and perm_kernels.h disagree");

struct PermResultImpl {
    tda_perm_result pub = {};
    std::unique_ptr<double[]> stat;  // null[0 .. B-1], then T(obs)
};

}  // namespace

extern "C" int tda_permutation_test(const tda_perm_args* a, tda_perm_result** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    PermPlan p;
    std::string msg;
    if (int rc = perm_plan(a, p, msg)) return fail(rc, msg);
    if (int rc = need_device(a->device)) return rc;
    const size_t S = p.S, B = p.B, rows = p.rows;

    SideCall call;
    if (int rc = call.open(kAuxPerm, a->device, 2)) return rc;
    hipStream_t s = call.stream();
    if (p.resident)
        if (int rc = call.lds_attr((const void*)k_perm_resident, kPermLdsBytes)) return rc;
    std::unique_ptr<PermResultImpl> R(new PermResultImpl());
    R->stat.reset(new double[rows]);
    if (int rc = call.reserve(p.total)) return rc;
    const double *d_w = call.at<const double>(p.o_w), *d_c = call.at<const double>(p.o_c);
    double* d_out = call.at<double>(p.o_out);
    uint8_t* d_lab = call.at<uint8_t>(p.o_lab);
    if (int rc = call.start()) return rc;
    HIPC(hipMemcpyAsync(call.at<char>(p.o_w), a->w, S * S * 8, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(call.at<char>(p.o_c), p.cw, sizeof p.cw, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(d_lab, a->lab, B * S, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(d_lab + B * S, a->obs, S, hipMemcpyHostToDevice, s));
    for (size_t r0 = 0; r0 < rows; r0 += p.chunk) {
        const size_t rc_ = std::min(p.chunk, rows - r0);
        if (p.resident) {
            const unsigned g = (unsigned)std::min<size_t>(kPermResGrid, (rc_ + kPermResT / 64 - 1) / (kPermResT / 64));
            hipLaunchKernelGGL(k_perm_resident, dim3(g), dim3(kPermResT), S * S * 8, s, d_w, (int)S, d_lab + r0 * S, d_c, (int)rc_, d_out + r0);
        } else {
            hipLaunchKernelGGL(k_perm_tiled, dim3((unsigned)((rc_ + kPermR - 1) / kPermR)), dim3(kPermT), 0, s, d_w, (int)S, d_lab + r0 * S, d_c,
                               (int)rc_, d_out + r0);
        }
        HIPC(hipGetLastError());
    }
    HIPC(hipMemcpyAsync(R->stat.get(), d_out, rows * 8, hipMemcpyDeviceToHost, s));
    if (int rc = call.finish()) return rc;
    tda_perm_result& r = R->pub;
    r.S = a->S;
    r.B = a->B;
    r.null = R->stat.get();
    r.t_obs = r.null[B];
    for (size_t b = 0; b < B; ++b) r.count += r.null[b] <= r.t_obs;
    r.pvalue = (double)(1 + r.count) / (double)(B + 1);
    r.device = a->device;
    return side_return(R, out, call.ms);
}

extern "C" void tda_perm_free(tda_perm_result* r) { side_free<PermResultImpl>(r); }
