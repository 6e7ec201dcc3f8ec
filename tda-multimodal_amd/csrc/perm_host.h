// perm_host.h -- host side of tda_permutation_test (include/tda_rips.h), part of rips.hip's
// translation unit (shares its error state and device checks).
//
// One call: everything is validated on the host first (after which the kernels read in bounds by
// construction), then w, the group weights and the label table go up, the observed labelling as
// one more row of the table (row B), so that it is computed by the same kernel code as the null
// distribution.  The rows are served in chunks of kPermChunkRows, which keeps the tiled grid within
// 65535; S alone picks the kernel.  The B + 1 statistics come back in one copy; the count and the
// p-value are taken on the host.  The workspace, its stream and its mutex are per device and this
// entry's own (kAuxPerm): no slot's stream is used, nothing is captured into a graph and the
// persistence pipeline sees no allocation of this call.
#pragma once
#include "perm_kernels.h"

namespace {

constexpr size_t kPermChunkRows = (size_t)65535 * kPermR;  // rows of the table per launch (TDA_PERM_CHUNK overrides it in tests)
constexpr size_t kPermLdsBytes = 128 * 1024;               // dynamic LDS the resident kernel may be launched with
constexpr unsigned kPermResGrid = 256;                     // resident workgroups per launch at most: one per CU of an MI355X
static_assert((size_t)kPermLdsS * kPermLdsS * 8 <= kPermLdsBytes, "the resident tile fits the LDS asked for");
static_assert(kPermMaxS == TDA_PERM_MAX_S, "the tiled kernel's label words cover every supported S");

struct PermResultImpl {
    tda_perm_result pub = {};
    std::unique_ptr<double[]> stat;  // null[0 .. B-1], then T(obs)
};

// on success cw[g] = 1 / (2 n_g (n_g - 1))
int perm_validate(const tda_perm_args* a, double* cw) {
    if (!a) return fail(TDA_E_INVALID, "args is NULL");
    if (!a->w) return fail(TDA_E_INVALID, "w is NULL");
    if (!a->obs) return fail(TDA_E_INVALID, "obs is NULL");
    if (!a->lab) return fail(TDA_E_INVALID, "lab is NULL");
    if (a->S < 2) return fail(TDA_E_INVALID, "S must be >= 2");
    if (a->B < 1) return fail(TDA_E_INVALID, "B must be >= 1");
    if (a->G < 2) return fail(TDA_E_INVALID, "G must be >= 2");
    if (a->reserved != 0) return fail(TDA_E_INVALID, "reserved must be 0");
    if (a->S > TDA_PERM_MAX_S) return fail(TDA_E_UNSUPPORTED, "permutation test: S > 2048 is not supported");
    if (a->G > TDA_PERM_MAX_GROUPS) return fail(TDA_E_UNSUPPORTED, "permutation test: G > 64 is not supported");
    if ((unsigned __int128)a->B * (uint64_t)a->S > (uint64_t)TDA_PERM_MAX_TABLE)
        return fail(TDA_E_UNSUPPORTED, "permutation test: a label table of more than 2^27 entries (B * S) is not supported: split B over several calls");
    const size_t S = (size_t)a->S, B = (size_t)a->B, G = (size_t)a->G;
    auto at = [&](size_t i, size_t j) { return "w[" + std::to_string(i) + "][" + std::to_string(j) + "]"; };
    for (size_t i = 0; i < S; ++i)
        for (size_t j = 0; j < S; ++j) {
            const double v = a->w[i * S + j];
            uint64_t bits, tb;
            memcpy(&bits, &v, 8);
            if (!std::isfinite(v) || v < 0.0) return fail(TDA_E_INVALID, at(i, j) + " = " + std::to_string(v) + " is not finite and >= 0");
            if (i == j && bits != 0) return fail(TDA_E_INVALID, at(i, j) + " = " + std::to_string(v) + ": the diagonal must be +0.0");
            memcpy(&tb, &a->w[j * S + i], 8);
            if (bits != tb) return fail(TDA_E_INVALID, at(i, j) + " and " + at(j, i) + " differ: w must be symmetric bit for bit");
        }
    size_t hist[256] = {};
    for (size_t i = 0; i < S; ++i) {
        if (a->obs[i] >= G)
            return fail(TDA_E_INVALID, "obs[" + std::to_string(i) + "] = " + std::to_string((int)a->obs[i]) + " is outside [0, G = " + std::to_string(G) + ")");
        ++hist[a->obs[i]];
    }
    for (size_t g = 0; g < G; ++g)
        if (hist[g] < 2) return fail(TDA_E_INVALID, "group " + std::to_string(g) + " has " + std::to_string(hist[g]) + " members: every group needs at least 2");
    for (size_t b = 0; b < B; ++b) {
        size_t h[256] = {};
        const uint8_t* row = a->lab + b * S;
        for (size_t i = 0; i < S; ++i) ++h[row[i]];
        if (memcmp(h, hist, sizeof h))
            return fail(TDA_E_INVALID, "lab[" + std::to_string(b) + "] is not a permutation of obs (its label histogram differs)");
    }
    for (size_t g = 0; g < G; ++g) cw[g] = 1.0 / (double)(2 * hist[g] * (hist[g] - 1));  // the product is exact: one rounding
    return 0;
}

}  // namespace

extern "C" int tda_permutation_test(const tda_perm_args* a, tda_perm_result** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    double cw[TDA_PERM_MAX_GROUPS] = {};
    if (int rc = perm_validate(a, cw)) return rc;
    if (!tda_device_ok(a->device)) return fail(TDA_E_NODEVICE, "no gfx950 device at ordinal " + std::to_string(a->device));
    const size_t S = (size_t)a->S, B = (size_t)a->B, rows = B + 1;
    size_t chunk = kPermChunkRows;
    if (const char* e = test_env("TDA_PERM_CHUNK")) chunk = std::min<size_t>(kPermChunkRows, std::max<size_t>(1, strtoull(e, nullptr, 10)));
    const bool resident = S <= (size_t)kPermLdsS && !test_env_is("TDA_PERM_TILED", "1");

    AuxWs& w = aux_ws(kAuxPerm, a->device);
    std::lock_guard<std::mutex> guard(w.mu);
    if (int rc = aux_open(w, 2)) return rc;
    hipStream_t s = w.stream;
    const hipEvent_t ev0 = w.ev[0], ev1 = w.ev[1];
    if (resident)
        if (int rc = aux_lds_attr(w, (const void*)k_perm_resident, kPermLdsBytes)) return rc;
    Carve cv;
    const size_t o_w = cv.take(S * S * 8), o_c = cv.take(sizeof cw), o_out = cv.take(rows * 8), o_lab = cv.take(rows * S);
    std::unique_ptr<PermResultImpl> R(new PermResultImpl());
    R->stat.reset(new double[rows]);
    if (int rc = aux_reserve(w, cv.o)) return rc;
    const double* d_w = (const double*)(w.buf.p + o_w);
    const double* d_c = (const double*)(w.buf.p + o_c);
    double* d_out = (double*)(w.buf.p + o_out);
    uint8_t* d_lab = (uint8_t*)(w.buf.p + o_lab);
    HIPC(hipEventRecord(ev0, s));
    HIPC(hipMemcpyAsync(w.buf.p + o_w, a->w, S * S * 8, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(w.buf.p + o_c, cw, sizeof cw, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(d_lab, a->lab, B * S, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(d_lab + B * S, a->obs, S, hipMemcpyHostToDevice, s));
    for (size_t r0 = 0; r0 < rows; r0 += chunk) {
        const size_t rc_ = std::min(chunk, rows - r0);
        if (resident) {
            const unsigned g = (unsigned)std::min<size_t>(kPermResGrid, (rc_ + kPermResT / 64 - 1) / (kPermResT / 64));
            hipLaunchKernelGGL(k_perm_resident, dim3(g), dim3(kPermResT), S * S * 8, s, d_w, (int)S, d_lab + r0 * S, d_c, (int)rc_, d_out + r0);
        } else {
            hipLaunchKernelGGL(k_perm_tiled, dim3((unsigned)((rc_ + kPermR - 1) / kPermR)), dim3(kPermT), 0, s, d_w, (int)S, d_lab + r0 * S, d_c,
                               (int)rc_, d_out + r0);
        }
        HIPC(hipGetLastError());
    }
    HIPC(hipMemcpyAsync(R->stat.get(), d_out, rows * 8, hipMemcpyDeviceToHost, s));
    HIPC(hipEventRecord(ev1, s));
    HIPC(hipStreamSynchronize(s));
    float ms = 0.0f;
    HIPC(hipEventElapsedTime(&ms, ev0, ev1));
    tda_perm_result& r = R->pub;
    r.S = a->S;
    r.B = a->B;
    r.null = R->stat.get();
    r.t_obs = r.null[B];
    for (size_t b = 0; b < B; ++b) r.count += r.null[b] <= r.t_obs;
    r.pvalue = (double)(1 + r.count) / (double)(B + 1);
    r.device = a->device;
    r.device_ms = ms;
    *out = &R.release()->pub;
    return 0;
}

extern "C" void tda_perm_free(tda_perm_result* r) {
    if (!r) return;
    delete reinterpret_cast<PermResultImpl*>(r);  // pub is the first member
}
