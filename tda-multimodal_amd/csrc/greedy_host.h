// greedy_host.h -- host side of tda_greedy_perm (include/tda_rips.h), part of
// rips.hip's translation unit (shares its error state, device checks and the
// distance kernel selection of the persistence entry).
//
// One call: per chunk of layers (greedy_plan, side_plan.h), the (Lc, N, N) f32
// distance matrices (enqueue_chunk_distances), then k_greedy_perm (one
// workgroup per layer) and k_gather_landmarks.  The workspace, its stream and
// its mutex are per device and this entry's own (side_call.h: no slot's stream
// is used, nothing is captured into a graph).  A chunk's device bytes stay
// within TDA_GREEDY_WS_BYTES (a single layer may exceed it: N = 8192 alone
// takes 256 MiB for its matrix).
#pragma once
#include "greedy_kernels.h"

namespace {

static_assert(kSideMaxN == (int64_t)kGpMaxQ * kGpT, "side_plan.h and greedy_kernels.h disagree");

struct GreedyResultImpl {
    tda_greedy_result pub = {};
    std::unique_ptr<int64_t[]> idx;
    std::unique_ptr<float[]> lam, dperm;
    float* sub_dev = nullptr;
    ~GreedyResultImpl() {
        if (!sub_dev) return;
        ws::AllocScope lock;  // a free synchronises the device: never beside a slot's capture
        (void)hipFree(sub_dev);
    }
};

void launch_greedy_perm(hipStream_t s, const float* dm, int L, int n, int k, int64_t* idx, float* lam) {
    if (n <= kGpT) hipLaunchKernelGGL(k_greedy_perm<1>, dim3(L), dim3(kGpT), 0, s, dm, n, k, idx, lam);
    else if (n <= 2 * kGpT) hipLaunchKernelGGL(k_greedy_perm<2>, dim3(L), dim3(kGpT), 0, s, dm, n, k, idx, lam);
    else if (n <= 4 * kGpT) hipLaunchKernelGGL(k_greedy_perm<4>, dim3(L), dim3(kGpT), 0, s, dm, n, k, idx, lam);
    else hipLaunchKernelGGL(k_greedy_perm<kGpMaxQ>, dim3(L), dim3(kGpT), 0, s, dm, n, k, idx, lam);
}

}  // namespace

extern "C" int tda_greedy_perm(const tda_greedy_args* a, tda_greedy_result** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    GreedyPlan p;
    std::string msg;
    if (int rc = greedy_plan(a, side_ws_cap(), p, msg)) return fail(rc, msg);
    if (int rc = need_device(a->device)) return rc;
    const size_t L = p.L, N = p.N, k = p.k, Lc = p.sq.Lc;
    const int n = (int)N;

    SideCall call;
    if (int rc = call.open(kAuxGreedy, a->device, 4)) return rc;  // the call's two events; ev[2], ev[3]: k_greedy_perm of a chunk
    hipStream_t s = call.stream();
    std::unique_ptr<GreedyResultImpl> R(new GreedyResultImpl());
    R->idx.reset(new int64_t[L * k]);
    R->lam.reset(new float[L * k]);
    if (p.want_dp) R->dperm.reset(new float[L * k * N]);
    const auto alloc_sub = [&]() -> int {  // the result's own buffer, in the same hold of the allocation scope
        HIPC(hipMalloc((void**)&R->sub_dev, p.sub_bytes));
        return 0;
    };
    if (int rc = call.reserve(p.total, alloc_sub)) return rc;
    if (a->x_on_device)
        if (int rc = call.after_caller(a->stream)) return rc;
    int64_t* d_idx = call.at<int64_t>(p.o_idx);
    float* d_lam = call.at<float>(p.o_lam);
    float* dm = call.at<float>(p.sq.o_dm);
    float* d_dp = p.want_dp ? call.at<float>(p.o_dp) : nullptr;
    double select_ms = 0.0;
    float ms = 0.0f;
    if (int rc = call.start()) return rc;
    for (size_t l0 = 0; l0 < L; l0 += Lc) {
        const size_t lc = std::min(Lc, L - l0);
        if (int rc = enqueue_chunk_distances(s, call.buf(), p.sq, (const char*)a->x + l0 * p.sq.x_layer, a->dtype, a->D, p.is_dist, lc, [] { return 0; }))
            return rc;
        HIPC(hipEventRecord(call.event(2), s));
        launch_greedy_perm(s, dm, (int)lc, n, (int)k, d_idx + l0 * k, d_lam + l0 * k);
        HIPC(hipGetLastError());
        HIPC(hipEventRecord(call.event(3), s));
        hipLaunchKernelGGL(k_gather_landmarks, dim3((unsigned)k, (unsigned)lc), dim3(256), 0, s, dm, n, (int)k, d_idx + l0 * k,
                           R->sub_dev + l0 * k * k, d_dp);
        HIPC(hipGetLastError());
        if (p.want_dp) HIPC(hipMemcpyAsync(R->dperm.get() + l0 * k * N, d_dp, lc * k * N * 4, hipMemcpyDeviceToHost, s));
        if (l0 + lc < L) {  // the next chunk reuses the buffers and the two kernel events
            HIPC(hipStreamSynchronize(s));
            if (int rc = call.elapsed(&ms, 2, 3)) return rc;
            select_ms += ms;
        }
    }
    HIPC(hipMemcpyAsync(R->idx.get(), d_idx, L * k * 8, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(R->lam.get(), d_lam, L * k * 4, hipMemcpyDeviceToHost, s));
    if (int rc = call.drain()) return rc;
    if (int rc = call.elapsed(&ms, 2, 3)) return rc;
    select_ms += ms;
    if (int rc = call.elapsed(&call.ms)) return rc;
    tda_greedy_result& r = R->pub;
    r.L = a->L;
    r.N = a->N;
    r.n_perm = a->n_perm;
    r.idx_perm = R->idx.get();
    r.lambdas = R->lam.get();
    r.dperm2all = p.want_dp ? R->dperm.get() : nullptr;
    r.sub_dev = R->sub_dev;
    r.device = a->device;
    r.select_ms = select_ms;
    return side_return(R, out, call.ms);
}

extern "C" void tda_greedy_free(tda_greedy_result* r) { side_free<GreedyResultImpl>(r); }
