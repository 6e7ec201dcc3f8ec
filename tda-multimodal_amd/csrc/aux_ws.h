// aux_ws.h -- the per-device workspace of the entries beside the persistence pipeline (UMAP, the
// spectral metrics, greedy landmarks, resampling, the permutation test and the eight diagram entries, which use it through dgm_call.h),
// part of rips.hip's translation unit.  Each entry has a stream, buffers and a mutex of its own: no slot's stream is used and
// nothing is captured into a graph.  The rules these entries share with the pipeline live in ws_life.h
// and are kept by calling it: a buffer grows through ws::grow (a failed growth leaves it empty) under
// ws::AllocScope (never beside a slot's graph capture).  What is stated here only:
// hipFuncSetAttribute runs once per workspace under g_attr_mu, which counts as a scope in
// ws_life.h's lock order (an entry's w.mu, then one scope).
#pragma once

namespace {

enum AuxEntry { kAuxUmap, kAuxSpectral, kAuxGreedy, kAuxResample, kAuxPerm, kAuxSw, kAuxBn, kAuxWs, kAuxPl, kAuxPi, kAuxHk, kAuxPc, kAuxPf, kAuxEntries };

struct AuxWs {
    int device = -1;
    hipStream_t stream = nullptr;
    hipEvent_t evin = nullptr;      // orders the stream after the caller's (aux_after_caller)
    hipEvent_t ev[4] = {};          // timing events (aux_events)
    ws::Buf<char> buf{ws::kDevice};
    ws::Buf<char> hout{ws::kMapped};
    std::vector<const void*> attr;  // kernels whose dynamic-LDS limit is set (aux_lds_attr)
    std::mutex mu;                  // held for the whole call
};
std::mutex g_aux_mu;
std::vector<AuxWs*> g_aux_ws[kAuxEntries];

AuxWs& aux_ws(AuxEntry entry, int dev) {
    std::lock_guard<std::mutex> g(g_aux_mu);
    for (auto* w : g_aux_ws[entry])
        if (w->device == dev) return *w;
    auto* w = new AuxWs();
    w->device = dev;
    g_aux_ws[entry].push_back(w);
    return *w;
}

// Everything below is called with w.mu held.

// the call's device, the stream (created on the first call) and the first n_events timing events
int aux_open(AuxWs& w, int n_events = 0) {
    HIPC(hipSetDevice(w.device));
    if (!w.stream) HIPC(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
    for (int i = 0; i < n_events; ++i)
        if (!w.ev[i]) HIPC(hipEventCreate(&w.ev[i]));
    return 0;
}

// device inputs: read after the caller's queued work (NULL = the null stream)
int aux_after_caller(AuxWs& w, void* caller) {
    if (!w.evin) HIPC(hipEventCreateWithFlags(&w.evin, hipEventDisableTiming));
    return order_after_caller(w.stream, w.evin, caller, w.device);
}

// At least `bytes` of w.buf, then `also()` (a call's further allocations), in one hold of the allocation scope.
template <typename Also>
int aux_reserve(AuxWs& w, size_t bytes, Also&& also) {
    ws::AllocScope lock;
    if (int rc = ws::grow(g_hip, w.buf, bytes, bytes)) return rc;
    return also();
}
int aux_reserve(AuxWs& w, size_t bytes) {
    return w.buf.cap >= bytes ? 0 : aux_reserve(w, bytes, [] { return 0; });  // the lock on growth only
}

int aux_reserve_pinned(AuxWs& w, size_t bytes) {
    if (w.hout.cap >= bytes) return 0;
    ws::AllocScope lock;
    return ws::grow(g_hip, w.hout, bytes, bytes);
}

// `fn` may be launched with up to `bytes` of dynamic LDS: set once per workspace (so once per device)
int aux_lds_attr(AuxWs& w, const void* fn, size_t bytes) {
    if (std::find(w.attr.begin(), w.attr.end(), fn) != w.attr.end()) return 0;
    std::lock_guard<std::mutex> g(g_attr_mu);
    HIPC(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    w.attr.push_back(fn);
    return 0;
}

// (an entry's buffer is cut with Carve, rips_plan.h)

}  // namespace
