// rips.hip -- host orchestration + C ABI (include/tda_rips.h) of the MI355X
// Vietoris-Rips persistence engine.  Built for gfx950 only:
//     hipcc --offload-arch=gfx950 -O3 -shared -fPIC rips.hip -o libtda_rips.so
//
// One call processes a batch of L layers (the reference's 32-layer sweep,
// debug_tda_pipeline.py:92-150) with ~8 + 3*maxdim kernel launches on one
// stream and a single host synchronisation at the end.
//
// The plan of a call -- which reducer and distance kernels run, every dynamic-LDS size and every
// offset into the device workspace -- is host arithmetic in rips_plan.h (HIP-free, with the
// structs and limits it shares with the kernels in rips_shapes.h; tests/test_rips_plan_cpu.py
// pins it); the launches that read it are in rips_enqueue.h.
#include <hip/hip_runtime.h>
#include <execinfo.h>
#include <link.h>
#include <signal.h>
#include <sys/syscall.h>
#include <unistd.h>
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/tda_rips.h"
#include "rips_kernels.h"
#include "rips_reduce_big.h"
#include "rips_reduce_par.h"
#include "rips_reduce_small.h"
#include "rips_retry.h"
#include "rips_plan.h"
#include "side_plan.h"
#include "ws_life.h"

using namespace tda;

namespace {

thread_local std::string g_err;

// TDA_SEGV_TRACE=1 (diagnostics): a host segfault prints the faulting thread's native frames
// (backtrace_symbols_fd: module + offset) before the default action
void segv_trace(int sig, siginfo_t* si, void*) {
    void* fr[64];
    const int nf = backtrace(fr, 64);
    char msg[128];
    const int m = snprintf(msg, sizeof msg, "[tda-segv] signal %d, address %p, thread %ld\n", sig, si ? si->si_addr : nullptr,
                           (long)syscall(SYS_gettid));
    if (m > 0) (void)!write(2, msg, (size_t)m);
    backtrace_symbols_fd(fr, nf, 2);
    signal(sig, SIG_DFL);
    raise(sig);
}
__attribute__((constructor)) void install_segv_trace() {
    const char* e = getenv("TDA_SEGV_TRACE");
    if (!e || e[0] != '1') return;
    struct sigaction sa;
    memset(&sa, 0, sizeof sa);
    sa.sa_sigaction = segv_trace;
    sa.sa_flags = SA_SIGINFO;
    sigaction(SIGSEGV, &sa, nullptr);
}

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIPC(x)                                                                                   \
    do {                                                                                          \
        hipError_t e_ = (x);                                                                      \
        if (e_ != hipSuccess) return fail(TDA_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

// The runtime of ws_life.h: each call forwarded to HIP and nothing else.  Buffers, graphs and
// captures are made and destroyed through it only (besides check_layout's probe buffer and the
// result buffer of tda_greedy_perm, which its caller owns).
struct HipRt {
    int host_alloc(void** p, size_t bytes, bool mapped) { return hipHostMalloc(p, bytes, mapped ? hipHostMallocMapped : hipHostMallocDefault); }
    int alloc(ws::Mem m, void** p, size_t bytes) { return m == ws::kDevice ? hipMalloc(p, bytes) : host_alloc(p, bytes, m == ws::kMapped); }
    int free(ws::Mem m, void* p) { return m == ws::kDevice ? hipFree(p) : hipHostFree(p); }
    int alias(void** dev, void* host) { return hipHostGetDevicePointer(dev, host, 0); }
    int begin_capture(void* s) { return hipStreamBeginCapture((hipStream_t)s, hipStreamCaptureModeThreadLocal); }
    int end_capture(void* s, void** graph) { return hipStreamEndCapture((hipStream_t)s, (hipGraph_t*)graph); }
    int instantiate(void** exec, void* graph) { return hipGraphInstantiate((hipGraphExec_t*)exec, (hipGraph_t)graph, nullptr, nullptr, 0); }
    int launch(void* exec, void* s) { return hipGraphLaunch((hipGraphExec_t)exec, (hipStream_t)s); }
    int destroy_exec(void* exec) { return hipGraphExecDestroy((hipGraphExec_t)exec); }
    int destroy_graph(void* graph) { return hipGraphDestroy((hipGraph_t)graph); }
    int record(void* ev, void* s) { return hipEventRecord((hipEvent_t)ev, (hipStream_t)s); }
    int fail(const char* call, int e) { return ::fail(TDA_E_HIP, std::string(call) + ": " + hipGetErrorString((hipError_t)e)); }
} g_hip;

// ------------------------------------------------------------------ workspace
struct Workspace {
    int device = -1;
    int slot = 0;
    bool init = false;
    hipStream_t stream = nullptr, stream2 = nullptr, stream3 = nullptr, stream4 = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, evf = nullptr, evj = nullptr, evs = nullptr, evp = nullptr, evh = nullptr, evsil = nullptr;
    // captured launch sequences; its gen() rises whenever a buffer baked into graphs moves
    ws::GraphCache graphs;
    // the buffers (ws_life.h: p, its device alias dev, cap in elements); all but hdist are baked into the graphs
    ws::Buf<char> dbuf{ws::kDevice, &graphs};
    ws::Buf<OutPair> hout{ws::kMapped, &graphs};
    ws::Buf<LayerStats> hstats{ws::kMapped, &graphs};  // k_emit writes it
    ws::Buf<int64_t> houtoff{ws::kMapped, &graphs};
    ws::Buf<char> hsil{ws::kMapped, &graphs};   // silhouette labels [S][N] i32, then scores [L][S] f64
    ws::Buf<float> htn{ws::kMapped, &graphs};   // TwoNN estimates [L] (k_twonn writes them)
    ws::Buf<char> hin{ws::kPinned, &graphs};    // staging of host inputs (stable graph source)
    ws::Buf<char> hdist{ws::kPinned};           // landing of the distance matrices (want_dist: f32, then f64)
    ws::Buf<char> xin{ws::kDevice, &graphs};    // gathered device input parts (ABI 6 x_parts)
    // sparse-cleared H2 pivot bitmap (Plan::piv2_sparse): the region known to be zero
    bool piv2_dirty = true;
    char* piv2_ptr = nullptr;
    size_t piv2_bytes = 0;
    std::vector<hipEvent_t> stage_ev;  // stage-time events (TDA_FLAG_STAGE_TIMES)
    std::vector<hipEvent_t> stage_ev2; // ... on the side stream
    std::vector<hipEvent_t> stage_ev3; // ... on the third stream
    std::vector<hipEvent_t> stage_ev4; // ... on the fourth stream
    hipEvent_t evin = nullptr;         // caller's stream -> library stream
    // the configuration a retry ended on (larger pools / another reducer), per
    // (N, maxdim, input kind): later calls of that shape start there instead of
    // failing the same way first
    struct Retry {
        int64_t N;
        int maxdim, input_kind;
        Attempt at;  // no_cap stays false: column caps are not remembered
    };
    std::vector<Retry> retry;
    // test hook (tda_debug_attempts): one record per attempt of the last entry on this slot, in
    // order, the sub-calls of a cap-miss re-run included; run_entry resets it
    struct AttemptRec {
        Attempt at;
        int errs;            // what next_attempt was given
        unsigned par_code;
        int64_t rec_used, rpool_used, bpool_used, evictions;  // ParCtl at the attempt's end; -1: not read
    };
    std::vector<AttemptRec> attempts;
    std::mutex mu;
};

// records an event after each stage when stage timing is on
struct StageTimer {
    std::vector<hipEvent_t>& ev;
    hipStream_t s;
    bool on;
    std::vector<const char*> names;
    StageTimer* fwd = nullptr;  // serial stage timing: marks go to the main stream's timer
    hipError_t rec(hipEvent_t e) { return hipEventRecord(e, s); }
    int mark(const char* name) {
        if (fwd) return fwd->mark(name);
        if (!on) return 0;
        size_t i = names.size() + 1;
        while (ev.size() <= i) {
            hipEvent_t e;
            HIPC(hipEventCreate(&e));
            ev.push_back(e);
        }
        HIPC(rec(ev[i]));
        names.push_back(name);
        return 0;
    }
    int begin() {
        if (!on || fwd) return 0;
        while (ev.empty()) {
            hipEvent_t e;
            HIPC(hipEventCreate(&e));
            ev.push_back(e);
        }
        HIPC(rec(ev[0]));
        return 0;
    }
};

// ------------------------------------------------------------------ caller streams
// Device input is read after the work the caller queued on its stream.  A NULL
// handle is the null (legacy default) stream -- what torch's default stream is
// on ROCm (raw handle 0).  Before r05 NULL meant "no ordering": a tensor that a
// torch kernel had just written on the default stream (r04's torch.cat of the
// coalesced sweeps) could be read by the library's non-blocking stream before
// that kernel ran, i.e. as stale / uninitialised memory.
//
// Distinct HIP runtimes (libamdhip64 objects, by inode) mapped in the process.
// The torch wheel ships its own copy with the same soname, so the dynamic linker
// normally maps ONE of the two; a second one (a dlmopen'ed namespace,
// RTLD_DEEPBIND) would own streams this library's runtime cannot use.
int hip_runtimes_loaded() {
    struct Acc {
        dev_t dev[8];
        ino_t ino[8];
        int n;
    } acc{};
    dl_iterate_phdr(
        [](struct dl_phdr_info* info, size_t, void* data) -> int {
            auto* a = (Acc*)data;
            const char* nm = info->dlpi_name;
            const char* base = nm ? strrchr(nm, '/') : nullptr;
            base = base ? base + 1 : nm;
            if (!base || strncmp(base, "libamdhip64", 11) != 0) return 0;
            struct stat st;
            if (stat(nm, &st) != 0) return 0;
            for (int i = 0; i < a->n; ++i)
                if (a->dev[i] == st.st_dev && a->ino[i] == st.st_ino) return 0;
            if (a->n < 8) a->dev[a->n] = st.st_dev, a->ino[a->n] = st.st_ino, ++a->n;
            return 0;
        },
        &acc);
    return acc.n;
}

// Order `lib` after the caller's stream (NULL = the null stream) with `ev`.  A
// non-NULL handle must be a stream of THIS library's HIP runtime on `dev`:
// hipStreamGetDevice validates it against the runtime's own stream set, so a
// handle from another runtime, a destroyed stream or garbage is refused with
// TDA_E_HIP instead of being dereferenced by hipEventRecord.
int order_after_caller(hipStream_t lib, hipEvent_t ev, void* caller, int dev) {
    // counted once per process (dl_iterate_phdr + stat per call cost ~10 us).  With
    // a second runtime mapped, NULL would be THIS runtime's null stream, not the caller's default
    // stream, so neither a handle nor NULL orders anything: the caller must pass the input ready
    static const int n_rt = hip_runtimes_loaded();
    if (n_rt > 1)
        return fail(TDA_E_HIP, "two HIP runtimes are loaded in this process: the caller's stream (a handle or NULL) cannot "
                               "be ordered against (pass the input ready instead, TDA_FLAG_INPUT_READY)");
    if (caller) {
        hipDevice_t d = -1;
        const hipError_t e = hipStreamGetDevice((hipStream_t)caller, &d);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(TDA_E_HIP, std::string("caller stream is not a stream of this library's HIP runtime: ") + hipGetErrorString(e));
        }
        if ((int)d != dev)
            return fail(TDA_E_INVALID, "caller stream is on device " + std::to_string((int)d) + ", the call on " + std::to_string(dev));
    }
    HIPC(hipEventRecord(ev, (hipStream_t)caller));
    HIPC(hipStreamWaitEvent(lib, ev, 0));
    return 0;
}

std::mutex g_ws_mu;
std::vector<Workspace*> g_ws;

Workspace* get_ws(int dev, int slot) {
    std::lock_guard<std::mutex> g(g_ws_mu);
    for (auto* w : g_ws)
        if (w->device == dev && w->slot == slot) return w;
    auto* w = new Workspace();
    w->device = dev;
    w->slot = slot;
    g_ws.push_back(w);
    return w;
}

// ------------------------------------------------------------------ build consistency
// hipcc compiles this file twice (device pass, then host pass minutes later) and both read the
// headers; an edit in between once gave a library whose host side packed kernel arguments
// differently from what the device side read.  The first workspace of the
// process checks the sizes of every structure that crosses the host/device boundary, as the
// device code sees them, against the host's: a skewed build fails loudly instead of faulting.
#define TDA_LAYOUT_STRUCTS(X)                                                                                     \
    X(LayerStats) X(DimBufs) X(Pair) X(PairSet) X(OutPair) X(AppBlock) X(PartList) X(SortArgs) X(Reduce2Bufs)  \
    X(Reduce2Cfg) X(ReduceAllCfg) X(SmallBufs) X(BigBufs) X(DenseBufs) X(ParCtl) X(ParBufs) X(ParLds)
#define TDA_LAYOUT_COUNT(T) +1
constexpr int kLayoutN = 0 TDA_LAYOUT_STRUCTS(TDA_LAYOUT_COUNT);
__global__ void k_layout_probe(uint32_t* out) {
    if (threadIdx.x != 0) return;
    int i = 0;
#define TDA_LAYOUT_DEV(T) out[i++] = (uint32_t)sizeof(T);
    TDA_LAYOUT_STRUCTS(TDA_LAYOUT_DEV)
#undef TDA_LAYOUT_DEV
}
int check_layout(hipStream_t s) {
    static std::mutex mu;
    static bool done = false;
    std::lock_guard<std::mutex> g(mu);
    if (done) return 0;
    uint32_t* d = nullptr;
    uint32_t h[kLayoutN] = {};
    HIPC(hipMalloc(&d, sizeof(h)));
    hipLaunchKernelGGL(k_layout_probe, dim3(1), dim3(64), 0, s, d);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(TDA_E_HIP, std::string("layout probe: ") + hipGetErrorString(e));
    static const char* names[kLayoutN] = {
#define TDA_LAYOUT_NAME(T) #T,
        TDA_LAYOUT_STRUCTS(TDA_LAYOUT_NAME)
#undef TDA_LAYOUT_NAME
    };
    const uint32_t host[kLayoutN] = {
#define TDA_LAYOUT_HOST(T) (uint32_t)sizeof(T),
        TDA_LAYOUT_STRUCTS(TDA_LAYOUT_HOST)
#undef TDA_LAYOUT_HOST
    };
    for (int i = 0; i < kLayoutN; ++i)
        if (h[i] != host[i])
            return fail(TDA_E_HIP, std::string("library build is inconsistent: sizeof(") + names[i] + ") is " + std::to_string(host[i]) +
                                       " on the host and " + std::to_string(h[i]) + " on the device (rebuild from one source tree)");
    done = true;
    return 0;
}

int ws_side_streams(Workspace& w) {
    if (w.stream2) return 0;
    HIPC(hipStreamCreateWithFlags(&w.stream2, hipStreamNonBlocking));
    HIPC(hipStreamCreateWithFlags(&w.stream3, hipStreamNonBlocking));
    HIPC(hipStreamCreateWithFlags(&w.stream4, hipStreamNonBlocking));
    return 0;
}

int ws_prepare(Workspace& w, const Plan& p) {
    if (!w.init) {
        // the side streams are created on the first multi-stream call (ws_side_streams):
        // a slot that only runs TDA_FLAG_ONE_STREAM calls holds one hardware queue
        HIPC(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
        HIPC(hipEventCreateWithFlags(&w.evh, hipEventDisableTiming));
        HIPC(hipEventCreateWithFlags(&w.evs, hipEventDisableTiming));
        HIPC(hipEventCreateWithFlags(&w.evp, hipEventDisableTiming));
        HIPC(hipEventCreateWithFlags(&w.evsil, hipEventDisableTiming));
        HIPC(hipEventCreate(&w.ev0));
        HIPC(hipEventCreate(&w.ev1));
        HIPC(hipEventCreateWithFlags(&w.evf, hipEventDisableTiming));
        HIPC(hipEventCreateWithFlags(&w.evj, hipEventDisableTiming));
        HIPC(hipEventCreateWithFlags(&w.evin, hipEventDisableTiming));
        if (int rc = check_layout(w.stream)) return rc;
        w.init = true;
    }
    if (w.dbuf.cap < p.total) w.piv2_dirty = true;
    const size_t cap = ws::want_half_more(p.total, w.dbuf.cap);
    ws::GrowStep step;
    if (int rc = ws::grow(g_hip, w.dbuf, p.total, cap, &step)) {
        if (step != ws::kGrowAlloc) return rc;
        (void)hipGetLastError();
        size_t fr = 0, tot = 0;
        (void)hipMemGetInfo(&fr, &tot);
        return fail(TDA_E_HIP, "device workspace of " + std::to_string(cap >> 20) + " MiB does not fit (free " +
                                   std::to_string(fr >> 20) + " of " + std::to_string(tot >> 20) + " MiB)");
    }
    const size_t L = (size_t)p.L;
    if (int rc = ws::grow(g_hip, w.hstats, L, L)) return rc;
    if (int rc = ws::grow(g_hip, w.houtoff, L * 4, L * 4)) return rc;
    const size_t want = ws::want_floor(L * 256, ws::kFloorStage);
    return ws::grow(g_hip, w.hout, want, want);
}

bool g_attr_done[64] = {false};
std::mutex g_attr_mu;
int set_lds_attrs(int dev) {
    std::lock_guard<std::mutex> lk(g_attr_mu);  // first calls on several workspace slots at once
    if (dev < 64 && g_attr_done[dev]) return 0;
    HIPC(hipFuncSetAttribute((const void*)k_h0<0, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    HIPC(hipFuncSetAttribute((const void*)k_h0<kH0BorWQ, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    HIPC(hipFuncSetAttribute((const void*)k_h0<kH0WaveQ, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    HIPC(hipFuncSetAttribute((const void*)k_bor_hook, hipFuncAttributeMaxDynamicSharedMemorySize, kBorHookLdsMax));
    HIPC(hipFuncSetAttribute((const void*)k_sort_resid, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    HIPC(hipFuncSetAttribute((const void*)k_emit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEmitLds));
#define TDA_ATTR_RED(LW, P1, P2) \
    HIPC(hipFuncSetAttribute((const void*)k_reduce_all<LW, P1, P2>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax))
    TDA_ATTR_RED(true, true, true);
    TDA_ATTR_RED(true, true, false);
    TDA_ATTR_RED(true, false, false);
    TDA_ATTR_RED(false, true, true);
    TDA_ATTR_RED(false, true, false);
    TDA_ATTR_RED(false, false, false);
#undef TDA_ATTR_RED
    HIPC(hipFuncSetAttribute((const void*)k_reduce_par<1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(ParLds)));
    HIPC(hipFuncSetAttribute((const void*)k_reduce_par<1, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(ParLds)));
    HIPC(hipFuncSetAttribute((const void*)k_reduce_par<2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(ParLds)));
    HIPC(hipFuncSetAttribute((const void*)k_reduce_par<2, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(ParLds)));
    HIPC(hipFuncSetAttribute((const void*)k_reduce_par<2, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(ParLds)));

    HIPC(hipFuncSetAttribute((const void*)k_h2_phase1, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    HIPC(hipFuncSetAttribute((const void*)k_edge_chunks, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEdgeSortLds));
    HIPC(hipFuncSetAttribute((const void*)k_silhouette, hipFuncAttributeMaxDynamicSharedMemorySize, kSilLdsMax));
    HIPC(hipFuncSetAttribute((const void*)k_twonn, hipFuncAttributeMaxDynamicSharedMemorySize, kTnLdsMax));
#define TDA_ATTR_CHAIN(K, F) HIPC(hipFuncSetAttribute((const void*)k_h1_chain<K, F>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    TDA_ATTR_CHAIN(1, 0) TDA_ATTR_CHAIN(2, 0) TDA_ATTR_CHAIN(3, 0) TDA_ATTR_CHAIN(4, 0) TDA_ATTR_CHAIN(6, 0)
    TDA_ATTR_CHAIN(9, 0) TDA_ATTR_CHAIN(12, 0) TDA_ATTR_CHAIN(16, 0) TDA_ATTR_CHAIN(21, 0)
    TDA_ATTR_CHAIN(1, 1) TDA_ATTR_CHAIN(2, 1) TDA_ATTR_CHAIN(3, 1) TDA_ATTR_CHAIN(4, 1) TDA_ATTR_CHAIN(6, 1)
    TDA_ATTR_CHAIN(9, 1) TDA_ATTR_CHAIN(12, 1)
    TDA_ATTR_CHAIN(1, 2) TDA_ATTR_CHAIN(2, 2) TDA_ATTR_CHAIN(3, 2) TDA_ATTR_CHAIN(4, 2) TDA_ATTR_CHAIN(6, 2)
    TDA_ATTR_CHAIN(9, 2) TDA_ATTR_CHAIN(12, 2)
#undef TDA_ATTR_CHAIN
    HIPC(hipFuncSetAttribute((const void*)k_prep_edges, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    HIPC(hipFuncSetAttribute((const void*)k_prep_tables, hipFuncAttributeMaxDynamicSharedMemorySize, (int)prep_tables_lds(kDenseMaxN)));
    HIPC(hipFuncSetAttribute((const void*)k_reduce_h2_finish, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    HIPC(hipFuncSetAttribute((const void*)k_apparent<1, false>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    HIPC(hipFuncSetAttribute((const void*)k_apparent<2, false>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    HIPC(hipFuncSetAttribute((const void*)k_apparent<1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    HIPC(hipFuncSetAttribute((const void*)k_apparent<2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    if (dev < 64) g_attr_done[dev] = true;
    return 0;
}

// result owned by the library
// The per-(layer, dim) arrays are one allocation, in the order count,
// offset, checksum, n_all_pairs, n_columns, n_residual, n_adds; birth/death
// and birth_idx/death_idx are each one allocation too (tda_rips.h).
struct ResultImpl {
    tda_rips_result pub;
    std::vector<uint64_t> blob;  // meta | num_edges | birth_idx, death_idx | thresh (padded) | birth, death
    std::vector<float> dist, stage_ms, tn;
    std::vector<double> dist64;
    std::vector<double> sil;
    std::vector<const char*> stage_name;
};

std::string err_flags(int e) {
    std::string s;
    if (e & ERR_RESID_CAP) s += " residual-column-capacity";
    if (e & ERR_PAIR_CAP) s += " pair-capacity";
    if (e & ERR_WORK_CAP) s += " working-column-capacity";
    if (e & ERR_VPOOL_CAP) s += " reduction-pool-capacity";
    if (e & ERR_OUT_CAP) s += " output-capacity";
    if (e & ERR_STEP_LIMIT) s += " reduction-step-limit";
    if (e & ERR_PAR2) s += " parallel-h2-reduction-abort";
    if (e & ERR_PAR) s += " parallel-reduction-abort";
    return s;
}

// ------------------------------------------------------------------ pipeline
// (re)point the public result at its one-allocation blob (tda_rips.h layout)
void point_result(ResultImpl& R, size_t total) {
    tda_rips_result& o = R.pub;
    const size_t S = (size_t)o.L * (o.maxdim + 1);
    const size_t o_ne = 7 * S, o_idx = o_ne + o.L, o_thr = o_idx + 2 * total, o_bd = o_thr + (o.L + 1) / 2;
    int64_t* m = (int64_t*)R.blob.data();
    o.count = m;
    o.offset = m + S;
    o.checksum = (const uint64_t*)(m + 2 * S);
    o.n_all_pairs = m + 3 * S;
    o.n_columns = m + 4 * S;
    o.n_residual = m + 5 * S;
    o.n_adds = m + 6 * S;
    o.num_edges = (const int64_t*)(R.blob.data() + o_ne);
    o.birth_idx = (const int64_t*)(R.blob.data() + o_idx);
    o.death_idx = o.birth_idx + total;
    o.thresh = (const float*)(R.blob.data() + o_thr);
    o.birth = (const float*)(R.blob.data() + o_bd);
    o.death = o.birth + total;
    o.blob = R.blob.data();
    o.blob_bytes = (int64_t)(R.blob.size() * 8);
    o.n_pairs = (int64_t)total;
}

// Layers ls[i] of R replaced by the one-layer results subs[i] (same N and maxdim): every
// per-layer block of the blob is rebuilt in layer order.  Distances, silhouettes and TwoNN
// stay R's (they do not depend on the reduction).
void splice_layers(ResultImpl& R, const std::vector<int>& ls, const std::vector<tda_rips_result*>& subs) {
    const tda_rips_result& o = R.pub;
    const int L = (int)o.L, nd = (int)o.maxdim + 1;
    std::vector<const tda_rips_result*> src((size_t)L, &o);
    std::vector<int> sl((size_t)L);
    for (int l = 0; l < L; ++l) sl[l] = l;
    for (size_t i = 0; i < ls.size(); ++i) src[ls[i]] = subs[i], sl[ls[i]] = 0;
    size_t total = 0;
    for (int l = 0; l < L; ++l)
        for (int d = 0; d < nd; ++d) total += (size_t)src[l]->count[sl[l] * nd + d];
    const size_t S = (size_t)L * nd;
    const size_t o_ne = 7 * S, o_idx = o_ne + L, o_thr = o_idx + 2 * total, o_bd = o_thr + (L + 1) / 2;
    std::vector<uint64_t> blob(o_bd + total, 0);
    int64_t* m = (int64_t*)blob.data();
    float* thr = (float*)(blob.data() + o_thr);
    int64_t* ne = (int64_t*)(blob.data() + o_ne);
    int64_t* idx = (int64_t*)(blob.data() + o_idx);
    float* bd = (float*)(blob.data() + o_bd);
    size_t e = 0;
    for (int l = 0; l < L; ++l) {
        const tda_rips_result& q = *src[l];
        const int k = sl[l];
        thr[l] = q.thresh[k];
        ne[l] = q.num_edges[k];
        for (int d = 0; d < nd; ++d) {
            const size_t a = (size_t)l * nd + d, b = (size_t)k * nd + d;
            const int64_t c = q.count[b];
            m[a] = c;
            m[S + a] = (int64_t)e;
            ((uint64_t*)m)[2 * S + a] = q.checksum[b];
            m[3 * S + a] = q.n_all_pairs[b];
            m[4 * S + a] = q.n_columns[b];
            m[5 * S + a] = q.n_residual[b];
            m[6 * S + a] = q.n_adds[b];
            const int64_t f = q.offset[b];
            for (int64_t i = 0; i < c; ++i, ++e) {
                bd[e] = q.birth[f + i];
                bd[total + e] = q.death[f + i];
                idx[e] = q.birth_idx[f + i];
                idx[total + e] = q.death_idx[f + i];
            }
        }
    }
    R.blob.swap(blob);
    point_result(R, total);
}

#include "rips_enqueue.h"
#if defined(TDA_PROFILE) || defined(TDA_PROF2)
#include "rips_prof.h"
#endif

int run_attempts(const tda_rips_args& a, int input_kind, const void* src, tda_rips_result** out, Attempt at);

// Column caps missed on some layers (ERR_CAP_MISS: a column's pivot lies above its cap -- a
// class that lives longer than capf * thresh, e.g. the one loop of a circle): each such layer is
// re-run ALONE without caps and spliced into the batch's result; the other layers keep their
// capped (exact) reductions.  A one-layer call simply re-runs without caps.
int rerun_cap_missed(const tda_rips_args& a, int input_kind, const void* host_or_dev, tda_rips_result** out, ResultImpl* R,
                     const std::vector<int>& ls, Attempt at) {
    std::unique_ptr<ResultImpl> own(R);
    at.no_cap = true;
    if (getenv("TDA_DEBUG")) fprintf(stderr, "[tda] column cap missed on %zu of %lld layers: re-run without caps\n", ls.size(), (long long)a.L);
    if (a.L == 1 || input_kind == 2) {
        const double dms = R->pub.device_ms;
        if (int rc = run_attempts(a, input_kind, host_or_dev, out, at)) return rc;
        (*out)->n_cap_reruns = a.L;
        (*out)->device_ms += dms;
        return 0;
    }
    const size_t esz = a.dtype == TDA_F64 ? 8 : 4;
    const size_t lb = (size_t)a.N * (input_kind == 1 ? (size_t)a.N : (size_t)a.D) * esz;  // bytes per layer
    const int64_t per = a.n_parts > 0 ? a.L / a.n_parts : a.L;
    std::vector<tda_rips_result*> subs;
    struct Free {
        std::vector<tda_rips_result*>& v;
        ~Free() {
            for (auto* r : v) delete reinterpret_cast<ResultImpl*>(r);
        }
    } free_subs{subs};
    double dms = R->pub.device_ms;
    for (int l : ls) {
        tda_rips_args b = a;
        const char* base = (const char*)(a.n_parts > 0 ? a.x_parts[l / per] : host_or_dev);
        b.x = base + (size_t)(a.n_parts > 0 ? l % per : l) * lb;
        b.L = 1;
        b.n_parts = 0;
        b.x_parts = nullptr;
        b.flags = (a.flags | TDA_FLAG_INPUT_READY) & ~TDA_FLAG_DIST64;  // the batch's call ordered and read it already
        b.want_dist = 0;
        b.labels = nullptr;
        b.n_label_sets = 0;
        b.want_twonn = 0;
        tda_rips_result* sub = nullptr;
        if (int rc = run_attempts(b, input_kind, b.x, &sub, at)) return rc;
        subs.push_back(sub);
        dms += sub->device_ms;
    }
    splice_layers(*R, ls, subs);
    R->pub.n_cap_reruns = (int64_t)ls.size();
    R->pub.device_ms = dms;
    *out = &own.release()->pub;
    return 0;
}

// silhouette labels: every set must be codes 0..K-1, all used, 2 <= K <= n - 1 (sklearn); sil_K: the largest K
int validate_labels(const tda_rips_args& a, int n, int nls, int& sil_K) {
    for (int q = 0; q < nls; ++q) {
        int K = 0;
        std::vector<int> f(kSilMaxK, 0);
        for (int i = 0; i < n; ++i) {
            const int32_t c = a.labels[(size_t)q * n + i];
            if (c < 0 || c >= kSilMaxK) return fail(TDA_E_INVALID, "silhouette labels must be codes 0..K-1 with K <= 32");
            ++f[c];
            K = std::max(K, c + 1);
        }
        for (int c = 0; c < K; ++c)
            if (!f[c]) return fail(TDA_E_INVALID, "silhouette labels must be contiguous codes 0..K-1 (LabelEncoder)");
        if (K < 2 || K > n - 1)
            return fail(TDA_E_INVALID, "Number of labels is " + std::to_string(K) + ". Valid values are 2 to n_samples - 1 (inclusive)");
        sil_K = std::max(sil_K, K);
    }
    return 0;
}

// The workspace sized for this call's plan and arguments, and the call's view of it.  Allocations,
// frees and graph drops (first call / growth) never overlap another slot's capture: the caller
// holds ws::AllocScope, and releases it before the input copies (the host-input memcpy
// serialised pipelined slots).
int prepare_buffers(Call& c) {
    const tda_rips_args& a = c.a;
    const Plan& p = c.p;
    Workspace& w = c.w;
    if (int rc = ws_prepare(w, p)) return rc;
    if (int rc = set_lds_attrs(a.device)) return rc;
    c.s = w.stream;
    c.B = w.dbuf.p;
    const int n = c.n = (int)p.N, L = c.L = (int)p.L;
    c.dist = (float*)(c.B + p.o_dist);
    c.stats = (LayerStats*)(c.B + p.o_stats);
    c.rowmax = (uint32_t*)(c.B + p.o_rowmax);
    c.esz = p.dtype == TDA_F64 ? 8 : 4;
    for (int d = 0; d <= p.maxdim; ++d) {
        c.ps.p[d] = (Pair*)(c.B + p.o_pairs[d]);
        c.ps.cap[d] = p.pcap[d];
    }

    // host inputs go through a pinned staging buffer: a stable graph source
    // (grown here, filled after the lock is released)
    c.xsrc = c.host_or_dev;
    c.nparts = c.input_kind == 2 ? 0 : a.n_parts;
    c.host_in = !a.x_on_device || c.input_kind == 2;
    c.dev_parts = !c.host_in && c.nparts > 0;
    c.xbytes = c.input_kind == 2 ? binom((uint64_t)n, 2) * 4
                                 : (size_t)L * n * (c.input_kind == 1 ? (size_t)n : (size_t)p.D) * c.esz;
    // want_dist: the matrices come back by an async copy queued behind the call's work (one
    // stream sync for both; r06: a blocking hipMemcpy after the sync cost ~20 us per small call)
    c.dbytes = a.want_dist ? (size_t)L * n * n * (4 + (p.want64 ? 8 : 0)) : 0;
    if (int rc = ws::grow(g_hip, w.hdist, c.dbytes, ws::want_floor(c.dbytes, ws::kFloorStage))) return rc;
    if (c.host_in) {
        if (int rc = ws::grow(g_hip, w.hin, c.xbytes, ws::want_floor(c.xbytes, ws::kFloorStage))) return rc;
        c.xsrc = w.hin.p;
    } else if (c.dev_parts) {
        if (int rc = ws::grow(g_hip, w.xin, c.xbytes, c.xbytes)) return rc;
        c.xsrc = w.xin.p;
    }

    // silhouette labels -> host-mapped buffer (stable address: a graph source)
    c.nls = (a.labels && a.n_label_sets > 0) ? (int)a.n_label_sets : 0;
    if (c.nls) {
        if (int rc = validate_labels(a, n, c.nls, c.sil_K)) return rc;
        c.sil_out_off = align_up((size_t)c.nls * n * 4, 16);
        const size_t need = c.sil_out_off + (size_t)L * c.nls * 8;
        if (int rc = ws::grow(g_hip, w.hsil, need, ws::want_floor(need, ws::kFloorSil))) return rc;
    }

    // TwoNN estimates -> host-mapped buffer (stable address: a graph source)
    c.want_tn = a.want_twonn != 0;
    c.no_ph = (a.flags & TDA_FLAG_NO_PERSISTENCE) != 0;
    if (c.want_tn)
        if (int rc = ws::grow(g_hip, w.htn, (size_t)L, ws::want_floor((size_t)L, ws::kFloorTn))) return rc;

    // TDA_FLAG_STAGE_SERIAL (with stage times) or TDA_FLAG_ONE_STREAM: every
    // stage on the main stream -- each pair of stage events then brackets one
    // kernel only, and a slot keeps to one hardware queue (several slots in
    // flight each get their own: SweepPipeline)
    c.serial_stages = ((a.flags & TDA_FLAG_STAGE_TIMES) && (a.flags & TDA_FLAG_STAGE_SERIAL)) || (a.flags & TDA_FLAG_ONE_STREAM);
    if (!c.serial_stages)
        if (int rc = ws_side_streams(w)) return rc;
    return 0;
}

// input copies and ordering, outside any lock scope
int stage_inputs(Call& c) {
    const tda_rips_args& a = c.a;
    Workspace& w = c.w;
    if (a.x_on_device && c.input_kind != 2 && !(a.flags & TDA_FLAG_INPUT_READY))
        if (int rc = order_after_caller(c.s, w.evin, a.stream, a.device)) return rc;
    if (c.host_in) {
        if (c.nparts > 0) {  // parts: one after the other into the staging buffer
            const size_t pb = c.xbytes / c.nparts;
            for (int i = 0; i < c.nparts; ++i) std::memcpy(w.hin.p + i * pb, a.x_parts[i], pb);
        } else if (c.xbytes) {
            std::memcpy(w.hin.p, c.host_or_dev, c.xbytes);
        }
    } else if (c.dev_parts) {
        // device parts: gathered into the workspace's own input buffer by one kernel on the
        // library stream (ordered after the caller's stream above, outside any captured graph)
        PartList pl = {};
        for (int i = 0; i < c.nparts; ++i) pl.p[i] = a.x_parts[i];
        const uint64_t words = c.xbytes / c.nparts / 4;
        const unsigned gx = (unsigned)std::min<uint64_t>(64, (words + 255) / 256);
        hipLaunchKernelGGL(k_gather_parts, dim3(std::max(1u, gx), c.nparts), dim3(256), 0, c.s, pl, words, (uint32_t*)w.xin.p);
        HIPC(hipGetLastError());
    }
    if (c.nls) std::memcpy(w.hsil.p, a.labels, (size_t)c.nls * c.n * 4);
    return 0;
}

// serial_stages: the side streams are aliased to the main one for the call and restored on return
struct StreamSwap {
    Workspace& w;
    hipStream_t s2, s3, s4;
    bool on;
    ~StreamSwap() {
        if (on) w.stream2 = s2, w.stream3 = s3, w.stream4 = s4;
    }
};

// what a captured launch sequence depends on; also settles the two switches that are part of it
void fill_graph_key(Call& c, ws::GraphKey& key) {
    const tda_rips_args& a = c.a;
    const Plan& p = c.p;
    c.dist_mfma = p.dist.mfma;
    // column caps only with ripser's default threshold (the enclosing radius: no essential
    // H1 / H2 class); a finite user threshold can leave classes essential (k_reduce_par)
    // caps also off when H2 runs on the serial k_reduce_big after a parallel H1 (TDA_PAR2=0, or an H2
    // abort): that kernel reads every layer's H1 pivots, so no layer's H1 may be left unfinished
    const bool h2_serial = p.par && p.maxdim >= 2 && !p.par2;
    c.capf = (c.at.no_cap || h2_serial || !(std::isinf(a.thresh) || a.thresh == 3.402823466e+38f)) ? 0.0f : par_capf();
    ws::make_key(key, [&](ws::GraphKey& gk) {
        gk.L = p.L;
        gk.N = p.N;
        gk.D = p.D;
        gk.maxdim = p.maxdim;
        gk.dtype = p.dtype;
        gk.input_kind = c.input_kind;
        gk.x_on_device = a.x_on_device;
        gk.flags = a.flags;
        gk.force_global = c.at.force_global;
        gk.scale = c.at.scale;
        gk.force_big = c.at.force_big;
        gk.no_par = c.at.no_par;
        gk.no_cap = c.at.no_cap;
        gk.capf = c.capf;
        gk.variant = (p.dense ? 1 : 0) | (p.big ? 2 : 0) | (p.fast ? 4 : 0) | (p.lds_mode ? 8 : 0) | (p.cmode << 4) | (p.par ? 1 << 8 : 0) | (c.dist_mfma ? 1 << 9 : 0) |
                     (p.wide ? 1 << 10 : 0) | (p.want64 ? 1 << 11 : 0) | (p.par2 ? 1 << 12 : 0) | (p.piv2_sparse ? 1 << 13 : 0) |
                     (p.dist.gram_layer ? 1 << 14 : 0);
        gk.dsplit = p.dist.dsplit;
        gk.pool_shift = p.par ? par_pool_shift() : 0;
        gk.par_steps[0] = p.par ? par_step_limit(1) : 0;
        gk.par_steps[1] = p.par2 ? par_step_limit(2) : 0;
        gk.thresh = a.thresh;
        gk.n_label_sets = c.nls;
        gk.sil_K = c.sil_K;  // baked into the k_silhouette launch (argument K and its LDS size)
        gk.twonn = c.want_tn;
        gk.tn_discard = c.want_tn ? a.twonn_discard : 0.0;
        gk.tn_eps = c.want_tn ? a.twonn_eps : 0.0f;
        gk.x = c.xsrc;
        gk.gen = c.w.graphs.gen();
    });
}

// The call's launch sequence on the device: a replay of the graph captured for this key, else a
// capture (instantiated, kept and launched), else -- stage-timed calls, TDA_GRAPH=0 -- eagerly.
int launch_or_capture(Call& c, const ws::GraphKey& gk) {
    // stage-timed calls run eagerly: timing events inside a capture need
    // external event nodes, which torch's bundled HIP runtime rejects
    const bool use_graph = !test_env_is("TDA_GRAPH", "0") && !c.tm.on;
    return ws::launch(g_hip, c.w.graphs, gk, use_graph, c.s, c.w.ev0, c.w.ev1, [&](bool capture) {
        c.capture = capture;
        return enqueue_schedule(c);
    });
}

// After the call's synchronisation: the layers' error flags OR-ed (without ERR_CAP_MISS).  An
// output overflow alone (ERR_OUT_CAP) is mended here: the pair buffer grows and k_emit runs again.
int collect_errors(Call& c, int& errs) {
    const Plan& p = c.p;
    Workspace& w = c.w;
    const int L = c.L;
    errs = 0;
    for (int l = 0; l < L; ++l) errs |= w.hstats.p[l].err & ~ERR_CAP_MISS;
    if (p.piv2_sparse) {  // clean again unless a layer's word list overflowed
        bool over = false;
        for (int l = 0; l < L; ++l) over |= (uint64_t)w.hstats.p[l].n_clr2 > p.clr_cap;
        // only k_apparent<2> lists the words it sets: when H2 was reduced by k_reduce_big<2>
        // (TDA_PAR2=0, or no_par >= 1 after a k_reduce_par abort) that kernel also set residual-pivot
        // bits nobody listed, so the next call must start from a full memset
        w.piv2_dirty = over || !p.par2;
    }
    if (errs == ERR_OUT_CAP) {
        size_t need = 0;
        for (int l = 0; l < L; ++l)
            for (int d = 0; d <= p.maxdim; ++d) need += (size_t)std::min<uint64_t>(w.hstats.p[l].count[d], p.pcap[d]);
        {
            ws::AllocScope lock;
            if (int rc = ws::grow(g_hip, w.hout, need + 16, ws::want_double(need + 16, w.hout.cap))) return rc;
        }
        for (int l = 0; l < L; ++l) w.hstats.p[l].err = 0;
        HIPC(hipMemcpyAsync(c.stats, w.hstats.p, sizeof(LayerStats) * L, hipMemcpyHostToDevice, c.s));
        launch_k_emit(c);
        HIPC(hipGetLastError());
        HIPC(hipStreamSynchronize(c.s));
        errs = 0;
        for (int l = 0; l < L; ++l) errs |= w.hstats.p[l].err & ~ERR_CAP_MISS;
    }
    return 0;
}

// what follows from the call's error flags (next_attempt, rips_retry.h); a failure sets the message
int decide_retry(Call& c, int errs, RetryStep& step) {
    step = {RetryStep::kDone, c.at};
    ParCtl ctl = {};
    const bool par_err = (errs & (ERR_PAR | ERR_PAR2)) != 0;
    // TDA_DEBUG: the pools a clean parallel reduction drew too (of its last launch: k_par_init zeroes them)
    const bool read_ctl = par_err || (c.p.par && getenv("TDA_DEBUG"));
    if (read_ctl) {
        HIPC(hipMemcpy(&ctl, c.B + c.p.o_pctl, sizeof(ctl), hipMemcpyDeviceToHost));
        if (getenv("TDA_DEBUG"))
            fprintf(stderr, "[tda] k_reduce_par %s: code %llu, evictions %llu, records %llu, pools %llu / %llu keys\n",
                    par_err ? "aborted" : "done", ctl.err, ctl.evictions, ctl.rec_used, ctl.rpool_used, ctl.bpool_used);
    }
    const unsigned code = par_err ? (unsigned)(ctl.err & 0xFFFF) : 0u;
    if (read_ctl)
        c.w.attempts.push_back({c.at, errs, code, (int64_t)ctl.rec_used, (int64_t)ctl.rpool_used, (int64_t)ctl.bpool_used, (int64_t)ctl.evictions});
    else
        c.w.attempts.push_back({c.at, errs, code, -1, -1, -1, -1});
    if (!errs) return 0;
    step = next_attempt(errs, code, c.at, c.p.big, test_env_is("TDA_PAR_STRICT", "1"), test_env_is("TDA_REDUCE", "wave"));
    if (step.what != RetryStep::kFail) return 0;
    if (errs & (ERR_PAR | ERR_PAR2))
        return fail(TDA_E_CAPACITY, "k_reduce_par aborted: item " + std::to_string(ctl.err >> 16) + " code " + std::to_string(code));
    return fail(TDA_E_CAPACITY, "device work buffer overflow:" + err_flags(errs));
}

// remember what this shape needed (capacity / reducer retries; column caps are not
// remembered: a cap miss re-runs only its own layers, and every call starts capped)
void remember_retry(Call& c) {
    const Attempt& at = c.at;
    if (!(at.force_global || at.scale || at.force_big || at.no_par)) return;
    for (auto& m : c.w.retry)
        if (m.N == c.p.N && m.maxdim == c.p.maxdim && m.input_kind == c.input_kind) {
            m.at.force_global = m.at.force_global || at.force_global;
            m.at.force_big = m.at.force_big || at.force_big;
            m.at.no_par = std::max(m.at.no_par, at.no_par);
            m.at.scale = std::max(m.at.scale, at.scale);
            return;
        }
    Attempt kept = at;
    kept.no_cap = false;
    c.w.retry.push_back({c.p.N, c.p.maxdim, c.input_kind, kept});
}

// ---- result: one allocation (tda_rips.h layout guarantee): a binding copies it in one read
ResultImpl* build_result(Call& c) {
    const tda_rips_args& a = c.a;
    const Plan& p = c.p;
    Workspace& w = c.w;
    const int n = c.n, L = c.L;
    auto* R = new ResultImpl();
    const int nd = p.maxdim + 1;
    const size_t S = (size_t)L * nd;
    size_t total = 0;
    for (int l = 0; l < L; ++l)
        for (int d = 0; d < nd; ++d) total += (size_t)std::min<int64_t>(w.hstats.p[l].count[d], (int64_t)p.pcap[d]);
    const size_t o_ne = 7 * S, o_idx = o_ne + L, o_thr = o_idx + 2 * total, o_bd = o_thr + (L + 1) / 2;
    R->blob.assign(o_bd + total, 0);
    int64_t* m_count = (int64_t*)R->blob.data();
    int64_t* m_off = m_count + S;
    uint64_t* m_cs = (uint64_t*)(m_count + 2 * S);
    int64_t* m_all = m_count + 3 * S;
    int64_t* m_cols = m_count + 4 * S;
    int64_t* m_res = m_count + 5 * S;
    int64_t* m_add = m_count + 6 * S;
    float* r_thr = (float*)(R->blob.data() + o_thr);
    int64_t* r_ne = (int64_t*)(R->blob.data() + o_ne);
    int64_t* r_idx = (int64_t*)(R->blob.data() + o_idx);
    float* r_bd = (float*)(R->blob.data() + o_bd);
    // layer-major result (tda_rips.h); the device wrote each (layer, dim) segment
    // at houtoff, in layer order (k_emit)
    size_t e = 0;
    for (int l = 0; l < L; ++l) {
        const LayerStats& st = w.hstats.p[l];
        r_thr[l] = st.thresh;
        r_ne[l] = st.num_edges;
        for (int d = 0; d < nd; ++d) {
            const size_t cnt = (size_t)std::min<int64_t>(st.count[d], (int64_t)p.pcap[d]);
            m_count[l * nd + d] = (int64_t)cnt;
            m_off[l * nd + d] = (int64_t)e;
            m_cs[l * nd + d] = st.checksum[d];
            m_all[l * nd + d] = st.all_pairs[d];
            m_cols[l * nd + d] = st.n_columns[d];
            m_res[l * nd + d] = st.n_residual[d] - st.nskip[d];
            m_add[l * nd + d] = st.n_adds[d];
            const size_t src = (size_t)w.houtoff.p[l * nd + d];
            for (size_t i = 0; i < cnt; ++i, ++e) {
                const OutPair q = w.hout.p[src + i];
                r_bd[e] = q.birth;
                r_bd[total + e] = q.death;
                r_idx[e] = q.birth_idx;
                r_idx[total + e] = q.death_idx;
            }
        }
    }
    tda_rips_result& o = R->pub;
    o.L = L;
    o.maxdim = p.maxdim;
    o.N = n;
    point_result(*R, total);
    if (a.want_dist) {  // landed by the async copies behind the call (synchronised by the caller)
        R->dist.resize((size_t)L * n * n);
        std::memcpy(R->dist.data(), w.hdist.p, sizeof(float) * L * n * n);
    }
    if (p.want64) {
        R->dist64.resize((size_t)L * n * n);
        std::memcpy(R->dist64.data(), w.hdist.p + sizeof(float) * L * n * n, sizeof(double) * L * n * n);
    }
    o.dist = a.want_dist ? R->dist.data() : nullptr;
    o.dist64 = p.want64 ? R->dist64.data() : nullptr;
    o.silhouette = nullptr;
    if (c.nls) {
        R->sil.assign((const double*)(w.hsil.p + c.sil_out_off), (const double*)(w.hsil.p + c.sil_out_off) + (size_t)L * c.nls);
        o.silhouette = R->sil.data();
    }
    o.twonn = nullptr;
    if (c.want_tn) {
        R->tn.assign(w.htn.p, w.htn.p + L);
        o.twonn = R->tn.data();
    }
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, w.ev0, w.ev1);
    o.device_ms = ms;
    // stage times: main stream, then stream2 (edge classes), stream4 (H0), stream3 (H2 columns, phase 1)
    for (const StageTimer* t : {&c.tm, &c.tm2, &c.tm4, &c.tm3})
        for (size_t i = 0; i < t->names.size(); ++i) {
            float ts = 0.0f;
            (void)hipEventElapsedTime(&ts, t->ev[i], t->ev[i + 1]);
            R->stage_ms.push_back(ts);
            R->stage_name.push_back(t->names[i]);
        }
    o.n_stages = (int32_t)R->stage_name.size();
    o.stage_name = R->stage_name.data();
    o.stage_ms = R->stage_ms.data();
    o.n_cap_reruns = 0;
    return R;
}

// TDA_HOST_PROF=1: host-side time of the call's parts (stderr, every 200 calls)
struct HostProf {
    using clk = std::chrono::steady_clock;
    clk::time_point entry, h0, h1, h2;
    void add(float device_ms) const {
        static double acc[5] = {0, 0, 0, 0, 0};
        static int calls = 0;
        const auto h3 = clk::now();
        auto us = [](clk::duration d) { return std::chrono::duration<double, std::micro>(d).count(); };
        acc[0] += us(h1 - h0);
        acc[1] += us(h2 - h1);
        acc[2] += us(h3 - h2);
        acc[3] += device_ms * 1e3;
        acc[4] += us(h0 - entry);
        if (++calls % 200 == 0) {
            fprintf(stderr, "[tda-host] per call: setup %.1f us, launch %.1f us, sync %.1f us (device %.1f us), result %.1f us\n",
                    acc[4] / 200, acc[0] / 200, acc[1] / 200, acc[3] / 200, acc[2] / 200);
            acc[0] = acc[1] = acc[2] = acc[3] = acc[4] = 0;
        }
    }
};

bool getenv_is(const char* name, const char* val) {
    const char* m = getenv(name);
    return m && !strcmp(m, val);
}

// One attempt of a call with the configuration `at`: plan, buffers, inputs, the launch sequence,
// one synchronisation, then either the result (*out) or, in `step`, the attempt to run next.
int run_pipeline(const tda_rips_args& a, int input_kind, const void* host_or_dev, tda_rips_result** out, const Attempt& at,
                 RetryStep& step) {
    HostProf hp;
    hp.entry = HostProf::clk::now();
    HIPC(hipSetDevice(a.device));
    Workspace& w = *get_ws(a.device, a.slot);
    std::unique_lock<std::mutex> guard(w.mu);  // released on return: a retry or a cap-miss re-run takes it again
    Call c(a, input_kind, host_or_dev, at, w);
    c.p = make_plan(a.L, a.N, a.D, a.maxdim, a.dtype, input_kind != 0,
                    input_kind == 0 && a.dtype == TDA_F64 && a.want_dist && (a.flags & TDA_FLAG_DIST64), at);
    const Plan& p = c.p;
    {
        ws::AllocScope lock;  // buffers in place; a capture re-takes it
        if (int rc = prepare_buffers(c)) return rc;
    }
    if (int rc = stage_inputs(c)) return rc;
    hipStream_t s = c.s;
    const int n = c.n, L = c.L;

    StreamSwap swap_guard{w, w.stream2, w.stream3, w.stream4, c.serial_stages};
    if (c.serial_stages) w.stream2 = w.stream3 = w.stream4 = s;
    c.tm.s = s, c.tm2.s = w.stream2, c.tm3.s = w.stream3, c.tm4.s = w.stream4;
    c.tm.on = c.tm2.on = c.tm3.on = c.tm4.on = (a.flags & TDA_FLAG_STAGE_TIMES) != 0;
    if (c.serial_stages) c.tm2.fwd = c.tm3.fwd = c.tm4.fwd = &c.tm;
    ws::GraphKey gk;
    fill_graph_key(c, gk);

    static const bool host_prof = getenv_is("TDA_HOST_PROF", "1");
    hp.h0 = HostProf::clk::now();
    if (p.piv2_sparse) {  // first use of the region, or the last call left it dirty: one full memset
        char* pv2 = c.B + p.o_piv[2];
        const size_t bytes = (size_t)L * p.piv_words[2] * 4;
        if (w.piv2_dirty || w.piv2_ptr != pv2 || w.piv2_bytes < bytes) {
            HIPC(hipMemsetAsync(pv2, 0, bytes, s));
            w.piv2_ptr = pv2;
            w.piv2_bytes = bytes;
        }
        w.piv2_dirty = true;  // until this call has cleared the words it set
    } else {
        // a plan without the sparse bitmap carves other buffers over the region a sparse plan left
        // zero: the next sparse call on this slot starts from a full memset (the same address and
        // size alone do not show it)
        w.piv2_dirty = true;
    }
    if (int rc = launch_or_capture(c, gk)) return rc;
    if (a.want_dist) {
        HIPC(hipMemcpyAsync(w.hdist.p, c.dist, sizeof(float) * L * n * n, hipMemcpyDeviceToHost, s));
        if (p.want64) HIPC(hipMemcpyAsync(w.hdist.p + sizeof(float) * L * n * n, c.B + p.o_d64, sizeof(double) * L * n * n, hipMemcpyDeviceToHost, s));
    }
    hp.h1 = HostProf::clk::now();
    // (an event sync or a busy-polled end event measured the same for one call at a time, r02; and
    // for six pipelined slots, hipStreamQuery polled in a loop: 697-701 vs 540-727 K layers/s, r06)
    HIPC(hipStreamSynchronize(s));
    hp.h2 = HostProf::clk::now();

    int errs = 0;
    if (int rc = collect_errors(c, errs)) return rc;
    if (errs && getenv("TDA_DEBUG"))
        fprintf(stderr, "[tda] N=%d L=%d errs=%s force_global=%d scale=%d\n", n, L, err_flags(errs).c_str(), (int)at.force_global, at.scale);
    if (int rc = decide_retry(c, errs, step)) return rc;
    if (step.what == RetryStep::kRetry) return 0;  // run_attempts runs step.next
#ifdef TDA_PROF2
    if (int rc = print_prof2(c)) return rc;
#endif
#ifdef TDA_PROFILE
    if (int rc = print_profile(c)) return rc;
#endif
    remember_retry(c);
    std::vector<int> cap_miss;  // layers whose capped reduction missed (ERR_CAP_MISS): re-run below without caps
    for (int l = 0; l < L; ++l)
        if (w.hstats.p[l].err & ERR_CAP_MISS) cap_miss.push_back(l);
    ResultImpl* R = build_result(c);
    if (host_prof) hp.add(R->pub.device_ms);
    if (!cap_miss.empty()) {
        guard.unlock();
        return rerun_cap_missed(a, input_kind, host_or_dev, out, R, cap_miss, at);
    }
    *out = &R->pub;
    return 0;
}

// the call, attempt after attempt (the workspace mutex is free between two), until the ladder
// says done or fail
int run_attempts(const tda_rips_args& a, int input_kind, const void* src, tda_rips_result** out, Attempt at) {
    for (;;) {
        RetryStep step = {RetryStep::kDone, at};
        if (int rc = run_pipeline(a, input_kind, src, out, at, step)) return rc;
        if (step.what != RetryStep::kRetry) return 0;
        at = step.next;
    }
}

// entry: start from the configuration an earlier call of this shape ended on
int run_entry(const tda_rips_args& a, int input_kind, const void* src, tda_rips_result** out) {
    Attempt at;
    {
        Workspace& w = *get_ws(a.device, a.slot);
        std::lock_guard<std::mutex> g(w.mu);
        w.attempts.clear();
    }
    // not when a test forces a reducer (the memo would override what it asks for)
    if (!test_env_is("TDA_RETRY_MEMO", "0") && !test_env("TDA_REDUCE") && !test_env("TDA_PAR") && !test_env("TDA_PAR_STRICT") &&
        !test_env("TDA_CHAIN")) {
        Workspace& w = *get_ws(a.device, a.slot);
        std::lock_guard<std::mutex> g(w.mu);
        for (const auto& m : w.retry)
            if (m.N == a.N && m.maxdim == a.maxdim && m.input_kind == input_kind) at = m.at;
    }
    return run_attempts(a, input_kind, src, out, at);
}

int validate(const tda_rips_args* a) {
    if (!a) return fail(TDA_E_INVALID, "args is NULL");
    if (a->n_parts < 0 || a->n_parts > TDA_MAX_PARTS) return fail(TDA_E_INVALID, "n_parts must be in [0, TDA_MAX_PARTS]");
    if (a->n_parts > 0) {
        if (!a->x_parts) return fail(TDA_E_INVALID, "x_parts is NULL");
        for (int i = 0; i < a->n_parts; ++i)
            if (!a->x_parts[i]) return fail(TDA_E_INVALID, "x_parts[" + std::to_string(i) + "] is NULL");
        if (a->L % a->n_parts) return fail(TDA_E_INVALID, "L must be a multiple of n_parts");
    } else if (!a->x && a->L * a->N > 0) {
        return fail(TDA_E_INVALID, "x is NULL");
    }
    if (a->L < 1) return fail(TDA_E_INVALID, "L must be >= 1");
    if (a->N < 1) return fail(TDA_E_INVALID, "N must be >= 1");
    if (!a->is_dist && a->D < 1) return fail(TDA_E_INVALID, "D must be >= 1");
    if (a->dtype != TDA_F32 && a->dtype != TDA_F64) return fail(TDA_E_INVALID, "dtype must be TDA_F32 or TDA_F64");
    if (a->modulus != 2) return fail(TDA_E_UNSUPPORTED, "only coeff=2 (Z/2) is supported");
    if (a->maxdim < 0 || a->maxdim > 2) return fail(TDA_E_UNSUPPORTED, "maxdim must be 0, 1 or 2");
    if (a->N > 8192) return fail(TDA_E_UNSUPPORTED, "N > 8192 is not supported");
    if (a->slot < 0 || a->slot >= TDA_MAX_SLOTS) return fail(TDA_E_INVALID, "slot must be in [0, TDA_MAX_SLOTS)");
    // H1 filtration keys pack a 32-bit row-simplex index: C(N, 3) < 2^32.  H2
    // above N = 568 uses edge-code keys (21-bit code + 42-bit index): C(N, 2) < 2^21
    if (a->maxdim == 1 && a->N > 2900) return fail(TDA_E_UNSUPPORTED, "maxdim=1 requires N <= 2900");
    if (a->maxdim == 2 && a->N > 2048) return fail(TDA_E_UNSUPPORTED, "maxdim=2 requires N <= 2048");
    if (std::isnan(a->thresh)) return fail(TDA_E_INVALID, "thresh is NaN");
    if ((a->flags & TDA_FLAG_NO_PERSISTENCE) && a->maxdim != 0) return fail(TDA_E_INVALID, "TDA_FLAG_NO_PERSISTENCE needs maxdim 0");
    if (a->want_twonn && !(a->twonn_discard >= 0.0 && a->twonn_discard < 1.0 && a->twonn_eps >= 0.0f))
        return fail(TDA_E_INVALID, "TwoNN needs 0 <= discard_fraction < 1 and eps >= 0");
    return 0;
}

}  // namespace

extern "C" {

int tda_rips_batch(const tda_rips_args* args, tda_rips_result** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    if (int rc = validate(args)) return rc;
    if (!tda_device_ok(args->device)) return fail(TDA_E_NODEVICE, "no gfx950 device at ordinal " + std::to_string(args->device));
    return run_entry(*args, args->is_dist ? 1 : 0, args->x, out);
}

int tda_rips_dm(const float* D, int64_t n_entries, int32_t modulus, int32_t dim_max, float threshold, int32_t do_cocycles,
                tda_rips_result** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    if (do_cocycles) return fail(TDA_E_UNSUPPORTED, "do_cocycles is not supported");
    if (n_entries < 0 || (n_entries > 0 && !D)) return fail(TDA_E_INVALID, "bad condensed distance vector");
    // ripser.cpp compressed_distance_matrix: rows = (1 + sqrt(1 + 8 n)) / 2
    int64_t N = (int64_t)((1.0 + std::sqrt(1.0 + 8.0 * (double)n_entries)) / 2.0);
    if (N * (N - 1) / 2 != n_entries) return fail(TDA_E_INVALID, "n_entries is not N(N-1)/2");
    tda_rips_args a;
    std::memset(&a, 0, sizeof(a));
    a.x = D;
    a.dtype = TDA_F32;
    a.L = 1;
    a.N = N;
    a.D = 0;
    a.is_dist = 1;
    a.maxdim = dim_max;
    a.thresh = threshold;
    a.modulus = modulus;
    a.device = 0;
    if (int rc = validate(&a)) return rc;
    if (!tda_device_ok(0)) return fail(TDA_E_NODEVICE, "no gfx950 device");
    return run_entry(a, 2, D, out);
}

void tda_rips_free(tda_rips_result* r) {
    if (!r) return;
    delete reinterpret_cast<ResultImpl*>(r);  // pub is the first member
}

const char* tda_last_error(void) { return g_err.c_str(); }

int tda_version(void) { return TDA_RIPS_ABI_VERSION; }

// test hook: the kernels dist_select() picks for (N, D, dtype) points under the current
// environment (the TDA_TEST_OVERRIDES gate included); host only, no device
int tda_debug_dist_plan(int64_t N, int64_t D, int32_t dtype, int32_t* mfma, int32_t* dsplit, int32_t* gram_layer) {
    if (N < 1 || D < 0 || (dtype != TDA_F32 && dtype != TDA_F64) || !mfma || !dsplit || !gram_layer)
        return fail(TDA_E_INVALID, "tda_debug_dist_plan: bad arguments");
    const DistSel s = dist_select((uint64_t)N, D, dtype, false);
    *mfma = s.mfma ? 1 : 0;
    *dsplit = s.dsplit;
    *gram_layer = s.gram_layer ? 1 : 0;
    return 0;
}

// test hook: the attempts the last tda_rips_batch / tda_rips_dm entry on (device, slot) ran, in order
// (cap-miss sub-calls appended): kAttemptFields int64 per attempt -- force_global, scale, force_big,
// no_par, no_cap, errs, par_code (what next_attempt was given), then rec_used, rpool_used, bpool_used,
// evictions of ParCtl where it was read (after an abort, or under TDA_DEBUG), else -1
int tda_debug_attempts(int32_t device, int32_t slot, int64_t* out, int32_t cap) {
    constexpr int kAttemptFields = TDA_ATTEMPT_FIELDS;
    if (device < 0 || slot < 0 || slot >= TDA_MAX_SLOTS || cap < 0 || (cap > 0 && !out)) return fail(TDA_E_INVALID, "tda_debug_attempts: bad arguments");
    Workspace& w = *get_ws(device, slot);
    std::lock_guard<std::mutex> g(w.mu);
    const int n = (int)w.attempts.size();
    for (int i = 0; i < n && (i + 1) * kAttemptFields <= cap; ++i) {
        const Workspace::AttemptRec& r = w.attempts[i];
        const int64_t v[kAttemptFields] = {r.at.force_global, r.at.scale, r.at.force_big, r.at.no_par, r.at.no_cap, r.errs, (int64_t)r.par_code,
                                           r.rec_used, r.rpool_used, r.bpool_used, r.evictions};
        std::memcpy(out + (size_t)i * kAttemptFields, v, sizeof v);
    }
    return n;
}

int tda_device_ok(int32_t device) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || device < 0 || device >= cnt) return 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return 0;
    return std::strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
}

}  // extern "C"

// the native sweep pipeline (include/tda_rips.h tda_pipe_*): the queue of sweep_pipe.h around tda_rips_batch
#include "sweep_pipe.h"

struct tda_pipe {
    tda::SweepPipe q;
    tda_pipe(int depth, int coalesce) : q(depth, coalesce, tda_rips_batch, tda_rips_free, tda_last_error) {}
};

extern "C" {

int tda_pipe_create(int32_t depth, int32_t coalesce, tda_pipe** out) {
    if (!out) return fail(TDA_E_INVALID, "out is NULL");
    *out = nullptr;
    if (depth < 1 || depth > TDA_MAX_SLOTS) return fail(TDA_E_INVALID, "depth must be in [1, TDA_MAX_SLOTS]");
    if (coalesce < 1 || coalesce > TDA_MAX_PARTS) return fail(TDA_E_INVALID, "coalesce must be in [1, TDA_MAX_PARTS]");
    *out = new tda_pipe(depth, coalesce);
    return 0;
}

int tda_pipe_submit(tda_pipe* pipe, const tda_rips_args* tmpl, int64_t tmpl_id, const void* x, int64_t L, int64_t N, int64_t D,
                    int32_t dtype, int32_t x_on_device, uint64_t* ticket) {
    if (!pipe || !tmpl || !ticket) return fail(TDA_E_INVALID, "tda_pipe_submit: a NULL argument");
    if (x_on_device && !(tmpl->flags & TDA_FLAG_INPUT_READY))
        return fail(TDA_E_INVALID, "tda_pipe_submit: device input needs TDA_FLAG_INPUT_READY");
    std::string err;
    const int rc = pipe->q.submit(*tmpl, tmpl_id, x, L, N, D, dtype, x_on_device, ticket, &err);
    return rc ? fail(rc, err) : 0;
}

int tda_pipe_flush(tda_pipe* pipe) {
    if (!pipe) return fail(TDA_E_INVALID, "pipe is NULL");
    pipe->q.flush();
    return 0;
}

int tda_pipe_wait(tda_pipe* pipe, uint64_t ticket, tda_rips_result** res, int64_t* lo, int64_t* hi, int32_t* n_sweeps,
                  uint64_t* call, int32_t mode) {
    if (!pipe || !res || !lo || !hi || !n_sweeps || !call) return fail(TDA_E_INVALID, "tda_pipe_wait: a NULL argument");
    if (mode < TDA_PIPE_POLL || mode > TDA_PIPE_DISPATCH) return fail(TDA_E_INVALID, "tda_pipe_wait: bad mode");
    tda::SweepPipe::Waited w = pipe->q.wait(ticket, (tda::SweepPipe::Mode)mode);
    *res = w.res;
    *lo = w.lo;
    *hi = w.hi;
    *n_sweeps = w.n_sweeps;
    *call = w.call;
    return w.rc < 0 ? fail(w.rc, w.err) : w.rc;
}

int tda_pipe_release(tda_pipe* pipe, uint64_t ticket) {
    if (!pipe) return fail(TDA_E_INVALID, "pipe is NULL");
    const int left = pipe->q.release(ticket);
    return left < 0 ? fail(TDA_E_INVALID, "tda_pipe_release: unknown or released ticket") : left;
}

void tda_pipe_destroy(tda_pipe* pipe) { delete pipe; }

}  // extern "C"

#include "aux_ws.h"  // the per-device workspace of the entries below, and its locking
#include "side_call.h"  // the frame of a call of theirs (their host plans: side_plan.h, dgm_plan.h)
// UMAP embedding (include/tda_umap.h): same library, same error state
#include "umap_host.h"
// effective dimensionality (include/tda_rips.h tda_effective_dim)
#include "ed_host.h"
// greedy furthest-point landmarks, ripser.py's n_perm (include/tda_rips.h tda_greedy_perm)
#include "greedy_host.h"
// resamples of a layer for bootstrap confidence bands (include/tda_rips.h tda_resample)
#include "resample_host.h"
// H0 persistence of subsamples for the persistent-homology dimension (include/tda_rips.h tda_subsample_h0)
#include "sh0_host.h"
// geodesic distances over the neighbourhood graph (include/tda_rips.h tda_geodesic)
#include "geo_host.h"
// the permutation test between groups of diagrams (include/tda_rips.h tda_permutation_test)
#include "perm_host.h"
// sliced Wasserstein distances between persistence diagrams (include/tda_dgm.h)
#include "dgm_host.h"
// bottleneck distances between persistence diagrams (include/tda_dgm.h)
#include "bn_host.h"
// 1-Wasserstein distances between persistence diagrams (include/tda_dgm.h)
#include "ws_host.h"
// persistence landscapes and persistence images (include/tda_dgm.h)
#include "vec_host.h"
// the heat (scale-space) kernel between persistence diagrams and its distance (include/tda_dgm.h)
#include "hk_host.h"
// persistence curves: Betti, lifespan, entropy, silhouette (include/tda_dgm.h)
#include "pc_host.h"
// the persistence Fisher distance between persistence diagrams (include/tda_dgm.h)
#include "pf_host.h"
