// ws_life.h -- the lifetime of what a workspace owns on the device: its buffers, a slot's cache of
// captured graphs, the launch path over that cache and the process-wide locks all of it runs
// under.  Plain C++17, no HIP and no Python: the runtime is a template parameter `Rt` (rips.hip's
// HipRt forwards each call to HIP; tests/ws_life_main.cpp's stand-in allocates with malloc, logs
// every call and aborts when a lock rule is broken), so the rules below are run on the CPU, plain
// and under the thread and address sanitizers (tests/test_ws_life_cpu.py).
//
// Rt: int alloc(Mem, void**, bytes), free(Mem, void*), alias(void** dev, void* host),
// begin_capture(stream), end_capture(stream, void** graph), instantiate(void** exec, graph),
// launch(exec, stream), destroy_exec(exec), destroy_graph(graph), record(event, stream): 0 or the
// runtime's error; and int fail(const char* call, int err), which turns that error into the
// library's return code (and message).  Handles are void* here.
#pragma once
#include <stdint.h>

#include <cstring>
#include <mutex>
#include <shared_mutex>
#include <vector>

namespace tda::ws {

// ------------------------------------------------------------------ the locks
// Graph capture + instantiation AND every workspace (re)allocation / free, across
// all slots of the process.  r03 saw a host segfault inside the first calls of
// two slots that ran concurrently; the cause was not isolated then.  The HIP
// calls those first calls made at the same time were: hipFuncSetAttribute
// (one-time, now under rips.hip's g_attr_mu), stream capture + hipGraphInstantiate on
// the two slots' streams, and hipMalloc / hipHostMalloc of the workspaces --
// and on growth hipFree / hipHostFree / hipGraphExecDestroy.  ThreadLocal
// capture only restricts the CAPTURING thread, and HIP's hipFree synchronises
// the whole device (all streams, a capturing one included) while another
// thread captures; it is the one call whose contract does not cover running
// beside a capture.  So no (re)allocation, free or graph destruction runs
// while any slot captures: they take this lock too (first call / growth only;
// replays never take it).
inline std::mutex g_capture_mu;
// Graph launches: replays (and direct launches) share it; a capture with its instantiation and
// first launch holds it alone.  r06 (tools/concurrency_stress.py: 8 slots, calls of mixed shapes
// at once): a freshly instantiated graph's first hipGraphLaunch faulted inside the HIP runtime
// (a null dereference) while other slots replayed theirs; one slot at a time never did.
inline std::shared_mutex g_launch_mu;

// The only ways to hold them.  Lock order: a workspace's own mutex, then one scope (never two;
// rips.hip's g_attr_mu counts as one); no scope is held across a copy or a synchronise.
// AllocScope: an allocation, a free or a graph destruction.  CaptureScope: a capture, its
// instantiation and the new graph's first launch.  LaunchScope: a replay or an eager launch sequence.
struct AllocScope {
    std::lock_guard<std::mutex> cap{g_capture_mu};
};
struct CaptureScope : AllocScope {
    std::unique_lock<std::shared_mutex> launch{g_launch_mu};
};
struct LaunchScope {
    std::shared_lock<std::shared_mutex> launch{g_launch_mu};
};

// ------------------------------------------------------------------ the graph cache
// What a captured launch sequence (everything between ev0 and ev1) depends on: it is replayed
// with a single graph launch when the same plan, input address and flags recur.
struct GraphKey {
    int64_t L, N, D;
    int maxdim, dtype, input_kind, x_on_device, flags, force_global, scale, force_big, variant, n_label_sets, sil_K, no_par, twonn, no_cap;
    int dsplit;  // K slices of the distance kernels (TDA_DIST_SPLIT can change them at the same (N, D): other launches, other offsets)
    int pool_shift;  // TDA_PAR_POOL_SHIFT (tests): other pool capacities, other offsets behind them
    float thresh, tn_eps, capf;
    double tn_discard;
    const void* x;
    uint64_t gen;
    uint64_t par_steps[2];  // the step limits baked into the k_reduce_par launches of H1 and H2 (TDA_PAR_STEPS_H1 / _H2, TDA_STEP_LIMIT)
};
// The one way to build a key: every byte zeroed (the padding too), then fill(k) sets the fields,
// so keys of equal fields are equal bytes.  (-0.0f and 0.0f differ, as they always have.)
template <class Fill>
void make_key(GraphKey& k, Fill&& fill) {
    std::memset(&k, 0, sizeof k);
    fill(k);
}

// The graph is kept as long as its exec: destroying it right after the instantiation (legal by the API)
// faulted in the instance's first launch when other slots' threads were calling at the same time (r06).
struct GraphEntry {
    GraphKey key;
    void *exec, *graph;
};

// A slot's captured graphs, under the slot's mutex.  At most kMax; the insert that would exceed
// it drops them all first.  gen() rises with every drop and is part of the key, so a key built
// before a drop finds nothing after it.
struct GraphCache {
    static constexpr size_t kMax = 16;
    uint64_t gen() const { return gen_; }
    size_t size() const { return entries_.size(); }
    const GraphEntry* find(const GraphKey& k) const {
        for (const auto& e : entries_)
            if (std::memcmp(&e.key, &k, sizeof k) == 0) return &e;  // by bytes: see make_key
        return nullptr;
    }
    // destroys every graph (under AllocScope or CaptureScope: never beside another slot's capture)
    template <class Rt>
    void drop(Rt& rt) {
        for (auto& e : entries_) (void)rt.destroy_exec(e.exec), (void)rt.destroy_graph(e.graph);
        entries_.clear();
        ++gen_;
    }
    // the new entry carries the generation it is inserted under (a later one if it evicted)
    template <class Rt>
    const GraphEntry& insert(Rt& rt, const GraphKey& k, void* exec, void* graph) {
        if (entries_.size() >= kMax) drop(rt);
        entries_.push_back({k, exec, graph});
        std::memcpy(&entries_.back().key, &k, sizeof k);  // every byte of it
        entries_.back().key.gen = gen_;
        return entries_.back();
    }

private:
    std::vector<GraphEntry> entries_;
    uint64_t gen_ = 0;
};

// ------------------------------------------------------------------ buffers
enum Mem { kPinned, kMapped, kDevice };  // host pinned; host pinned and mapped (dev: its device alias); device
enum GrowStep { kGrowFree, kGrowAlloc };  // kGrowAlloc: the allocation or the fetch of its device alias

// One buffer of `cap` elements, made as Buf<T>{kind} or Buf<T>{kind, &cache}.  baked: the cache
// whose graphs hold its address (null: none do).
template <class T>
struct Buf {
    Mem mem;
    GraphCache* baked = nullptr;
    T *p = nullptr, *dev = nullptr;
    size_t cap = 0;
};

// The sizes asked for when `need` does not fit: at least a floor (the pipeline's: staging and
// landing bytes, output pairs; silhouette bytes; TwoNN floats; the gathered parts have none) ...
constexpr size_t kFloorStage = 1 << 16, kFloorSil = 1 << 12, kFloorTn = 64;
inline size_t want_floor(size_t need, size_t floor) { return need > floor ? need : floor; }
// ... or a multiple of what it was: the device workspace; the output pairs after an overflow
inline size_t want_half_more(size_t need, size_t cap) { return want_floor(need, cap + cap / 2); }
inline size_t want_double(size_t need, size_t cap) { return want_floor(need, 2 * cap); }

// `b` holds `need` elements afterwards, `want` (>= need) if it had to grow: the graphs that bake
// its address go first, then the free, then the allocation.  A failed step (*failed says which)
// returns rt.fail's code with the buffer EMPTY -- never a freed pointer under its old capacity.
// Under AllocScope.
template <class Rt, class T>
int grow(Rt& rt, Buf<T>& b, size_t need, size_t want, GrowStep* failed = nullptr) {
    if (b.cap >= need) return 0;
    GrowStep unused, &step = failed ? *failed : unused;
    if (b.baked) b.baked->drop(rt);
    void *old = b.p, *p = nullptr, *dev = nullptr;
    b.p = b.dev = nullptr;
    b.cap = 0;
    step = kGrowFree;
    if (int e = old ? rt.free(b.mem, old) : 0) return rt.fail(b.mem == kDevice ? "hipFree" : "hipHostFree", e);
    step = kGrowAlloc;
    if (int e = rt.alloc(b.mem, &p, want * sizeof(T))) return rt.fail(b.mem == kDevice ? "hipMalloc" : "hipHostMalloc", e);
    if (int e = b.mem == kMapped ? rt.alias(&dev, p) : 0) {
        (void)rt.free(b.mem, p);
        return rt.fail("hipHostGetDevicePointer", e);
    }
    b.p = (T*)p, b.dev = (T*)dev, b.cap = want;
    return 0;
}

// ------------------------------------------------------------------ the launch path
template <class Rt>
int replay(Rt& rt, void* exec, void* s, void* ev0, void* ev1) {
    if (int e = rt.record(ev0, s)) return rt.fail("hipEventRecord", e);
    if (int e = rt.launch(exec, s)) return rt.fail("hipGraphLaunch", e);
    if (int e = rt.record(ev1, s)) return rt.fail("hipEventRecord", e);
    return 0;
}

// A call's launch sequence on stream s: a replay of the graph cached for `key`, else a capture of
// enqueue(true) (instantiated, cached and launched), else -- use_graph off -- enqueue(false)
// eagerly.  enqueue returns 0 or the library's code.  The eviction sits where it always has,
// inside insert: after the instantiation and before the new graph's first launch.
template <class Rt, class Enqueue>
int launch(Rt& rt, GraphCache& gc, const GraphKey& key, bool use_graph, void* s, void* ev0, void* ev1, Enqueue&& enqueue) {
    const GraphEntry* ge = use_graph ? gc.find(key) : nullptr;
    if (ge || !use_graph) {
        LaunchScope lock;
        return ge ? replay(rt, ge->exec, s, ev0, ev1) : enqueue(false);
    }
    // capture + instantiate one graph at a time across the process: concurrent captures from
    // several slot threads crashed the HIP runtime once (r03, host segfault inside a first call
    // of two slots); replays run concurrently with each other, but not with a capture and its
    // first launch
    CaptureScope lock;
    if (int e = rt.begin_capture(s)) return rt.fail("hipStreamBeginCapture", e);
    const int rc = enqueue(true);
    void *graph = nullptr, *exec = nullptr;
    const int ce = rt.end_capture(s, &graph);
    if (rc || ce) {  // the enqueue's own code first
        if (graph) (void)rt.destroy_graph(graph);
        return rc ? rc : rt.fail("hipStreamEndCapture", ce);
    }
    if (int e = rt.instantiate(&exec, graph)) {
        (void)rt.destroy_graph(graph);
        return rt.fail("hipGraphInstantiate", e);
    }
    return replay(rt, gc.insert(rt, key, exec, graph).exec, s, ev0, ev1);
}

}  // namespace tda::ws
