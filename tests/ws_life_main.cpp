// Stand-alone driver of csrc/ws_life.h (CPU; tests/test_ws_life_cpu.py builds and runs it, plain
// and under the thread and the address / undefined-behaviour sanitizers).  The runtime is a
// stand-in: buffers, graphs and executable graphs are malloc blocks (a double free or a use after
// free is the address sanitizer's to see), every call is logged in order, the n-th call of a kind
// can be told to fail, and two process-wide counters -- captures that are open, and graphs that
// are instantiated but not yet launched -- abort the program when another thread allocates, frees
// or destroys beside an open capture, or launches inside such a window.  Prints "ok <case>" per
// case and "all ok" at the end; the first failed check prints its line and exits 1.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <set>
#include <thread>
#include <vector>

#include "ws_life.h"

using namespace tda::ws;

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                          \
        }                                                          \
    } while (0)

namespace {

enum Kind { kAlloc, kFree, kAlias, kBegin, kEnd, kInst, kLaunch, kDestroyExec, kDestroyGraph, kRecord, kKinds };

std::atomic<int> g_captures{0}, g_windows{0};
std::atomic<long> g_allocs{0}, g_frees{0};
std::mutex g_live_mu;
std::set<void*> g_live;  // every block the stand-in handed out and has not taken back
thread_local bool t_capturing = false, t_window = false;

void rule(bool ok, const char* what) {
    if (ok) return;
    std::fprintf(stderr, "lock rule broken: %s\n", what);
    std::abort();
}
void* make(size_t bytes) {
    void* p = std::malloc(bytes ? bytes : 1);
    CHECK(p != nullptr);
    std::lock_guard<std::mutex> g(g_live_mu);
    CHECK(g_live.insert(p).second);
    ++g_allocs;
    return p;
}
void unmake(void* p) {
    {
        std::lock_guard<std::mutex> g(g_live_mu);
        CHECK(g_live.erase(p) == 1);  // handed out, and taken back exactly once
        ++g_frees;
    }
    std::free(p);
}

struct FakeRt {
    struct Ev {
        Kind k;
        const void* h;
        size_t bytes;
    };
    std::vector<Ev> log;
    bool logging = true;
    int fail_in[kKinds] = {};        // > 0: the fail_in-th call of the kind from now returns an error
    std::function<void()> on_launch;  // runs inside launch()
    const char* failed_call = nullptr;
    void* open_exec = nullptr;  // instantiated, not yet launched

    bool step(Kind k, const void* h = nullptr, size_t bytes = 0) {  // false: this call is to fail
        if (logging) log.push_back({k, h, bytes});
        return !(fail_in[k] > 0 && --fail_in[k] == 0);
    }
    static void beside_capture(const char* what) { rule(g_captures.load() - (t_capturing ? 1 : 0) == 0, what); }

    int alloc(Mem, void** p, size_t bytes) {
        beside_capture("an allocation while another thread captures");
        if (!step(kAlloc, nullptr, bytes)) return 2;
        *p = make(bytes);
        return 0;
    }
    int free(Mem, void* p) {
        beside_capture("a free while another thread captures");
        if (!step(kFree, p)) return 3;
        unmake(p);
        return 0;
    }
    int alias(void** dev, void* host) {
        if (!step(kAlias, host)) return 4;
        *dev = host;
        return 0;
    }
    // an open capture and an open window last a few time slices, so that a thread that does not
    // wait for them is seen
    static void linger() {
        for (int i = 0; i < 4; ++i) std::this_thread::yield();
    }
    int begin_capture(void*) {
        if (!step(kBegin)) return 5;
        t_capturing = true;
        ++g_captures;
        linger();
        return 0;
    }
    int end_capture(void*, void** graph) {
        t_capturing = false;
        --g_captures;
        if (!step(kEnd)) return 6;  // *graph stays null
        *graph = make(8);
        return 0;
    }
    int instantiate(void** exec, void* graph) {
        if (!step(kInst, graph)) return 7;
        *exec = open_exec = make(8);
        t_window = true;
        ++g_windows;
        linger();
        return 0;
    }
    int launch(void* exec, void*) {
        std::this_thread::yield();  // a launch takes a while too: replays are still under way when another slot captures
        rule(g_windows.load() - (t_window ? 1 : 0) == 0, "a launch between another thread's instantiation and its first launch");
        if (on_launch) on_launch();
        if (exec == open_exec) open_exec = nullptr, t_window = false, --g_windows;
        return step(kLaunch, exec) ? 0 : 8;
    }
    int destroy_exec(void* exec) {
        beside_capture("an executable graph destroyed while another thread captures");
        if (exec == open_exec) open_exec = nullptr, t_window = false, --g_windows;
        step(kDestroyExec, exec);
        unmake(exec);
        return 0;
    }
    int destroy_graph(void* graph) {
        beside_capture("a graph destroyed while another thread captures");
        step(kDestroyGraph, graph);
        unmake(graph);
        return 0;
    }
    int record(void* ev, void*) { return step(kRecord, ev) ? 0 : 9; }
    int fail(const char* call, int e) {
        failed_call = call;
        return -100 - e;
    }
    // an eager launch sequence's kernels (the enqueue callable calls it)
    void eager_kernels() { rule(g_windows.load() - (t_window ? 1 : 0) == 0, "an eager launch inside another thread's window"); }

    std::vector<Kind> kinds() const {
        std::vector<Kind> v;
        for (const auto& e : log) v.push_back(e.k);
        return v;
    }
    int count(Kind k) const {
        int n = 0;
        for (const auto& e : log) n += e.k == k;
        return n;
    }
};

int g_stream, g_ev0, g_ev1;  // handles: only their addresses matter
void* const S = &g_stream;
void* const E0 = &g_ev0;
void* const E1 = &g_ev1;

// a key of the cache `gc` whose fields are all set and distinct; `tweak` then changes what a case wants
GraphKey key_of(const GraphCache& gc, const std::function<void(GraphKey&)>& tweak = nullptr) {
    GraphKey k;
    make_key(k, [&](GraphKey& g) {
        g.L = 32, g.N = 48, g.D = 3;
        g.maxdim = 2, g.dtype = 1, g.input_kind = 0, g.x_on_device = 1, g.flags = 4, g.force_global = 0, g.scale = 1, g.force_big = 0;
        g.variant = 0x1234, g.n_label_sets = 2, g.sil_K = 5, g.no_par = 0, g.twonn = 1, g.no_cap = 0, g.dsplit = 2, g.pool_shift = 0;
        g.thresh = 0.0f, g.tn_eps = 1e-6f, g.capf = 0.5f, g.tn_discard = 0.1, g.x = &g_stream, g.gen = gc.gen(), g.par_steps[0] = g.par_steps[1] = 1ull << 26;
        if (tweak) tweak(g);
    });
    return k;
}
GraphKey key_n(const GraphCache& gc, int64_t n) {
    return key_of(gc, [n](GraphKey& g) { g.L = 1000 + n; });
}

int capture_ok(FakeRt& rt, GraphCache& gc, const GraphKey& k) {
    return launch(rt, gc, k, true, S, E0, E1, [](bool capture) { return capture ? 0 : 77; });
}
void finish(FakeRt& rt, GraphCache& gc) {  // a case's end: nothing of it is left
    gc.drop(rt);
    CHECK(g_live.empty() && g_allocs == g_frees && g_captures == 0 && g_windows == 0);
}

// who holds the two global locks, asked from another thread (trying a lock one's own thread holds is undefined)
struct Held {
    bool launch_exclusive, launch_any, capture;
};
Held probe_locks() {
    Held h = {};
    std::thread([&h] {
        const bool shared = g_launch_mu.try_lock_shared();
        if (shared) g_launch_mu.unlock_shared();
        const bool excl = shared && g_launch_mu.try_lock();
        if (excl) g_launch_mu.unlock();
        const bool cap = g_capture_mu.try_lock();
        if (cap) g_capture_mu.unlock();
        h = {!shared, !excl, !cap};
    }).join();
    return h;
}

// ---------------------------------------------------------------- cases
template <class T>
void grow_failures_of(Mem mem) {
    for (Kind k : {kFree, kAlloc, kAlias}) {  // the step that fails
        if (k == kAlias && mem != kMapped) continue;
        FakeRt rt;
        Buf<T> b{mem};
        CHECK(grow(rt, b, 100, 100) == 0 && b.p && b.cap == 100 && (b.dev != nullptr) == (mem == kMapped));
        T* const old = b.p;
        rt.fail_in[k] = 1;
        GrowStep step = k == kFree ? kGrowAlloc : kGrowFree;
        CHECK(grow(rt, b, 200, 200, &step) != 0);
        CHECK(step == (k == kFree ? kGrowFree : kGrowAlloc));
        CHECK(rt.failed_call != nullptr);
        CHECK(b.p == nullptr && b.dev == nullptr && b.cap == 0);  // empty: no freed pointer under the old capacity
        if (k == kFree) CHECK(rt.free(mem, old) == 0);            // the runtime refused it: still the caller's to hand back
        // a smaller need than the old capacity: it must allocate, not pass a stale capacity check
        CHECK(grow(rt, b, 50, 50) == 0 && b.p && b.cap == 50 && (b.dev != nullptr) == (mem == kMapped));
        for (int i = 0; i < 50; ++i) b.p[i] = T(i);
        CHECK(rt.free(mem, b.p) == 0);
        CHECK(g_live.empty() && g_allocs == g_frees);  // every allocation freed exactly once
    }
}
void grow_failure_leaves_empty() {
    for (Mem mem : {kPinned, kMapped, kDevice}) {
        grow_failures_of<char>(mem);
        grow_failures_of<int64_t>(mem);
    }
}

void baked_growth_drops_first() {
    FakeRt rt;
    GraphCache gc;
    Buf<char> baked{kPinned, &gc}, plain{kPinned};
    CHECK(grow(rt, baked, 10, 10) == 0 && grow(rt, plain, 10, 10) == 0);
    for (int i = 0; i < 3; ++i) CHECK(capture_ok(rt, gc, key_n(gc, i)) == 0);
    const uint64_t gen = gc.gen();
    CHECK(gc.size() == 3);

    rt.log.clear();
    CHECK(grow(rt, plain, 20, 20) == 0);  // no graph holds its address
    CHECK((rt.kinds() == std::vector<Kind>{kFree, kAlloc}) && gc.gen() == gen && gc.size() == 3);

    rt.log.clear();
    CHECK(grow(rt, baked, 20, 20) == 0);
    CHECK((rt.kinds() == std::vector<Kind>{kDestroyExec, kDestroyGraph, kDestroyExec, kDestroyGraph, kDestroyExec, kDestroyGraph, kFree, kAlloc}));
    CHECK(gc.gen() == gen + 1 && gc.size() == 0 && gc.find(key_n(gc, 0)) == nullptr);

    rt.log.clear();
    CHECK(grow(rt, baked, 20, 1 << 20) == 0 && grow(rt, baked, 0, 0) == 0 && grow(rt, plain, 7, 64) == 0);  // they fit
    CHECK(rt.log.empty() && gc.gen() == gen + 1 && baked.cap == 20);

    CHECK(rt.free(kPinned, baked.p) == 0 && rt.free(kPinned, plain.p) == 0);
    finish(rt, gc);
}

struct Pair24 {  // an element of the output buffer's size
    char b[24];
};
void growth_policy() {
    FakeRt rt;
    auto bytes = [&rt] {  // the sizes allocated since the last look
        std::vector<size_t> v;
        for (const auto& e : rt.log)
            if (e.k == kAlloc) v.push_back(e.bytes);
        rt.log.clear();
        return v;
    };
    using V = std::vector<size_t>;
    // the device workspace: max(need, 1.5 x what it was)
    Buf<char> dbuf{kDevice};
    for (size_t need : {1000, 1200, 1400, 5000, 100, 5001}) CHECK(grow(rt, dbuf, need, want_half_more(need, dbuf.cap)) == 0);
    CHECK((bytes() == V{1000, 1500, 5000, 7500}) && dbuf.cap == 7500);
    // the output pairs: max(256 L, 1 << 16) per call, then max(need, 2 x what it was) after an overflow
    Buf<Pair24> hout{kMapped};
    for (size_t L : {32, 256, 300, 8}) CHECK(grow(rt, hout, want_floor(L * 256, kFloorStage), want_floor(L * 256, kFloorStage)) == 0);
    CHECK((bytes() == V{65536 * 24, 76800 * 24}) && hout.cap == 76800);
    for (size_t need : {76801, 400000}) CHECK(grow(rt, hout, need, want_double(need, hout.cap)) == 0);
    CHECK((bytes() == V{153600 * 24, 400000 * 24}) && hout.cap == 400000);
    // per-layer records and offsets: exactly L and 4 L
    Buf<int64_t> hstats{kMapped}, houtoff{kMapped};
    for (size_t L : {32, 8, 48}) CHECK(grow(rt, hstats, L, L) == 0 && grow(rt, houtoff, 4 * L, 4 * L) == 0);
    CHECK((bytes() == V{32 * 8, 128 * 8, 48 * 8, 192 * 8}));
    // staging and landing bytes: floor 1 << 16 (a call that needs none allocates none)
    Buf<char> hin{kPinned}, hdist{kPinned};
    for (size_t need : {0, 100, 65536, 70000}) CHECK(grow(rt, hin, need, want_floor(need, kFloorStage)) == 0 && grow(rt, hdist, need, want_floor(need, kFloorStage)) == 0);
    CHECK((bytes() == V{65536, 65536, 70000, 70000}));
    // silhouette bytes: floor 1 << 12; TwoNN floats: floor 64; gathered parts: none
    Buf<char> hsil{kMapped}, xin{kDevice};
    Buf<float> htn{kMapped};
    for (size_t need : {200, 4096, 5000}) CHECK(grow(rt, hsil, need, want_floor(need, kFloorSil)) == 0);
    for (size_t L : {32, 64, 100}) CHECK(grow(rt, htn, L, want_floor(L, kFloorTn)) == 0);
    for (size_t need : {96, 90, 97}) CHECK(grow(rt, xin, need, need) == 0);
    CHECK((bytes() == V{4096, 5000, 64 * 4, 100 * 4, 96, 97}));
    CHECK(rt.free(kDevice, dbuf.p) == 0 && rt.free(kMapped, hout.p) == 0 && rt.free(kMapped, hstats.p) == 0 && rt.free(kMapped, houtoff.p) == 0);
    CHECK(rt.free(kPinned, hin.p) == 0 && rt.free(kPinned, hdist.p) == 0 && rt.free(kMapped, hsil.p) == 0 && rt.free(kMapped, htn.p) == 0);
    CHECK(rt.free(kDevice, xin.p) == 0 && g_live.empty());
}

void cache_hit_miss_evict() {
    FakeRt rt;
    GraphCache gc;
    for (int i = 0; i < 16; ++i) {
        CHECK(gc.find(key_n(gc, i)) == nullptr);
        CHECK(capture_ok(rt, gc, key_n(gc, i)) == 0);
        CHECK((int)gc.size() == i + 1);
    }
    for (int i = 0; i < 16; ++i) CHECK(gc.find(key_n(gc, i)) != nullptr);
    CHECK(gc.gen() == 0);

    // the seventeenth: the sixteen are destroyed after its own instantiation and before its own launch
    std::vector<const void*> execs, graphs;
    for (int i = 0; i < 16; ++i) execs.push_back(gc.find(key_n(gc, i))->exec), graphs.push_back(gc.find(key_n(gc, i))->graph);
    const GraphKey k17 = key_n(gc, 16);
    rt.log.clear();
    CHECK(capture_ok(rt, gc, k17) == 0);
    std::vector<Kind> want = {kBegin, kEnd, kInst};
    for (int i = 0; i < 16; ++i) want.push_back(kDestroyExec), want.push_back(kDestroyGraph);
    want.insert(want.end(), {kRecord, kLaunch, kRecord});
    CHECK(rt.kinds() == want);
    for (int i = 0; i < 16; ++i) CHECK(rt.log[3 + 2 * i].h == execs[i] && rt.log[4 + 2 * i].h == graphs[i]);
    CHECK(gc.size() == 1 && gc.gen() == 1);
    CHECK(gc.find(k17) == nullptr);  // built under the old generation
    const GraphEntry* e = gc.find(key_n(gc, 16));
    CHECK(e && e->key.gen == 1 && e->exec == rt.log[36].h && e->graph == rt.log[2].h);
    for (int i = 0; i < 16; ++i) CHECK(gc.find(key_n(gc, i)) == nullptr);

    // one field apart from a cached key: a miss, whichever field
    CHECK(capture_ok(rt, gc, key_of(gc)) == 0 && gc.find(key_of(gc)) != nullptr);
    const std::vector<std::function<void(GraphKey&)>> fields = {
        [](GraphKey& g) { ++g.L; }, [](GraphKey& g) { ++g.N; }, [](GraphKey& g) { ++g.D; }, [](GraphKey& g) { ++g.maxdim; },
        [](GraphKey& g) { ++g.dtype; }, [](GraphKey& g) { ++g.input_kind; }, [](GraphKey& g) { ++g.x_on_device; },
        [](GraphKey& g) { ++g.flags; }, [](GraphKey& g) { ++g.force_global; }, [](GraphKey& g) { ++g.scale; },
        [](GraphKey& g) { ++g.force_big; }, [](GraphKey& g) { ++g.variant; }, [](GraphKey& g) { ++g.n_label_sets; },
        [](GraphKey& g) { ++g.sil_K; }, [](GraphKey& g) { ++g.no_par; }, [](GraphKey& g) { ++g.twonn; }, [](GraphKey& g) { ++g.no_cap; },
        [](GraphKey& g) { ++g.dsplit; }, [](GraphKey& g) { g.thresh = -0.0f; }, [](GraphKey& g) { g.thresh = 1.0f; },
        [](GraphKey& g) { g.tn_eps *= 2; }, [](GraphKey& g) { g.capf *= 2; }, [](GraphKey& g) { g.tn_discard *= 2; },
        [](GraphKey& g) { g.x = &g_ev0; }, [](GraphKey& g) { ++g.gen; }, [](GraphKey& g) { ++g.pool_shift; },
        [](GraphKey& g) { g.par_steps[0] = 4; }, [](GraphKey& g) { g.par_steps[1] = 4; }};
    // every member is in the list (thresh twice): 3 of 8 bytes, 16 ints, 3 floats (and 4 bytes of padding), then 5 of 8 bytes
    static_assert(sizeof(GraphKey) == 3 * 8 + 16 * 4 + 3 * 4 + 4 + 5 * 8, "GraphKey changed: bring `fields` up to date");
    CHECK(fields.size() == 3 + 16 + 3 + 5 + 1);
    for (const auto& f : fields) CHECK(gc.find(key_of(gc, f)) == nullptr);

    // equal fields over differently filled memory: equal bytes
    GraphKey a, b;
    std::memset(&a, 0xAA, sizeof a);
    std::memset(&b, 0x55, sizeof b);
    const auto same = [](GraphKey& g) { g.L = 3, g.N = 5, g.thresh = 2.5f, g.tn_discard = 0.25, g.x = &g_ev1, g.gen = 9; };
    make_key(a, same);
    make_key(b, same);
    CHECK(std::memcmp(&a, &b, sizeof a) == 0);
    finish(rt, gc);
}

void capture_failures() {
    FakeRt rt;
    GraphCache gc;
    const GraphKey k = key_of(gc);
    // the enqueue fails: its code comes back, the captured graph is destroyed once, nothing is cached
    rt.log.clear();
    CHECK(launch(rt, gc, k, true, S, E0, E1, [](bool) { return 42; }) == 42);
    CHECK((rt.kinds() == std::vector<Kind>{kBegin, kEnd, kDestroyGraph}) && gc.size() == 0 && g_live.empty());
    CHECK(capture_ok(rt, gc, k) == 0 && gc.size() == 1);  // the next call captures again
    gc.drop(rt);
    // ... and when the capture's end fails as well (no graph): still the enqueue's code
    rt.log.clear();
    rt.fail_in[kEnd] = 1;
    CHECK(launch(rt, gc, key_of(gc), true, S, E0, E1, [](bool) { return 42; }) == 42);
    CHECK((rt.kinds() == std::vector<Kind>{kBegin, kEnd}) && gc.size() == 0 && g_live.empty());
    // the capture's end fails
    rt.log.clear();
    rt.fail_in[kEnd] = 1;
    CHECK(capture_ok(rt, gc, key_of(gc)) == -106 && !std::strcmp(rt.failed_call, "hipStreamEndCapture"));
    CHECK((rt.kinds() == std::vector<Kind>{kBegin, kEnd}) && gc.size() == 0 && g_live.empty() && g_captures == 0);
    rt.log.clear();
    CHECK(capture_ok(rt, gc, key_of(gc)) == 0 && gc.size() == 1 && rt.count(kBegin) == 1);
    gc.drop(rt);
    // the instantiation fails: the graph is destroyed once
    rt.log.clear();
    rt.fail_in[kInst] = 1;
    CHECK(capture_ok(rt, gc, key_of(gc)) == -107 && !std::strcmp(rt.failed_call, "hipGraphInstantiate"));
    CHECK((rt.kinds() == std::vector<Kind>{kBegin, kEnd, kInst, kDestroyGraph}) && gc.size() == 0 && g_live.empty() && g_windows == 0);
    rt.log.clear();
    CHECK(capture_ok(rt, gc, key_of(gc)) == 0 && gc.size() == 1 && rt.count(kBegin) == 1);
    // the capture cannot begin: nothing else is called
    gc.drop(rt);
    rt.log.clear();
    rt.fail_in[kBegin] = 1;
    CHECK(capture_ok(rt, gc, key_of(gc)) == -105 && rt.log.size() == 1 && gc.size() == 0);
    finish(rt, gc);
}

void replay_and_eager() {
    FakeRt rt;
    GraphCache gc;
    // a capture: the enqueue and the first launch run with both locks held alone
    Held in_enqueue = {}, in_launch = {};
    rt.on_launch = [&] { in_launch = probe_locks(); };
    CHECK(launch(rt, gc, key_of(gc), true, S, E0, E1, [&](bool capture) {
              CHECK(capture);
              in_enqueue = probe_locks();
              return 0;
          }) == 0);
    CHECK(in_enqueue.launch_exclusive && in_enqueue.capture && in_launch.launch_exclusive && in_launch.capture);
    // a hit: record, launch, record and nothing else, under the shared side of the launch lock only
    const GraphEntry* e = gc.find(key_of(gc));
    CHECK(e != nullptr);
    rt.log.clear();
    int enqueued = 0;
    CHECK(launch(rt, gc, key_of(gc), true, S, E0, E1, [&](bool) { return ++enqueued; }) == 0);
    CHECK(enqueued == 0 && (rt.kinds() == std::vector<Kind>{kRecord, kLaunch, kRecord}));
    CHECK(rt.log[0].h == E0 && rt.log[1].h == e->exec && rt.log[2].h == E1);
    CHECK(in_launch.launch_any && !in_launch.launch_exclusive && !in_launch.capture);
    // a failed replay step comes back as the runtime's failure
    rt.fail_in[kLaunch] = 1;
    CHECK(launch(rt, gc, key_of(gc), true, S, E0, E1, [&](bool) { return 0; }) == -108 && !std::strcmp(rt.failed_call, "hipGraphLaunch"));
    // graphs off: the enqueue runs once, eagerly, under the shared side; nothing is called or cached
    rt.log.clear();
    Held eager = {};
    CHECK(launch(rt, gc, key_n(gc, 1), false, S, E0, E1, [&](bool capture) {
              CHECK(!capture);
              ++enqueued;
              rt.eager_kernels();
              eager = probe_locks();
              return 0;
          }) == 0);
    CHECK(enqueued == 1 && rt.log.empty() && gc.size() == 1 && gc.find(key_n(gc, 1)) == nullptr);
    CHECK(eager.launch_any && !eager.launch_exclusive && !eager.capture);
    CHECK(launch(rt, gc, key_of(gc), false, S, E0, E1, [](bool) { return 5; }) == 5);  // a cached key too, and its code comes back
    // the three scopes by name
    {
        AllocScope lock;
        const Held h = probe_locks();
        CHECK(h.capture && !h.launch_any);
    }
    {
        CaptureScope lock;
        const Held h = probe_locks();
        CHECK(h.capture && h.launch_exclusive);
    }
    {
        LaunchScope lock;
        const Held h = probe_locks();
        CHECK(!h.capture && h.launch_any && !h.launch_exclusive);
    }
    rt.on_launch = nullptr;
    finish(rt, gc);
}

// kSlots threads, one per slot as in the library (a slot's cache and buffers are its own, under its
// own mutex), kCalls calls each from a fixed seed.
constexpr int kSlots = 8, kCalls = 5000;
std::atomic<int> g_ready{0};
void slot_thread(int slot) {
    FakeRt rt;
    rt.logging = false;
    GraphCache gc;
    Buf<char> baked{kMapped, &gc}, plain{kPinned}, aux{kDevice};
    uint64_t rng = 0x9E3779B97F4A7C15ull * (uint64_t)(slot + 1);
    auto next = [&rng] {
        rng = rng * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(rng >> 33);
    };
    int64_t fresh = 0;
    for (++g_ready; g_ready.load() < kSlots;) std::this_thread::yield();  // all slots start together
    const auto enqueue = [&rt](bool capture) {
        if (!capture) rt.eager_kernels();
        return 0;
    };
    for (int i = 0; i < kCalls; ++i) {
        const uint32_t r = next() % 100;
        if (r < 88) {  // the slot's steady key: a replay unless a drop came in between
            CHECK(launch(rt, gc, key_n(gc, 0), true, S, E0, E1, enqueue) == 0);
        } else if (r < 92) {  // a new key: a capture, from the sixteenth on an eviction
            CHECK(launch(rt, gc, key_n(gc, ++fresh), true, S, E0, E1, enqueue) == 0);
        } else if (r < 94) {  // graphs off
            CHECK(launch(rt, gc, key_n(gc, 0), false, S, E0, E1, enqueue) == 0);
        } else if (r < 96) {  // a baked buffer grows: the slot's graphs go
            AllocScope lock;
            const size_t need = baked.cap + 1 + next() % 64;
            CHECK(grow(rt, baked, need, need) == 0 && gc.size() == 0);
        } else if (r < 98) {  // an unbaked one: they stay
            AllocScope lock;
            const size_t n = gc.size(), need = plain.cap + 1 + next() % 64;
            CHECK(grow(rt, plain, need, need) == 0 && gc.size() == n);
        } else {  // an entry beside the pipeline: its buffer, then a further allocation in the same hold
            AllocScope lock;
            const size_t need = next() % 4 ? 1 : aux.cap + 1 + next() % 256;
            CHECK(grow(rt, aux, need, need) == 0);
            void* extra = nullptr;
            CHECK(rt.alloc(kDevice, &extra, 64) == 0 && rt.free(kDevice, extra) == 0);
        }
        if (baked.p) baked.p[baked.cap - 1] = (char)i;  // the buffers are the slot's to write
        if (plain.p) plain.p[plain.cap - 1] = (char)i;
    }
    AllocScope lock;
    gc.drop(rt);
    for (Buf<char>* b : {&baked, &plain, &aux})
        if (b->p) CHECK(rt.free(b->mem, b->p) == 0);
}
void threads() {
    std::vector<std::thread> th;
    for (int s = 0; s < kSlots; ++s) th.emplace_back(slot_thread, s);
    for (auto& t : th) t.join();
    CHECK(g_live.empty() && g_allocs == g_frees && g_allocs > 0 && g_captures == 0 && g_windows == 0);
}

}  // namespace

int main() {
#define RUN(c) c(), std::printf("ok %s\n", #c), std::fflush(stdout)
    RUN(grow_failure_leaves_empty);
    RUN(baked_growth_drops_first);
    RUN(growth_policy);
    RUN(cache_hit_miss_evict);
    RUN(capture_failures);
    RUN(replay_and_eager);
    RUN(threads);
    std::printf("all ok\n");
    return 0;
}
