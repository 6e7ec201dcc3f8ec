// Stand-alone driver of csrc/sweep_pipe.h (CPU; tests/test_sweep_pipe_cpu.py builds and runs it,
// plain and under the thread and the address / undefined-behaviour sanitizers).  The batch call is
// a stand-in that sleeps a few hundred microseconds and returns a result that says what it was
// given: L, N, the slot (in `maxdim`), its serial number (in `n_pairs`) and the parts' pointers
// (in `blob`).  Prints "ok <case>" per case and "all ok" at the end; the first failed check
// prints its line and exits 1.
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "sweep_pipe.h"

using tda::SweepPipe;

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                          \
        }                                                          \
    } while (0)

namespace {

std::atomic<int> g_allocs{0}, g_frees{0}, g_serial{0};
std::mutex g_live_mu;
std::set<tda_rips_result*> g_live;
thread_local std::string g_err;

int fake_batch(const tda_rips_args* a, tda_rips_result** out) {
    std::this_thread::sleep_for(std::chrono::microseconds(300));
    if (a->maxdim == 99) {  // a call the stand-in refuses
        g_err = "boom " + std::to_string(a->L);
        return TDA_E_HIP;
    }
    const int n = a->n_parts ? a->n_parts : 1;
    auto* r = new tda_rips_result();
    auto** parts = new const void*[n];
    for (int i = 0; i < n; ++i) parts[i] = a->n_parts ? a->x_parts[i] : a->x;
    r->L = a->L;
    r->N = a->N;
    r->maxdim = a->slot;
    r->n_pairs = g_serial++;
    r->blob = parts;
    r->blob_bytes = (int64_t)(n * sizeof(void*));
    r->device_ms = (double)a->thresh;  // the template travelled
    g_allocs++;
    std::lock_guard<std::mutex> g(g_live_mu);
    g_live.insert(r);
    *out = r;
    return 0;
}

void fake_free(tda_rips_result* r) {
    {
        std::lock_guard<std::mutex> g(g_live_mu);
        CHECK(g_live.erase(r) == 1);  // freed exactly once
    }
    delete[] static_cast<const void* const*>(r->blob);
    delete r;
    g_frees++;
}

const char* fake_error() { return g_err.c_str(); }

// sweeps: kSweeps arrays of 4 * 48 * 3 floats (room for every shape used below)
constexpr int kSweeps = 256, kStride = 4 * 48 * 3;
std::vector<float> g_data(kSweeps* kStride, 0.5f);
const void* sweep(int k) { return &g_data[(size_t)k * kStride]; }

tda_rips_args tmpl(float thresh = 1.5f, int maxdim = 2) {
    tda_rips_args a = {};
    a.maxdim = maxdim;
    a.thresh = thresh;
    a.modulus = 2;
    a.flags = TDA_FLAG_ONE_STREAM;
    return a;
}

uint64_t sub(SweepPipe& p, const tda_rips_args& t, int64_t tid, int k, int64_t L = 4, int64_t N = 12, int32_t dtype = TDA_F32,
             int32_t on_dev = 0) {
    uint64_t ticket = 0;
    std::string err;
    CHECK(p.submit(t, tid, sweep(k), L, N, 3, dtype, on_dev, &ticket, &err) == 0);
    return ticket;
}

// done without anybody waiting on it (polling dispatches nothing)
bool done_within(SweepPipe& p, uint64_t ticket, int ms) {
    for (int i = 0; i < ms * 10; ++i) {
        if (p.wait(ticket, SweepPipe::kPoll).rc != SweepPipe::kBusy) return true;
        std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
    return false;
}

const void* part_of(const SweepPipe::Waited& w, int i) { return static_cast<const void* const*>(w.res->blob)[i]; }

void case_order_and_slots() {
    SweepPipe p(2, 3, fake_batch, fake_free, fake_error);
    const tda_rips_args t = tmpl();
    std::vector<uint64_t> tk;
    for (int k = 0; k < 7; ++k) tk.push_back(sub(p, t, 1, k));
    // full batches left on their own; the partial last one has not
    CHECK(done_within(p, tk[0], 2000) && done_within(p, tk[5], 2000));
    std::this_thread::sleep_for(std::chrono::milliseconds(3));
    const SweepPipe::Waited busy = p.wait(tk[6], SweepPipe::kPoll);
    CHECK(busy.rc == SweepPipe::kBusy && busy.n_sweeps == 1 && busy.res == nullptr);
    std::vector<SweepPipe::Waited> w;
    for (int k = 0; k < 7; ++k) w.push_back(p.wait(tk[k]));  // the wait on ticket 6 dispatches it
    for (int k = 0; k < 7; ++k) {
        const int call = k / 3, idx = k % 3, n = call < 2 ? 3 : 1;
        CHECK(w[k].rc == 0 && w[k].res);
        CHECK(w[k].lo == 4 * idx && w[k].hi == 4 * idx + 4 && w[k].n_sweeps == n);
        CHECK(w[k].res->L == 4 * n && w[k].res->N == 12 && w[k].res->device_ms == 1.5);
        CHECK(part_of(w[k], idx) == sweep(k));                      // its own layers, in submission order
        CHECK(w[k].call == w[call * 3].call && w[k].res == w[call * 3].res);  // one result per call
        CHECK(w[k].res->maxdim == TDA_MAX_SLOTS - 2 + call % 2);     // call n on worker n % depth, the top slots
    }
    CHECK(w[0].call != w[3].call && w[3].call != w[6].call);
    // the calls of one slot stay ordered: call 2 ran after call 0 (same worker)
    CHECK(w[6].res->n_pairs > w[0].res->n_pairs);
    // freed exactly once, with the last ticket
    CHECK(g_frees == 0);
    CHECK(p.release(tk[0]) == 2 && p.release(tk[2]) == 1 && g_frees == 0);
    CHECK(p.release(tk[2]) == TDA_E_INVALID && p.wait(tk[2]).rc == TDA_E_INVALID);
    CHECK(p.wait(tk[1]).rc == 0);  // the others of the call still read it
    CHECK(p.release(tk[1]) == 0 && g_frees == 1);
    CHECK(p.release(tk[1]) == TDA_E_INVALID && p.wait(tk[0]).rc == TDA_E_INVALID);
    for (int k = 3; k < 7; ++k) CHECK(p.release(tk[k]) >= 0);
    CHECK(g_frees == 3 && g_allocs == 3);
    CHECK(p.wait(12345 << 4).rc == TDA_E_INVALID);
    std::puts("ok order_and_slots");
}

void case_key_changes_and_flush() {
    SweepPipe p(3, 4, fake_batch, fake_free, fake_error);
    const tda_rips_args t = tmpl(), t2 = tmpl(0.25f);
    std::vector<uint64_t> tk;
    tk.push_back(sub(p, t, 1, 0));
    tk.push_back(sub(p, t, 1, 1));
    tk.push_back(sub(p, t, 1, 2, 4, 33));  // another N in the middle: the two before it go
    CHECK(done_within(p, tk[0], 2000));
    CHECK(p.wait(tk[2], SweepPipe::kPoll).rc == SweepPipe::kBusy);
    tk.push_back(sub(p, t, 1, 3, 2, 33));             // another L
    tk.push_back(sub(p, t, 1, 4, 2, 33, TDA_F64));    // another dtype
    tk.push_back(sub(p, t, 1, 5, 2, 33, TDA_F64, 1)); // another residence
    tk.push_back(sub(p, t2, 2, 6, 2, 33, TDA_F64, 1)); // another argument template
    tk.push_back(sub(p, t2, 2, 7, 2, 33, TDA_F64, 1));
    CHECK(done_within(p, tk[5], 2000));
    CHECK(p.wait(tk[7], SweepPipe::kPoll).rc == SweepPipe::kBusy);
    p.flush();  // the partial last batch
    CHECK(done_within(p, tk[7], 2000));
    const int n_of[] = {2, 2, 1, 1, 1, 1, 2, 2};
    const int64_t n_pts[] = {12, 12, 33, 33, 33, 33, 33, 33};
    for (int k = 0; k < 8; ++k) {
        const SweepPipe::Waited w = p.wait(tk[k]);
        CHECK(w.rc == 0 && w.n_sweeps == n_of[k] && w.res->N == n_pts[k]);
        CHECK(part_of(w, (int)(w.lo / (w.hi - w.lo))) == sweep(k));
        CHECK(w.res->device_ms == (k < 6 ? 1.5 : 0.25));
    }
    // kDispatch sends a pending batch off without blocking
    const uint64_t last = sub(p, t, 1, 8);
    const int rc = p.wait(last, SweepPipe::kDispatch).rc;
    CHECK(rc == SweepPipe::kBusy || rc == 0);
    CHECK(done_within(p, last, 2000));
    std::puts("ok key_changes_and_flush");
}  // destroyed with every ticket unreleased

void case_errors() {
    SweepPipe p(2, 3, fake_batch, fake_free, fake_error);
    const tda_rips_args t = tmpl(), refused = tmpl(1.5f, 99);
    g_data[(size_t)4 * kStride + 77] = std::numeric_limits<float>::quiet_NaN();
    g_data[(size_t)9 * kStride + 5] = std::numeric_limits<float>::infinity();
    std::vector<uint64_t> tk;
    for (int k = 0; k < 9; ++k) tk.push_back(sub(p, t, 1, k));
    tk.push_back(sub(p, t, 1, 9, 4, 12, TDA_F32, 1));  // device input is not looked at
    for (int k = 0; k < 2; ++k) tk.push_back(sub(p, refused, 2, 10 + k));
    tk.push_back(sub(p, t, 1, 12));
    for (int k = 0; k < 13; ++k) {
        const SweepPipe::Waited w = p.wait(tk[k]);
        if (k >= 3 && k < 6) {  // the call of the sweep with the NaN, all three of its tickets
            CHECK(w.rc == TDA_E_INVALID && w.err == "Input contains NaN or infinity." && !w.res && w.n_sweeps == 3);
        } else if (k == 10 || k == 11) {  // the refused call: its code and its message (8 layers)
            CHECK(w.rc == TDA_E_HIP && w.err == "boom 8" && !w.res);
        } else {
            CHECK(w.rc == 0 && w.res && w.err.empty());
        }
        CHECK(p.release(tk[k]) >= 0);
    }
    g_data[(size_t)4 * kStride + 77] = 0.5f;
    g_data[(size_t)9 * kStride + 5] = 0.5f;
    // f64 input: the same bit test on 64-bit words
    std::vector<double> d(4 * 12 * 3, 1.0);
    uint64_t ticket = 0;
    std::string err;
    CHECK(p.submit(t, 1, d.data(), 4, 12, 3, TDA_F64, 0, &ticket, &err) == 0);
    CHECK(p.wait(ticket).rc == 0 && p.release(ticket) == 0);
    d[100] = -std::numeric_limits<double>::infinity();
    CHECK(p.submit(t, 1, d.data(), 4, 12, 3, TDA_F64, 0, &ticket, &err) == 0);
    CHECK(p.wait(ticket).rc == TDA_E_INVALID && p.release(ticket) == 0);
    // bad submissions never get a ticket
    CHECK(p.submit(t, 1, nullptr, 4, 12, 3, TDA_F32, 0, &ticket, &err) == TDA_E_INVALID && !err.empty());
    CHECK(p.submit(t, 1, sweep(0), 0, 12, 3, TDA_F32, 0, &ticket, &err) == TDA_E_INVALID);
    CHECK(p.submit(t, 1, sweep(0), 4, 12, 3, 7, 0, &ticket, &err) == TDA_E_INVALID);
    p.close();
    CHECK(p.submit(t, 1, sweep(0), 4, 12, 3, TDA_F32, 0, &ticket, &err) == TDA_E_INVALID && err == "the pipeline is closed");
    CHECK(g_allocs == g_frees);
    std::puts("ok errors");
}

void case_destroy() {
    const int before = g_allocs;
    {
        SweepPipe p(2, 3, fake_batch, fake_free, fake_error);
        const tda_rips_args t = tmpl();
        for (int k = 0; k < 4; ++k) sub(p, t, 1, k);  // one full call, one pending sweep, no ticket released
        uint64_t early = sub(p, t, 1, 4);
        CHECK(p.release(early) == 1);  // released before its call ran
    }
    CHECK(g_allocs == before + 2 && g_allocs == g_frees);
    {
        SweepPipe p(1, 2, fake_batch, fake_free, fake_error);
        const tda_rips_args t = tmpl();
        const uint64_t a = sub(p, t, 1, 0), b = sub(p, t, 1, 1);
        CHECK(p.release(a) == 1 && p.release(b) == 0);  // every ticket back before the call is done: the worker frees
        const uint64_t c = sub(p, t, 1, 2);
        p.close();  // tickets outlive close()
        const SweepPipe::Waited w = p.wait(c);
        CHECK(w.rc == 0 && part_of(w, 0) == sweep(2) && w.res->maxdim == TDA_MAX_SLOTS - 1);
        p.close();
    }
    CHECK(g_allocs == before + 4 && g_allocs == g_frees);
    std::puts("ok destroy");
}

void case_two_threads() {
    SweepPipe p(3, 4, fake_batch, fake_free, fake_error);
    const tda_rips_args t = tmpl();
    auto body = [&](int first) {
        std::vector<uint64_t> tk;
        for (int k = 0; k < 100; ++k) {
            tk.push_back(sub(p, t, 1, first + k));
            if (k >= 10) {  // a window of ten in flight, like a layer loop
                const SweepPipe::Waited w = p.wait(tk[k - 10]);
                CHECK(w.rc == 0 && part_of(w, (int)(w.lo / 4)) == sweep(first + k - 10));
                CHECK(p.release(tk[k - 10]) >= 0);
            }
        }
        for (int k = 90; k < 100; ++k) {
            const SweepPipe::Waited w = p.wait(tk[k]);
            CHECK(w.rc == 0 && part_of(w, (int)(w.lo / 4)) == sweep(first + k));
            CHECK(p.release(tk[k]) >= 0);
        }
    };
    std::thread a(body, 0), b(body, 100);
    a.join();
    b.join();
    CHECK(g_allocs == g_frees);
    std::puts("ok two_threads");
}

// several threads block on one ticket; whoever returns first releases it, and with it the call
void case_waiters_on_one_ticket() {
    SweepPipe p(2, 2, fake_batch, fake_free, fake_error);
    const tda_rips_args t = tmpl();
    for (int round = 0; round < 50; ++round) {
        const uint64_t tk = sub(p, t, 1, round);  // pending: the first wait dispatches it
        std::atomic<int> got{0}, gone{0};
        auto body = [&] {
            const SweepPipe::Waited w = p.wait(tk);
            if (w.rc == 0) {
                ++got;
                p.release(tk);  // only the first of these succeeds
            } else {
                CHECK(w.rc == TDA_E_INVALID && !w.res);
                ++gone;
            }
        };
        std::thread a(body), b(body), c(body);
        a.join();
        b.join();
        c.join();
        CHECK(got >= 1 && got + gone == 3);
        CHECK(p.wait(tk).rc == TDA_E_INVALID);
    }
    // a ticket released while another thread waits for its call, which has not run yet
    const uint64_t tk = sub(p, t, 1, 60);
    std::thread waiter([&] {
        const int rc = p.wait(tk).rc;
        CHECK(rc == TDA_E_INVALID || rc == 0);
    });
    std::this_thread::sleep_for(std::chrono::microseconds(100));
    p.release(tk);
    waiter.join();
    p.close();
    CHECK(g_allocs == g_frees);
    std::puts("ok waiters_on_one_ticket");
}

}  // namespace

int main() {
    case_order_and_slots();
    case_key_changes_and_flush();
    case_errors();
    case_destroy();
    case_two_threads();
    case_waiters_on_one_ticket();
    CHECK(g_allocs == g_frees && g_live.empty());
    std::puts("all ok");
    return 0;
}
