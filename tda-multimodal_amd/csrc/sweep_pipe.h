// sweep_pipe.h -- the queue of a native sweep pipeline (include/tda_rips.h, tda_pipe_*): `depth`
// worker threads, one per workspace slot, run coalesced tda_rips_batch calls while the caller
// keeps submitting; the caller holds one ticket per sweep.  Plain C++17, no HIP and no Python:
// the batch call, its free and its error text are function pointers, so the queue compiles and
// runs on the CPU with a stand-in (tests/sweep_pipe_main.cpp).
//
// Dispatch rules (those of ripser.SweepPipeline): the pending batch goes to a worker when it
// holds `coalesce` sweeps, when a sweep of another shape, dtype, residence or argument template
// arrives, when one of its tickets is waited on, and at flush / close.  Call n runs on worker
// n % depth, so the calls of one slot stay ordered.
#pragma once
#include <stdint.h>

#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/tda_rips.h"

namespace tda {

class SweepPipe {
public:
    using Runner = int (*)(const tda_rips_args*, tda_rips_result**);
    using Freer = void (*)(tda_rips_result*);
    using LastError = const char* (*)();

    static constexpr int kIdxBits = 4;  // a ticket is (call id << 4) | index of the sweep in its call
    static_assert((1 << kIdxBits) >= TDA_MAX_PARTS, "a ticket's index field holds every part of a call");

    // what wait() hands back: rc != 0 means the call failed and err holds its message
    struct Waited {
        int rc = 0;
        std::string err;
        tda_rips_result* res = nullptr;
        int64_t lo = 0, hi = 0;  // the ticket's layers of the call's result
        int32_t n_sweeps = 0;
        uint64_t call = 0;
    };

    SweepPipe(int depth, int coalesce, Runner run, Freer free_result, LastError last_error)
        : depth_(depth), coalesce_(coalesce), run_(run), free_(free_result), last_error_(last_error), workers_(depth) {
        for (int i = 0; i < depth_; ++i) workers_[i].th = std::thread([this, i] { work(i); });
    }
    SweepPipe(const SweepPipe&) = delete;
    SweepPipe& operator=(const SweepPipe&) = delete;

    // close(), then whatever tickets are still unreleased lose their results
    ~SweepPipe() {
        close();
        for (auto& kv : calls_)
            if (kv.second->res) free_(kv.second->res);
    }

    // One sweep: (L, N, D) of `dtype` at x, in host memory or (on_device) on tmpl->device.  *tmpl
    // gives every other argument of the call; sweeps share a call only under one tmpl_id, and the
    // template is copied when a batch starts, so equal ids must mean equal contents.  x (and
    // tmpl->labels) must stay valid until the ticket's wait() returns.  0, or TDA_E_INVALID
    // (closed pipe, bad shape) with the message in *err.
    int submit(const tda_rips_args& tmpl, int64_t tmpl_id, const void* x, int64_t L, int64_t N, int64_t D, int32_t dtype,
               int32_t on_device, uint64_t* ticket, std::string* err) {
        if (!x || L < 1 || N < 1 || D < 1) return bad(err, "tda_pipe_submit: x is NULL or a dimension is < 1");
        if (dtype != TDA_F32 && dtype != TDA_F64) return bad(err, "dtype must be TDA_F32 or TDA_F64");
        std::lock_guard<std::mutex> g(mu_);
        if (closed_) return bad(err, "the pipeline is closed");
        const Key key = {L, N, D, tmpl_id, dtype, on_device ? 1 : 0};
        if (pending_ && !(pending_->key == key)) dispatch_locked();
        if (!pending_) {
            auto c = std::make_unique<Call>();
            c->id = next_call_++;
            c->key = key;
            c->args = tmpl;
            pending_ = c.get();
            calls_.emplace(c->id, std::move(c));
        }
        Call* c = pending_;
        *ticket = (c->id << kIdxBits) | (uint64_t)c->parts.size();
        c->parts.push_back(x);
        c->refs++;
        if ((int)c->parts.size() >= coalesce_) dispatch_locked();
        return 0;
    }

    void flush() {
        std::lock_guard<std::mutex> g(mu_);
        dispatch_locked();
    }

    enum Mode { kPoll = 0, kBlock = 1, kDispatch = 2 };

    // kBlock: block until the ticket's call has run (dispatching it first if it is still
    // pending).  kPoll: never block and dispatch nothing; kDispatch: dispatch the ticket's batch
    // if it is pending, then as kPoll.  A call that has not run yet gives rc = kBusy (with
    // n_sweeps so far and call filled).  TDA_E_INVALID for a ticket that is unknown or released.
    static constexpr int kBusy = 1;
    Waited wait(uint64_t ticket, Mode mode = kBlock) {
        Waited w;
        std::unique_lock<std::mutex> g(mu_);
        Call* c = find_locked(ticket);
        if (!c) {
            w.rc = TDA_E_INVALID;
            w.err = "tda_pipe_wait: unknown or released ticket";
            return w;
        }
        if (c == pending_ && mode != kPoll) dispatch_locked();
        if (mode == kBlock) {
            // looked up again at every wake-up: another thread may release the ticket (and with the
            // call's last one the call itself goes) while this one sleeps
            done_cv_.wait(g, [&] { return !(c = find_locked(ticket)) || c->done; });
            if (!c) {
                w.rc = TDA_E_INVALID;
                w.err = "tda_pipe_wait: the ticket was released during the wait";
                return w;
            }
        }
        const int64_t i = (int64_t)(ticket & ((1u << kIdxBits) - 1));
        w.lo = i * c->key.L;
        w.hi = w.lo + c->key.L;
        w.n_sweeps = (int32_t)c->parts.size();
        w.call = c->id;
        if (!c->done) {
            w.rc = kBusy;
            return w;
        }
        w.rc = c->rc;
        w.err = c->err;
        w.res = c->res;
        return w;
    }

    // The ticket is finished with; the call's result is freed with its last ticket (at once if
    // the call is done, else when it is).  Returns the call's tickets still unreleased (>= 0), or
    // TDA_E_INVALID for an unknown or released ticket.
    int release(uint64_t ticket) {
        tda_rips_result* dead = nullptr;
        int left;
        {
            std::lock_guard<std::mutex> g(mu_);
            Call* c = find_locked(ticket);
            if (!c) return TDA_E_INVALID;
            c->released |= 1u << (ticket & ((1u << kIdxBits) - 1));
            left = --c->refs;
            if (left == 0 && c->done) {
                dead = c->res;
                calls_.erase(c->id);
            }
        }
        if (dead) free_(dead);
        return left;
    }

    // Dispatch what is pending, let the workers finish their queues and join them.  Tickets stay
    // valid for wait() and release(); submit() fails from here on.
    void close() {
        {
            std::lock_guard<std::mutex> g(mu_);
            if (closed_) return;
            dispatch_locked();
            closed_ = true;
        }
        for (auto& w : workers_) w.cv.notify_one();
        for (auto& w : workers_) w.th.join();
    }

    int depth() const { return depth_; }

private:
    struct Key {
        int64_t L, N, D, tmpl;
        int32_t dtype, on_device;
        bool operator==(const Key& o) const {
            return L == o.L && N == o.N && D == o.D && tmpl == o.tmpl && dtype == o.dtype && on_device == o.on_device;
        }
    };
    struct Call {
        uint64_t id = 0;
        Key key = {};
        tda_rips_args args = {};
        std::vector<const void*> parts;
        int refs = 0;           // tickets not yet released
        uint32_t released = 0;  // bit i: ticket i was released
        bool done = false;
        int rc = 0;
        std::string err;
        tda_rips_result* res = nullptr;
    };
    struct Worker {
        std::thread th;
        std::condition_variable cv;
        std::deque<Call*> q;
    };

    static int bad(std::string* err, const char* msg) {
        if (err) *err = msg;
        return TDA_E_INVALID;
    }

    Call* find_locked(uint64_t ticket) {
        auto it = calls_.find(ticket >> kIdxBits);
        if (it == calls_.end()) return nullptr;
        Call* c = it->second.get();
        const uint64_t i = ticket & ((1u << kIdxBits) - 1);
        if (i >= c->parts.size() || (c->released >> i & 1u)) return nullptr;
        return c;
    }

    void dispatch_locked() {
        if (!pending_) return;
        Worker& w = workers_[n_dispatched_++ % (uint64_t)depth_];
        w.q.push_back(pending_);
        pending_ = nullptr;
        w.cv.notify_one();
    }

    // every element finite: no exponent field of all ones (NaN and +-inf)
    static bool all_finite(const void* p, int64_t n, bool f64) {
        unsigned bad = 0;
        if (f64) {
            const uint64_t* q = static_cast<const uint64_t*>(p);
            for (int64_t i = 0; i < n; ++i) bad |= (unsigned)((q[i] & 0x7FF0000000000000ull) == 0x7FF0000000000000ull);
        } else {
            const uint32_t* q = static_cast<const uint32_t*>(p);
            for (int64_t i = 0; i < n; ++i) bad |= (unsigned)((q[i] & 0x7F800000u) == 0x7F800000u);
        }
        return !bad;
    }

    // one coalesced call on worker i's slot (outside the lock: parts, key and args are final once dispatched)
    void run_call(int i, Call* c, int* rc, std::string* err, tda_rips_result** res) {
        const Key& k = c->key;
        const int n = (int)c->parts.size();
        if (!k.on_device)
            for (const void* p : c->parts)
                if (!all_finite(p, k.L * k.N * k.D, k.dtype == TDA_F64)) {
                    *rc = TDA_E_INVALID;
                    *err = "Input contains NaN or infinity.";
                    return;
                }
        tda_rips_args a = c->args;
        a.dtype = k.dtype;
        a.x_on_device = k.on_device;
        a.L = k.L * n;
        a.N = k.N;
        a.D = k.D;
        a.slot = TDA_MAX_SLOTS - depth_ + i;  // the top `depth` slots: slot 0 keeps to plain calls
        if (n == 1) {
            a.x = c->parts[0];
            a.x_parts = nullptr;
            a.n_parts = 0;
        } else {  // parts: gathered on the device by the library
            a.x = nullptr;
            a.x_parts = c->parts.data();
            a.n_parts = n;
        }
        *rc = run_(&a, res);
        if (*rc != 0) {
            *err = last_error_();
            *res = nullptr;
        }
    }

    void work(int i) {
        Worker& w = workers_[i];
        std::unique_lock<std::mutex> g(mu_);
        for (;;) {
            w.cv.wait(g, [&] { return !w.q.empty() || closed_; });
            if (w.q.empty()) return;  // closed and drained
            Call* c = w.q.front();
            w.q.pop_front();
            g.unlock();
            int rc = 0;
            std::string err;
            tda_rips_result* res = nullptr;
            run_call(i, c, &rc, &err, &res);
            g.lock();
            c->rc = rc;
            c->err = std::move(err);
            c->res = res;
            c->done = true;
            if (c->refs == 0) {  // every ticket was released before the call ran
                calls_.erase(c->id);
                g.unlock();
                if (res) free_(res);
                g.lock();
            }
            done_cv_.notify_all();
        }
    }

    const int depth_, coalesce_;
    const Runner run_;
    const Freer free_;
    const LastError last_error_;
    std::mutex mu_;
    std::condition_variable done_cv_;
    std::vector<Worker> workers_;
    std::unordered_map<uint64_t, std::unique_ptr<Call>> calls_;  // pending, queued, running, or done with tickets out
    Call* pending_ = nullptr;
    uint64_t next_call_ = 1, n_dispatched_ = 0;
    bool closed_ = false;
};

}  // namespace tda
