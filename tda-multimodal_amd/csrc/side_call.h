// side_call.h -- the frame of a call of an entry beside the persistence pipeline (greedy_host.h, resample_host.h,
// perm_host.h, ed_host.h, umap_host.h; the diagram entries through dgm_call.h, which sits on it), part of
// rips.hip's translation unit.  The frame is the workspace of (entry, device) of aux_ws.h and its lock, held
// until the frame goes.  It offers the steps of a call one by one and forces no order on them: every entry
// makes the runtime calls it has always made, in the order it has always made them (an entry that reads the
// caller's device memory orders itself after the caller before or after it reserves; the spectral entries
// record no events).  Every step returns an error code.
#pragma once

namespace {

int need_device(int dev) { return tda_device_ok(dev) ? 0 : fail(TDA_E_NODEVICE, "no gfx950 device at ordinal " + std::to_string(dev)); }

struct SideCall {
    // the workspace and its lock, the device, the stream and the first n_events timing events
    int open(AuxEntry entry, int dev, int n_events = 0) {
        w = &aux_ws(entry, dev);
        guard = std::unique_lock<std::mutex>(w->mu);
        return aux_open(*w, n_events);
    }
    int lds_attr(const void* fn, size_t bytes) { return aux_lds_attr(*w, fn, bytes); }  // fn's dynamic-LDS limit
    int reserve(size_t bytes) { return aux_reserve(*w, bytes); }
    template <typename Also>
    int reserve(size_t bytes, Also&& also) {  // with a call's further allocations, in the same hold of the allocation scope
        return aux_reserve(*w, bytes, also);
    }
    int reserve_pinned(size_t bytes) { return aux_reserve_pinned(*w, bytes); }
    int after_caller(void* caller) { return aux_after_caller(*w, caller); }  // device inputs: read after the caller's queued work

    hipStream_t stream() const { return w->stream; }
    hipEvent_t event(int i) const { return w->ev[i]; }
    char* buf() const { return w->buf.p; }
    template <typename T>
    T* at(size_t offset) const {
        return (T*)(w->buf.p + offset);
    }
    const void* pinned() const { return w->hout.p; }  // the pinned result, and the address the device writes it at
    void* pinned_dev() const { return w->hout.dev; }

    int start() {  // ev[0]
        HIPC(hipEventRecord(w->ev[0], w->stream));
        return 0;
    }
    int drain() {  // ev[1] and the synchronise
        HIPC(hipEventRecord(w->ev[1], w->stream));
        HIPC(hipStreamSynchronize(w->stream));
        return 0;
    }
    int elapsed(float* t, int from = 0, int to = 1) {
        HIPC(hipEventElapsedTime(t, w->ev[from], w->ev[to]));
        return 0;
    }
    float ms = 0.0f;  // finish: the device time between ev[0] and ev[1]
    int finish() {
        if (int rc = drain()) return rc;
        return elapsed(&ms);
    }

private:
    AuxWs* w = nullptr;
    std::unique_lock<std::mutex> guard;  // w->mu, until the frame goes
};

// An entry's result is an Impl whose first member is the public struct `pub`.  Its return, with or without
// a launch: the result handed to the caller; and its free (NULL is a no-op).
template <typename Impl, typename Pub>
int side_return(std::unique_ptr<Impl>& R, Pub** out, float ms = 0.0f) {
    R->pub.device_ms = ms;
    *out = &R.release()->pub;
    return 0;
}
template <typename Impl, typename Pub>
void side_free(Pub* r) {
    delete reinterpret_cast<Impl*>(r);
}

}  // namespace
