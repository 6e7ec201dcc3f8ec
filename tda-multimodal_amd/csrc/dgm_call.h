// dgm_call.h -- the frame of a call of include/tda_dgm.h, shared by its eight entries (dgm_host.h,
// bn_host.h, ws_host.h, vec_host.h, hk_host.h, pc_host.h, pf_host.h), part of rips.hip's translation unit.
//
// Every entry has one shape: plan on the host (dgm_plan.h), lay the call's buffer out -- the arrays
// the device reads first, then the regions it only writes --, upload the first part in one copy,
// launch, download one region, and time the whole between two events of the entry's workspace
// (aux_ws.h, through the steps of side_call.h's frame, on which this one sits).  An entry says what
// it uploads and what it needs (upload, device), then
//     begin   the workspace of (entry, device), its lock for the rest of the call, the stream and
//             the two events, the kernel's dynamic-LDS limit if it needs one, the buffer,
//             ev[0], the upload;
//     ...     its own launches on stream(), reading and writing at<T>(offset);
//     end     the download, ev[1], the synchronise and the time between the events (ms).
// begin and end return an error code (HIPC returns from the function it stands in).
#pragma once
#include "dgm_plan.h"
#include "side_call.h"

namespace {

struct DgmCall : SideCall {
    // `bytes` at p, uploaded by begin: its 256-byte-aligned offset in the call's buffer
    size_t upload(const void* p, size_t bytes) {
        const size_t o = cv.take(bytes);
        items.push_back({o, p, bytes});
        up_bytes = cv.o;
        return o;
    }
    template <typename T>
    size_t upload(const std::vector<T>& v) {
        return upload(v.data(), v.size() * sizeof(T));
    }
    // a region only the device writes, after everything uploaded
    size_t device(size_t bytes) { return cv.take(bytes); }

    int begin(AuxEntry entry, int dev, const void* lds_fn = nullptr, size_t lds_bytes = 0) {
        host.resize(up_bytes);
        for (const Item& i : items)
            if (i.bytes) std::memcpy(host.data() + i.at, i.p, i.bytes);
        if (int rc = open(entry, dev, 2)) return rc;
        if (lds_fn)
            if (int rc = lds_attr(lds_fn, lds_bytes)) return rc;
        if (int rc = reserve(cv.o)) return rc;
        if (int rc = start()) return rc;
        HIPC(hipMemcpyAsync(buf(), host.data(), up_bytes, hipMemcpyHostToDevice, stream()));
        return 0;
    }
    int end(void* dst, size_t offset, size_t bytes) {
        HIPC(hipMemcpyAsync(dst, buf() + offset, bytes, hipMemcpyDeviceToHost, stream()));
        return finish();  // ms: the device time between the two events
    }

private:
    struct Item {
        size_t at;
        const void* p;
        size_t bytes;
    };
    Carve cv;
    std::vector<Item> items;
    size_t up_bytes = 0;
    std::vector<char> host;  // the upload, packed
};

// the four arrays of a PairPlan, uploaded first and in this order
struct PairAt {
    size_t pts, off, pairs, order;
    PairAt(DgmCall& call, const PairPlan& pl) : pts(call.upload(pl.pts)), off(call.upload(pl.off)), pairs(call.upload(pl.pairs)), order(call.upload(pl.order)) {}
};

// an entry's return, with or without a launch: side_return
template <typename Impl, typename Pub>
int dgm_return(std::unique_ptr<Impl>& R, Pub** out, float ms = 0.0f) {
    return side_return(R, out, ms);
}

}  // namespace
