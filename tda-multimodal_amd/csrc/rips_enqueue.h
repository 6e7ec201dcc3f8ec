// rips_enqueue.h -- one call's context (struct Call) and its launch sequence: a function per
// stage, and enqueue_schedule, which says which stage goes on which stream after which event.
// Part of rips.hip's translation unit (Plan, Workspace, StageTimer, HIPC and fail come from there).
// The sequence runs eagerly or inside a stream capture (launch_or_capture); the order of the
// enqueues on each stream is what a captured graph bakes in.
#pragma once

// Everything one attempt of a call needs, on the stack of run_pipeline; the stage functions take it
// by reference (never copied: the host side of a small call is counted in microseconds).
struct Call {
    const tda_rips_args& a;
    const int input_kind;  // 0 = points (dtype), 1 = square distance (dtype), 2 = condensed f32
    const void* const host_or_dev;
    const Attempt at;
    Workspace& w;
    Plan p;
    hipStream_t s = nullptr;  // the library's main stream: all work is ordered after the caller's stream on it
    char* B = nullptr;        // device workspace base
    int n = 0, L = 0;
    size_t esz = 4;
    float* dist = nullptr;
    LayerStats* stats = nullptr;
    uint32_t* rowmax = nullptr;
    // the input as the launch sequence reads it (pinned staging, gathered parts or the caller's pointer)
    const void* xsrc = nullptr;
    int nparts = 0;
    bool host_in = false, dev_parts = false;
    size_t xbytes = 0, dbytes = 0;
    // kernel argument blocks (wire_buffers; ps: run_pipeline, the output-capacity re-emit needs it too)
    PairSet ps = {};
    DimBufs db[3] = {};
    Reduce2Bufs rb = {};
    SortArgs sa = {};
    SmallBufs sb = {};
    DenseBufs dnb = {};
    BigBufs gb = {};
    ParBufs pb = {};
    Pair *pairs1 = nullptr, *pairs2 = nullptr;
    StageTimer tm, tm2, tm3, tm4;  // main stream, stream2, stream3, stream4
    // switches derived from the arguments (run_pipeline) ...
    bool no_ph = false;  // TDA_FLAG_NO_PERSISTENCE: distances + side metrics only
    int nls = 0, sil_K = 0;
    size_t sil_out_off = 0;
    bool want_tn = false, serial_stages = false, dist_mfma = false;
    bool capture = false;  // the sequence is being captured: ev0 / ev1 are recorded around the graph launch instead
    float capf = 0.0f;
    // ... and from the plan (enqueue_schedule)
    int order = 0;
    bool split2 = false, h2_side = false, h2_late = false, app1_side = false;
    uint64_t h2_late_grid = 0;
    uint32_t h2_late_delay_us = 0;

    Call(const tda_rips_args& a_, int kind, const void* src, const Attempt& at_, Workspace& w_)
        : a(a_), input_kind(kind), host_or_dev(src), at(at_), w(w_), tm{w_.stage_ev, nullptr, false, {}},
          tm2{w_.stage_ev2, nullptr, false, {}}, tm3{w_.stage_ev3, nullptr, false, {}}, tm4{w_.stage_ev4, nullptr, false, {}} {}
    Call(const Call&) = delete;
    // ev0 / ev1 bracket the whole sequence; a graph replay records them around the launch
    hipError_t rec_t(hipEvent_t e) const { return capture ? hipSuccess : hipEventRecord(e, s); }
};

#define MARK(name) \
    do {           \
        if (int rc_ = c.tm.mark(name)) return rc_; \
    } while (0)

// the kernels' argument blocks, from the plan's offsets into the workspace
void wire_buffers(Call& c) {
    const Plan& p = c.p;
    char* B = c.B;
    for (int d = 1; d <= p.maxdim; ++d) {
        DimBufs& db = c.db[d];
        db.cleared = d == 1 ? nullptr : (const uint32_t*)(B + p.o_piv[d - 1]);
        db.cleared_words = d == 1 ? 0 : p.piv_words[d - 1];
        db.pivbits = (uint32_t*)(B + p.o_piv[d]);
        db.piv_words = p.piv_words[d];
        db.resid = (uint64_t*)(B + p.o_resid[d]);
        db.rcap = p.rcap[d];
        db.ncand = p.ncand[d];
        db.clr = d == 2 && p.piv2_sparse ? (uint64_t*)(B + p.o_clr2) : nullptr;
        db.clr_cap = d == 2 && p.piv2_sparse ? p.clr_cap : 0;
        c.sa.resid[d] = db.resid;
        c.sa.rcap[d] = db.rcap;
    }
    Reduce2Bufs& rb = c.rb;
    rb.rmap_keys = (uint64_t*)(B + p.o_rmk);
    rb.rmap_vals = (uint32_t*)(B + p.o_rmv);
    rb.rmap_stride = p.rmap_stride;
    rb.roff = (uint64_t*)(B + p.o_voff);
    rb.rlen = (uint32_t*)(B + p.o_vlen);
    rb.rpool = (uint64_t*)(B + p.o_vpool);
    rb.rpool_cap = p.vpool_cap;
    rb.wtmp = (uint64_t*)(B + p.o_wt);
    rb.wtmp_stride = 2 * (p.lds_mode ? 8192 : p.wcap_g);
    rb.wlog = (uint64_t*)(B + p.o_wk);
    rb.windex = (uint64_t*)(B + p.o_wl);
    rb.wfill = (uint32_t*)(B + p.o_wp);
    rb.wcap = p.wcap_g;
    rb.mst = (const uint32_t*)(B + p.o_mst);
    rb.mst_words = p.mst_words;
    c.pairs1 = (Pair*)(B + p.o_pairs[1]);
    c.pairs2 = p.maxdim >= 2 ? (Pair*)(B + p.o_pairs[2]) : c.pairs1;
    if (p.dense) {
        SmallBufs& sb = c.sb;
        sb.p1_next = (uint32_t*)(B + p.o_p1next);
        sb.p1_key = (uint64_t*)(B + p.o_p1k);
        sb.p1_info = (uint32_t*)(B + p.o_p1i);
        sb.p1_pidx = (uint32_t*)(B + p.o_p1x);
        sb.roff2 = (uint64_t*)(B + p.o_roff2);
        sb.rlen2 = (uint32_t*)(B + p.o_rlen2);
        sb.rpool2 = (uint64_t*)(B + p.o_rpool2);
        sb.rpool2_cap = p.vpool_cap;
        sb.p1_used = (unsigned long long*)(B + p.o_p1used);
        sb.p1_wcap = kP1WCap;
        DenseBufs& dnb = c.dnb;
        dnb.recs = (EdgeRec*)(B + p.o_recs);
        dnb.cls = (uint32_t*)(B + p.o_cls);
        dnb.res1 = (uint32_t*)(B + p.o_res1);
        dnb.inv32 = (uint32_t*)(B + p.o_inv32);
        dnb.rank_of = (uint16_t*)(B + p.o_rof);
        dnb.tri_stride = p.tri_stride;
        dnb.cls2 = (uint16_t*)(B + p.o_cls2);
        dnb.n2p = p.n2p;
        dnb.inv = (uint16_t*)(B + p.o_inv);
        dnb.E = (uint32_t)binom((uint64_t)c.n, 2);
        dnb.inv_stride = p.inv_stride;
        dnb.K = p.dK;
        dnb.epos = (uint32_t*)(B + p.o_epos);
        dnb.cobt = (uint16_t*)(B + p.o_cobt);
        dnb.cob_stride = p.cob_stride;
        dnb.eM = (uint64_t*)(B + p.o_eM);
        dnb.necnt = (uint32_t*)(B + p.o_necnt);
    }
    if (p.big) {
        BigBufs& gb = c.gb;
        gb.log = rb.wlog;
        gb.index = rb.windex;
        gb.fill = rb.wfill;
        gb.bref = (uint32_t*)(B + p.o_bref);
        gb.cap = p.wcap_g;
        gb.bcap = p.wcap_g;
        gb.step_limit = step_limit();
        gb.wide = p.wide ? 1 : 0;
        gb.dcode = (const uint32_t*)(B + p.o_dcode);
        gb.dsort = (const uint64_t*)(B + p.o_dsort);
        gb.ecap = p.ecap;
    }
    if (p.par) {
        ParBufs& pb = c.pb;
        pb.ctl = (ParCtl*)(B + p.o_pctl);
        pb.item_base = (uint64_t*)(B + p.o_pitem);
        pb.okey = (uint64_t*)(B + p.o_pokey);
        pb.oval = (uint64_t*)(B + p.o_poval);
        pb.ostride = p.ostride;
        pb.colpiv = (uint64_t*)(B + p.o_colpiv);
        pb.rec = (uint64_t*)(B + p.o_prec);
        pb.rec_cap = p.rec_cap;
        pb.rpool = (uint64_t*)(B + p.o_prpool);
        pb.rpool_cap = p.rpool_cap;
        pb.bpool = (uint64_t*)(B + p.o_pbpool);
        pb.bpool_cap = p.bpool_cap;
        pb.rq = (uint64_t*)(B + p.o_prq);
        pb.rq_cap = p.rq_cap;
        pb.step_limit = step_limit();
        pb.capf = c.capf;
        pb.dbg = p.o_pdbg ? (uint64_t*)(B + p.o_pdbg) : nullptr;  // profile builds only
    }
}

// ---- distances of (L, n, D) point clouds: the one kernel selection (DistSel, rips_plan.h) for every
// entry that needs the sklearn-exact f32 matrix.  rowmax must be zeroed before; gpart / npart are
// read only when sel.partials().  mark(name) closes a stage (the call's stage timer, or a no-op).
struct DistLaunch {
    const void* x;  // device (L, n, D), f32 or f64
    int dtype, n;
    int64_t D;
    int L;
    DistSel sel;
    float* dist;
    uint32_t* rowmax;
    double *gpart, *npart, *d64;
};
template <class Mark>
int launch_point_distances(hipStream_t s, const DistLaunch& d, Mark&& mark) {
    const void* x = d.x;
    const int n = d.n, L = d.L;
    float* dist = d.dist;
    uint32_t* rowmax = d.rowmax;
    double *gpart = d.gpart, *npart = d.npart, *d64 = d.d64;
    const int dsplit = d.sel.dsplit;
    const bool mfma = d.sel.mfma, gram_layer = d.sel.gram_layer;
    dim3 grid((n + 15) / 16, (n + 15) / 16, L);
    const unsigned nt = (unsigned)((n + kDmT - 1) / kDmT);
    const dim3 gsplit(nt * (nt + 1) / 2, L, (unsigned)dsplit);
    const dim3 gcomb((unsigned)std::min<uint64_t>(1024, ((uint64_t)n * n + 255) / 256), L);
    if (mfma && dsplit > 1 && d.dtype == TDA_F64) {
        hipLaunchKernelGGL((k_distance_mfma<double, 0, true>), gsplit, dim3(256), 0, s, (const double*)x, n, (int)d.D, dist, rowmax,
                           gpart, npart, (double*)nullptr);
        hipLaunchKernelGGL((k_distance_combine<double, 0>), gcomb, dim3(256), 0, s, gpart, npart, dsplit, n, dist, rowmax, d64);
        hipLaunchKernelGGL(k_rowmax, dim3((n + 3) / 4, L), dim3(256), 0, s, dist, n, rowmax);
    } else if (mfma && (dsplit > 1 || gram_layer)) {
        if (gram_layer)
            hipLaunchKernelGGL(k_gram_layer, dim3((unsigned)dsplit, L), dim3(256), 0, s, (const float*)x, n, (int)d.D, gpart, npart);
        else
            hipLaunchKernelGGL((k_distance_mfma<float, 0, true>), gsplit, dim3(256), 0, s, (const float*)x, n, (int)d.D, dist, rowmax,
                               gpart, npart);
        if (int rc = mark(gram_layer ? "k_gram_layer" : "k_distance_mfma")) return rc;  // the Gram kernel alone (bench roofline): combine, row maxima: own stages
        hipLaunchKernelGGL((k_distance_combine<float, 0>), gcomb, dim3(256), 0, s, gpart, npart, dsplit, n, dist, rowmax);
        if (int rc = mark("k_distance_combine")) return rc;
        hipLaunchKernelGGL(k_rowmax, dim3((n + 3) / 4, L), dim3(256), 0, s, dist, n, rowmax);
    } else if (mfma && d.dtype == TDA_F64)
        hipLaunchKernelGGL((k_distance_mfma<double>), dim3(nt * (nt + 1) / 2, L), dim3(256), 0, s, (const double*)x, n, (int)d.D,
                           dist, rowmax, (double*)nullptr, (double*)nullptr, d64);
    else if (mfma)
        hipLaunchKernelGGL((k_distance_mfma<float>), dim3(nt * (nt + 1) / 2, L), dim3(256), 0, s, (const float*)x, n, (int)d.D,
                           dist, rowmax, (double*)nullptr, (double*)nullptr);
    else if (d.dtype == TDA_F64)
        hipLaunchKernelGGL(k_distance<double>, grid, dim3(256), 0, s, (const double*)x, n, (int)d.D, dist, rowmax, d64);
    else
        hipLaunchKernelGGL(k_distance<float>, grid, dim3(256), 0, s, (const float*)x, n, (int)d.D, dist, rowmax);
    return 0;
}

// (L, n, n) distance matrices of either dtype -> the f32 matrices every entry works on (upper triangle, diagonal 0)
void launch_square_dist(hipStream_t s, const void* x, int dtype, int n, int L, float* dist) {
    const unsigned gx = (unsigned)std::min<uint64_t>(1024, ((uint64_t)n * n + 255) / 256);
    if (dtype == TDA_F64)
        hipLaunchKernelGGL(k_square_dist<double>, dim3(gx, L), dim3(256), 0, s, (const double*)x, n, dist);
    else
        hipLaunchKernelGGL(k_square_dist<float>, dim3(gx, L), dim3(256), 0, s, (const float*)x, n, dist);
}

// The f32 matrices of a chunk of lc layers at x (points, or distance matrices: is_dist), into sq.o_dm of the
// workspace at B (SqDistPlan, side_plan.h): host input goes through sq.o_x first; staged() queues what else the
// entry uploads per chunk, where it always has (after the input).
template <class Staged>
int enqueue_chunk_distances(hipStream_t s, char* B, const SqDistPlan& sq, const void* x, int dtype, int64_t D, bool is_dist, size_t lc, Staged&& staged) {
    if (sq.host_in) {
        HIPC(hipMemcpyAsync(B + sq.o_x, x, lc * sq.x_layer, hipMemcpyHostToDevice, s));
        x = B + sq.o_x;
    }
    if (int rc = staged()) return rc;
    float* dm = (float*)(B + sq.o_dm);
    if (!is_dist) {
        HIPC(hipMemsetAsync(B + sq.o_rm, 0, lc * sq.N * 4, s));  // the distance kernels fold row maxima in (unused by these entries)
        const DistLaunch dl = {x, dtype, (int)sq.N, D, (int)lc, sq.sel, dm, (uint32_t*)(B + sq.o_rm), (double*)(B + sq.o_gp), (double*)(B + sq.o_np), nullptr};
        if (int rc = launch_point_distances(s, dl, [](const char*) { return 0; })) return rc;
    } else {
        launch_square_dist(s, x, dtype, (int)sq.N, (int)lc, dm);
    }
    HIPC(hipGetLastError());
    return 0;
}

// ---- distances (+ row maxima for the enclosing radius)
int enqueue_distances(Call& c) {
    const tda_rips_args& a = c.a;
    const Plan& p = c.p;
    hipStream_t s = c.s;
    char* B = c.B;
    const int n = c.n, L = c.L;
    float* dist = c.dist;
    uint32_t* rowmax = c.rowmax;
    if (c.input_kind == 0) {
        const void* x = c.xsrc;
        if (!a.x_on_device) {
            HIPC(hipMemcpyAsync(B + p.o_x, x, (size_t)L * n * p.D * c.esz, hipMemcpyHostToDevice, s));
            x = B + p.o_x;
        }
        const DistLaunch dl = {x, p.dtype, n, p.D, L, p.dist, dist, rowmax, (double*)(B + p.o_gpart), (double*)(B + p.o_npart),
                               p.want64 ? (double*)(B + p.o_d64) : nullptr};
        if (int rc = launch_point_distances(s, dl, [&](const char* name) { return c.tm.mark(name); })) return rc;
    } else {
        const void* x = c.xsrc;
        unsigned gx = (unsigned)std::min<uint64_t>(1024, ((uint64_t)n * n + 255) / 256);
        if (c.input_kind == 1) {
            if (!a.x_on_device) {
                HIPC(hipMemcpyAsync(B + p.o_x, x, (size_t)L * n * n * c.esz, hipMemcpyHostToDevice, s));
                x = B + p.o_x;
            }
            launch_square_dist(s, x, p.dtype, n, L, dist);
        } else {
            const uint64_t ne = binom((uint64_t)n, 2);
            if (ne) HIPC(hipMemcpyAsync(B + p.o_x, x, ne * 4, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_square_from_condensed, dim3(gx), dim3(256), 0, s, (const float*)(B + p.o_x), n, dist);
        }
        HIPC(hipGetLastError());
        hipLaunchKernelGGL(k_rowmax, dim3((n + 3) / 4, L), dim3(256), 0, s, dist, n, rowmax);
    }
    HIPC(hipGetLastError());
    MARK(c.input_kind != 0 ? "k_square_dist" : c.dist_mfma ? (p.dist.partials() && p.dtype == TDA_F32 ? "k_rowmax" : "k_distance_mfma") : "k_distance");
    return 0;
}

// H0 of n > kSmallN on stream4: the LDS-staged one-wave Prim up to kH0WaveMaxN, above it
// Borůvka over the whole GPU and the elder rule
int enqueue_h0_large(Call& c) {
    const tda_rips_args& a = c.a;
    const Plan& p = c.p;
    hipStream_t s4 = c.w.stream4;
    char* B = c.B;
    const int n = c.n, L = c.L;
    float* dist = c.dist;
    LayerStats* stats = c.stats;
    // the block size, both LDS carves, the rounds and the elder-rule variant: h0_shape (rips_plan.h)
    const H0Shape h0 = h0_shape(n);
    const int T = h0.T;
    const bool dlds = h0.dlds;
    const uint64_t ch = h0.ch;
    const size_t lds = h0.lds;
    if (dlds) {
        hipLaunchKernelGGL((k_h0<kH0WaveQ, true>), dim3(L), dim3(T), lds, s4, dist, n, a.thresh, stats, (uint32_t*)(B + p.o_mst),
                           p.mst_words, (Pair*)(B + p.o_pairs[0]), p.pcap[0], (uint64_t*)(B + p.o_h0s), ilog2(ch),
                           (const BorCtl*)nullptr);
        return 0;
    }
    // Borůvka over the whole GPU: ceil(log2 N) rounds of (cheapest edges, hooking)
    int32_t* bcomp = (int32_t*)(B + p.o_bcomp);
    uint64_t* bcheap = (uint64_t*)(B + p.o_bcheap);
    BorCtl* bctl = (BorCtl*)(B + p.o_bctl);
    hipLaunchKernelGGL(k_bor_init, dim3(L), dim3(256), 0, s4, c.rowmax, n, a.thresh, stats, bcomp, bcheap, bctl);
    const size_t hl = h0.hl;
    const int rounds = h0.rounds;
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(k_bor_min, dim3((unsigned)((n + 3) / 4), L), dim3(256), 0, s4, dist, n, stats, bcomp, bcheap, bctl,
                           r == 0 ? 1 : 0);
        if (r == 0)
            if (int rc = c.tm4.mark("k_bor_min")) return rc;
        hipLaunchKernelGGL(k_bor_hook, dim3(L), dim3(1024), hl, s4, n, bcomp, bcheap, bctl, (uint64_t*)(B + p.o_h0s));
        if (r == 0)
            if (int rc = c.tm4.mark("k_bor_hook")) return rc;
    }
    HIPC(hipGetLastError());
    if (int rc = c.tm4.mark("k_bor_rounds")) return rc;
    // elder rule: one wave with register labels up to N = 64 * kH0BorWQ, thread 0 above
    if (h0.elder == kH0ElderWave)
        hipLaunchKernelGGL((k_h0<kH0BorWQ, false, true>), dim3(L), dim3(T), lds, s4, dist, n, a.thresh, stats,
                           (uint32_t*)(B + p.o_mst), p.mst_words, (Pair*)(B + p.o_pairs[0]), p.pcap[0], (uint64_t*)(B + p.o_h0s),
                           ilog2(ch), (const BorCtl*)bctl);
    else
        hipLaunchKernelGGL((k_h0<0, false, true>), dim3(L), dim3(T), lds, s4, dist, n, a.thresh, stats, (uint32_t*)(B + p.o_mst),
                           p.mst_words, (Pair*)(B + p.o_pairs[0]), p.pcap[0], (uint64_t*)(B + p.o_h0s), ilog2(ch),
                           (const BorCtl*)bctl);
    return 0;
}

// ---- H0 on its own stream: it overlaps the apparent-pair kernels, which
// do not need the spanning forest (a forest edge is an H0 death, never an
// apparent column; the reductions skip forest edges among the residuals).
// The triangle ranks of the dense H1 chain go on a second side stream.
// Enqueued after apparent<1>, so the critical path's kernels are queued first.
int enqueue_side(Call& c) {
    const tda_rips_args& a = c.a;
    const Plan& p = c.p;
    Workspace& w = c.w;
    char* B = c.B;
    const int n = c.n, L = c.L;
    float* dist = c.dist;
    LayerStats* stats = c.stats;
    hipStream_t s2 = w.stream2, s4 = w.stream4;
    HIPC(hipStreamWaitEvent(s2, w.evf, 0));
    HIPC(hipStreamWaitEvent(s4, w.evf, 0));
    if (int rc = c.tm2.begin()) return rc;
    if (int rc = c.tm4.begin()) return rc;
    if (c.no_ph) {
        // TDA_FLAG_NO_PERSISTENCE: no spanning forest, no H0 pairs
    } else if (n <= kSmallN) {
        hipLaunchKernelGGL(k_h0_wave, dim3(L), dim3(64), 64 * 64 * 4 + 64 * 4 + 64 * 8, s4, dist, n, c.rowmax, a.thresh, stats,
                           (uint32_t*)(B + p.o_mst), p.mst_words, (Pair*)(B + p.o_pairs[0]), p.pcap[0]);
    } else {
        if (int rc = enqueue_h0_large(c)) return rc;
    }
    HIPC(hipGetLastError());
    if (!c.no_ph)
        if (int rc = c.tm4.mark("k_h0")) return rc;
    HIPC(hipEventRecord(w.evh, s4));
    if (c.nls) {  // silhouette scores on the same distance matrices (sklearn semantics), after the H0 join
        const size_t lds = silhouette_lds(c.sil_K, n);
        hipLaunchKernelGGL(k_silhouette, dim3(L, c.nls), dim3(kSilT), lds, s4, dist, n, (const int32_t*)w.hsil.dev, c.sil_K,
                           (double*)(w.hsil.dev + c.sil_out_off));
        HIPC(hipGetLastError());
        if (int rc = c.tm4.mark("k_silhouette")) return rc;
    }
    if (c.want_tn) {  // TwoNN intrinsic dimension on the same distance matrices
        // beside H0 on the ranks stream when there are no ranks (the raw-activation sweeps:
        // H0 and TwoNN only read the distances; r03 raw4096: they ran back to back on s4)
        // (only without H1: with H1 the main stream joins s2 before the reduction, and
        // TwoNN there would sit on the critical path -- ADVICE r03)
        const bool tn_s2 = !p.dense && p.maxdim == 0;
        const int pw2 = twonn_pw2(n);
        hipLaunchKernelGGL(k_twonn, dim3(L), dim3(kTnT), (size_t)pw2 * 4, tn_s2 ? s2 : s4, dist, n, a.twonn_discard, a.twonn_eps, pw2,
                           w.htn.dev);
        HIPC(hipGetLastError());
        if (int rc = (tn_s2 ? c.tm2 : c.tm4).mark("k_twonn")) return rc;
    }
    if (c.nls || c.want_tn) HIPC(hipEventRecord(w.evsil, s4));
    if (p.dense) {  // triangle ranks for the dense H1 chain, off the critical path
        const dim3 pg((unsigned)L, (unsigned)((c.dnb.E + kPrepEdges - 1) / kPrepEdges + 1));  // + the rank-sort block
        hipLaunchKernelGGL(k_prep_edges, pg, dim3(kPrepT), p.prep_lds, s2, dist, n, c.rowmax, a.thresh, c.dnb, p.cmode, stats);
        HIPC(hipGetLastError());
        if (int rc = c.tm2.mark("k_prep_edges")) return rc;
        // blocks per layer: 8 up to 64 layers (sweep48, 32 layers: 27 -> 18 us), 4 above (256 layers:
        // 83 us with 4, 96 with 8 -- the per-block staging and scan then cost more than the spread saves)
        const int ptb = test_env("TDA_PREP_TAB_BLOCKS") ? std::max(1, atoi(test_env("TDA_PREP_TAB_BLOCKS")))
                                                       : (L <= 64 ? 2 * kPrepTabBlocks : kPrepTabBlocks);
        hipLaunchKernelGGL(k_prep_tables, dim3(L, ptb), dim3(kPrepTabT), prep_tables_lds(n), s2, dist, n, c.dnb, p.cmode, stats);
        HIPC(hipGetLastError());
        if (int rc = c.tm2.mark("k_prep_tables")) return rc;
    }
    HIPC(hipEventRecord(w.evj, s2));
    return 0;
}

// apparent pairs of dim d (parallel over the candidate columns); the residual columns go to db[d].resid
void enqueue_apparent(Call& c, int d, hipStream_t st, uint64_t total_override = 0) {
    const tda_rips_args& a = c.a;
    const Plan& p = c.p;
    const int n = c.n, L = c.L;
    float* dist = c.dist;
    LayerStats* stats = c.stats;
    uint32_t* rowmax = c.rowmax;
    DimBufs* db = c.db;
    uint64_t blocks = (p.ncand[d] + 255) / 256;
    // total blocks over all layers: measured (r01, sweep48) 1024 beats 4096,
    // whose grid holds every CU while the critical small kernels wait; off
    // the dense path the apparent kernels run alone: 4096 (r02, grid144:
    // apparent<2> 1.08 -> 0.87 ms; staging the 83-KB matrix in LDS: 2.25 ms)
    const char* app_env = test_env("TDA_APP_GRID");
    const uint64_t app_total = app_env ? strtoull(app_env, nullptr, 10) : total_override ? total_override : (p.dense ? 1024 : 4096);
    unsigned gx = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks, std::max<uint64_t>(1, app_total / L)));
    const int app_lds_max = test_env("TDA_APP_LDS_MAXN") ? atoi(test_env("TDA_APP_LDS_MAXN")) : kAppLdsMaxN;
    const bool dl = n <= app_lds_max && 16 + (size_t)n * n * 4 <= (size_t)kLdsMax;
    const size_t alds = 16 + (dl ? (size_t)n * n * 4 : 0);
    // N <= 64: the small-N pass (32-bit decode, 4 vertices per LDS read); TDA_APP_SMALL=0 -> k_apparent
    if (n <= 64 && dl && !test_env_is("TDA_APP_SMALL", "0")) {
        // the pivot bitmap copied in LDS when it fits and a block's simplices outnumber a quarter
        // of its words (every block flushes the whole copy): r06, 160 layers per call,
        // apparent<1> 24.7 -> 19.3 us, apparent<2> 73.7 -> 57.0 us; at 32 layers per call (540
        // triangles per block) the flushes cost more than the atomics saved: call 0.171 -> 0.177 ms.
        // TDA_APP_PIV_LDS=0 / 1: never / always.
        const uint64_t per_block = (p.ncand[d] + gx - 1) / gx;
        const bool pl_fit = db[d].piv_words * 4 <= kSmallPivLdsMax;
        const bool pl_on = test_env_is("TDA_APP_PIV_LDS", "1") ? pl_fit
                           : test_env_is("TDA_APP_PIV_LDS", "0") ? false
                                                                : pl_fit && per_block * 4 >= db[d].piv_words;
        const uint32_t pl_words = pl_on ? (uint32_t)db[d].piv_words : 0u;
        const size_t slds = 16 + small_piv_offset(n) + 4ull * pl_words;
        if (d == 1)
            hipLaunchKernelGGL((k_apparent_small<1>), dim3(gx, L), dim3(256), slds, st, dist, n, stats, db[d], rowmax, a.thresh, pl_words);
        else
            hipLaunchKernelGGL((k_apparent_small<2>), dim3(gx, L), dim3(256), slds, st, dist, n, stats, db[d], rowmax, a.thresh, pl_words);
    } else {
        // L a multiple of 8: a 1-D grid whose blocks take their layers XCD by XCD (app_block)
        const int xl = (L % 8 == 0 && !test_env_is("TDA_APP_XCD", "0")) ? L : 0;
        const dim3 ag = xl ? dim3(gx * (unsigned)L) : dim3(gx, L);
        // H1 above the LDS-matrix range: 16 x 16 edge tiles over LDS-staged v-tiles (TDA_APP_TILE=0: one edge per thread)
        const bool tiled = d == 1 && !dl && !test_env_is("TDA_APP_TILE", "0");
        if (tiled) {
            const uint64_t nt = ((uint64_t)n + kAppTS - 1) / kAppTS, tiles = nt * (nt + 1) / 2;
            const unsigned tx = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(tiles, std::max<uint64_t>(1, app_total / L)));
            const dim3 tg = xl ? dim3(tx * (unsigned)L) : dim3(tx, L);
            hipLaunchKernelGGL(k_apparent_tile, tg, dim3(256), 0, st, dist, n, stats, db[d], rowmax, a.thresh, xl);
        } else if (d == 1 && dl)
            hipLaunchKernelGGL((k_apparent<1, true>), ag, dim3(256), alds, st, dist, n, stats, db[d], rowmax, a.thresh, xl);
        else if (d == 1)
            hipLaunchKernelGGL((k_apparent<1, false>), ag, dim3(256), alds, st, dist, n, stats, db[d], rowmax, a.thresh, xl);
        else if (dl)
            hipLaunchKernelGGL((k_apparent<2, true>), ag, dim3(256), alds, st, dist, n, stats, db[d], rowmax, a.thresh, xl);
        else
            hipLaunchKernelGGL((k_apparent<2, false>), ag, dim3(256), alds, st, dist, n, stats, db[d], rowmax, a.thresh, xl);
    }
}

// residual columns of dims d0 .. d0 + nd - 1 sorted by filtration key
void enqueue_sort(Call& c, int d0, int nd, hipStream_t st, uint64_t max_chunk = 16384) {
    const Plan& p = c.p;
    // LDS chunk: the largest residual list of these dims, at most max_chunk keys
    uint64_t cap = 64;
    for (int d = d0; d < d0 + nd; ++d) cap = std::max<uint64_t>(cap, std::min<uint64_t>(next_pow2(p.rcap[d]), max_chunk));
    hipLaunchKernelGGL(k_sort_resid, dim3(c.L, nd), dim3(1024), cap * 8, st, c.stats, c.sa, (uint64_t*)(c.B + p.o_tmp), p.max_rcap,
                       c.rb.rmap_keys, c.rb.rmap_stride, ilog2(cap), d0);
}

// H2 phase 1 (its early exits read the chain's residual H1 pivots as they
// appear); in the one-stream timing mode it runs right after the chain,
// so it sees what it sees when it runs beside it
int enqueue_phase1(Call& c, hipStream_t st) {
    const Plan& p = c.p;
    const int L = c.L;
    // blocks per layer: each holds ~46 KB of LDS (one wave), so the whole grid is occupancy-bound:
    // ~1 K blocks over all layers (r04, sweep48 serial stage: L = 32: 96 -> 32 blocks 35 -> 28 us;
    // L = 128: 96 -> 16 blocks 108 -> 73 us); small batches keep up to kP1Grid
    const int p1g = test_env("TDA_P1_GRID") ? std::max(1, atoi(test_env("TDA_P1_GRID")))
                                            : std::min(kP1Grid, std::max(16, 1024 / std::max(1, L)));
    hipLaunchKernelGGL(k_h2_phase1, dim3(L, (p1g + p.p1_waves - 1) / p.p1_waves), dim3(64 * p.p1_waves), p.p1_lds, st, c.dist, c.n, c.stats, c.db[2], c.sb, (const uint16_t*)c.dnb.cls2,
                       p.n2p, p.bm_words, (const uint32_t*)c.dnb.res1, (uint32_t)p.piv_words[1], step_limit());
    HIPC(hipGetLastError());
    if (int rc = (st == c.s ? c.tm : c.tm3).mark("k_h2_phase1")) return rc;
    HIPC(hipEventRecord(c.w.evp, st));
    return 0;
}

// apparent<2> + their sort on the third stream
int enqueue_h2_columns(Call& c) {
    if (int rc = c.tm3.begin()) return rc;
    enqueue_apparent(c, 2, c.w.stream3, c.h2_late ? c.h2_late_grid : 0);
    HIPC(hipGetLastError());
    if (int rc = c.tm3.mark("k_apparent<2>")) return rc;
    // beside k_reduce_par<1> (one 72-KB workgroup per CU) the sort's LDS chunk must fit next to
    // it: 4096 keys (32 KB); a 128-KB chunk waited for the H1 reduction (grid144: 0.85 ms)
    enqueue_sort(c, 2, 1, c.w.stream3, c.h2_side ? 4096 : 16384);
    HIPC(hipGetLastError());
    if (int rc = c.tm3.mark("k_sort_resid<2>")) return rc;
    return 0;
}

// dense H1 (N <= 64): one k_h1_chain instantiation per (words, mode)
int enqueue_chain(Call& c, hipStream_t st) {
    const Plan& p = c.p;
    switch (p.dK * 3 + p.cmode) {
#define TDA_CHAIN(K, F)                                                                                                              \
    case K * 3 + F:                                                                                                                  \
        hipLaunchKernelGGL((k_h1_chain<K, F>), dim3(c.L), dim3(kChainT), p.chain_lds, st, c.dist, c.n, c.stats, c.db[1], c.rb, c.dnb, \
                           step_limit(), c.pairs1, p.pcap[1]);                                                                       \
        break;
        TDA_CHAIN(1, 0) TDA_CHAIN(2, 0) TDA_CHAIN(3, 0) TDA_CHAIN(4, 0) TDA_CHAIN(6, 0) TDA_CHAIN(9, 0) TDA_CHAIN(12, 0)
        TDA_CHAIN(16, 0) TDA_CHAIN(21, 0)
        TDA_CHAIN(1, 1) TDA_CHAIN(2, 1) TDA_CHAIN(3, 1) TDA_CHAIN(4, 1) TDA_CHAIN(6, 1) TDA_CHAIN(9, 1) TDA_CHAIN(12, 1)
        TDA_CHAIN(1, 2) TDA_CHAIN(2, 2) TDA_CHAIN(3, 2) TDA_CHAIN(4, 2) TDA_CHAIN(6, 2) TDA_CHAIN(9, 2) TDA_CHAIN(12, 2)
#undef TDA_CHAIN
        default:
            return fail(TDA_E_INVALID, "no k_h1_chain instantiation for this N");
    }
    HIPC(hipGetLastError());
    return 0;
}

int enqueue_h2_finish(Call& c, hipStream_t st) {
    const Plan& p = c.p;
    hipLaunchKernelGGL(k_reduce_h2_finish, dim3(c.L), dim3(64), p.rcfg.bytes, st, c.dist, c.n, c.stats, c.db[1], c.db[2], c.rb, p.rcfg, c.sb,
                       (const uint32_t*)c.dnb.res1, c.pairs2, p.pcap[2]);
    HIPC(hipGetLastError());
    return 0;
}

// edge codes of the wide H2 keys (thresholds are known: after the H0 join)
int enqueue_edge_codes(Call& c, hipStream_t es, StageTimer& et) {
    const Plan& p = c.p;
    char* B = c.B;
    const int n = c.n, L = c.L;
    // the sorted lengths end in dsort: with an odd number of merge passes the keys start in dtmp
    const uint64_t E = binom((uint64_t)n, 2), CH = 1ull << kEdgeSortLog2;
    int passes = 0;
    for (uint64_t w = CH; w < E; w <<= 1) ++passes;
    uint64_t* ka = (uint64_t*)(B + ((passes & 1) ? p.o_dtmp : p.o_dsort));
    uint64_t* kb = (uint64_t*)(B + ((passes & 1) ? p.o_dsort : p.o_dtmp));
    const unsigned gk = (unsigned)std::min<uint64_t>(1024, ((uint64_t)n * n + 255) / 256);
    hipLaunchKernelGGL(k_edge_keys, dim3(gk, L), dim3(256), 0, es, c.dist, n, ka, p.ecap);
    hipLaunchKernelGGL(k_edge_chunks, dim3((unsigned)((E + CH - 1) / CH), L), dim3(1024), kEdgeSortLds, es, ka, E, p.ecap);
    for (uint64_t w = CH; w < E; w <<= 1) {
        hipLaunchKernelGGL(k_edge_merge, dim3((unsigned)((E + kMergeSeg - 1) / kMergeSeg), L), dim3(256), 0, es, ka, kb, E,
                           p.ecap, w);
        std::swap(ka, kb);
    }
    HIPC(hipGetLastError());
    if (int rc = et.mark("k_edge_sort")) return rc;
    const unsigned gx = (unsigned)std::min<uint64_t>(1024, ((uint64_t)n * n + 255) / 256);
    hipLaunchKernelGGL(k_edge_codes, dim3(gx, L), dim3(256), 0, es, c.dist, n, c.stats, (const uint64_t*)(B + p.o_dsort), p.ecap,
                       (uint32_t*)(B + p.o_dcode));
    HIPC(hipGetLastError());
    return et.mark("k_edge_codes");
}

// H1 (and, with par2, H2) on the persistent workers of k_reduce_par: k_par_init, the late fork
// of the H2 branch, k_reduce_par, k_par_emit.  start_dim: the first dim left to k_reduce_big.
int enqueue_par(Call& c, int& start_dim) {
    const Plan& p = c.p;
    Workspace& w = c.w;
    hipStream_t s = c.s;
    const int n = c.n, L = c.L;
    float* dist = c.dist;
    LayerStats* stats = c.stats;
    DimBufs* db = c.db;
    const Reduce2Bufs& rb = c.rb;
    const ParBufs& pb = c.pb;
    const BigBufs& gb = c.gb;
    HIPC(hipMemsetAsync(pb.rq, 0, p.rq_cap * 8, s));
    hipLaunchKernelGGL(k_par_init, dim3(64, L), dim3(256), 0, s, stats, L, p.rcap[1], pb, 1);
    HIPC(hipGetLastError());
    MARK("k_par_init");
    if (c.h2_late) {  // the H2 branch (and the wide edge codes) beside the H1 reduction
        HIPC(hipEventRecord(w.evs, s));
        HIPC(hipStreamWaitEvent(w.stream3, w.evs, 0));
        if (c.h2_late_delay_us && !c.serial_stages)
            hipLaunchKernelGGL(k_delay, dim3(1), dim3(64), 0, w.stream3, c.h2_late_delay_us);
        if (int rc = enqueue_h2_columns(c)) return rc;
        if (p.wide)
            if (int rc = enqueue_edge_codes(c, w.stream3, c.tm3)) return rc;
        HIPC(hipEventRecord(w.evp, w.stream3));
    }
    // persistent workers (one 71-KB-LDS workgroup per CU by default); the surplus exits at once
    const unsigned par_grid = par_grid_size();
    const uint32_t* no_clr = nullptr;
    ParBufs pb1 = pb, pb2 = pb;  // the reduction launches alone: each dimension's own step limit (tests)
    pb1.step_limit = par_step_limit(1);
    pb2.step_limit = par_step_limit(2);
    if (p.packed)
        hipLaunchKernelGGL((k_reduce_par<1, true>), dim3(par_grid), dim3(kParT), sizeof(ParLds), s, dist, n, L, stats, db[1], no_clr,
                           (uint64_t)0, rb, pb1, gb.dcode, gb.dsort, gb.ecap);
    else
        hipLaunchKernelGGL((k_reduce_par<1, false>), dim3(par_grid), dim3(kParT), sizeof(ParLds), s, dist, n, L, stats, db[1], no_clr,
                           (uint64_t)0, rb, pb1, gb.dcode, gb.dsort, gb.ecap);
    HIPC(hipGetLastError());
    MARK("k_reduce_par");
    // H2 next: residual H1 pivots into the dim-1 bitmap (k_reduce_par<2>) or map (k_reduce_big)
    hipLaunchKernelGGL(k_par_emit<1>, dim3(L), dim3(1024), 0, s, stats, db[1], rb, pb, c.pairs1, p.pcap[1],
                       p.maxdim < 2 ? 0 : p.par2 ? 2 : 1, (const uint64_t*)nullptr, (uint64_t)0);
    HIPC(hipGetLastError());
    MARK("k_par_emit");
    start_dim = 2;
    if (!p.par2) return 0;
    // H2 columns on the same workers (an H1 abort skips it: k_par_init keeps the flag)
    if (c.h2_side) HIPC(hipStreamWaitEvent(s, w.evp, 0));  // join: H2 columns (third stream)
    HIPC(hipMemsetAsync(pb.rq, 0, p.rq_cap * 8, s));
    hipLaunchKernelGGL(k_par_init, dim3(64, L), dim3(256), 0, s, stats, L, p.rcap[2], pb, 2);
    HIPC(hipGetLastError());
    if (p.wide)  // N > 568: edge-code keys (k_edge_codes ran above)
        hipLaunchKernelGGL((k_reduce_par<2, false, true>), dim3(par_grid), dim3(kParT), sizeof(ParLds), s, dist, n, L, stats,
                           db[2], (const uint32_t*)db[1].pivbits, db[1].piv_words, rb, pb2, gb.dcode, gb.dsort, gb.ecap);
    else if (n <= kPar2PackedMaxN)
        hipLaunchKernelGGL((k_reduce_par<2, true>), dim3(par_grid), dim3(kParT), sizeof(ParLds), s, dist, n, L, stats, db[2],
                           (const uint32_t*)db[1].pivbits, db[1].piv_words, rb, pb2, gb.dcode, gb.dsort, gb.ecap);
    else
        hipLaunchKernelGGL((k_reduce_par<2, false>), dim3(par_grid), dim3(kParT), sizeof(ParLds), s, dist, n, L, stats, db[2],
                           (const uint32_t*)db[1].pivbits, db[1].piv_words, rb, pb2, gb.dcode, gb.dsort, gb.ecap);
    HIPC(hipGetLastError());
    MARK("k_reduce_par<2>");
    hipLaunchKernelGGL(k_par_emit<2>, dim3(L), dim3(1024), 0, s, stats, db[2], rb, pb, c.pairs2, p.pcap[2], 0,
                       p.wide ? gb.dsort : (const uint64_t*)nullptr, p.ecap);
    HIPC(hipGetLastError());
    MARK("k_par_emit<2>");
    start_dim = 3;
    return 0;
}

// the serial reducers: k_reduce_big for the dims from start_dim up (none left after a parallel
// H1 and H2), else one wave per layer (k_reduce_all, working tables in LDS or HBM)
void enqueue_serial_reduce(Call& c, int start_dim) {
    const Plan& p = c.p;
    hipStream_t s = c.s;
    const int n = c.n, L = c.L;
    if (p.big) {
        if (start_dim <= p.maxdim)
            hipLaunchKernelGGL(k_reduce_big, dim3(L), dim3(kBigT), 0, s, c.dist, n, p.maxdim, c.stats, c.db[1], c.db[2], c.rb, c.gb, c.pairs1,
                               c.pairs2, p.pcap[1], p.maxdim >= 2 ? p.pcap[2] : 0, start_dim);
        return;
    }
    const bool p1 = n <= 1024, p2 = n <= 256;
    const ReduceAllCfg& rc = p.rcfg;
#define TDA_LAUNCH_RED(LW, P1, P2)                                                                                                    \
    hipLaunchKernelGGL((k_reduce_all<LW, P1, P2>), dim3(L), dim3(64), rc.bytes, s, c.dist, n, p.maxdim, c.stats, c.db[1], c.db[2], c.rb, rc, \
                       c.pairs1, c.pairs2, p.pcap[1], p.maxdim >= 2 ? p.pcap[2] : 0)
    if (p.lds_mode) {
        if (p2) TDA_LAUNCH_RED(true, true, true); else if (p1) TDA_LAUNCH_RED(true, true, false); else TDA_LAUNCH_RED(true, false, false);
    } else {
        if (p2) TDA_LAUNCH_RED(false, true, true); else if (p1) TDA_LAUNCH_RED(false, true, false); else TDA_LAUNCH_RED(false, false, false);
    }
#undef TDA_LAUNCH_RED
}

// k_emit alone: the call's end, and the re-emit after the output buffer grew (ERR_OUT_CAP)
void launch_k_emit(Call& c) {
    const Plan& p = c.p;
    Workspace& w = c.w;
    hipLaunchKernelGGL(k_emit, dim3(c.L), dim3(1024), kEmitLds, c.s, c.stats, c.L, p.maxdim, c.ps, (uint64_t*)(c.B + p.o_fk),
                       (uint32_t*)(c.B + p.o_fv), p.sstride, w.houtoff.dev, w.hout.dev, (uint64_t)w.hout.cap, w.hstats.dev);
}

// ---- emission order, straight into host-mapped memory
int enqueue_emit(Call& c) {
    const Plan& p = c.p;
    launch_k_emit(c);
    HIPC(hipGetLastError());
    MARK("k_emit");
    if (p.piv2_sparse) {  // the H2 pivot bitmap back to zero: only the words this call set
        hipLaunchKernelGGL(k_clear_words, dim3(1024, c.L), dim3(256), 0, c.s, c.stats, (const uint64_t*)(c.B + p.o_clr2), p.clr_cap,
                           (uint32_t*)(c.B + p.o_piv[2]), p.piv_words[2]);
        HIPC(hipGetLastError());
        MARK("k_clear_words");
    }
    return 0;
}

// order 5 (N <= 64, H0-H2): apparent<1> opens the H2 branch's stream (its pivot
// bitmap is apparent<2>'s clearing test), so the branch runs on one queue up to
// phase 1; the main stream picks up apparent<1>'s residuals for sort<1> and the chain
int enqueue_h2_branch_order5(Call& c) {
    Workspace& w = c.w;
    hipStream_t s = c.s;
    HIPC(hipStreamWaitEvent(w.stream3, w.evf, 0));
    if (int rc = c.tm3.begin()) return rc;
    enqueue_apparent(c, 1, w.stream3);
    HIPC(hipGetLastError());
    if (int rc = c.tm3.mark("k_apparent<1>")) return rc;
    HIPC(hipEventRecord(w.evs, w.stream3));
    enqueue_apparent(c, 2, w.stream3);
    HIPC(hipGetLastError());
    if (int rc = c.tm3.mark("k_apparent<2>")) return rc;
    enqueue_sort(c, 2, 1, w.stream3, 16384);
    HIPC(hipGetLastError());
    if (int rc = c.tm3.mark("k_sort_resid<2>")) return rc;
    HIPC(hipStreamWaitEvent(w.stream3, w.evj, 0));  // edge classes (k_prep_*)
    if (int rc = enqueue_phase1(c, w.stream3)) return rc;
    HIPC(hipStreamWaitEvent(s, w.evs, 0));
    enqueue_sort(c, 1, 1, s);
    HIPC(hipGetLastError());
    MARK("k_sort_resid<1>");
    return 0;
}

// H1 .. Hmaxdim up to the joins: apparent pairs (parallel) and residual sorts, with the H2
// columns forked onto the third stream where the plan has a reducer that runs beside them
int enqueue_columns(Call& c) {
    const Plan& p = c.p;
    Workspace& w = c.w;
    hipStream_t s = c.s;
    if (c.app1_side) {
        if (int rc = enqueue_h2_branch_order5(c)) return rc;
    } else {
        enqueue_apparent(c, 1, s);
        HIPC(hipGetLastError());
        MARK("k_apparent<1>");
    }
    if (c.order == 0)
        if (int rc = enqueue_side(c)) return rc;
    if (c.app1_side) {
        // enqueued above
    } else if (c.split2) {
        HIPC(hipEventRecord(w.evs, s));
        if (c.order == 3) {
            enqueue_sort(c, 1, 1, s);
            HIPC(hipGetLastError());
            MARK("k_sort_resid<1>");
        }
        HIPC(hipStreamWaitEvent(w.stream3, w.evs, 0));
        if (c.order == 2) HIPC(hipStreamWaitEvent(w.stream3, w.evj, 0));
        if (int rc = enqueue_h2_columns(c)) return rc;
        HIPC(hipStreamWaitEvent(w.stream3, w.evj, 0));  // edge classes (k_prep_*)
        if (!c.serial_stages)
            if (int rc = enqueue_phase1(c, w.stream3)) return rc;
        if (c.order != 3) {
            enqueue_sort(c, 1, 1, s);
            HIPC(hipGetLastError());
            MARK("k_sort_resid<1>");
        }
    } else if (c.h2_side && c.h2_late) {
        // (fork after k_par_init: enqueue_par)
        enqueue_sort(c, 1, 1, s);
        HIPC(hipGetLastError());
        MARK("k_sort_resid<1>");
    } else if (c.h2_side) {
        // parallel H1 and H2: the H2 columns' apparent pass and sort run on
        // the third stream beside the H1 reduction (k_reduce_par<2> joins
        // them).  k_par_emit<1> may OR residual H1 pivots into the bitmap
        // k_apparent<2> reads as its clearing test while it runs: a triangle
        // seen cleared is skipped there, otherwise it becomes a residual
        // column that k_reduce_par<2> skips -- never an apparent pair (a
        // cleared triangle is an H1 death, and apparent pairs are
        // persistence pairs), so pairs and checksums do not depend on the race.
        HIPC(hipEventRecord(w.evs, s));
        HIPC(hipStreamWaitEvent(w.stream3, w.evs, 0));
        if (int rc = enqueue_h2_columns(c)) return rc;
        HIPC(hipEventRecord(w.evp, w.stream3));
        enqueue_sort(c, 1, 1, s);
        HIPC(hipGetLastError());
        MARK("k_sort_resid<1>");
    } else {
        for (int d = 2; d <= p.maxdim; ++d) {
            enqueue_apparent(c, d, s);
            HIPC(hipGetLastError());
            MARK("k_apparent<2>");
        }
        enqueue_sort(c, 1, p.maxdim, s);
        HIPC(hipGetLastError());
        MARK("k_sort_resid");
    }
    return 0;
}

// The whole launch sequence of one call, between ev0 and ev1.
int enqueue_schedule(Call& c) {
    const Plan& p = c.p;
    Workspace& w = c.w;
    hipStream_t s = c.s;
    const int L = c.L;
    wire_buffers(c);
    HIPC(c.rec_t(w.ev0));
    if (int rc = c.tm.begin()) return rc;
    MARK("event_gap");  // an empty interval: what two back-to-back events measure with no kernel between (bench.py subtracts it)
    HIPC(hipMemsetAsync(c.B + p.memset_lo, 0, p.memset_hi - p.memset_lo, s));
    MARK("memset");
    if (int rc = enqueue_distances(c)) return rc;
    HIPC(hipEventRecord(w.evf, s));  // fork point of the side streams

    // capture order of the launches (the graph executor dispatches in it):
    // TDA_ORDER=0 apparent<1> first; 1 side streams first; 2 side streams
    // first and the H2 branch after the triangle ranks; 3 side streams first,
    // sort<1> enqueued before the H2 branch; 5 (N <= 64 with H2) as 3, with
    // apparent<1> at the head of the H2 branch's stream: sweep48 0.182 ->
    // 0.175 ms device, L = 4 0.136 -> 0.131 ms (replayed graph; eager slower)
    // 5 up to 64 layers per call; 3 above (sweep48x4, 128 layers: 0.42 vs 0.48 ms with 5)
    // r04 (after the §6.4-6.5 kernel changes, graph replay, one call at a time): L = 32 order 2 0.167 ms
    // device vs 0.174 with 5; L = 4 order 5 0.124 ms vs 0.138 with 2
    c.order = test_env("TDA_ORDER") ? atoi(test_env("TDA_ORDER")) : (L <= 16 ? 5 : L <= 64 ? 2 : 3);
    if (p.maxdim < 1 || c.order >= 1)
        if (int rc = enqueue_side(c)) return rc;
    // N <= 64 with H2: the H2 columns (apparent<2>, their sort, phase 1) run
    // on a third stream beside the H1 chain; they only need apparent<1>'s
    // pivot bitmap, and the chain records its residual pivots separately
    c.split2 = p.dense && p.maxdim >= 2;
    c.h2_side = !p.dense && p.par && p.par2 && p.maxdim >= 2;
    // the H2 branch forks once k_reduce_par<1> is about to start (after k_par_init), not after
    // apparent<1>: launched together with the H1 prerequisites, the GPU-filling apparent<2> pass
    // slowed them (torus2048_h2 trace: sort<1> 0.06 -> 7 ms, the edge chunk sort 0.5 -> 15 ms, the
    // H1 reduction starting at 26.6 ms); after k_par_init it fills the CUs the H1 workers leave.
    // The wide edge codes (H2 keys only) move onto the branch too.  TDA_H2_LATE=0: the r04 fork.
    c.h2_late = c.h2_side && !test_env_is("TDA_H2_LATE", "0");
    // A k_reduce_par worker fills a CU (two 256-VGPR waves per SIMD), so apparent<2> blocks
    // dispatched before the H1 workers keep them off every CU they hold (torus2048_h2: the H1
    // reduction 124 -> 154 ms); on a small grid the pass itself crawls (128 blocks: 30 -> 194 ms).
    // The branch starts after a short device-side delay instead, so the H1 workers are resident
    // first and apparent<2> fills the CUs they leave as the column queue drains.
    c.h2_late_grid = test_env("TDA_H2_LATE_GRID") ? strtoull(test_env("TDA_H2_LATE_GRID"), nullptr, 10) : 0;
    c.h2_late_delay_us = test_env("TDA_H2_LATE_DELAY") ? (uint32_t)atoi(test_env("TDA_H2_LATE_DELAY")) : 50;
    c.app1_side = c.split2 && c.order == 5 && !c.serial_stages;  // enqueue_h2_branch_order5

    if (p.maxdim >= 1) {
        if (int rc = enqueue_columns(c)) return rc;
        if (p.serial_tables) {
            HIPC(hipMemsetAsync(c.rb.windex, 0, (size_t)L * p.wcap_g * 2 * 8, s));
            HIPC(hipMemsetAsync(c.rb.wfill, 0, (size_t)L * p.wcap_g / 4 * 4, s));
        }
        HIPC(hipStreamWaitEvent(s, w.evh, 0));  // join: forest edges (clearing of H1 columns)
        HIPC(hipStreamWaitEvent(s, w.evj, 0));  // join: triangle ranks
        MARK("wait:join");  // keeps the side streams' time out of the next kernel's stage
        if (p.dense) {
            if (int rc = enqueue_chain(c, s)) return rc;
            MARK("k_h1_chain");
            if (p.maxdim >= 2) {
                if (c.serial_stages)
                    if (int rc = enqueue_phase1(c, s)) return rc;
                HIPC(hipStreamWaitEvent(s, w.evp, 0));  // phase-1 results
                MARK("wait:phase1");
                if (int rc = enqueue_h2_finish(c, s)) return rc;
                MARK("k_reduce_h2_finish");
            }
        } else {
            int start_dim = 1;
            if (p.big && p.wide && !c.h2_late)
                if (int rc = enqueue_edge_codes(c, s, c.tm)) return rc;
            if (p.big && p.par)
                if (int rc = enqueue_par(c, start_dim)) return rc;
            enqueue_serial_reduce(c, start_dim);
        }
        HIPC(hipGetLastError());
        if (!p.dense && !(p.par && (p.maxdim < 2 || p.par2))) MARK(p.big ? "k_reduce_big" : "k_reduce_all");
    } else {
        HIPC(hipStreamWaitEvent(s, w.evh, 0));
        HIPC(hipStreamWaitEvent(s, w.evj, 0));
    }

    if (c.nls || c.want_tn) HIPC(hipStreamWaitEvent(s, w.evsil, 0));  // join: silhouette scores, TwoNN on s4
    if (c.want_tn) HIPC(hipStreamWaitEvent(s, w.evj, 0));            // join: TwoNN on s2
    if (int rc = enqueue_emit(c)) return rc;
    HIPC(c.rec_t(w.ev1));
    return 0;
}
