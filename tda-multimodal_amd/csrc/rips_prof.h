// rips_prof.h -- what the -DTDA_PROFILE / -DTDA_PROF2 builds print after a call (stderr): the
// kernels' cycle counters in LayerStats::prof and k_reduce_par's long-column log.  Included by
// rips.hip under those macros only (part of its translation unit, after struct Call).
#pragma once

#ifdef TDA_PROF2
// per-wave phase cycles of the long columns (k_reduce_par, the last launch)
int print_prof2(Call& c) {
    const Plan& p = c.p;
    char* B = c.B;
    if (!p.par) return 0;
    ParCtl ctl;
    HIPC(hipMemcpy(&ctl, B + p.o_pctl, sizeof(ctl), hipMemcpyDeviceToHost));
    const uint64_t nrec = std::min<uint64_t>(ctl.pad[2], kParDbgCap);
    std::vector<uint64_t> d(nrec * kParP2Words);
    if (nrec) HIPC(hipMemcpy(d.data(), B + p.o_pdbg + (size_t)kParDbgCap * 32, nrec * kParP2Words * 8, hipMemcpyDeviceToHost));
    static const char* nm[8] = {"room+barrier", "min", "pivot+loads", "keys", "appends", "toggles", "refills", "owner"};
    uint64_t best = ~0ull, bsteps = 0;
    for (uint64_t i = 0; i < nrec; ++i)
        if (d[i * kParP2Words + 2] > bsteps) bsteps = d[i * kParP2Words + 2], best = d[i * kParP2Words];
    for (uint64_t i = 0; i < nrec; ++i) {
        const uint64_t* r = &d[i * kParP2Words];
        if (r[0] != best) continue;
        uint64_t tot = 0;
        for (int u = 0; u < 8; ++u) tot += r[3 + u];
        fprintf(stderr, "[tda-prof2] layer %llu column %llu wave %llu: %llu steps, %.0f cycles/step:", (unsigned long long)(r[0] >> 40),
                (unsigned long long)(r[0] & ((1ull << 40) - 1)), (unsigned long long)r[1], (unsigned long long)r[2], (double)tot / (double)r[2]);
        for (int u = 0; u < 8; ++u) fprintf(stderr, " %s %.0f", nm[u], (double)r[3 + u] / (double)r[2]);
        fprintf(stderr, "\n");
    }
    return 0;
}
#endif

#ifdef TDA_PROFILE
// dense path (N <= 64): the H1 chain's slowest layer, k_prep_edges, k_h0_wave and H2 phase 1
void print_profile_dense(Call& c) {
    Workspace& w = c.w;
    const int L = c.L;
    int arg = 0;
    uint64_t p1max = 0;
    for (int l = 0; l < L; ++l) {
        if (w.hstats.p[l].prof[0][0] > w.hstats.p[arg].prof[0][0]) arg = l;
        p1max = std::max<uint64_t>(p1max, w.hstats.p[l].prof[1][0]);
    }
    const uint64_t* q = w.hstats.p[arg].prof[0];
    fprintf(stderr, "[tda-prof] dense H1 slowest layer %d adds %lld: total %llu pivot %llu (calls %llu ties %llu) cob_app %llu add_owner %llu new_pair %llu cycles; H2 phase-1 slowest wave %llu cycles\n",
            arg, (long long)w.hstats.p[arg].n_adds[1], (unsigned long long)q[0], (unsigned long long)q[1], (unsigned long long)q[7],
            (unsigned long long)q[2], (unsigned long long)q[3], (unsigned long long)q[4], (unsigned long long)q[5],
            (unsigned long long)p1max);
    uint64_t sc = 0, cb = 0, tt = 0, ad = 0, mx = 0, mxa = 0;
    for (int l = 0; l < L; ++l) {
        sc += w.hstats.p[l].prof[1][4];
        cb += w.hstats.p[l].prof[1][5];
        tt += w.hstats.p[l].prof[1][6];
        ad += w.hstats.p[l].prof[1][7];
        if (w.hstats.p[l].prof[1][2] > mx) {
            mx = w.hstats.p[l].prof[1][2];
            mxa = w.hstats.p[l].prof[1][3] & 0xFFFF;
        }
    }
    {
        const uint64_t* e = w.hstats.p[0].prof[4];
        fprintf(stderr, "[tda-prof] k_prep_edges layer 0 (us from block entry): sort block thresh %.2f staged %.2f sorted %.2f end %.2f; mask blocks (max) thresh %.2f staged %.2f end %.2f\n",
                e[0] * 0.01, e[1] * 0.01, e[2] * 0.01, e[3] * 0.01, e[4] * 0.01, e[5] * 0.01, e[6] * 0.01);
    }
    {
        const uint64_t* h = w.hstats.p[0].prof[3];
        fprintf(stderr, "[tda-prof] k_h0_wave layer 0 (cycles from entry): thresh %llu prim %llu sort %llu unionfind %llu end %llu; chain staging (slowest layer) %llu\n",
                (unsigned long long)h[1], (unsigned long long)h[2], (unsigned long long)h[3], (unsigned long long)h[4],
                (unsigned long long)h[5], (unsigned long long)q[6]);
    }
    fprintf(stderr, "[tda-prof] H2 phase 1: all columns %llu cycles (scan %llu cob %llu), %llu adds; slowest column %llu cycles (%llu adds)\n",
            (unsigned long long)tt, (unsigned long long)sc, (unsigned long long)cb, (unsigned long long)ad, (unsigned long long)mx,
            (unsigned long long)mxa);
}

// k_reduce_par: the long-column timeline of its last launch (H2's when it ran, else H1's) and
// the longest column's phase counters
int print_profile_par(Call& c) {
    const Plan& p = c.p;
    Workspace& w = c.w;
    char* B = c.B;
    {
        ParCtl ctl;
        HIPC(hipMemcpy(&ctl, B + p.o_pctl, sizeof(ctl), hipMemcpyDeviceToHost));
        const uint64_t nlog = std::min<uint64_t>(ctl.pad[1], kParDbgCap);
        std::vector<uint64_t> d(nlog * 4);
        if (nlog) HIPC(hipMemcpy(d.data(), B + p.o_pdbg, nlog * 32, hipMemcpyDeviceToHost));
        std::vector<uint64_t> order(nlog);
        for (uint64_t i = 0; i < nlog; ++i) order[i] = i;
        std::sort(order.begin(), order.end(), [&](uint64_t x, uint64_t y) { return d[x * 4 + 2] - d[x * 4 + 1] > d[y * 4 + 2] - d[y * 4 + 1]; });
        uint64_t tend = 0;
        for (uint64_t i = 0; i < nlog; ++i) tend = std::max(tend, d[i * 4 + 2]);
        fprintf(stderr, "[tda-prof] k_reduce_par timeline: %llu columns of >= %llu steps; last one ends %.3f ms after the first workgroup started\n",
                (unsigned long long)nlog, (unsigned long long)kParDbgMinSteps, nlog ? (tend - ctl.pad[0]) * 1e-5 : 0.0);
        for (uint64_t k = 0; k < std::min<uint64_t>(nlog, 12); ++k) {
            const uint64_t i = order[k];
            fprintf(stderr, "[tda-prof]   layer %llu column %llu: start %.3f ms, %.3f ms, %llu steps%s\n",
                    (unsigned long long)(d[i * 4] >> 40), (unsigned long long)(d[i * 4] & ((1ull << 40) - 1)),
                    (d[i * 4 + 1] - ctl.pad[0]) * 1e-5, (d[i * 4 + 2] - d[i * 4 + 1]) * 1e-5,
                    (unsigned long long)(d[i * 4 + 3] & ~(1ull << 63)), (d[i * 4 + 3] >> 63) ? " (resumed)" : "");
        }
    }
    const uint64_t* q = w.hstats.p[0].prof[2];
    fprintf(stderr, "[tda-prof] k_reduce_par longest column: %llu steps, %llu cycles: front_min %llu, pivot+rows %llu, apparent adds %llu, refills %llu (%llu), owner path %llu; avg front log %llu, compactions %llu, spills %llu\n",
            (unsigned long long)q[6], (unsigned long long)q[0], (unsigned long long)q[1], (unsigned long long)q[2], (unsigned long long)q[3],
            (unsigned long long)q[4], (unsigned long long)((q[7] >> 16) & 0xFFFF), (unsigned long long)q[5], (unsigned long long)(q[7] & 0xFFFF),
            (unsigned long long)((q[7] >> 32) & 0xFFFF), (unsigned long long)(q[7] >> 48));
    const uint64_t* u = w.hstats.p[0].prof[3];
    fprintf(stderr, "[tda-prof]   inside adds: keys %llu, capacity %llu, front toggles %llu, bucket appends %llu cycles; %llu record adds (%llu keys); refills moved %llu keys; wave 0 toggled %llu front / %llu back keys\n",
            (unsigned long long)u[0], (unsigned long long)u[3], (unsigned long long)u[1], (unsigned long long)u[2],
            (unsigned long long)u[4], (unsigned long long)u[5], (unsigned long long)u[6], (unsigned long long)(u[7] >> 32),
            (unsigned long long)(u[7] & 0xFFFFFFFFull));
    const uint64_t* v = w.hstats.p[0].prof[4];
    fprintf(stderr, "[tda-prof]   record adds: room %llu, col_add %llu cycles, keys front %llu / all %llu; refill pass 3 %llu cycles; %llu saves (%llu keys) %llu cycles\n",
            (unsigned long long)v[0], (unsigned long long)v[1], (unsigned long long)v[2], (unsigned long long)v[3], (unsigned long long)v[5],
            (unsigned long long)v[6], (unsigned long long)v[7], (unsigned long long)v[4]);
    const uint64_t* y = w.hstats.p[0].prof[1];
    fprintf(stderr, "[tda-prof]   refill phases: search %llu, loads+min %llu, histogram %llu, level choice %llu, toggles %llu, appends %llu, compactions %llu cycles; %llu keys kept in front\n",
            (unsigned long long)y[0], (unsigned long long)y[1], (unsigned long long)y[2], (unsigned long long)y[3],
            (unsigned long long)y[4], (unsigned long long)y[5], (unsigned long long)y[6], (unsigned long long)y[7]);
    return 0;
}

int print_profile(Call& c) {
    const Plan& p = c.p;
    Workspace& w = c.w;
    const int n = c.n, L = c.L;
    if (p.dense && !p.par) print_profile_dense(c);
    if (n > kSmallN) {
        const uint64_t* h = w.hstats.p[0].prof[0];
        fprintf(stderr, "[tda-prof] k_h0 layer 0 (cycles from entry): staged %llu, thresh+edges %llu, forest %llu, sort %llu, end %llu\n",
                (unsigned long long)h[0], (unsigned long long)h[1], (unsigned long long)h[2], (unsigned long long)h[3],
                (unsigned long long)h[4]);
    }
    if (p.par)
        if (int rc = print_profile_par(c)) return rc;
    if (p.big && !p.par)
        for (int d = 1; d <= p.maxdim; ++d) {
            const uint64_t* q = w.hstats.p[0].prof[d];
            fprintf(stderr, "[tda-prof] big dim %d layer 0: cob0 %llu pop %llu owner_add %llu app_add %llu store %llu reset %llu total %llu cycles; owner adds %llu entries %llu, all adds %lld\n",
                    d, (unsigned long long)q[0], (unsigned long long)q[1], (unsigned long long)q[2], (unsigned long long)q[3],
                    (unsigned long long)q[4], (unsigned long long)q[5], (unsigned long long)q[7], (unsigned long long)(q[6] >> 40),
                    (unsigned long long)(q[6] & ((1ull << 40) - 1)), (long long)w.hstats.p[0].n_adds[d]);
        }
    for (int d = 1; d <= p.maxdim; ++d) {
        uint64_t mx[8] = {0};
        int arg = 0;
        for (int l = 0; l < L; ++l)
            if (w.hstats.p[l].prof[d][7] > mx[7]) {
                arg = l;
                for (int i = 0; i < 8; ++i) mx[i] = w.hstats.p[l].prof[d][i];
            }
        fprintf(stderr, "[tda-prof] dim %d slowest layer %d adds %lld: scan %llu lookup %llu dec+facet %llu cob_app %llu toggles %llu reset %llu compact %llu total %llu cycles\n",
                d, arg, (long long)w.hstats.p[arg].n_adds[d], (unsigned long long)mx[0], (unsigned long long)mx[1], (unsigned long long)mx[2],
                (unsigned long long)mx[3], (unsigned long long)mx[4], (unsigned long long)mx[5], (unsigned long long)mx[6], (unsigned long long)mx[7]);
    }
    return 0;
}
#endif
