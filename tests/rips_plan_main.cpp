// Stand-alone driver of the persistence call's host plan (csrc/rips_plan.h) for
// tests/test_rips_plan_cpu.py: host C++ only.  For every line of eleven integers on stdin
//     L N D maxdim dtype is_dist want64 force_global scale force_big no_par
// (after a first line with the sizes of the structs the plan carves by and two limits)
// it prints the line back after "case" and then every field of the Plan that make_plan builds for
// it as name=value (arrays as a,b,c,d; rcfg and the DistSel included), grouped by consumer.  The
// test knobs are read from the environment, as in the library.  make_plan runs twice per case and
// the program fails (exit 3) if the two plans differ in any printed field.  The knobs that are no
// field of a Plan go to stderr, one line: step_limit, par_step_limit(1), par_step_limit(2), par_pool_shift.
// With the arguments `h0 LO HI` it prints the H0 shape (h0_shape) of every N in LO .. HI instead.
#include <cstdio>
#include <string>

#include "rips_plan.h"

using namespace tda;

static std::string out;

static void put(const char* name, unsigned long long v) { out += std::string(" ") + name + "=" + std::to_string(v); }
template <typename T>
static void put4(const char* name, const T (&v)[4]) {
    out += std::string(" ") + name + "=";
    for (int i = 0; i < 4; ++i) out += (i ? "," : "") + std::to_string((unsigned long long)v[i]);
}
static void group(const char* name) { out += std::string(out.empty() ? "" : "\n") + name; }

#define F(field) put(#field, (unsigned long long)p.field)
#define F4(field) put4(#field, p.field)

static std::string print(const Plan& p) {
    out.clear();
    group("shape"), F(L), F(N), F(D), F(maxdim), F(dtype), F(is_dist), F(want64);
    group("sizes"), F4(ncand), F4(piv_words), F4(rcap), F4(pcap), F(mst_words), F(max_rcap), F(rmap_stride), F(vpool_cap), F(wcap_g),
        F(sstride);
    group("reducer"), F(lds_mode), F(big), F(par), F(par2), F(packed), F(wide), F(serial_tables), F(dense), F(piv2_sparse);
    group("distances"), F(dist.mfma), F(dist.dsplit), F(dist.gram_layer), F(o_x), F(o_gpart), F(o_npart), F(o_dist), F(o_d64), F(o_rowmax);
    group("memset"), F(memset_lo), F(memset_hi), F(o_stats), F(o_mst), F4(o_piv), F(o_p1used), F(o_p1next), F(o_res1), F(o_necnt), F(clr_cap),
        F(o_clr2);
    group("h0"), F(o_h0s), F(o_bcomp), F(o_bcheap), F(o_bctl);
    group("apparent"), F4(o_resid), F(o_tmp), F(o_rmk), F(o_rmv), F(o_vlen), F(o_vpool), F(o_voff);
    group("rcfg"), F(rcfg.bytes), F(rcfg.dist_lds), F(rcfg.step_limit);
    for (int d = 0; d < 3; ++d) {
        const Reduce2Cfg& r = p.rcfg.dim[d];
        out += " rcfg.dim" + std::to_string(d) + "=" + std::to_string(r.wcap) + "," + std::to_string(r.rmap_lds_cap) + "," + std::to_string(r.piv_lds);
    }
    group("dense"), F(dK), F(cmode), F(fast), F(inv_stride), F(tri_stride), F(cob_stride), F(chain_lds), F(p1_lds), F(p1_waves), F(n2p),
        F(bm_words), F(prep_lds), F(o_recs), F(o_cls2), F(o_cls), F(o_inv), F(o_epos), F(o_eM), F(o_inv32), F(o_rof), F(o_cobt), F(o_p1k),
        F(o_p1i), F(o_p1x), F(o_roff2), F(o_rlen2), F(o_rpool2);
    group("serial"), F(o_wt), F(o_wk), F(o_wl), F(o_wp), F(o_bref), F(ecap), F(o_dsort), F(o_dtmp), F(o_dcode);
    group("par"), F(ostride), F(rec_cap), F(rpool_cap), F(bpool_cap), F(rq_cap), F(o_pctl), F(o_pitem), F(o_pokey), F(o_poval), F(o_colpiv),
        F(o_prec), F(o_prpool), F(o_pbpool), F(o_prq), F(o_pdbg);
    group("output"), F4(o_pairs), F(o_fk), F(o_fv), F(o_pptr), F(o_pcap), F(o_outoff), F(total);
    return out;
}

// `h0 LO HI` as arguments: no plans; one line of the limits the H0 and side-metric launches are held to,
// then for every N in LO .. HI the H0 shape (h0_shape) and the side metrics' dynamic LDS, as name=value
static int h0_scan(int lo, int hi) {
    printf("limits kLdsMax=%d kBorHookLdsMax=%d kTnLdsMax=%d kSilLdsMax=%d kSilMaxK=%d kSilT=%d kTnT=%d kH0BorWQ=%d kH0WaveMaxN=%d\n", kLdsMax,
           kBorHookLdsMax, kTnLdsMax, kSilLdsMax, kSilMaxK, kSilT, kTnT, kH0BorWQ, kH0WaveMaxN);
    for (int n = lo; n <= hi; ++n) {
        const H0Shape h = h0_shape(n), again = h0_shape(n);
        if (h.T != again.T || h.base != again.base || h.ch != again.ch || h.lds != again.lds || h.hl != again.hl || h.elder != again.elder) return 3;
        printf("N=%d T=%d base=%zu dlds=%d ch=%llu chunk_log2=%d lds=%zu hl=%zu rounds=%d elder=%d pw2=%d tn_lds=%zu sil_lds=%zu\n", n, h.T, h.base,
               (int)h.dlds, (unsigned long long)h.ch, ilog2(h.ch), h.lds, h.hl, h.rounds, h.elder, twonn_pw2(n), (size_t)twonn_pw2(n) * 4,
               silhouette_lds(kSilMaxK, n));
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && std::string(argv[1]) == "h0") return h0_scan(atoi(argv[2]), atoi(argv[3]));
    printf("sizeof Pair=%zu LayerStats=%zu BorCtl=%zu ParCtl=%zu kLdsMax=%d kDenseMaxN=%d\n", sizeof(Pair), sizeof(LayerStats), sizeof(BorCtl),
           sizeof(ParCtl), kLdsMax, kDenseMaxN);
    fprintf(stderr, "knobs step_limit=%llu par_steps_h1=%llu par_steps_h2=%llu par_pool_shift=%d\n", (unsigned long long)step_limit(),
            (unsigned long long)par_step_limit(1), (unsigned long long)par_step_limit(2), par_pool_shift());
    long long L, N, D;
    int maxdim, dtype, is_dist, want64, fg, scale, fb, no_par;
    while (scanf("%lld %lld %lld %d %d %d %d %d %d %d %d", &L, &N, &D, &maxdim, &dtype, &is_dist, &want64, &fg, &scale, &fb, &no_par) == 11) {
        Attempt at;
        at.force_global = fg != 0;
        at.scale = scale;
        at.force_big = fb != 0;
        at.no_par = no_par;
        const std::string first = print(make_plan(L, N, D, maxdim, dtype, is_dist != 0, want64 != 0, at));
        if (print(make_plan(L, N, D, maxdim, dtype, is_dist != 0, want64 != 0, at)) != first) return 3;
        printf("case %lld %lld %lld %d %d %d %d %d %d %d %d\n%s\n", L, N, D, maxdim, dtype, is_dist, want64, fg, scale, fb, no_par, first.c_str());
    }
    return 0;
}
