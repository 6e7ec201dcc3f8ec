// pf_kernels.h -- the persistence Fisher distance between diagrams on gfx950
// (include/tda_dgm.h has the definitions, the order of the sums, the promises and B(n1, n2)).
//
// k_pf_parts: one workgroup of one wave per part of a pair (dgm_plan.h: kPfLanes = 64 evaluation
// points of Z = U then V).  Lane l owns z = 64 k + l, builds its point from the two diagrams
// (pf_z) and keeps it in registers.  The sources are staged kPfChunk = 128 at a time, U_i and V_i
// side by side (4 KiB of LDS, static; a staging lane builds pi(p) itself), and every lane walks
// them in order, all lanes reading the same LDS address (a broadcast, no bank conflict), into two
// accumulators: rhoU over U_i and rhoV over V_i.  The two exponentials of a step are independent
// chains, as the two of a heat term are.  A density's sum is one series over i = 0 .. M - 1
// whatever the chunk, so the chunk does not enter the order.  Then rhoU, rhoV and
// sqrt(rhoU * rhoV) of the 64 lanes are added by the butterfly of hk_kernels.h (a lane beyond
// 2 M counts +0.0) and lane 0 stores the part's three sums.  The square root is __dsqrt_rn, the
// correctly rounded one: promise 1 of the header rests on it.  Choices: 64 threads -- the tree is
// a wave's, with no barrier but those of the staging, and the block size is the same for every
// size class since it enters the tree; every wave stages all the sources again (16 bytes per
// source from L2 against 64 exponentials), which a workgroup of several waves would share at the
// price of a tree across waves; 4 KiB of LDS leaves the wave slots (32 per CU) as the
// occupancy limit.  One 1024 x 1024 pair is 64 workgroups: a quarter of the CUs, one wave each.
//
// k_pf_sum: one wave per pair, part k in lane k (at most 64 parts; a lane without a part holds
// +0.0), the same butterfly for each of the three sums, and lane 0 stores them.
//
// No atomics, no fused multiply-add (pf_term, the product under the root and every addition),
// and nothing in either kernel depends on the grid: the classes of pf_host.h only trim the
// number of idle workgroups.
#pragma once
#include "hk_kernels.h"  // bn_d2, bn_pt, hk_wave_sum, kPfLanes, kPfChunk (dgm_plan.h)

namespace tda {

constexpr int kPfMaxN = 1024;  // TDA_PF_MAX_POINTS
static_assert(kPfLanes == 64, "a part's evaluation points are the lanes of one wave");
static_assert(kPfChunk % kPfLanes == 0, "a chunk is staged in whole rounds of the wave");
static_assert((2 * 2 * kPfMaxN + kPfLanes - 1) / kPfLanes <= 64, "k_pf_sum holds a pair's parts in one wave");
constexpr int kPfSumThreads = 256;

// pi(p): the projection on the diagonal, one rounded addition and an exact halving
__device__ __forceinline__ bn_d2 pf_pi(bn_d2 p) {
#pragma clang fp contract(off)
    const double m = (p.x + p.y) * 0.5;
    return bn_d2{m, m};
}

// U_i = F_i for i < n1, else pi(G_{i - n1}); V_i = G_i for i < n2, else pi(F_{i - n2}).  0 <= i < n1 + n2.
__device__ __forceinline__ bn_d2 pf_u(const TDA_GLB bn_d2* F, int n1, const TDA_GLB bn_d2* G, int i) { return i < n1 ? F[i] : pf_pi(G[i - n1]); }
__device__ __forceinline__ bn_d2 pf_v(const TDA_GLB bn_d2* F, const TDA_GLB bn_d2* G, int n2, int i) { return i < n2 ? G[i] : pf_pi(F[i - n2]); }

// e(z, w): individually rounded operations in the header's order, never contracted
__device__ __forceinline__ double pf_term(bn_d2 z, bn_d2 w, double nc2) {
#pragma clang fp contract(off)
    const double db = z.x - w.x, dd = z.y - w.y;
    const double r2 = db * db + dd * dd;
    const double t = nc2 * r2;
    return t < -(double)TDA_PF_CUT ? 0.0 : exp(t);
}

__global__ __launch_bounds__(kPfLanes) void k_pf_parts(const double* __restrict__ pts, const int64_t* __restrict__ off,
                                                       const int32_t* __restrict__ pairs, const int32_t* __restrict__ order,
                                                       const int64_t* __restrict__ part_off, double nc2, double* __restrict__ part) {
    __shared__ bn_d2 su[kPfChunk], sv[kPfChunk];
    const int w = order[blockIdx.x];
    const int i = pairs[2 * w], j = pairs[2 * w + 1];
    const int64_t oi = off[i], oj = off[j];
    const int n1 = (int)(off[i + 1] - oi), n2 = (int)(off[j + 1] - oj);
    const int M = n1 + n2;
    const int parts = (2 * M + kPfLanes - 1) / kPfLanes;
    const int k = blockIdx.y;
    if (k >= parts) return;  // uniform over the workgroup: the class's grid is that of its largest pair
    const TDA_GLB bn_d2* F = (const TDA_GLB bn_d2*)pts + oi;
    const TDA_GLB bn_d2* G = (const TDA_GLB bn_d2*)pts + oj;
    const int lane = threadIdx.x;
    const int z = k * kPfLanes + lane;
    const bool live = z < 2 * M;
    bn_d2 me = {0.0, 0.0};
    if (live) me = z < M ? pf_u(F, n1, G, z) : pf_v(F, G, n2, z - M);
    double ru = 0.0, rv = 0.0;
    for (int c0 = 0; c0 < M; c0 += kPfChunk) {
        const int nq = min(kPfChunk, M - c0);
        __syncthreads();  // the previous chunk has been read
        for (int e = lane; e < nq; e += kPfLanes) {
            ((TDA_LDS bn_d2*)su)[e] = pf_u(F, n1, G, c0 + e);
            ((TDA_LDS bn_d2*)sv)[e] = pf_v(F, G, n2, c0 + e);
        }
        __syncthreads();
        if (live)
            for (int q = 0; q < nq; ++q) {
#pragma clang fp contract(off)
                ru = ru + pf_term(me, bn_pt(su, q), nc2);
                rv = rv + pf_term(me, bn_pt(sv, q), nc2);
            }
    }
    double sh = 0.0;
    if (live) {
#pragma clang fp contract(off)
        const double p = ru * rv;
        sh = __dsqrt_rn(p);
    }
    const double ta = hk_wave_sum(ru), tb = hk_wave_sum(rv), th = hk_wave_sum(sh);  // a dead lane holds +0.0 in all three
    if (lane == 0) {
        const size_t o = 3 * (size_t)(part_off[w] + k);
        st_glb(part, o, ta);
        st_glb(part, o + 1, tb);
        st_glb(part, o + 2, th);
    }
}

// the pairs w0 .. w1 - 1; sums: (a, b, h) of every pair
__global__ __launch_bounds__(kPfSumThreads) void k_pf_sum(const double* __restrict__ part, const int64_t* __restrict__ part_off, int64_t w0,
                                                          int64_t w1, double* __restrict__ sums) {
    const int64_t w = w0 + (int64_t)blockIdx.x * (kPfSumThreads / 64) + (threadIdx.x >> 6);
    if (w >= w1) return;  // uniform over the wave
    const int lane = threadIdx.x & 63;
    const int64_t o = part_off[w], n = part_off[w + 1] - o;  // n <= 64
    double v[3] = {0.0, 0.0, 0.0};
    if (lane < n)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = ld_glb(part, 3 * (size_t)(o + lane) + c);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = hk_wave_sum(v[c]);
    if (lane == 0)
#pragma unroll
        for (int c = 0; c < 3; ++c) st_glb(sums, 3 * (size_t)w + c, v[c]);
}

}  // namespace tda
