// hk_kernels.h -- the heat (persistence scale-space) kernel between diagrams on gfx950
// (include/tda_dgm.h has the definitions, the order of the sum, the promises and C(n1, n2)).
//
// k_hk_parts: one workgroup of one wave per part of an evaluation (dgm_plan.h: kHkRows = 64
// rows of the first diagram by kHkChunk = 256 columns of the second).  The part's columns are
// staged in LDS once (4 KiB, static); lane l owns row 64 rb + l, keeps its point in registers
// and walks the columns q in order, every lane reading the same LDS address (a broadcast, no
// bank conflict), adding t(p, q) = exp(-c8 r2) - exp(-c8 m2) to one accumulator: a row's sum
// over a chunk has one order.  The 64 row sums are then added by a butterfly (l ^ 1, l ^ 2,
// ... l ^ 32; a + b == b + a, so every lane ends with the same bits) and lane 0 stores the
// part.  Choices: one row per lane -- the two exponentials of a term are independent chains,
// which together with the other waves of the CU is expected to keep the float64 pipe busy
// (the share of its peak was not measured, and a single pair at the limit gives a SIMD one
// wave), and a second row would double the registers of the exp expansion; 64 threads -- the
// row tree is a wave's, with no barrier but the one after staging, and the block size is the
// same for every size class since it enters the tree; 4 KiB of LDS and the registers of one exp leave the wave slots
// (32 per CU) as the occupancy limit.  One 4096 x 4096 pair is 1024 workgroups, four per CU.
//
// k_hk_sum: one wave per evaluation adds its parts -- lane l those numbered l, l + 64, ... in
// order, then the same butterfly -- and lane 0 stores cn * sum.  An evaluation without parts
// (an empty diagram) gives cn * +0.0 = +0.0.
//
// No atomics, no fused multiply-add in r2 and m2 (hk_term), and nothing in either kernel
// depends on the grid: the classes of hk_host.h only trim the number of idle workgroups.
#pragma once
#include "bn_kernels.h"  // bn_d2
#include "dgm_plan.h"    // kHkRows, kHkChunk
#include "rips_device.h"

namespace tda {

constexpr int kHkMaxN = 4096;  // TDA_HK_MAX_POINTS
static_assert(kHkRows == 64, "a part's rows are the lanes of one wave");
constexpr int kHkSumThreads = 256;

// t(p, q): individually rounded operations in the header's order, never contracted
__device__ __forceinline__ double hk_term(bn_d2 p, bn_d2 q, double nc8) {
#pragma clang fp contract(off)
    const double db = p.x - q.x, dd = p.y - q.y;
    const double mb = p.x - q.y, md = p.y - q.x;
    const double r2 = db * db + dd * dd;
    const double m2 = mb * mb + md * md;
    const double e1 = exp(nc8 * r2), e2 = exp(nc8 * m2);
    return e1 - e2;
}

__device__ __forceinline__ double hk_wave_sum(double v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = v + __longlong_as_double((long long)shfl_xor_u64((uint64_t)__double_as_longlong(v), m));
    return v;
}

__global__ __launch_bounds__(kHkRows) void k_hk_parts(const double* __restrict__ pts, const int64_t* __restrict__ off,
                                                      const int32_t* __restrict__ pairs, const int32_t* __restrict__ order,
                                                      const int64_t* __restrict__ part_off, double nc8, double* __restrict__ part) {
    __shared__ bn_d2 sq[kHkChunk];
    const int w = order[blockIdx.x];
    const int i = pairs[2 * w], j = pairs[2 * w + 1];
    const int64_t oi = off[i], oj = off[j];
    const int n1 = (int)(off[i + 1] - oi), n2 = (int)(off[j + 1] - oj);
    const int ncc = (n2 + kHkChunk - 1) / kHkChunk;
    const int parts = ((n1 + kHkRows - 1) / kHkRows) * ncc;
    const int k = blockIdx.y;
    if (k >= parts) return;  // uniform over the workgroup: the class's grid is that of its largest evaluation
    const int rb = k / ncc, cc = k - rb * ncc;
    const int q0 = cc * kHkChunk, nq = min(kHkChunk, n2 - q0);
    const int lane = threadIdx.x;
    for (int e = lane; e < nq; e += kHkRows) ((TDA_LDS bn_d2*)sq)[e] = ((const TDA_GLB bn_d2*)pts)[oj + q0 + e];
    __syncthreads();
    const int p = rb * kHkRows + lane;
    double acc = 0.0;
    if (p < n1) {
        const bn_d2 me = ((const TDA_GLB bn_d2*)pts)[oi + p];
        for (int q = 0; q < nq; ++q) {
#pragma clang fp contract(off)
            acc = acc + hk_term(me, bn_pt(sq, q), nc8);
        }
    }
    acc = hk_wave_sum(acc);
    if (lane == 0) st_glb(part, (size_t)(part_off[w] + k), acc);
}

// the evaluations w0 .. w1 - 1
__global__ __launch_bounds__(kHkSumThreads) void k_hk_sum(const double* __restrict__ part, const int64_t* __restrict__ part_off, int64_t w0,
                                                          int64_t w1, double cn, double* __restrict__ kern) {
    const int64_t w = w0 + (int64_t)blockIdx.x * (kHkSumThreads / 64) + (threadIdx.x >> 6);
    if (w >= w1) return;  // uniform over the wave
    const int lane = threadIdx.x & 63;
    const int64_t o = part_off[w], n = part_off[w + 1] - o;
    double acc = 0.0;
    for (int64_t k = lane; k < n; k += 64) {
#pragma clang fp contract(off)
        acc = acc + ld_glb(part, (size_t)(o + k));
    }
    acc = hk_wave_sum(acc);
    if (lane == 0) st_glb(kern, (size_t)w, cn * acc);
}

}  // namespace tda
