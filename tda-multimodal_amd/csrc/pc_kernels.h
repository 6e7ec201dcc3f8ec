// pc_kernels.h -- persistence curves (include/tda_dgm.h tda_persistence_curve) on gfx950:
//     acc = +0.0; for p in row order: if K_p(t) > 0: acc = acc + (c_p * K_p(t))
// with K the indicator of [b, d) or the tent, the product and the sum each rounded (contraction
// is off wherever a term is formed or added: pc_add), and with TDA_PC_NORMALIZE one division.
//
// Both kernels give one lane one grid value t and let it walk the diagram's rows in row order.
// The rows sit in LDS as (b, d) pairs and coefficients; at every step all lanes of a wave read
// the same row, so each read is one broadcast, and the serial order per (diagram, grid value)
// holds by construction: no reduction across lanes, no atomics, every value written once.  A
// value is therefore a function of its rows, its t and the flags alone; the kernels differ only
// in how lanes are handed out.
//
// k_pc_packed (n <= kPcPackRows rows): a wave per (diagram, tile of 64 grid values), four such
//   items per workgroup, each wave staging its own diagram (one row per lane).  The sweep's
//   diagrams hold tens of points and its grids about 100 values: a workgroup per diagram would
//   leave most of it idle.
// k_pc_chunked (any n): a workgroup per (diagram, tile of 256 grid values), the rows staged in
//   chunks of kPcRows; a lane keeps its acc in a register across the chunks.
#pragma once
#include "bn_kernels.h"  // bn_d2, bn_pt
#include "rips_device.h"

namespace tda {

constexpr int kPcThreads = 256;
constexpr int kPcWaves = kPcThreads / 64;
constexpr int kPcPackRows = 64;  // rows of a packed diagram at most: one per lane of its wave
constexpr int kPcRows = 1024;    // rows of a chunk: 24 KiB of LDS with the coefficients

// acc after the row (b, d, c) at t.  TENT: the tent, else the indicator; COEF: c is read, else it is 1 and the term is K itself.
template <bool TENT, bool COEF>
__device__ __forceinline__ double pc_add(double acc, double t, bn_d2 q, double c) {
#pragma clang fp contract(off)
    double k;
    if constexpr (TENT) {
        const double m = fmin(t - q.x, q.y - t);
        k = m > 0.0 ? m : 0.0;
    } else {
        k = (q.x <= t && t < q.y) ? 1.0 : 0.0;
    }
    double term = k;
    if constexpr (COEF) term = c * k;
    const double sum = acc + term;
    return k > 0.0 ? sum : acc;  // outside the support nothing is added, not even a zero
}

// the value stored: acc, or with W (TDA_PC_NORMALIZE) acc / W[s], +0.0 for W[s] == 0 and for a zero quotient of either sign
__device__ __forceinline__ double pc_value(double acc, const double* __restrict__ W, int s) {
    if (!W) return acc;
    const double w = ld_glb(W, (size_t)s);
    if (w == 0.0) return 0.0;
    const double q = acc / w;
    return q == 0.0 ? 0.0 : q;
}

// items = (diagrams of the launch) * tiles, tiles = ceil(G / 64); order: the launch's diagram ids
template <bool TENT, bool COEF>
__global__ __launch_bounds__(kPcThreads) void k_pc_packed(const double* __restrict__ pts, const double* __restrict__ coef,
                                                          const int64_t* __restrict__ off, const int32_t* __restrict__ order,
                                                          const double* __restrict__ W, const double* __restrict__ grid, int G, int tiles,
                                                          int64_t items, double* __restrict__ out) {
    __shared__ bn_d2 sp[kPcWaves][kPcPackRows];
    __shared__ double sc[kPcWaves][COEF ? kPcPackRows : 1];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t item = (int64_t)blockIdx.x * kPcWaves + wave;
    const bool live = item < items;  // uniform over the wave
    int s = 0, n = 0, g = 0;
    if (live) {
        s = order[item / tiles];
        g = (int)(item % tiles) * 64 + lane;
        const int64_t o = off[s];
        n = (int)(off[s + 1] - o);  // <= kPcPackRows: the class
        if (lane < n) {
            ((TDA_LDS bn_d2*)sp[wave])[lane] = ((const TDA_GLB bn_d2*)pts)[o + lane];
            if constexpr (COEF) st_lds(sc[wave], (size_t)lane, ld_glb(coef, (size_t)(o + lane)));
        }
    }
    __syncthreads();
    if (!live || g >= G) return;
    const double tv = ld_glb(grid, (size_t)g);
    double acc = 0.0;
#pragma unroll 4
    for (int p = 0; p < n; ++p) acc = pc_add<TENT, COEF>(acc, tv, bn_pt(sp[wave], p), COEF ? ld_lds(sc[wave], (size_t)p) : 1.0);
    st_glb(out, (size_t)s * (size_t)G + (size_t)g, pc_value(acc, W, s));
}

// grid: (diagrams of the launch, ceil(G / kPcThreads)); order: the launch's diagram ids
template <bool TENT, bool COEF>
__global__ __launch_bounds__(kPcThreads) void k_pc_chunked(const double* __restrict__ pts, const double* __restrict__ coef,
                                                           const int64_t* __restrict__ off, const int32_t* __restrict__ order,
                                                           const double* __restrict__ W, const double* __restrict__ grid, int G,
                                                           double* __restrict__ out) {
    __shared__ bn_d2 sp[kPcRows];
    __shared__ double sc[COEF ? kPcRows : 1];
    const int t = threadIdx.x;
    const int s = order[blockIdx.x];
    const int64_t o = off[s];
    const int n = (int)(off[s + 1] - o);
    const int g = (int)blockIdx.y * kPcThreads + t;
    const double tv = g < G ? ld_glb(grid, (size_t)g) : 0.0;  // a lane beyond the grid stages rows and stores nothing
    double acc = 0.0;
    for (int c0 = 0; c0 < n; c0 += kPcRows) {
        const int pc = min(kPcRows, n - c0);
        __syncthreads();  // the previous chunk has been read
        for (int i = t; i < pc; i += kPcThreads) {
            ((TDA_LDS bn_d2*)sp)[i] = ((const TDA_GLB bn_d2*)pts)[o + c0 + i];
            if constexpr (COEF) st_lds(sc, (size_t)i, ld_glb(coef, (size_t)(o + c0 + i)));
        }
        __syncthreads();
#pragma unroll 4
        for (int p = 0; p < pc; ++p) acc = pc_add<TENT, COEF>(acc, tv, bn_pt(sp, p), COEF ? ld_lds(sc, (size_t)p) : 1.0);
    }
    if (g < G) st_glb(out, (size_t)s * (size_t)G + (size_t)g, pc_value(acc, W, s));
}

}  // namespace tda
