// dgm_kernels.h -- sliced Wasserstein distance between persistence diagrams on gfx950
// (include/tda_dgm.h has the definition).
//
// k_sw_pairs: grid (pair, direction chunk), one workgroup each.  The host has
// already dropped the non-finite points, so a diagram is a run of finite (b, d)
// rows.  The workgroup copies both diagrams into LDS once (births and deaths as
// two arrays, so that consecutive lanes read consecutive doubles), then per
// direction of its chunk:
//   1. forms V1 and V2, npow = next_pow2(n1 + n2) doubles each, entries >= n
//      set to +inf;
//   2. sorts both ascending with one bitonic network over the two arrays (a
//      stage is npow compare-exchanges, npow / 2 per array, and one barrier);
//      every real value is finite, so the pads end up at the back;
//   3. writes |V1[k] - V2[k]| for k < n and 0 for the pads over V1 (the pads
//      are never subtracted: inf - inf is NaN) and adds V1 up with a fixed
//      halving tree in LDS.
// The tree's shape depends on npow alone, not on the workgroup size or the
// grid, and no atomics are used: a pair's value is a pure function of its two
// point multisets and the direction table.  Both multisets go through the
// same expressions (sw_proj / sw_diag, with explicit fma so that the compiler
// has no contraction to choose), which makes SW(A, A) exactly 0 and SW(A, B)
// equal to SW(B, A) bit for bit.
//
// LDS: (2 n + 2 npow) doubles, 128 KiB at the n = 4096 limit.  Compare-exchange
// strides below 32 doubles are a 2-way bank conflict on ds_read_b64 (32 lanes
// touch two 256-byte rows); strides of 32 and more are conflict-free.
//
// k_sw_sum: one thread per pair adds the pair's M values in index order and
// scales by 1 / M.
#pragma once
#include "rips_device.h"

namespace tda {

constexpr int kSwMaxN = 4096;  // n1 + n2 of a pair at most (TDA_SW_MAX_POINTS)
constexpr int kSwMaxM = 1024;  // directions at most (TDA_SW_MAX_DIRECTIONS)

// p . u and pi(p) . u for p = (b, d), u = (c, s)
__device__ __forceinline__ double sw_proj(double b, double d, double c, double s) { return fma(b, c, d * s); }
__device__ __forceinline__ double sw_diag(double b, double d, double c, double s) {
    const double m = 0.5 * (b + d);
    return fma(m, c, m * s);
}

// dynamic LDS of a workgroup whose pair has n points: births, deaths, V1, V2
__host__ __device__ inline size_t sw_lds_bytes(int n, int npow) { return (size_t)(2 * n + 2 * npow) * sizeof(double); }

// pts (total, 2): the finite points of all diagrams; off [S + 1]: their row boundaries; pairs (P, 2);
// order [gridDim.x]: the pairs of this launch (one size class); dirs (M, 2) = (cos, sin);
// part (P, M): out.  Direction chunk y covers [y * dc, min(M, (y + 1) * dc)).
__global__ __launch_bounds__(1024) void k_sw_pairs(const double* __restrict__ pts, const int64_t* __restrict__ off,
                                                   const int32_t* __restrict__ pairs, const int32_t* __restrict__ order,
                                                   const double* __restrict__ dirs, int M, int dc, double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int t = threadIdx.x, T = blockDim.x;
    const int pr = order[blockIdx.x];
    const int64_t a0 = off[pairs[2 * pr]], b0 = off[pairs[2 * pr + 1]];
    const int n1 = (int)(off[pairs[2 * pr] + 1] - a0), n2 = (int)(off[pairs[2 * pr + 1] + 1] - b0);
    const int n = n1 + n2;
    if (n > kSwMaxN) return;  // the host refuses such a pair before any launch
    int npow = 1;
    while (npow < n) npow <<= 1;
    double* pb = (double*)smem;
    double* pd = pb + n;
    double* v1 = pd + n;
    double* v2 = v1 + npow;
    for (int e = t; e < n; e += T) {
        const double* p = pts + 2 * (e < n1 ? a0 + e : b0 + (e - n1));
        pb[e] = p[0];
        pd[e] = p[1];
    }
    const int i_end = min(M, ((int)blockIdx.y + 1) * dc);
    for (int i = (int)blockIdx.y * dc; i < i_end; ++i) {
        const double c = dirs[2 * i], s = dirs[2 * i + 1];
        __syncthreads();  // the points are in LDS; the previous direction's sum has been read
        for (int e = t; e < npow; e += T) {
            double x1 = __builtin_inf(), x2 = __builtin_inf();
            if (e < n) {
                const double pj = sw_proj(pb[e], pd[e], c, s), dg = sw_diag(pb[e], pd[e], c, s);
                x1 = e < n1 ? pj : dg;
                x2 = e < n1 ? dg : pj;
            }
            v1[e] = x1;
            v2[e] = x2;
        }
        // v1 and v2 are adjacent: compare-exchange q of a stage works on array q / (npow / 2)
        for (int k = 2; k <= npow; k <<= 1) {
            for (int j = k >> 1; j >= 1; j >>= 1) {
                __syncthreads();
                for (int q = t; q < npow; q += T) {
                    const int h = q & (npow / 2 - 1);
                    const int lo = ((h & ~(j - 1)) << 1) | (h & (j - 1)), hi = lo | j;
                    double* v = q < npow / 2 ? v1 : v2;
                    const double x = v[lo], y = v[hi];
                    if ((x > y) == ((lo & k) == 0)) {
                        v[lo] = y;
                        v[hi] = x;
                    }
                }
            }
        }
        __syncthreads();
        for (int e = t; e < npow; e += T) v1[e] = e < n ? fabs(v1[e] - v2[e]) : 0.0;
        for (int h = npow >> 1; h >= 1; h >>= 1) {
            __syncthreads();
            for (int e = t; e < h; e += T) v1[e] += v1[e + h];
        }
        __syncthreads();
        if (t == 0) part[(size_t)pr * M + i] = n ? v1[0] : 0.0;
    }
}

__global__ __launch_bounds__(256) void k_sw_sum(const double* __restrict__ part, int64_t P, int M, double* __restrict__ dist) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const double* r = part + p * M;
    double acc = 0.0;
    for (int i = 0; i < M; ++i) acc += r[i];
    dist[p] = acc / (double)M;
}

}  // namespace tda
