// resample_kernels.h -- the resampling stage of the bootstrap confidence bands on gfx950.
//
// A resample b of a layer is the m points ix = idx[b][0 .. m-1] of its N.  On the layer's f32
// distance matrix dm (symmetric, zero diagonal):
//     H[l][b] = max_i min_{j < m} dm[l][ix[j]][i]     (k_resample_hausdorff)
// H is the Hausdorff distance between the cloud and the resample: the resample is a subset of the
// cloud, so the other directed distance is 0.  For the Rips filtration parameterised by the
// diameter, d_B(dgm(X), dgm(X*)) <= 2 d_GH(X, X*) <= 2 H(X, X*) (Chazal, de Silva, Oudot 2014): 2 H
// bounds how far a diagram moves under the resample without any persistence computation.
// The kernel only copies and compares f32 values of dm, never computes one, so its output is
// exact and independent of the shape of any reduction: for a dm without NaN the numpy restatement
// dm[ix].min(0).max() gives the same bits.  The comparisons are `<` and `>`, so a NaN in dm is
// skipped where numpy would propagate it; only unchecked device input can hold one.
//
// k_resample_hausdorff reads dm by the sampled ROW and runs its lanes over the column i (dm is
// symmetric), so every read is coalesced.  Two paths, chosen by kRsLdsN:
//   N <= kRsLdsN: a workgroup stages the layer's whole matrix in LDS once (N * N * 4 <= 64 KiB of
//     static LDS) and serves kRsPerBlock resamples from it, one wave per resample at a time: lanes
//     over i (two columns per lane), the sampled row index the same for the whole wave, then a
//     wave maximum.  No barrier after the staging.
//   above: one workgroup per (resample, layer), threads over i, the loop over the m rows reads
//     global memory, then a block maximum (plain f32).
// A lane without a column starts from -inf and folds nothing in, so it cannot win the maximum.
// The kernel has not been tuned beyond this layout (bootstrap: what is measured).
#pragma once
#include "rips_device.h"

namespace tda {

constexpr int kRsLdsN = 128;     // the LDS path's largest N: kRsLdsN^2 * 4 = 64 KiB
constexpr int kRsT = 256;        // threads of a workgroup, on both paths
constexpr int kRsPerBlock = 16;  // resamples served by one workgroup of the LDS path

__device__ __forceinline__ float rs_wave_max(float v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const float o = __shfl_xor(v, s, 64);
        v = o > v ? o : v;
    }
    return v;
}

// idx: the chunk's first table, (nb, m) int32 per layer, layers idx_lstride entries apart (0: one
// table for all); H: the chunk's first value, layers h_lstride entries apart.
// kLds: grid (ceil(nb / kRsPerBlock), layers); else grid (nb, layers).
template <bool kLds>
__global__ __launch_bounds__(kRsT) void k_resample_hausdorff(const float* __restrict__ dm, int n, int m, int nb,
                                                             const int32_t* __restrict__ idx, size_t idx_lstride, float* __restrict__ H,
                                                             size_t h_lstride) {
    const int l = blockIdx.y, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const float* Dl = dm + (size_t)l * n * n;
    const int32_t* il = idx + (size_t)l * idx_lstride;
    float* Hl = H + (size_t)l * h_lstride;
    const float ninf = -__builtin_inff(), pinf = __builtin_inff();
    if constexpr (kLds) {
        __shared__ float tile[kRsLdsN * kRsLdsN];
        for (int e = t; e < n * n; e += kRsT) tile[e] = Dl[e];
        __syncthreads();
        const int i0 = lane, i1 = lane + 64;
        for (int r = wv; r < kRsPerBlock; r += kRsT / 64) {
            const int b = blockIdx.x * kRsPerBlock + r;
            if (b >= nb) break;  // the whole wave: b does not depend on the lane
            const int32_t* ix = il + (size_t)b * m;
            float mn0 = pinf, mn1 = pinf;
            for (int j = 0; j < m; ++j) {
                const float* row = tile + ix[j] * n;
                const float v0 = i0 < n ? row[i0] : pinf, v1 = i1 < n ? row[i1] : pinf;
                mn0 = v0 < mn0 ? v0 : mn0;
                mn1 = v1 < mn1 ? v1 : mn1;
            }
            float mx = i0 < n ? mn0 : ninf;
            if (i1 < n) mx = mn1 > mx ? mn1 : mx;
            mx = rs_wave_max(mx);
            if (lane == 0) Hl[b] = mx;
        }
    } else {
        __shared__ float part[kRsT / 64];
        const int b = blockIdx.x;
        const int32_t* ix = il + (size_t)b * m;
        float mx = ninf;
        for (int i = t; i < n; i += kRsT) {
            float mn = pinf;
#pragma unroll 4
            for (int j = 0; j < m; ++j) {
                const float v = Dl[(size_t)ix[j] * n + i];
                mn = v < mn ? v : mn;
            }
            mx = mn > mx ? mn : mx;
        }
        mx = rs_wave_max(mx);
        if (lane == 0) part[wv] = mx;
        __syncthreads();
        if (t == 0) {
#pragma unroll
            for (int w = 1; w < kRsT / 64; ++w) mx = part[w] > mx ? part[w] : mx;
            Hl[b] = mx;
        }
    }
}

}  // namespace tda
