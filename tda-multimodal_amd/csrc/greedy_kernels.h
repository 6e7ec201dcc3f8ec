// greedy_kernels.h -- greedy furthest-point landmarks (ripser.py's n_perm) on gfx950.
//
// Upstream get_greedy_perm [ripser.py], on the layer's f32 distance matrix dm
// (symmetric, zero diagonal):
//     ds = dm[0, :]; idx_perm[0] = 0
//     for i in 1 .. k-1:
//         idx = argmax(ds)            # first occurrence: the lowest index among equal maxima
//         idx_perm[i] = idx; lambdas[i-1] = ds[idx]
//         ds = minimum(ds, dm[idx, :])
//     lambdas[k-1] = max(ds)
// Every output is an index or an f32 value of dm that is copied and compared,
// never computed, so the kernel reproduces the host loop exactly.
//
// k_greedy_perm: one workgroup of kGpT threads per layer, every layer of the
// call in flight.  ds lives in registers, Q entries per thread (entry q of
// thread t is column q * kGpT + t, so a row read is coalesced); N <= Q * kGpT.
// A selection step is: read row `cur`, ds = min(ds, row), per-thread maximum,
// wave64 butterfly, cross-wave through LDS (one barrier per step: the LDS
// partials are double-buffered), and every thread ends up with the winner.
// The steps are sequential (each row read depends on the previous winner), so
// a step costs one dependent global read plus the two reductions.
//
// The maximum is taken over ONE 64-bit key per entry: the order-preserving
// image of the f32 value in the high word and ~column in the low word.  Keys
// of different columns differ, so the unsigned maximum is a total order --
// larger value first, then the smaller column -- and the winner is numpy's
// argmax whatever the shape of the reduction tree.  Columns j >= N (pad lanes)
// carry the value -1, below every distance.
#pragma once
#include "rips_device.h"

namespace tda {

constexpr int kGpT = 1024;  // threads of k_greedy_perm
constexpr int kGpMaxQ = 8;  // ds entries per thread at most: N <= 8192

// f32 -> u32 with the same order (negative values below positive ones)
__device__ __forceinline__ uint32_t gp_ord(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float gp_unord(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }
__device__ __forceinline__ uint64_t gp_key(float v, uint32_t j) { return ((uint64_t)gp_ord(v) << 32) | (uint32_t)~j; }

template <int Q>
__global__ __launch_bounds__(kGpT) void k_greedy_perm(const float* __restrict__ dm, int n, int k, int64_t* __restrict__ idx_perm,
                                                      float* __restrict__ lambdas) {
    __shared__ uint64_t part[2][kGpT / 64];
    const int l = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const float* Dl = dm + (size_t)l * n * n;
    int64_t* ip = idx_perm + (size_t)l * k;
    float* lam = lambdas + (size_t)l * k;
    float ds[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) ds[q] = q * kGpT + t < n ? __builtin_inff() : -1.0f;
    int cur = 0;
    for (int i = 0; i < k; ++i) {
        if (t == 0) ip[i] = cur;
        const float* row = Dl + (size_t)cur * n;
        float r[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {  // all the loads of the row first: one latency per step
            const int j = q * kGpT + t;
            r[q] = j < n ? row[j] : -1.0f;
        }
        uint64_t best = 0;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            // minimum(ds, row); a pad lane keeps -1
            ds[q] = r[q] < ds[q] ? r[q] : ds[q];
            const uint64_t key = gp_key(ds[q], (uint32_t)(q * kGpT + t));
            best = key > best ? key : best;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const uint64_t o = __shfl_xor(best, m, 64);
            best = o > best ? o : best;
        }
        if (lane == 0) part[i & 1][wv] = best;
        __syncthreads();
        best = part[i & 1][lane & (kGpT / 64 - 1)];
#pragma unroll
        for (int m = kGpT / 128; m >= 1; m >>= 1) {
            const uint64_t o = __shfl_xor(best, m, 64);
            best = o > best ? o : best;
        }
        if (t == 0) lam[i] = gp_unord((uint32_t)(best >> 32));
        cur = (int)~(uint32_t)best;
        if (cur >= n) cur = 0;  // never taken for n >= 1: a pad lane cannot win
    }
}

// sub[l][a][b] = dm[l][idx[a]][idx[b]] (the landmarks' own matrix, what persistence runs on) and,
// when dperm is given, dperm[l][a][:] = dm[l][idx[a]][:] (ripser.py's dperm2all).  One workgroup
// per (landmark a, layer l).
__global__ __launch_bounds__(256) void k_gather_landmarks(const float* __restrict__ dm, int n, int k, const int64_t* __restrict__ idx_perm,
                                                          float* __restrict__ sub, float* __restrict__ dperm) {
    const int a = blockIdx.x, l = blockIdx.y;
    const int64_t* ip = idx_perm + (size_t)l * k;
    const float* row = dm + ((size_t)l * n + (size_t)ip[a]) * n;
    float* so = sub + ((size_t)l * k + a) * k;
    for (int b = threadIdx.x; b < k; b += blockDim.x) so[b] = row[ip[b]];
    if (dperm) {
        float* po = dperm + ((size_t)l * k + a) * n;
        for (int j = threadIdx.x; j < n; j += blockDim.x) po[j] = row[j];
    }
}

}  // namespace tda
