// sh0_kernels.h -- H0 persistence of subsamples on gfx950: Prim's algorithm over an index table.
//
// Subsample b of a layer has s = sizes[b] positions; position j holds the point p_j = idx[b][j]
// (include/tda_rips.h tda_subsample_h0 pins the definition).  On the layer's f32 matrix dm:
//     the tree is {0}, key[j] = dm[p_0][p_j]
//     step t = 1 .. s-1: j* = the position outside the tree with the smallest key (`<`, the lowest
//     position among equal keys); death[t-1] = key[j*]; acc += term(key[j*]); j* joins the tree;
//     key[j] = dm[p_j*][p_j] wherever that is < key[j]
// and E = acc, a double owned by one lane and added to in step order, never reduced in parallel.
// A death is a value of dm, copied and compared, never computed.
//
// The argmin is a 64-bit minimum over (ordered key bits << 32 | position): sh0_ord maps a float to
// an unsigned integer of the same order (-0.0 as +0.0, so that two zeros tie as `<` has them), the
// position in the low word gives the tie rule, and whatever the keys hold (a NaN of unchecked
// device input included) some position outside the tree is chosen while there is one: the loop
// runs s - 1 steps and every index it reads was validated on the host or is 0.
//
// Two paths, chosen by the plan (sh0_plan.h):
//   resident, N <= kSh0LdsN and m <= kSh0LdsM: a workgroup stages the layer's whole matrix in LDS
//     once (N * N * 4 <= 64 KiB of static LDS) and serves kSh0PerBlock subsamples from it, one wave
//     per subsample at a time.  A lane holds the keys, the points and the in-tree flags of the
//     positions lane and lane + 64 in registers; the argmin is a wave reduction by shuffles, the
//     winner's key and point come by one shuffle each.  No barrier after the staging.
//   global, everything else: one 256-thread workgroup per (subsample, layer).  The keys (f32) and
//     the points (u16, 0xFFFF once in the tree: N <= 8192) live in dynamic LDS, 6 m bytes behind a
//     128-byte head.  A thread owns the positions t, t + 256, ...: one pass updates their keys from
//     row p_j* (a gather from global memory at the columns p_j) and takes their minimum for the next
//     step, then a wave reduction, four partials in the head (two sets, used in turn) and ONE
//     barrier per step.
// Neither path has been tuned beyond this layout (what is measured).
#pragma once
#include "resample_kernels.h"

namespace tda {

constexpr int kSh0T = 256;          // threads of a workgroup, on both paths
constexpr int kSh0LdsN = kRsLdsN;   // the resident path's largest N: kSh0LdsN^2 * 4 = 64 KiB
constexpr int kSh0LdsM = 128;       // and its largest row length: two positions per lane
constexpr int kSh0PerBlock = 16;    // subsamples served by one workgroup of the resident path
constexpr int kSh0Head = 128;       // global path: u64 part[2][4], then i32 partp[2][4], in front of the keys
constexpr uint64_t kSh0None = ~0ull;  // no candidate: above every (key, position)

// an unsigned integer ordered as the floats are; -0.0 and +0.0 map to one value
__device__ __forceinline__ uint32_t sh0_ord(float w) {
    uint32_t u = __float_as_uint(w);
    if (u == 0x80000000u) u = 0;
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ uint64_t sh0_pack(float w, int j) { return (uint64_t)sh0_ord(w) << 32 | (uint32_t)j; }

__device__ __forceinline__ uint64_t sh0_wave_min(uint64_t v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const uint64_t o = __shfl_xor(v, s, 64);
        v = o < v ? o : v;
    }
    return v;
}

// kPow: term(w) = pow(w, alpha); else w * w when sq, else w (both exact in f64)
template <bool kPow>
__device__ __forceinline__ double sh0_term(float w, bool sq, double alpha) {
    const double d = (double)w;
    if constexpr (kPow) return pow(d, alpha);
    return sq ? d * d : d;
}

// idx: the chunk's first table, (nb, m) int32 per layer, layers idx_lstride entries apart (0: one
// table for all); sizes: the chunk's first size; E: the chunk's first value, layers e_lstride
// entries apart; deaths (or NULL): the chunk's first row of m - 1, layers d_lstride entries apart.
// kLds: grid (ceil(nb / kSh0PerBlock), layers), no dynamic LDS; else grid (nb, layers), dynamic LDS
// kSh0Head + 6 m bytes.
template <bool kLds, bool kPow>
__global__ __launch_bounds__(kSh0T) void k_subsample_h0(const float* __restrict__ dm, int n, int m, int nb, const int32_t* __restrict__ idx,
                                                        size_t idx_lstride, const int32_t* __restrict__ sizes, int sq, double alpha,
                                                        double* __restrict__ E, size_t e_lstride, float* __restrict__ deaths, size_t d_lstride) {
    const int l = blockIdx.y, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const float* Dl = dm + (size_t)l * n * n;
    const int32_t* il = idx + (size_t)l * idx_lstride;
    double* El = E + (size_t)l * e_lstride;
    float* dlay = deaths ? deaths + (size_t)l * d_lstride : nullptr;
    if constexpr (kLds) {
        __shared__ float tile[kSh0LdsN * kSh0LdsN];
        for (int e = t; e < n * n; e += kSh0T) tile[e] = Dl[e];
        __syncthreads();
        const int j0 = lane, j1 = lane + 64;
        for (int r = wv; r < kSh0PerBlock; r += kSh0T / 64) {
            const int b = blockIdx.x * kSh0PerBlock + r;
            if (b >= nb) break;  // the whole wave: b does not depend on the lane
            const int s = sizes[b];
            const int32_t* ix = il + (size_t)b * m;
            float* dl = dlay ? dlay + (size_t)b * (m - 1) : nullptr;
            const int p0 = j0 < s ? ix[j0] : 0, p1 = j1 < s ? ix[j1] : 0;
            const float* row = tile + ix[0] * n;
            float k0 = row[p0], k1 = row[p1];
            bool in0 = j0 >= s || j0 == 0, in1 = j1 >= s;  // in the tree, or no such position
            double acc = 0.0;
            for (int step = 1; step < s; ++step) {
                const uint64_t c0 = in0 ? kSh0None : sh0_pack(k0, j0), c1 = in1 ? kSh0None : sh0_pack(k1, j1);
                const uint64_t best = sh0_wave_min(c0 < c1 ? c0 : c1);
                const int js = (int)(uint32_t)best;
                const bool hi = (js & 64) != 0;
                const float kw = __shfl(hi ? k1 : k0, js & 63, 64);
                const int ps = __shfl(hi ? p1 : p0, js & 63, 64);  // a validated index or 0: the row read stays in the tile
                if (lane == 0) {
                    if (dl) dl[step - 1] = kw;
                    acc += sh0_term<kPow>(kw, sq != 0, alpha);
                }
                in0 = in0 || js == j0, in1 = in1 || js == j1;
                row = tile + ps * n;
                const float w0 = row[p0], w1 = row[p1];
                k0 = !in0 && w0 < k0 ? w0 : k0;
                k1 = !in1 && w1 < k1 ? w1 : k1;
            }
            if (lane == 0) El[b] = acc;
            if (dl)
                for (int j = s - 1 + lane; j < m - 1; j += 64) dl[j] = 0.0f;
        }
    } else {
        extern __shared__ __align__(16) unsigned char sh0_lds[];
        uint64_t* part = reinterpret_cast<uint64_t*>(sh0_lds);       // [2][4]
        int* partp = reinterpret_cast<int*>(sh0_lds + 64);           // [2][4]
        float* keys = reinterpret_cast<float*>(sh0_lds + kSh0Head);  // [m]
        uint16_t* pts = reinterpret_cast<uint16_t*>(keys + m);       // [m]
        const int b = blockIdx.x;
        const int s = sizes[b];
        const int32_t* ix = il + (size_t)b * m;
        float* dl = dlay ? dlay + (size_t)b * (m - 1) : nullptr;
        const float* row = Dl + (size_t)ix[0] * n;
        uint64_t loc = kSh0None;
        int locp = 0;
        for (int j = t; j < s; j += kSh0T) {
            const int p = ix[j];
            const float w = row[p];
            keys[j] = w;
            pts[j] = j ? (uint16_t)p : (uint16_t)0xFFFF;
            const uint64_t c = sh0_pack(w, j);
            if (j && c < loc) loc = c, locp = p;
        }
        double acc = 0.0;
        for (int step = 1; step < s; ++step) {
            const uint64_t wbest = sh0_wave_min(loc);
            const int wp = __shfl(locp, (int)(uint32_t)wbest & 63, 64);  // position j belongs to lane j & 63
            const int set = (step & 1) * 4;
            if (lane == 0) part[set + wv] = wbest, partp[set + wv] = wp;
            __syncthreads();  // the one barrier of a step: set `set` is written again two barriers from here
            uint64_t best = part[set];
            int ps = partp[set];
#pragma unroll
            for (int w = 1; w < kSh0T / 64; ++w) {
                const uint64_t o = part[set + w];
                if (o < best) best = o, ps = partp[set + w];
            }
            const int js = (int)(uint32_t)best;
            if (t == 0) {
                const float kw = (unsigned)js < (unsigned)s ? keys[js] : 0.0f;  // its owner wrote it before the barrier and skips it below
                if (dl) dl[step - 1] = kw;
                acc += sh0_term<kPow>(kw, sq != 0, alpha);
            }
            row = Dl + (size_t)ps * n;  // ps: a validated index or 0
            loc = kSh0None, locp = 0;
            for (int j = t; j < s; j += kSh0T) {
                const unsigned p = pts[j];
                if (j == js) {
                    pts[j] = 0xFFFF;
                    continue;
                }
                if (p == 0xFFFFu) continue;
                float k = keys[j];
                const float w = row[p];
                if (w < k) keys[j] = k = w;
                const uint64_t c = sh0_pack(k, j);
                if (c < loc) loc = c, locp = (int)p;
            }
        }
        if (t == 0) El[b] = acc;
        if (dl)
            for (int j = s - 1 + t; j < m - 1; j += kSh0T) dl[j] = 0.0f;
    }
}

}  // namespace tda
