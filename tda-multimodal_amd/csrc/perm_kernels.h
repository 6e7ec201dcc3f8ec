// perm_kernels.h -- the permutation test between groups of diagrams (include/tda_rips.h
// tda_permutation_test) on gfx950.
//
// A labelling l of the S diagrams (one uint8 group code each) has the statistic
//     col_j = sum over i = 0 .. S-1 in that order, from +0.0, of w[i][j] where l_i == l_j
//     t_j   = c[l_j] * col_j                                   (never fused with an addition)
//     T(l)  = 64 lane sums over j = lane, lane + 64, ... in that order from +0.0, then the xor
//             butterfly 1, 2, 4, 8, 16, 32                     (perm_wave_sum, as hk_wave_sum)
// on the (S, S) float64 matrix w (symmetric, +0.0 diagonal, finite, >= 0: checked on the host) and
// the group weights c.  Both kernels below evaluate exactly this, for the rows of a label table;
// which one runs is decided by S alone, and neither the grid, the row's position nor the number of
// rows enters an addition's order.  No atomics; every row's value is written once.
//
// k_perm_resident (S <= kPermLdsS): the workgroup stages w in dynamic LDS once (S * S * 8 bytes,
//   128 KiB at S = 128: one workgroup of 16 waves per CU) and serves rows of the table from it, one
//   wave per row at a time, waves striding over the rows.  Lanes run over j (two columns per lane),
//   i is uniform over the wave: a row read of w is consecutive 8-byte words, conflict-free.  l_j sits
//   in a register and l_i is broadcast from the lane that holds it (v_readlane, i is uniform).  One
//   barrier after the staging, none after it.
// k_perm_tiled (S <= 2048): a workgroup of 256 threads serves kPermR rows of the table.  A thread
//   owns one column j of a slab of 256 columns and keeps col_j for the kPermR labellings in
//   registers while the rows of w stream past in ascending i, so w is read once per kPermR
//   labellings.  A thread is the only reader of its column, so the rows go from global memory (L2)
//   straight to its registers; what goes through LDS is what threads share: the kPermR labels of
//   every i, packed in one 8-byte word per i (one broadcast read per row), and the slab's t_j, which
//   wave 0 adds into its lane sums in ascending j (wave 0's lane k takes columns k, k + 64, k + 128,
//   k + 192 of the slab, then the next slab's).  The slabs and the waves only partition the columns;
//   every addition is in the order above.
#pragma once
#include "rips_device.h"

namespace tda {

constexpr int kPermLdsS = 128;    // the resident path's largest S: kPermLdsS^2 * 8 = 128 KiB of the CU's 160 KiB
constexpr int kPermResT = 1024;   // threads of a resident workgroup: 16 waves, 4 per SIMD (what ds_read_b64 needs to reach the LDS rate)
constexpr int kPermMaxS = 2048;   // TDA_PERM_MAX_S
constexpr int kPermT = 256;       // threads of a tiled workgroup = columns of a slab
constexpr int kPermR = 8;         // labellings served by a tiled workgroup: their labels at i are one 8-byte word
static_assert(kPermLdsS <= 128, "two columns per lane");
static_assert(kPermR == 8, "a row's labels are the bytes of one uint64_t");

__device__ __forceinline__ double perm_wave_sum(double v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = v + __longlong_as_double((long long)shfl_xor_u64((uint64_t)__double_as_longlong(v), m));
    return v;
}

// lab: (nrows, S) codes; out[r] = T(lab[r]).  Dynamic LDS: S * S * 8 bytes.  Any grid.
__global__ __launch_bounds__(kPermResT) void k_perm_resident(const double* __restrict__ w, int S, const uint8_t* __restrict__ lab,
                                                             const double* __restrict__ c, int nrows, double* __restrict__ out) {
    extern __shared__ double perm_tile[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (int e = t; e < S * S; e += kPermResT) st_lds(perm_tile, (size_t)e, ld_glb(w, (size_t)e));
    __syncthreads();
    const int j0 = lane, j1 = lane + 64;
    const bool has0 = j0 < S, has1 = j1 < S;
    const int a0 = has0 ? j0 : S - 1, a1 = has1 ? j1 : S - 1;  // a lane without a column reads a valid word and selects nothing
    const int n0 = S < 64 ? S : 64;
    for (int r = blockIdx.x * (kPermResT / 64) + wv; r < nrows; r += gridDim.x * (kPermResT / 64)) {  // the whole wave: r does not depend on the lane
        const uint8_t* L = lab + (size_t)r * S;
        const int l0 = has0 ? (int)ld_glb(L, (size_t)j0) : 255, l1 = has1 ? (int)ld_glb(L, (size_t)j1) : 255;  // 255: no group's code
        double c0 = 0.0, c1 = 0.0;
#pragma unroll 8
        for (int i = 0; i < n0; ++i) {
#pragma clang fp contract(off)
            const int li = __builtin_amdgcn_readlane(l0, i);
            const double w0 = ld_lds(perm_tile, (size_t)(i * S + a0)), w1 = ld_lds(perm_tile, (size_t)(i * S + a1));
            c0 = c0 + (li == l0 ? w0 : 0.0);
            c1 = c1 + (li == l1 ? w1 : 0.0);
        }
#pragma unroll 8
        for (int i = 64; i < S; ++i) {
#pragma clang fp contract(off)
            const int li = __builtin_amdgcn_readlane(l1, i - 64);
            const double w0 = ld_lds(perm_tile, (size_t)(i * S + a0)), w1 = ld_lds(perm_tile, (size_t)(i * S + a1));
            c0 = c0 + (li == l0 ? w0 : 0.0);
            c1 = c1 + (li == l1 ? w1 : 0.0);
        }
        double acc = 0.0;
        {
#pragma clang fp contract(off)
            const double t0 = has0 ? ld_glb(c, (size_t)l0) * c0 : 0.0;
            const double t1 = has1 ? ld_glb(c, (size_t)l1) * c1 : 0.0;
            acc = acc + t0;
            if (has1) acc = acc + t1;
        }
        acc = perm_wave_sum(acc);
        if (lane == 0) st_glb(out, (size_t)r, acc);
    }
}

// lab: (nrows, S) codes; out[r] = T(lab[r]).  Grid: ceil(nrows / kPermR).
__global__ __launch_bounds__(kPermT) void k_perm_tiled(const double* __restrict__ w, int S, const uint8_t* __restrict__ lab,
                                                       const double* __restrict__ c, int nrows, double* __restrict__ out) {
    __shared__ uint64_t li8[kPermMaxS];    // byte k of li8[i]: the code of diagram i in the workgroup's k-th labelling
    __shared__ double tj[kPermR][kPermT];  // the slab's t_j
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int b0 = blockIdx.x * kPermR;
    const int nr = min(kPermR, nrows - b0);
    for (int i = t; i < S; i += kPermT) {
        uint64_t v = 0;
#pragma unroll
        for (int k = 0; k < kPermR; ++k) {
            const int r = b0 + (k < nr ? k : 0);  // past the table's end: the first labelling again, its value is not written
            v |= (uint64_t)ld_glb(lab, (size_t)r * S + i) << (8 * k);
        }
        st_lds(li8, (size_t)i, v);
    }
    __syncthreads();
    double part[kPermR];  // wave 0: the lane sums
#pragma unroll
    for (int k = 0; k < kPermR; ++k) part[k] = 0.0;
    for (int s0 = 0; s0 < S; s0 += kPermT) {
        const int j = s0 + t;
        const bool has = j < S;
        const int a = has ? j : S - 1;  // a thread without a column reads a valid word and contributes +0.0
        const uint64_t lj = ld_lds(li8, (size_t)a);
        const double* wc = w + a;
        double col[kPermR];
#pragma unroll
        for (int k = 0; k < kPermR; ++k) col[k] = 0.0;
#pragma unroll 4
        for (int i = 0; i < S; ++i) {
#pragma clang fp contract(off)
            const double wij = ld_glb(wc, (size_t)i * S);
            const uint64_t x = ld_lds(li8, (size_t)i) ^ lj;  // byte k is 0 where the k-th labelling groups i with j
#pragma unroll
            for (int k = 0; k < kPermR; ++k) col[k] = col[k] + (((x >> (8 * k)) & 0xff) == 0 ? wij : 0.0);
        }
#pragma unroll
        for (int k = 0; k < kPermR; ++k) {
#pragma clang fp contract(off)
            tj[k][t] = has ? ld_glb(c, (size_t)((lj >> (8 * k)) & 0xff)) * col[k] : 0.0;
        }
        __syncthreads();
        if (wv == 0) {
#pragma unroll
            for (int k = 0; k < kPermR; ++k) {
#pragma unroll
                for (int q = 0; q < kPermT / 64; ++q) {
#pragma clang fp contract(off)
                    part[k] = part[k] + tj[k][q * 64 + lane];  // columns s0 + lane, + 64, + 128, + 192: ascending j
                }
            }
        }
        __syncthreads();  // tj is rewritten by the next slab
    }
    if (wv == 0) {
#pragma unroll
        for (int k = 0; k < kPermR; ++k) {
            const double v = perm_wave_sum(part[k]);
            if (lane == 0 && k < nr) st_glb(out, (size_t)(b0 + k), v);
        }
    }
}

}  // namespace tda
