// geo_kernels.h -- geodesic distances over the neighbourhood graph on gfx950 (include/tda_rips.h
// tda_geodesic pins the definition): the graph W in place on a layer's f32 matrix dm, then its
// min-plus closure G in place on W.
//
// The graph.  k_geo_select gives every row its k-th smallest key (ord(dm[i][j]) << 32 | j over
// j != i, sh0_ord's order): a workgroup per row stages the row's ordered bits in LDS and builds the
// key from its highest bit down, one count of the row per bit (the smallest t with at least k keys
// <= t; the keys of a row are distinct, so t is the k-th key itself).  Bits 13 .. 31 of a key are
// zero (j < 8192) and are skipped: 45 counts, whatever the row holds.  k_geo_graph then keeps
// dm[i][j] where key(i, j) <= t_i or key(j, i) <= t_j (dm is symmetric bit for bit, so key(j, i) is
// formed from dm[i][j]: the pass reads and writes its own element only), or where dm[i][j] <= radius,
// writes +inf elsewhere and 0 on the diagonal, and counts the kept pairs i < j.
//
// The closure, two schedules chosen by the plan (geo_plan.h):
//   resident, N <= kGeoLdsN: one workgroup per layer, the matrix in 64 KiB of static LDS (rows padded
//     to a multiple of 4 with +inf), the ascending-k loop with one barrier per k.  A thread owns one
//     group of four columns and every (256 / groups)-th row: the row operand G[k][c .. c+3] is one
//     ds_read_b128 per step, the column operand G[i][k] one ds_read_b32 per row.  Step k leaves row k
//     and column k as they are (G[k][k] is 0, or +inf in the pad), so the loop runs in place.
//   blocked, above: 64 x 64 tiles over the matrix where it lies (stride N; a tile reads +inf and
//     stores nothing beyond N, and inf + x and min need no special case: no -inf or NaN can arise
//     from non-negative input).  Round t: k_geo_diag closes tile (t, t) with the loop above; then
//     k_geo_product<false> forms every tile (t, j), j != t, as min(old, closed (x) old), a min-plus
//     product; then k_geo_product<true> every tile (i, j), i <= j, both != t, as
//     min(old, (t, i)^T (x) (t, j)).  Both products read ROW tiles of round t only, so both operands
//     are read wide along rows, and write the mirror tile (j, t) or (j, i) from the same registers:
//     the bitwise symmetry holds by construction (a diagonal tile (i, i) is symmetric because min is
//     exact and its two sums are the same operands).  A thread holds a 4 x 4 sub-tile in registers.
// No loop's trip count and no address depends on a value of dm.
// Nothing here has been tuned beyond this layout (what is measured).
#pragma once
#include "sh0_kernels.h"

namespace tda {

constexpr int kGeoT = 256;       // threads of a workgroup, every kernel
constexpr int kGeoLdsN = 128;    // the resident closure's largest N: kGeoLdsN^2 * 4 = 64 KiB
constexpr int kGeoTile = 64;     // the side of a tile of the blocked closure
constexpr int kGeoMaxN = 8192;   // the longest row k_geo_select stages (32 KiB of ordered bits)
constexpr int kGeoIdxBits = 13;  // a column index fits these bits of a key's low word
static_assert(kGeoMaxN == 1 << kGeoIdxBits && kGeoT == 4 * kGeoTile && kGeoTile % 4 == 0 && kGeoLdsN % 4 == 0, "geo_kernels.h: layout");

__device__ __forceinline__ float geo_inf() { return __uint_as_float(0x7F800000u); }

// thr[l][i] = the k-th smallest key of row i (1 <= k <= n - 1, n >= 2).  grid (n, layers).
__global__ __launch_bounds__(kGeoT) void k_geo_select(const float* __restrict__ dm, int n, int k, uint64_t* __restrict__ thr) {
    __shared__ uint32_t ord[kGeoMaxN];
    __shared__ int part[2][kGeoT / 64];
    const int i = blockIdx.x, l = blockIdx.y, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const float* row = dm + ((size_t)l * n + i) * n;
    for (int j = t; j < n; j += kGeoT) ord[j] = sh0_ord(row[j]);
    __syncthreads();
    uint64_t pre = 0;
    int set = 0;
    for (int bit = 63; bit >= 0; --bit) {
        if (bit == 31) bit = kGeoIdxBits - 1;  // bits 13 .. 31 are zero in every key
        const uint64_t cand = pre | ((1ull << bit) - 1);
        const uint32_t hi = (uint32_t)(cand >> 32), lo = (uint32_t)cand;
        int c = 0;
        for (int j = t; j < n; j += kGeoT) {
            const uint32_t o = ord[j];
            c += (j != i) & ((o < hi) | ((o == hi) & ((uint32_t)j <= lo)));
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) c += __shfl_xor(c, s, 64);
        if (lane == 0) part[set][wv] = c;
        __syncthreads();  // the one barrier of a count: set `set` is written again two barriers from here
        c = part[set][0] + part[set][1] + part[set][2] + part[set][3];
        set ^= 1;
        if (c < k) pre |= 1ull << bit;
    }
    if (t == 0) thr[(size_t)l * n + i] = pre;
}

// W over dm: thr (kNN) or NULL (radius).  n_edges[l] += the kept pairs i < j.  grid (<= 1024, layers).
__global__ __launch_bounds__(kGeoT) void k_geo_graph(float* __restrict__ dm, int n, const uint64_t* __restrict__ thr, double radius,
                                                     unsigned long long* __restrict__ n_edges) {
    const int l = blockIdx.y;
    float* Dl = dm + (size_t)l * n * n;
    const uint64_t* tl = thr ? thr + (size_t)l * n : nullptr;
    unsigned cnt = 0;
    for (size_t e = (size_t)blockIdx.x * kGeoT + threadIdx.x; e < (size_t)n * n; e += (size_t)gridDim.x * kGeoT) {
        const int i = (int)(e / n), j = (int)(e % n);
        if (i == j) {
            Dl[e] = 0.0f;
            continue;
        }
        const float v = Dl[e];
        bool keep;
        if (tl) {
            const uint64_t o = (uint64_t)sh0_ord(v) << 32;
            keep = (o | (uint32_t)j) <= tl[i] || (o | (uint32_t)i) <= tl[j];
        } else {
            keep = (double)v <= radius;
        }
        if (!keep) Dl[e] = geo_inf();
        cnt += keep && i < j;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) cnt += __shfl_xor(cnt, s, 64);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(n_edges + l, (unsigned long long)cnt);
}

// The ascending-k loop on an n x n matrix in LDS, rows ld floats apart (ld a multiple of 4, ld <= 128,
// columns n .. ld-1 hold +inf).  Every thread of the workgroup calls it; it ends with a barrier.
__device__ __forceinline__ void geo_close_lds(float* S, int n, int ld) {
    const int ld4 = ld >> 2, t = threadIdx.x, c = t % ld4, r0 = t / ld4, rstep = kGeoT / ld4;
    float4* S4 = reinterpret_cast<float4*>(S);
    for (int k = 0; k < n; ++k) {
        if (r0 < rstep) {  // the threads past the last whole row of groups have no share
            const float4 b = S4[k * ld4 + c];
            for (int i = r0; i < n; i += rstep) {
                const float a = S[i * ld + k];
                float4 v = S4[i * ld4 + c];
                v.x = fminf(v.x, a + b.x), v.y = fminf(v.y, a + b.y), v.z = fminf(v.z, a + b.z), v.w = fminf(v.w, a + b.w);
                S4[i * ld4 + c] = v;
            }
        }
        __syncthreads();
    }
}

// the resident closure: grid (layers), n <= kGeoLdsN
__global__ __launch_bounds__(kGeoT) void k_geo_resident(float* __restrict__ dm, int n) {
    __shared__ __align__(16) float S[kGeoLdsN * kGeoLdsN];
    float* Dl = dm + (size_t)blockIdx.x * n * n;
    const int ld = (n + 3) & ~3;
    for (int e = threadIdx.x; e < n * ld; e += kGeoT) {
        const int i = e / ld, j = e % ld;
        S[e] = j < n ? Dl[i * n + j] : geo_inf();
    }
    __syncthreads();
    geo_close_lds(S, n, ld);
    for (int e = threadIdx.x; e < n * ld; e += kGeoT) {
        const int i = e / ld, j = e % ld;
        if (j < n) Dl[i * n + j] = S[e];
    }
}

// tile (ti, tj) of a layer's matrix into LDS, row-major, +inf beyond n
__device__ __forceinline__ void geo_load_tile(float* S, const float* __restrict__ Dl, int n, int ti, int tj) {
    for (int e = threadIdx.x; e < kGeoTile * kGeoTile; e += kGeoT) {
        const int i = ti * kGeoTile + e / kGeoTile, j = tj * kGeoTile + e % kGeoTile;
        S[e] = (i < n && j < n) ? Dl[(size_t)i * n + j] : geo_inf();
    }
}

// blocked, phase 1: tile (kb, kb) closed in LDS.  grid (layers).
__global__ __launch_bounds__(kGeoT) void k_geo_diag(float* __restrict__ dm, int n, int kb) {
    __shared__ __align__(16) float S[kGeoTile * kGeoTile];
    float* Dl = dm + (size_t)blockIdx.x * n * n;
    geo_load_tile(S, Dl, n, kb, kb);
    __syncthreads();
    geo_close_lds(S, kGeoTile, kGeoTile);
    for (int e = threadIdx.x; e < kGeoTile * kGeoTile; e += kGeoT) {
        const int i = kb * kGeoTile + e / kGeoTile, j = kb * kGeoTile + e % kGeoTile;
        if (i < n && j < n) Dl[(size_t)i * n + j] = S[e];
    }
}

// blocked, phases 2 and 3: C(ti, tj) = min(C, A^T (x) B), A = tile (kb, ti), B = tile (kb, tj), and the
// mirror tile (tj, ti) from the same registers.  With a, b numbering the nt - 1 tiles other than kb:
// kRest false (phase 2): grid (nt - 1, 1, layers), ti = kb (A is the closed diagonal tile, B is C's old value);
// kRest true (phase 3): grid (nt - 1, nt - 1, layers), the blocks a > b leave at once.
template <bool kRest>
__global__ __launch_bounds__(kGeoT) void k_geo_product(float* __restrict__ dm, int n, int kb) {
    __shared__ __align__(16) float A[kGeoTile * kGeoTile], B[kGeoTile * kGeoTile];
    if (kRest && blockIdx.y > blockIdx.x) return;  // the whole workgroup: the upper triangle only
    const int tj = (int)blockIdx.x + ((int)blockIdx.x >= kb), ti = kRest ? (int)blockIdx.y + ((int)blockIdx.y >= kb) : kb;
    float* Dl = dm + (size_t)blockIdx.z * n * n;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int i0 = ti * kGeoTile + ty * 4, j0 = tj * kGeoTile + tx * 4;
    float C[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) C[r][c] = (i0 + r < n && j0 + c < n) ? Dl[(size_t)(i0 + r) * n + j0 + c] : geo_inf();
    geo_load_tile(A, Dl, n, kb, ti);
    geo_load_tile(B, Dl, n, kb, tj);
    __syncthreads();  // every read of the tiles is done before any thread stores (phase 2 stores over B's source)
    const float4* A4 = reinterpret_cast<const float4*>(A);
    const float4* B4 = reinterpret_cast<const float4*>(B);
#pragma unroll 4
    for (int k = 0; k < kGeoTile; ++k) {
        const float4 av = A4[k * (kGeoTile / 4) + ty], bv = B4[k * (kGeoTile / 4) + tx];
        const float a[4] = {av.x, av.y, av.z, av.w}, b[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) C[r][c] = fminf(C[r][c], a[r] + b[c]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (i0 + r < n && j0 + c < n) {
                Dl[(size_t)(i0 + r) * n + j0 + c] = C[r][c];
                if (ti != tj) Dl[(size_t)(j0 + c) * n + i0 + r] = C[r][c];
            }
}

// n_comp[l] += the rows i with no finite G[i][j], j < i: a wave per row.  grid (ceil(n / 4), layers).
__global__ __launch_bounds__(kGeoT) void k_geo_components(const float* __restrict__ G, int n, int* __restrict__ n_comp) {
    const int l = blockIdx.y, lane = threadIdx.x & 63, i = blockIdx.x * (kGeoT / 64) + (threadIdx.x >> 6);
    if (i >= n) return;  // the whole wave
    const float* row = G + ((size_t)l * n + i) * n;
    bool any = false;
    for (int j = lane; j < i; j += 64) any |= row[j] < geo_inf();
    if (__ballot(any) == 0 && lane == 0) atomicAdd(n_comp + l, 1);
}

}  // namespace tda
