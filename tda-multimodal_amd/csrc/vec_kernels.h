// vec_kernels.h -- persistence landscapes and persistence images on gfx950
// (include/tda_dgm.h has the definitions, the promises and the bound C(n)).
//
// k_pl_tents<PER>: one workgroup (4 waves) per (diagram, tile of kPlTile grid
// values), the diagram's finite points in LDS as (b, d) rows.  A wave takes one
// grid value t at a time: lane l evaluates the tents of the points l, l + 64, ...
// (PER of them, the size class's n / 64) into registers as bit patterns -- a tent
// is a non-negative double, +0.0 for "no tent", so the patterns order like the
// values -- and the k-th largest needs no sort:
//     round: m = the largest pattern strictly below the previous round's (a wave
//            max), c = how many tents attain it (a wave sum); lanes pos .. pos + c - 1
//            take m as their lambda, pos += c;
// until pos >= K or m == 0 (only zeros are left: the lanes keep their +0.0).  K <=
// 64, so lane k - 1 holds lambda_k and stores it.  Every round emits at least one
// value: at most K rounds.  Ties and K > n need nothing special, and the value
// is one of the tents, whatever the launch shape.
//
// k_pi_image: one workgroup per (diagram, 32 x 32 pixel tile), 2 x 2 pixels per
// thread.  The points are taken in chunks of kPiChunk in row order; per chunk the
// workgroup fills two LDS tables erf((edge - c) r), one erf per (point, edge of
// the tile) and axis, and each thread then adds, point by point,
//     acc[i][j] = fma(w_p gx_p[i], gy_p[j], acc[i][j]),  g = (e[k + 1] - e[k]) / 2.
// A pixel's sum therefore runs over p in row order with one rounding per term,
// and its operands depend on the point and the pixel's two edges alone: neither
// the tile, the chunk nor the other diagrams enter the bits.  The accumulation
// is a plain FMA loop, not an MFMA (DESIGN.md says why).
#pragma once
#include "bn_kernels.h"  // bn_d2
#include "rips_device.h"

namespace tda {

constexpr int kVecMaxN = 4096;  // TDA_VEC_MAX_POINTS
constexpr int kPlMaxK = 64;     // TDA_PL_MAX_DEPTH: one lane per depth
constexpr int kPlThreads = 256;
constexpr int kPlWaves = kPlThreads / 64;
constexpr int kPlTile = 16;  // grid values per workgroup

// dynamic LDS of a k_pl_tents workgroup whose diagram has n points
__host__ __device__ constexpr size_t pl_lds_bytes(int n) { return (size_t)(n > 0 ? n : 1) * 16; }

template <int PER>
__global__ __launch_bounds__(kPlThreads) void k_pl_tents(const double* __restrict__ pts, const int64_t* __restrict__ off,
                                                         const int32_t* __restrict__ order, const double* __restrict__ grid, int G, int K,
                                                         double* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char pl_smem[];
    bn_d2* sp = (bn_d2*)pl_smem;
    const int s = order[blockIdx.x];
    const int64_t o = off[s];
    const int n = (int)(off[s + 1] - o);  // <= 64 PER (the class) and <= the launch's LDS rows
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int i = t; i < n; i += kPlThreads) ((TDA_LDS bn_d2*)sp)[i] = ((const TDA_GLB bn_d2*)pts)[o + i];
    __syncthreads();
    const int g0 = blockIdx.y * kPlTile;
    for (int gi = wave; gi < kPlTile; gi += kPlWaves) {
        const int g = g0 + gi;
        if (g >= G) break;  // uniform over the wave
        const double tv = grid[g];
        uint64_t f[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int p = j * 64 + lane;
            double v = 0.0;
            if (p < n) {
                const bn_d2 q = bn_pt(sp, p);
                const double m = fmin(tv - q.x, q.y - tv);
                v = m > 0.0 ? m : 0.0;  // +0.0, never -0.0
            }
            f[j] = (uint64_t)__double_as_longlong(v);
        }
        uint64_t prev = ~0ull;  // above every pattern
        double val = 0.0;
        int pos = 0;
        while (pos < K) {  // at most K rounds: each emits at least one value
            uint64_t m = 0;
#pragma unroll
            for (int j = 0; j < PER; ++j)
                if (f[j] < prev && f[j] > m) m = f[j];
            m = wave_max_u64(m);
            if (m == 0) break;  // zeros only from here on
            uint64_t c = 0;
#pragma unroll
            for (int j = 0; j < PER; ++j) c += f[j] == m ? 1u : 0u;
            const int cnt = (int)wave_sum_u64(c);
            if (lane >= pos && lane < pos + cnt) val = __longlong_as_double((long long)m);
            pos += cnt;
            prev = m;
        }
        if (lane < K) st_glb(out, ((size_t)s * K + lane) * (size_t)G + g, val);
    }
}

constexpr int kPiTile = 32;   // pixels per axis of a workgroup's tile
constexpr int kPiChunk = 32;  // points per pass over the tables
constexpr int kPiThreads = 256;
constexpr int kPiMaxPixels = 256;  // TDA_PI_MAX_PIXELS

__global__ __launch_bounds__(kPiThreads) void k_pi_image(const double* __restrict__ pts, const double* __restrict__ wgt,
                                                         const int64_t* __restrict__ off, const double* __restrict__ xe,
                                                         const double* __restrict__ ye, int W, int H, double r, double* __restrict__ out) {
    __shared__ double ex[kPiChunk][kPiTile + 1], ey[kPiChunk][kPiTile + 1], sw[kPiChunk];
    const int s = blockIdx.x;
    const int tiles_j = (H + kPiTile - 1) / kPiTile;
    const int i0 = ((int)blockIdx.y / tiles_j) * kPiTile, j0 = ((int)blockIdx.y % tiles_j) * kPiTile;
    const int ni = min(kPiTile, W - i0), nj = min(kPiTile, H - j0);  // the tile's pixels: edges 0 .. ni, 0 .. nj
    const int t = threadIdx.x;
    const int li = (t >> 4) * 2, lj = (t & 15) * 2;  // this thread's 2 x 2 pixels within the tile
    double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0;
    const int64_t o = off[s];
    const int n = (int)(off[s + 1] - o);
    constexpr int kTab = kPiChunk * (kPiTile + 1);
    for (int c0 = 0; c0 < n; c0 += kPiChunk) {
        const int pc = min(kPiChunk, n - c0);
        __syncthreads();  // the previous chunk's tables have been read
        for (int e = t; e < 2 * kTab; e += kPiThreads) {
            const int axis = e >= kTab ? 1 : 0;
            const int rem = e - axis * kTab;
            const int p = rem / (kPiTile + 1), k = rem - p * (kPiTile + 1);
            double v = 0.0;  // beyond the chunk or the tile: a pixel of zero mass
            if (p < pc && k <= (axis ? nj : ni)) {
                const double edge = axis ? ye[j0 + k] : xe[i0 + k];
                const double c = pts[2 * (o + c0 + p) + axis];  // b, or pi
                v = erf((edge - c) * r);
            }
            (axis ? ey : ex)[p][k] = v;
        }
        if (t < kPiChunk) sw[t] = t < pc ? wgt[o + c0 + t] : 0.0;
        __syncthreads();
        for (int p = 0; p < pc; ++p) {
            const double w = sw[p];
            const double x0 = ex[p][li], x1 = ex[p][li + 1], x2 = ex[p][li + 2];
            const double y0 = ey[p][lj], y1 = ey[p][lj + 1], y2 = ey[p][lj + 2];
            const double wx0 = w * (0.5 * (x1 - x0)), wx1 = w * (0.5 * (x2 - x1));
            const double gy0 = 0.5 * (y1 - y0), gy1 = 0.5 * (y2 - y1);
            a00 = fma(wx0, gy0, a00);
            a01 = fma(wx0, gy1, a01);
            a10 = fma(wx1, gy0, a10);
            a11 = fma(wx1, gy1, a11);
        }
    }
    const int i = i0 + li, j = j0 + lj;
    double* o_s = out + (size_t)s * W * H;
    if (i < W && j < H) st_glb(o_s, (size_t)i * H + j, a00);
    if (i < W && j + 1 < H) st_glb(o_s, (size_t)i * H + j + 1, a01);
    if (i + 1 < W && j < H) st_glb(o_s, (size_t)(i + 1) * H + j, a10);
    if (i + 1 < W && j + 1 < H) st_glb(o_s, (size_t)(i + 1) * H + j + 1, a11);
}

}  // namespace tda
