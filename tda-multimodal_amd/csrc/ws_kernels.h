// ws_kernels.h -- 1-Wasserstein distance between persistence diagrams on gfx950
// (include/tda_dgm.h has the definition and what is promised about the value).
//
// k_ws_pairs: one workgroup per pair.  The host has dropped the non-finite
// points and oriented the pair (dgm_plan.h dgm_orient): the first diagram is the
// longer one.  Both diagrams are copied into LDS once as (b, d) rows.  Costs are
// never stored: c(p, q) = sqrt(db db + dd dd) and c(p) = (d - b) / sqrt(2) are
// recomputed where they are needed, each the same sequence of individually
// rounded operations (no fused multiply-add), so the same bits everywhere.
//
// The assignment problem, in its reduced form.  The columns are the points of
// the first diagram (nc of them, thread j owns column j), the rows those of the
// second (nr <= nc).  Every row is assigned: to a column at c(p, q), or to a
// diagonal slot of its own at c(q).  A column that stays free pays c(p); that is
// its starting dual v_j = c(p_j), after which a free column costs nothing more
// (the rectangular problem with the costs c(p, q) - c(p)).  A row's diagonal
// slot can be reached from that row alone and its dual stays 0, so it is never a
// column of the search: it is a second way for a scanned row to end the path.
//
// Successive shortest augmenting paths with dual potentials (Hungarian in the
// Jonker-Volgenant form), one row added at a time.  Per added row r a Dijkstra
// scan over the columns, every thread following the same control flow:
//   - thread j keeps column j's tentative distance d_j, its dual v_j and whether
//     the column is scanned in registers, and its predecessor row in LDS;
//   - a step scans one row i0 at distance D (the root at 0): its diagonal slot is
//     a candidate end at D + (c(q_i0) - u_i0), and every unscanned column is
//     relaxed with D + ((c(p_j, q_i0) - u_i0) - v_j);
//   - one block-wide min-with-index over the unscanned columns: the distances as
//     order-preserving 64-bit keys, a DPP wave reduction, the lowest lane of the
//     minimum by ballot, one (key, index) slot per wave in LDS (two sets of slots
//     used in turn, so one barrier per step), lowest index on ties;
//   - the path ends at the best diagonal candidate if that is <= the minimum (or
//     no column is left), else the minimum's column is scanned: a free column
//     ends the path, a matched one hands its row to the next step;
//   - the duals of the scanned rows and columns move by (end distance - own
//     distance), each by the thread of its column; thread 0 flips the path.
// No atomics.
//
// Every loop is bounded before it starts: nr rows added, at most nc + 1 steps
// per row (each step but the last scans a column not scanned before),
// min(nc, nr) + 1 edges flipped per path.  Running into a bound writes NaN for
// the pair (the host reports it); it cannot happen unless the matching state is
// corrupt.
//
// The value written is the sum of the costs of the matching found, recomputed
// from the points and added by one thread in a fixed order: the columns in
// increasing j (c(p_j, q) if matched, else c(p_j)), then the rows in increasing i
// (c(q_i) if at the diagonal, else +0).  It is not an expression in the duals.
// The workgroup size does not enter it: the scan's choices depend on the
// distances and the column indices alone.
#pragma once
#include "rips_device.h"

namespace tda {

constexpr int kWsMaxN = 512;               // finite points per diagram (TDA_WS_MAX_POINTS)
constexpr int kWsMaxWaves = kWsMaxN / 64;  // the largest workgroup is kWsMaxN threads
constexpr int kWsFree = -1, kWsDiag = -2;  // a row's mate: not assigned yet; its diagonal slot

// dynamic LDS of a workgroup whose pair has nc and nr points (monotone in both): the points, the
// columns' cost terms, the rows' duals, predecessor and mate of the columns, mate of the rows, and the
// fixed part (two sets of per-wave (key, index) slots, the flag): 32 nc + 28 nr + 200
__host__ __device__ constexpr size_t ws_lds_bytes(int nc, int nr) {
    return (size_t)(nc + nr) * 16 + (size_t)nc * 8 + (size_t)nr * 8 + 2 * kWsMaxWaves * 8 + (size_t)2 * nc * 4 + (size_t)nr * 4 +
           (2 * kWsMaxWaves + 2) * 4;
}

typedef double ws_d2 __attribute__((ext_vector_type(2)));  // (b, d): a native vector, so that address-space casts apply

// the two costs: individually rounded operations in the header's order, never contracted
__device__ __forceinline__ double ws_cross(ws_d2 p, ws_d2 q) {
#pragma clang fp contract(off)
    const double db = p.x - q.x, dd = p.y - q.y;
    const double bb = db * db, d2 = dd * dd;
    return __builtin_sqrt(bb + d2);
}
__device__ __forceinline__ double ws_diag(ws_d2 p) {
#pragma clang fp contract(off)
    const double pers = p.y - p.x;
    return pers * 0.70710678118654752440;
}
__device__ __forceinline__ ws_d2 ws_pt(const ws_d2* p, int i) { return ((const TDA_LDS ws_d2*)p)[i]; }

// doubles as 64-bit keys that order like the values (-0 below +0); no key of a number is ~0
__device__ __forceinline__ uint64_t ws_key(double x) {
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ double ws_unkey(uint64_t k) {
    return __longlong_as_double((long long)((k >> 63) ? k & 0x7fffffffffffffffull : ~k));
}

// pts (total, 2): the finite points of all diagrams; off [S + 1]: their row boundaries; pairs (P, 2),
// oriented; order [gridDim.x]: the pairs of this launch (one size class); dist [P]: out.  match, if
// not NULL: out, from moff[pair] on one entry per point of the pair's first diagram, the index of its
// partner in the second or -1.  blockDim.x is a multiple of 64, at least max(n1, n2), at most kWsMaxN.
__global__ __launch_bounds__(kWsMaxN) void k_ws_pairs(const double* __restrict__ pts, const int64_t* __restrict__ off,
                                                      const int32_t* __restrict__ pairs, const int32_t* __restrict__ order,
                                                      double* __restrict__ dist, const int64_t* __restrict__ moff,
                                                      int32_t* __restrict__ match) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, T = blockDim.x, nwaves = T >> 6, wave = tid >> 6, lane = tid & 63;
    const int pr = order[blockIdx.x];
    const int64_t c0 = off[pairs[2 * pr]], r0 = off[pairs[2 * pr + 1]];
    const int nc = (int)(off[pairs[2 * pr] + 1] - c0), nr = (int)(off[pairs[2 * pr + 1] + 1] - r0);
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    if (nc > T || nr > T || T > kWsMaxN) {  // the host refuses such a pair before any launch
        if (tid == 0) dist[pr] = nan;
        return;
    }
    ws_d2* pc = (ws_d2*)smem;
    ws_d2* pw = pc + nc;
    double* term = (double*)(pw + nr);                    // [nc] the columns' cost terms (the final sum)
    double* u = term + nc;                                // [nr] the rows' duals; their cost terms at the end
    uint64_t* red = (uint64_t*)(u + nr);                  // [2][kWsMaxWaves] per-wave minimum keys
    int32_t* way = (int32_t*)(red + 2 * kWsMaxWaves);     // [nc] the row a column was reached from
    int32_t* mate_c = way + nc;                           // [nc] the row assigned to a column, or -1
    int32_t* mate_r = mate_c + nc;                        // [nr] the column of a row, kWsFree or kWsDiag
    int32_t* slot = mate_r + nr;                          // [2][kWsMaxWaves] per-wave index of the minimum
    int32_t* flag = slot + 2 * kWsMaxWaves;               // [1] a flip ran into its bound
    const ws_d2* g = (const ws_d2*)pts;  // rows of two doubles: 16-byte aligned with the buffer
    const bool col = tid < nc;
    if (col) {
        st_lds(pc, tid, g[c0 + tid]);
        st_lds(mate_c, tid, (int32_t)-1);
    }
    if (tid < nr) {
        st_lds(pw, tid, g[r0 + tid]);
        st_lds(u, tid, 0.0);
        st_lds(mate_r, tid, (int32_t)kWsFree);
    }
    if (tid == 0) st_lds(flag, 0, 0);
    __syncthreads();
    const ws_d2 mine = col ? ws_pt(pc, tid) : ws_d2{0.0, 0.0};
    double v = ws_diag(mine);  // a free column pays its diagonal cost

    const int depth = min(nc, nr) + 1;
    int set = 0;
    bool bad = false;
    for (int r = 0; r < nr; ++r) {
        double d = inf;     // column tid's tentative distance
        bool used = false;  // column tid is scanned
        int i0 = r, best_row = -1, end = kWsDiag;  // end: the free column that ends the path, kWsFree for a diagonal slot
        double D = 0.0, best = inf, delta = 0.0;
        for (int step = 0; step <= nc; ++step) {
            const ws_d2 q = ws_pt(pw, i0);
            const double ui = ld_lds(u, i0);
            const double cd = D + (ws_diag(q) - ui);
            if (cd < best) {
                best = cd;
                best_row = i0;
            }
            if (col && !used) {
                const double nd = D + ((ws_cross(mine, q) - ui) - v);
                if (nd < d) {
                    d = nd;
                    st_lds(way, tid, (int32_t)i0);
                }
            }
            const uint64_t key = col && !used ? ws_key(d) : ~0ull;
            const uint64_t wmin = wave_min_u64(key);
            const uint64_t at = __ballot(key == wmin);
            if (lane == 0) {
                st_lds(red, set * kWsMaxWaves + wave, wmin);
                st_lds(slot, set * kWsMaxWaves + wave, (int32_t)((wave << 6) + __builtin_ctzll(at)));
            }
            __syncthreads();
            uint64_t gmin = ~0ull;
            int js = -1;
            for (int w = 0; w < nwaves; ++w) {
                const uint64_t k = ld_lds(red, set * kWsMaxWaves + w);
                if (k < gmin) {
                    gmin = k;
                    js = ld_lds(slot, set * kWsMaxWaves + w);
                }
            }
            set ^= 1;  // the other set next: this one is read until the next barrier
            const double gd = ws_unkey(gmin);
            if (js < 0 || !(gd < best)) {  // no column left, or the diagonal is no worse
                end = kWsFree;
                delta = best;
                break;
            }
            if (tid == js) used = true;
            const int m = ld_lds(mate_c, js);
            if (m < 0) {
                end = js;
                delta = gd;
                break;
            }
            i0 = m;
            D = gd;
        }
        if (end == kWsDiag || (end == kWsFree && best_row < 0)) {
            bad = true;
            break;
        }
        // the duals: every scanned column and its row by the column's thread, the root by thread 0
        if (used) {
            const double s = delta - d;
            v -= s;
            const int m = ld_lds(mate_c, tid);
            if (m >= 0) st_lds(u, m, ld_lds(u, m) + s);
        }
        if (tid == 0) st_lds(u, r, ld_lds(u, r) + delta);
        __syncthreads();
        if (tid == 0) {
            int j = end;
            if (end == kWsFree) {  // best_row moves to its diagonal slot and gives up its column (the root has none)
                j = ld_lds(mate_r, best_row);
                st_lds(mate_r, best_row, (int32_t)kWsDiag);
            }
            for (int k = 0; k < depth && j >= 0; ++k) {
                const int i = ld_lds(way, j), jn = ld_lds(mate_r, i);
                st_lds(mate_c, j, (int32_t)i);
                st_lds(mate_r, i, (int32_t)j);
                j = i == r ? -1 : jn;
            }
            if (j >= 0) st_lds(flag, 0, 1);
        }
        __syncthreads();
        if (ld_lds(flag, 0)) {
            bad = true;
            break;
        }
    }
    if (bad) {
        if (tid == 0) dist[pr] = nan;
        return;
    }

    // the costs of the matching found, from the points; thread 0 adds them in their fixed order
    if (col) {
        const int m = ld_lds(mate_c, tid);
        st_lds(term, tid, m >= 0 ? ws_cross(mine, ws_pt(pw, m)) : ws_diag(mine));
        if (match) match[moff[pr] + tid] = m;
    }
    if (tid < nr) st_lds(u, tid, ld_lds(mate_r, tid) == kWsDiag ? ws_diag(ws_pt(pw, tid)) : 0.0);
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int j = 0; j < nc; ++j) sum += ld_lds(term, j);
        for (int i = 0; i < nr; ++i) sum += ld_lds(u, i);
        dist[pr] = sum;
    }
}

}  // namespace tda
