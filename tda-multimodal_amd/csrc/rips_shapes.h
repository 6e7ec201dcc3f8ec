// rips_shapes.h -- what the host plan of a persistence call (rips_plan.h) and the kernels both
// need: the structs whose size the plan carves the device workspace by, the binomials, and the
// limits that decide which kernel runs and how much LDS it gets.  Plain C++, no HIP: the kernel
// headers include it, and so does tests/rips_plan_main.cpp with a host compiler alone.  Each
// block names the kernel header that uses it and says what the value means there.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define TDA_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define TDA_HOST_DEVICE inline
#endif

namespace tda {

// ---------------------------------------------------------------- binomials (rips_device.h)
// C(n, k) for k <= 5 without 64-bit division: 32-bit exact-division steps
// (C(n,k) = C(n,k-1) * (n-k+1) / k, split so every quotient is exact) and one
// 32x32->64 multiply at the end.  Valid for n < 65536 (checked on the host).
TDA_HOST_DEVICE uint64_t binom(uint64_t n64, int k) {
    const uint32_t n = (uint32_t)n64;
    if (k == 0) return 1;
    if (n < (uint32_t)k) return 0;
    if (k == 1) return n;
    const uint32_t c2 = (n & 1) ? n * ((n - 1) >> 1) : (n >> 1) * (n - 1);  // < 2^31 for n < 65536
    if (k == 2) return c2;
    // C3 = c2 * (n-2) / 3, c2 = 3q + r
    const uint32_t q2 = c2 / 3u, r2 = c2 - 3u * q2;
    const uint64_t c3 = (uint64_t)q2 * (n - 2) + (r2 * (n - 2)) / 3u;
    if (k == 3) return c3;
    const uint64_t c4 = (c3 >> 2) * (n - 3) + ((uint32_t)(c3 & 3) * (n - 3)) / 4u;
    if (k == 4) return c4;
    const uint64_t q4 = c4 / 5u, r4 = c4 - 5u * q4;
    return q4 * (n - 4) + (r4 * (n - 4)) / 5u;
}

// ---------------------------------------------------------------- layout (rips_kernels.h)
struct Pair {
    float birth, death;
    int64_t birth_idx, death_idx;
};

struct LayerStats {  // zeroed every call; copied to the host result
    float thresh;
    int32_t err;  // bit flags, see ERR_*
    int64_t num_edges;
    int64_t count[4];      // emitted pairs per dim
    uint64_t checksum[4];  // sum of pair_hash over all pairs
    int64_t all_pairs[4];
    int64_t n_columns[4];
    int64_t n_residual[4];
    int64_t n_adds[4];     // column additions in the serial reduction
    int64_t nskip[4];      // residual columns cleared by the serial reduction (host: n_residual - nskip)
    uint64_t rmask[4];     // residual pivot map mask used by the dim's reducer (HBM map consumers)
    int64_t ntri;          // N <= 64: triangles <= thresh (k_prep_tables)
    int64_t n_clr2;        // sparse-cleared H2 pivot bitmap: words k_apparent<2> listed for the end-of-call clear
    uint64_t prof[5][8];   // -DTDA_PROFILE builds: cycle counters (per dim; [3]: k_h0_wave, [4]: k_prep_layer)
};

constexpr uint64_t kRCapMax = 1ull << 22;    // residual columns per layer and dim
constexpr uint64_t kPCapMax = 1ull << 16;    // emitted pairs per layer and dim (H>=1)
constexpr int kLdsMax = 160 * 1024;
constexpr int kSmallN = 64;                  // one-wave H0 + LDS-resident reduction up to here
constexpr int kAppLdsMaxN = 128;             // k_apparent stages the distance matrix in LDS up to here
constexpr int kBigMinN = 256;                // large-N reducer above this N (global mode)

// ---------------------------------------------------------------- distances (rips_kernels.h)
constexpr int64_t kDistMfmaMinD = 32;        // k_distance_mfma (FP64 MFMA Gram tiles) from this D up
#ifndef TDA_DM_KC  // build-time A/B knob (tools/): K chunk of k_distance_mfma
#define TDA_DM_KC 32
#endif
constexpr int kDmT = 64, kDmKC = TDA_DM_KC;  // k_distance_mfma: rows of a tile, K chunk
constexpr int kGlMaxNB = 9, kGlMaxN = 16 * kGlMaxNB;  // k_gram_layer: 16-row blocks / rows of a layer at most

// ---------------------------------------------------------------- H0 (rips_kernels.h)
struct BorCtl {
    unsigned long long nmst;  // forest edges found
    uint32_t done, pad;
};
constexpr int kH0WaveMaxN = 190;  // 4 n^2 B of LDS staging
constexpr int kH0BorWQ = 16;      // Borůvka path: one-wave elder rule with register labels up to N = 1024
constexpr int kBorHookLdsMax = 150 * 1024;  // k_bor_hook's dynamic LDS attribute

// ---------------------------------------------------------------- side metrics (rips_kernels.h)
constexpr int kSilT = 256;     // k_silhouette: points per pass (threads of a block)
constexpr int kSilMaxK = 32;   // k_silhouette: clusters of a label set at most
constexpr int kSilLdsMax = 128 * 1024;  // k_silhouette's dynamic LDS attribute
constexpr int kTnT = 1024;     // k_twonn: threads of a block
constexpr int kTnLdsMax = 8192 * 4;     // k_twonn's dynamic LDS attribute

// ---------------------------------------------------------------- one wave per layer (rips_reduce.h)
struct Reduce2Cfg {  // per-dim LDS carve, decided on the host
    uint32_t wcap, rmap_lds_cap;  // rmap_lds_cap = 0 -> global map
    int piv_lds;
};
struct ReduceAllCfg {
    Reduce2Cfg dim[3];
    uint64_t step_limit;  // pivots per column before giving up (exit guarantee)
    int dist_lds;
    uint32_t bytes;  // dynamic LDS of the launch
};

// ---------------------------------------------------------------- the dense path (rips_reduce_small.h)
constexpr int kDenseMaxN = 64;
constexpr int kChainMaxCols = 512;        // non-cleared H1 residual columns / stored R_j per layer
// k_h1_chain variants (template MODE)
constexpr int kChainGeneral = 0, kChainFast = 1, kChainTable = 2;
// bitmap words per lane supported by k_h1_chain instantiations (FAST / TABLE: up to 12)
constexpr int kChainKs[] = {1, 2, 3, 4, 6, 9, 12, 16, 21};
constexpr int kChainFastMaxK = 12;
constexpr uint32_t kP1LogCap = 1024;      // k_h2_phase1: entries of a wave's key log
constexpr int kP1MaxWaves = 2;            // k_h2_phase1: waves per block at most

// ---------------------------------------------------------------- the serial radix heap (rips_reduce_big.h)
constexpr int kNB = 33;        // radix buckets (f32 diameter bits)

// ---------------------------------------------------------------- the parallel reducer (rips_reduce_par.h)
struct ParCtl {  // zeroed by k_par_init
    unsigned long long next;     // next fresh item
    unsigned long long rq_head, rq_tail;
    unsigned long long bpool_used, rpool_used, rec_used;
    unsigned long long abort;
    unsigned long long err;      // first error code (diagnostics)
    unsigned long long total;    // items over all layers
    unsigned long long evictions;
    unsigned long long pad[6];
};
constexpr uint32_t kParDbgCap = 4096;
constexpr uint32_t kParP2Words = 12;       // -DTDA_PROF2 record: layer << 40 | column, wave, steps, 8 phase cycle sums, spare
constexpr int kParLv = 65;                 // radix levels over the whole 64-bit key (par_bucket): 0 .. 64
constexpr unsigned kParGrid = 512;           // k_reduce_par workgroups at most (pool sizing): two 72-KB-LDS workgroups per CU
// default: one per CU -- the longest column is the critical path and runs
// faster without a second workgroup on its CU (r02, tools/ab_pargrid.sh:
// grid144 10.5 -> 8.5 ms, torus1024 61 -> 58.5 ms at 256 vs 512)
constexpr unsigned kParGridDefault = 256;

}  // namespace tda
