/*
 * tda_rips.h -- C ABI of the MI355X (gfx950) Vietoris-Rips persistence engine.
 *
 * Drop-in boundary for the reference's hot path: the third-party call
 *     result = ripser(cloud_low_dim, maxdim=MAX_DIM); dgms = result['dgms']
 * at debug_tda_pipeline.py:109-110, analyze_tda_over_layers.py:76 and
 * experiments/adversarial_compositional_binding/analyze_adversarial_tda.py:100.
 * The reference binds ripser's C++ core through Cython (package `ripser`,
 * unpinned, README.md:28; not vendored in the reference) with two entry points,
 *     rips_dm(float* D, int N, int modulus, int dim_max, float threshold,
 *             int do_cocycles)                                   [upstream]
 *     rips_dm_sparse(int* I, int* J, float* V, int NEdges, int N, int modulus,
 *             int dim_max, float threshold, int do_cocycles)     [upstream]
 * returning {births_and_deaths_by_dim, cocycles_by_dim, num_edges}.
 * `tda_rips_dm` below replaces `rips_dm` one-for-one (same argument meaning:
 * D is the condensed strict-upper-triangle distance vector in row-major (i<j)
 * order, exactly what ripser.py passes after `dm[I > J]`).  `tda_rips_batch`
 * is the layer-loop entry (point clouds in, distance + persistence on the
 * GPU) that the reference's per-layer loop (debug_tda_pipeline.py:92-150)
 * calls once per sweep instead of once per layer.
 *
 * Conventions
 *  - All functions return 0 on success or a negative TDA_E* code; the message
 *    is kept in thread-local storage and returned by tda_last_error().
 *  - Inputs are never owned by the library.  Results are library-owned until
 *    tda_rips_free().
 *  - coeff/modulus must be 2 (the reference never overrides ripser's default);
 *    other values return TDA_E_UNSUPPORTED.  do_cocycles != 0 likewise.
 *  - No torch types cross this boundary: plain pointers and sizes.
 */
#ifndef TDA_RIPS_H
#define TDA_RIPS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TDA_RIPS_ABI_VERSION 8

/* error codes */
#define TDA_OK 0
#define TDA_E_INVALID (-1)      /* bad shape / argument / non-finite input   */
#define TDA_E_UNSUPPORTED (-2)  /* coeff != 2, cocycles, maxdim > 2, ...     */
#define TDA_E_HIP (-3)          /* HIP runtime error (message has details)   */
#define TDA_E_CAPACITY (-4)     /* a device work buffer overflowed           */
#define TDA_E_NODEVICE (-5)     /* no gfx950 device visible                  */

/* dtype of the point-cloud input */
#define TDA_F32 0
#define TDA_F64 1

/* arguments of one batched call: L layers of N points in R^D */
typedef struct tda_rips_args {
    const void *x;      /* (L, N, D) row-major points, or (L, N, N) distances   */
    int32_t dtype;      /* TDA_F32 | TDA_F64                                    */
    int32_t x_on_device;/* 1: x is a device pointer on `device`; 0: host memory */
    int64_t L, N, D;    /* D ignored when is_dist                               */
    int32_t is_dist;    /* 1: x holds (L, N, N) distance matrices (upper used)  */
    int32_t maxdim;     /* 0, 1 or 2                                            */
    float thresh;       /* +inf -> enclosing radius (ripser.py default)         */
    int32_t modulus;    /* must be 2                                            */
    int32_t device;     /* HIP device ordinal                                   */
    void *stream;       /* device input (x_on_device) is read after the work queued
                           on this hipStream_t so far; NULL = the null (legacy
                           default) stream, which is torch's default stream.  ABI 7:
                           before, NULL meant no ordering.  A handle that is not a
                           stream of the library's HIP runtime on `device` is
                           refused (TDA_E_HIP).  Ignored with TDA_FLAG_INPUT_READY
                           and for host input.                                   */
    int32_t want_dist;  /* 1: also return the (L, N, N) f32 distance matrices   */
    int32_t flags;      /* TDA_FLAG_* bits (0 = none)                           */
    /* optional silhouette scores on the same distance matrices (ABI >= 2):
     * sklearn.metrics.silhouette_score(cloud, labels), called by the reference
     * beside ripser at debug_tda_pipeline.py:117-118 (shape / color labels) and
     * analyze_adversarial_tda.py:108-111.  `labels` is host memory [n_label_sets][N]
     * of LabelEncoder codes 0..K-1 (every code present, 2 <= K <= min(N-1, 32)),
     * shared by all L layers.  NULL / 0 = none. */
    const int32_t *labels;
    int32_t n_label_sets;
    /* optional TwoNN intrinsic dimension per layer on the same distance
     * matrices (ABI >= 3): the reference's compute_intrinsic_dimensionality
     * (metrics.py:113-208: two nearest neighbours per point, mu = r2/r1,
     * discard the largest `twonn_discard` fraction, slope of -log(1-F) on
     * log(mu) through the origin).  0 = off. */
    int32_t want_twonn;
    float twonn_eps;       /* eps (reference default 1e-10; compared in f32)   */
    double twonn_discard;  /* discard_fraction (reference default 0.1; f64 as
                              in int(len * (1.0 - discard_fraction)))          */
    /* ABI >= 5: workspace slot 0 .. TDA_MAX_SLOTS-1 on `device`.  Each slot has
     * its own streams, device buffers, host-mapped outputs and captured
     * graphs, so calls on different slots (from different host threads) run
     * concurrently on the GPU -- e.g. consecutive sweeps of a layer loop in
     * flight at once; calls on one slot are serialised. */
    int32_t slot;
    /* ABI >= 6: input in parts (dynamic batching of consecutive sweeps).  When
     * n_parts > 0, x is ignored and the L layers are the concatenation of the
     * n_parts arrays x_parts[0 .. n_parts-1], each (L / n_parts, N, D) (or
     * (L / n_parts, N, N) with is_dist), all in host memory or all on `device`
     * as x_on_device says.  The library gathers them into its own buffer (one
     * copy kernel on its stream, after the caller's stream), so the captured
     * graph reads one stable address whatever the parts' addresses are. */
    const void *const *x_parts;
    int32_t n_parts;
} tda_rips_args;

#define TDA_MAX_SLOTS 8
#define TDA_MAX_PARTS 16

/* per (layer, dim) emitted persistence pairs, in the reference's emission
 * order: H0 = Kruskal order of the finite deaths then one [0, inf) per
 * component; Hk = columns in (birth desc, birth-simplex index asc) order.
 * birth_idx/death_idx are combinatorial-number-system simplex indices
 * (H0: birth vertex, death edge; essential classes: death_idx = -1). */
typedef struct tda_rips_result {
    int64_t L, maxdim, N;
    const int64_t *count;     /* [L][maxdim+1] pairs per layer and dim          */
    const int64_t *offset;    /* [L][maxdim+1] offset into the pair arrays      */
    const float *birth;       /* [total] */
    const float *death;       /* [total] (+inf for essential)                   */
    const int64_t *birth_idx; /* [total] */
    const int64_t *death_idx; /* [total] */
    const float *thresh;      /* [L] threshold actually used (enclosing radius) */
    const int64_t *num_edges; /* [L] condensed distances <= thresh              */
    const uint64_t *checksum; /* [L][maxdim+1] order-free hash of ALL pairs     */
    const int64_t *n_all_pairs;/* [L][maxdim+1] all pairs incl. zero-persistence*/
    const int64_t *n_columns; /* [L][maxdim+1] columns considered per dim       */
    const int64_t *n_residual;/* [L][maxdim+1] columns needing reduction        */
    const int64_t *n_adds;    /* [L][maxdim+1] column additions (serial part)   */
    const float *dist;        /* [L][N][N] when want_dist, else NULL            */
    /* Layout guarantee (lets a binding copy them in three reads): count,
     * offset, checksum, n_all_pairs, n_columns, n_residual and n_adds are
     * consecutive [L][maxdim+1] blocks of one allocation, in that order
     * (count + k * L * (maxdim+1) is the k-th); death = birth + total and
     * death_idx = birth_idx + total. */
    double device_ms;         /* device time of the call (HIP events)           */
    /* per-stage device times, filled when args.flags & TDA_FLAG_STAGE_TIMES:
     * stage_ms[i] is the time between consecutive stream events bracketing
     * stage i (one kernel, memset or copy), named by stage_name[i]. */
    int32_t n_stages;
    const char *const *stage_name;
    const float *stage_ms;
    /* [L][n_label_sets] silhouette scores when args.labels was given, else NULL */
    const double *silhouette;
    /* [L] TwoNN intrinsic dimension when args.want_twonn (NaN where the
     * reference returns NaN), else NULL (ABI >= 3) */
    const float *twonn;
    /* ABI >= 3: count .. n_adds, num_edges, birth_idx / death_idx, thresh
     * (padded to 8 bytes) and birth / death, in this order, are ONE
     * allocation of blob_bytes bytes starting at blob (8-byte aligned
     * blocks), so a binding copies every per-pair array in one read;
     * n_pairs = total pairs over all layers and dims. */
    const void *blob;
    int64_t blob_bytes;
    int64_t n_pairs;
    /* ABI >= 4: [L][N][N] float64 distances (sqrt in f64 before any rounding:
     * what sklearn's pairwise_distances returns for float64 points and
     * ripser.py hands back as dperm2all) when args.flags & TDA_FLAG_DIST64,
     * want_dist and float64 point clouds, else NULL */
    const double *dist64;
    /* ABI >= 8: layers of this call re-run without column caps.  With the
     * default threshold (enclosing radius) the parallel reducer stores only
     * the keys of a column up to birth + 0.5 * thresh; a column whose pivot
     * lies above that (a class living longer than half the radius) flags its
     * layer, and the library re-runs that layer alone, uncapped, and splices
     * it in.  Results are exact either way; this only reports the cost. */
    int64_t n_cap_reruns;
} tda_rips_result;

#define TDA_FLAG_STAGE_TIMES 1
/* with TDA_FLAG_STAGE_TIMES: run every stage on one stream so each stage time
 * is one kernel's duration (no overlap with, or queueing behind, the side
 * streams); for per-kernel measurement only */
#define TDA_FLAG_STAGE_SERIAL 2
/* with want_dist and float64 point clouds: also return result->dist64 */
#define TDA_FLAG_DIST64 4
/* distances and the side metrics asked for (want_twonn, labels) only: no
 * persistence at all (maxdim must be 0); every diagram is empty and thresh /
 * num_edges are 0.  What metrics.compute_intrinsic_dimensionality needs
 * (reference metrics.py:113-208 computes no persistence). */
#define TDA_FLAG_NO_PERSISTENCE 8
/* every kernel of the call on the slot's one stream (no side streams): the
 * call's own latency grows, but a slot that only runs such calls holds one
 * hardware queue, so several slots driven from their own host threads
 * (args.slot) run their batches side by side (ripser.SweepPipeline) */
#define TDA_FLAG_ONE_STREAM 16
/* ABI >= 7: device input is complete (the caller synchronised after producing
 * it): no ordering after args.stream at all */
#define TDA_FLAG_INPUT_READY 32

/* Batched point clouds (or distance matrices) -> persistence diagrams. */
int tda_rips_batch(const tda_rips_args *args, tda_rips_result **out);

/* One condensed distance vector (length N(N-1)/2, i<j row-major) -> diagrams.
 * Replaces ripser.py's rips_dm (see header comment). */
int tda_rips_dm(const float *D, int64_t n_entries, int32_t modulus, int32_t dim_max, float threshold,
                int32_t do_cocycles, tda_rips_result **out);

void tda_rips_free(tda_rips_result *r);
const char *tda_last_error(void);
int tda_version(void);
/* 1 if a gfx950 device is visible, 0 otherwise (never aborts). */
int tda_device_ok(int32_t device);
/* Test hook (host only, no device): which distance kernels (N, D) points of
 * `dtype` run on under the current environment -- mfma: the FP64 matrix-core
 * Gram kernels instead of the scalar one; dsplit: K slices (1: unsplit);
 * gram_layer: the whole-layer Gram kernel (f32, N <= 144) instead of 64x64
 * tiles.  Returns 0 or TDA_E_INVALID. */
int tda_debug_dist_plan(int64_t N, int64_t D, int32_t dtype, int32_t *mfma, int32_t *dsplit, int32_t *gram_layer);
/* Test hook: the attempts of the retry ladder that the last tda_rips_batch /
 * tda_rips_dm entry on (device, slot) ran, in order, the one-layer sub-calls
 * of a column-cap re-run appended.  TDA_ATTEMPT_FIELDS int64 per attempt:
 * force_global, scale, force_big, no_par, no_cap, the error flags and the
 * k_reduce_par code the ladder decided on, then the records, record keys,
 * bucket keys and evictions the parallel reducer's last launch drew (read
 * after an abort or under TDA_DEBUG; else -1).  At most cap / TDA_ATTEMPT_FIELDS
 * records are written to out; returns the number of attempts, or
 * TDA_E_INVALID. */
#define TDA_ATTEMPT_FIELDS 11
int tda_debug_attempts(int32_t device, int32_t slot, int64_t *out, int32_t cap);

/*
 * Normalised effective dimensionality of B activation matrices (B, N, D):
 * replaces the reference's TorchScript compute_effective_dimensionality
 * (metrics.py:5-44): S = svdvals(X_b), ED_b = (sum S)^2 /
 * max(sum S^2, 1e-10) / max(min(N, D), 1), as float32 into out[B] (host).
 * The squared singular values are the eigenvalues of the f64 Gram matrix
 * (X X^T on the FP64 matrix cores when N <= D, X^T X otherwise), found by
 * parallel Jacobi on the GPU (csrc/ed_kernels.h).  min(N, D) <= 1024.
 */
typedef struct tda_ed_args {
    const void *x;          /* (B, N, D) row-major, host or device               */
    int32_t dtype;          /* TDA_F32 | TDA_F64                                 */
    int32_t x_on_device;    /* 1: x is a device pointer on `device`              */
    int64_t B, N, D;
    int32_t device;
    void *stream;           /* device input is read after it; NULL = null stream  */
} tda_ed_args;

int tda_effective_dim(const tda_ed_args *args, float *out);

/*
 * Greedy furthest-point landmarks (ripser.py's n_perm, get_greedy_perm
 * [upstream]) of L layers on the GPU: per layer, on the library's own f32
 * distance matrix dm (the sklearn-exact kernels for f32 points; for
 * distance-matrix input the upper triangle, diagonal 0),
 *     ds = dm[0, :]; idx_perm[0] = 0
 *     i = 1 .. n_perm-1: idx = argmax(ds) (the lowest index among equal
 *         maxima); idx_perm[i] = idx; lambdas[i-1] = ds[idx];
 *         ds = minimum(ds, dm[idx, :])
 *     lambdas[n_perm-1] = max(ds)             (r_cover, the covering radius)
 * Every output is an index or a value of dm, copied: results are exact.
 * The landmarks' own (n_perm, n_perm) matrices stay on the device (sub_dev) so
 * that tda_rips_batch can run on them (is_dist, x_on_device,
 * TDA_FLAG_INPUT_READY) without a round trip over the host; N is bounded by
 * 8192 here, the point-count limits of tda_rips_batch then apply to n_perm.
 * The call runs on a stream of its own (not a slot's), L layers in flight,
 * and synchronises before it returns.  Its device workspace holds the
 * (Lc, N, N) f32 matrices of Lc layers at a time (with the staged input and
 * the distance kernels' partial sums): Lc is the largest count whose workspace
 * stays within TDA_GREEDY_WS_BYTES, at least one layer.
 * Errors before any device work: n_perm < 1 or n_perm > N: TDA_E_INVALID;
 * N > 8192: TDA_E_UNSUPPORTED; float64 POINT clouds: TDA_E_UNSUPPORTED
 * (sklearn's row-wise and full-matrix float64 distances disagree, so there is
 * no exact contract); distance matrices of either dtype are accepted.
 * Added to ABI 8 (new symbols only; no existing struct changed).
 */
#define TDA_GREEDY_WS_BYTES (4ull << 30)

typedef struct tda_greedy_args {
    const void *x;          /* (L, N, D) points or (L, N, N) distances, host or device */
    int32_t dtype;          /* TDA_F32 | TDA_F64 (TDA_F64: distance matrices only)  */
    int32_t x_on_device;    /* 1: x is a device pointer on `device`                 */
    int64_t L, N, D;        /* D ignored when is_dist                               */
    int32_t is_dist;        /* 1: x holds (L, N, N) distance matrices (upper used)  */
    int32_t n_perm;         /* landmarks per layer, 1 .. N                          */
    int32_t device;         /* HIP device ordinal                                   */
    void *stream;           /* device input is read after it; NULL = null stream    */
    int32_t want_dperm2all; /* 1: also return the (L, n_perm, N) landmark rows      */
} tda_greedy_args;

typedef struct tda_greedy_result {
    int64_t L, N, n_perm;
    const int64_t *idx_perm; /* host [L][n_perm] landmark indices, idx_perm[l][0] = 0 */
    const float *lambdas;    /* host [L][n_perm] insertion radii; the last is r_cover */
    const float *dperm2all;  /* host [L][n_perm][N] when want_dperm2all, else NULL    */
    const float *sub_dev;    /* DEVICE [L][n_perm][n_perm] f32 on `device`: the
                                landmarks' distance matrices, valid until
                                tda_greedy_free                                       */
    int32_t device;
    double device_ms;        /* device time of the call (HIP events)                  */
    double select_ms;        /* of which the selection kernel (k_greedy_perm)         */
} tda_greedy_result;

int tda_greedy_perm(const tda_greedy_args *args, tda_greedy_result **out);
void tda_greedy_free(tda_greedy_result *r);

/*
 * Resamples of L layers on the GPU: the device stage of the bootstrap
 * confidence bands of persistence diagrams (Fasy et al. 2014, Chazal et al.
 * 2014).  A resample b of a layer is the m points idx[b][0 .. m-1] of its N
 * (with or without repetition; the table is the caller's).  Per layer, on the
 * library's own f32 distance matrix dm (as tda_greedy_perm: the sklearn-exact
 * kernels for f32 points; for distance-matrix input the upper triangle,
 * diagonal 0), the call returns
 *     hausdorff[l][b] = max_i min_{j < m} dm[l][idx[b][j]][i]
 * the Hausdorff distance between the cloud and the resample (a resample is a
 * subset of the cloud, so the other directed distance is 0).  Every output is
 * a value of dm, copied and compared, never computed: results are exact and
 * independent of any reduction order.  The comparisons are `<` and `>`: a NaN
 * in dm (possible only in device input, which is not checked; host input is
 * refused by the Python binding) is skipped, where numpy's min / max would
 * propagate it.
 * Why the Hausdorff distance: for the Rips filtration parameterised by the
 * diameter (as here), d_B(dgm(X), dgm(X*)) <= 2 d_GH(X, X*) <= 2 H(X, X*)
 * (Chazal, de Silva and Oudot 2014), so 2 H bounds, per resample, how far any
 * diagram moves, at the cost of no persistence computation.
 * The call runs on a stream of its own (not a slot's) and synchronises before
 * it returns.  Its device workspace holds the distance stage of Lc layers at a
 * time, Lc the largest count that stays within TDA_GREEDY_WS_BYTES (at least
 * one layer; a table per layer counts in), and beside that, whole, the (L, B)
 * result (L * B * 4 bytes) and a shared table (B * m * 4 bytes).  N <= 8192,
 * m <= 8192 and L * B <= 2^27 (so the result takes at most 512 MiB).
 * Errors before any device work: a NULL pointer, B < 1, m < 1 or an index
 * outside [0, N): TDA_E_INVALID; N > 8192, m > 8192, L * B > 2^27 or float64
 * POINT clouds (as tda_greedy_perm, and for its reason): TDA_E_UNSUPPORTED.
 * Added to ABI 8 (new symbols only; no existing struct changed).
 */
#define TDA_RESAMPLE_MAX_OUT (1ll << 27)

typedef struct tda_resample_args {
    const void *x;          /* (L, N, D) points or (L, N, N) distances, host or device */
    int32_t dtype;          /* TDA_F32 | TDA_F64 (TDA_F64: distance matrices only)  */
    int32_t x_on_device;    /* 1: x is a device pointer on `device`                 */
    int64_t L, N, D;        /* D ignored when is_dist                               */
    int32_t is_dist;        /* 1: x holds (L, N, N) distance matrices (upper used)  */
    int32_t device;         /* HIP device ordinal                                   */
    void *stream;           /* device input is read after it; NULL = null stream    */
    int64_t B;              /* resamples per layer, >= 1                            */
    int32_t m;              /* points per resample, 1 .. 8192                       */
    int32_t idx_per_layer;  /* 0: idx is (B, m), shared by every layer; 1: (L, B, m) */
    const int32_t *idx;     /* HOST indices into 0 .. N-1                           */
} tda_resample_args;

typedef struct tda_resample_result {
    int64_t L, N, B, m;
    const float *hausdorff;  /* host [L][B]                                          */
    int32_t device;
    double device_ms;        /* device time of the call (HIP events)                 */
} tda_resample_result;

int tda_resample(const tda_resample_args *args, tda_resample_result **out);
void tda_resample_free(tda_resample_result *r);

/*
 * H0 persistence of subsamples of L layers on the GPU: the device stage of the
 * persistent-homology dimension (Adams et al. 2020; Birdal et al. 2021).  The
 * H0 deaths of a subsample are the edge weights of the minimum spanning tree
 * of its points; E_alpha is the sum of their alpha-th powers.
 * Per layer l, dm is the matrix of tda_resample: the library's own f32
 * distances, symmetric with a zero diagonal (the sklearn-exact kernels for f32
 * points; for distance-matrix input the upper triangle).  Subsample b has
 * s = sizes[b] positions, 1 <= s <= m; position j holds the point
 * p_j = idx[b][j] (repeats allowed; entries from sizes[b] on are never read).
 * With W[i][j] = dm[l][p_i][p_j], Prim started at position 0:
 *     the tree is {0}, key[j] = W[0][j]
 *     for t = 1 .. s-1:
 *         j* = the position outside the tree with the smallest key
 *              (comparisons are `<`; among equal keys the LOWEST position)
 *         death[b][t-1] = key[j*]
 *         acc += term(key[j*])
 *         j* joins the tree
 *         key[j] = W[j*][j] wherever that is < key[j]
 * acc is a double that starts at 0.0 and is added to sequentially in step
 * order (one lane owns it; the sum is never reduced in parallel).  term(w) is
 * (double)w for alpha == 1, (double)w * (double)w for alpha == 2 and
 * pow((double)w, alpha) for any other alpha.  E[l][b] = acc; for s == 1 it is
 * 0.0 and there are no deaths.
 * What follows: every death is an f32 value of dm, copied and compared, never
 * computed.  For alpha 1 and 2 every term is exact in f64 and the order of the
 * additions is fixed, so E equals a sequential numpy loop bit for bit.  For
 * another alpha the terms differ from another library's pow by the two
 * roundings; every term is non-negative, so the sum is within
 * (s + 16) * 2^-52 relative of that loop.  The sorted deaths are the finite H0
 * deaths of ripser on the subsample: the multiset of MST weights is unique,
 * the lowest-position rule only fixes the order of the deaths and of the sum.
 * Non-finite distances: the Python binding refuses host input that holds
 * them; device input is not checked, the result for it is unspecified, and
 * the kernel still terminates and stays in bounds (the argmin is a 64-bit
 * minimum over (ordered key bits, position): a position is always chosen).
 * The call is of the resampling family: it runs on tda_resample's stream and
 * workspace (it adds neither to the process), captures no graph, and
 * synchronises before it returns.  The workspace holds the distance stage of
 * Lc layers at a time (as tda_resample; a table per layer and the deaths count
 * in), and beside that, whole, E (L * B * 8 bytes), sizes and a shared table.
 * Checked on the host before any device work, in this order: a NULL pointer,
 * L, N, D < 1 or a bad dtype, B < 1, m < 1, a sizes[b] outside [1, m], an
 * index outside [0, N) among the first sizes[b] entries of a row, alpha not
 * finite or <= 0: TDA_E_INVALID.  N > 8192, m > 8192, L * B > 2^27,
 * want_deaths with L * B * (m - 1) > 2^27, float64 POINT clouds:
 * TDA_E_UNSUPPORTED.
 * Added to ABI 8 (new symbols only; no existing struct changed).
 */
#define TDA_SH0_MAX_OUT (1ll << 27)

typedef struct tda_subsample_h0_args {
    const void *x;          /* (L, N, D) points or (L, N, N) distances, host or device */
    int32_t dtype;          /* TDA_F32 | TDA_F64 (TDA_F64: distance matrices only)  */
    int32_t x_on_device;    /* 1: x is a device pointer on `device`                 */
    int64_t L, N, D;        /* D ignored when is_dist                               */
    int32_t is_dist;        /* 1: x holds (L, N, N) distance matrices (upper used)  */
    int32_t device;         /* HIP device ordinal                                   */
    void *stream;           /* device input is read after it; NULL = null stream    */
    int64_t B;              /* subsamples per layer, >= 1                           */
    int32_t m;              /* the table's row length, 1 .. 8192                    */
    int32_t idx_per_layer;  /* 0: idx is (B, m), shared by every layer; 1: (L, B, m) */
    const int32_t *idx;     /* HOST indices into 0 .. N-1                           */
    const int32_t *sizes;   /* HOST [B], shared by all layers: 1 <= sizes[b] <= m   */
    double alpha;           /* the power of a death in E: finite, > 0               */
    int32_t want_deaths;    /* 1: return the deaths too                             */
} tda_subsample_h0_args;

typedef struct tda_subsample_h0_result {
    int64_t L, N, B, m;
    const double *E;        /* host [L][B]                                          */
    const float *deaths;    /* host [L][B][m-1] in step order when want_deaths,
                               entries from sizes[b]-1 on are 0; else NULL          */
    int32_t device;
    double device_ms;       /* device time of the call (HIP events)                 */
} tda_subsample_h0_result;

int tda_subsample_h0(const tda_subsample_h0_args *args, tda_subsample_h0_result **out);
void tda_subsample_h0_free(tda_subsample_h0_result *r);

/*
 * Geodesic distances over the neighbourhood graph of L layers on the GPU:
 * Isomap's metric, the input of persistent homology in Naitzat, Zhitnikov and
 * Lim 2020 ("Topology of deep neural networks").  The result is a distance
 * matrix for the entries that take one (tda_rips_batch, tda_subsample_h0,
 * tda_resample, tda_greedy_perm with is_dist).
 * Per layer, dm is the matrix of tda_resample: the library's own f32
 * distances, symmetric with a zero diagonal.
 * The graph.  Exactly one of n_neighbors = k >= 1 and radius >= 0 is given
 * (n_neighbors = 0 and radius < 0 mean "not given"; radius may be +inf).
 *   kNN: with ord(w) the unsigned integer ordered as the floats are (-0.0 as
 *     +0.0; tda_subsample_h0's) and key(i, j) = ord(dm[i][j]) << 32 | j, the
 *     neighbours of row i are the min(k, N - 1) columns j != i of smallest
 *     key: the lowest index wins ties.  {i, j} is an edge if j is a neighbour
 *     of i OR i is a neighbour of j.
 *   radius: {i, j}, i != j, is an edge iff (double)dm[i][j] <= radius.
 * W[i][j] = dm[i][j] on an edge, +inf otherwise, W[i][i] = 0.
 * The closure.  G is the min-plus closure of W in f32: every G[i][j] is the
 * result of a tree of rounded f32 additions over the edge weights of one walk
 * from i to j in the graph (W[i][j] itself, or 0 for i == j, when the tree is
 * a leaf), and no walk gives a smaller result under the same schedule.  For
 * every schedule: G[i][i] = 0; G[i][j] and G[j][i] are the same bits;
 * G[i][j] <= W[i][j]; G[i][j] = +inf exactly when i and j lie in different
 * components (while every walk sum stays finite in f32: weights up to
 * FLT_MAX / N); a layer's bits do not depend on L, on the chunk of layers it
 * is served in, or on the other layers of the call.
 * With G* the exact shortest length, u = 2^-24 and c the height of the
 * deepest tree the schedule can build,
 *     |G[i][j] - G*[i][j]| <= ((1 + u)^c - 1) * G*[i][j]
 * (rounded addition and min are monotone: by induction over the schedule's
 * steps the computed value lies between (1 - u)^h and (1 + u)^h times the
 * exact value of that step, h the height so far).  Two schedules:
 *   N <= 128: the ascending-k loop G[i][j] = min(G[i][j], G[i][k] + G[k][j]),
 *     k = 0 .. N-1.  A step adds at most 1 to a height and the steps k == i
 *     and k == j change nothing: c = max(N - 2, 0) <= N - 1.
 *   N > 128: tiles of B = 64, T = ceil(N / 64) rounds.  Round t closes the
 *     diagonal tile with the ascending-k loop (+B), then forms the tiles of
 *     its row as one min-plus product with the closed tile (+1), then every
 *     other tile as one product of two of those (+1): c = (B + 2) * T.
 * Where every walk sum is exact in f32 (small integer weights) G == G* bit
 * for bit under either schedule.
 * Outputs: dist[l] = G (or W with graph_only, the closure skipped);
 * n_components[l] = the number of rows i with no finite G[i][j], j < i
 * (-1 with graph_only); n_edges[l] = the undirected edges of the graph.
 * Non-finite or negative distances: host matrices that hold them are refused;
 * device input is not checked, the result for it is unspecified, and every
 * kernel still terminates and stays in bounds (no loop's trip count and no
 * address depends on a value of dm).
 * The call is of the resampling family: it runs on tda_resample's stream and
 * workspace (it adds neither to the process), captures no graph, and
 * synchronises before it returns.  The workspace holds the distance stage of
 * Lc layers at a time (as tda_resample; the rows' thresholds count in); the
 * graph and the closure are formed in place on dm and read back chunk by
 * chunk.  N <= 8192 and L * N * N <= 2^28 (the result takes at most 1 GiB).
 * Checked on the host before any device work, in this order: a NULL pointer,
 * L, N, D < 1 or a bad dtype, n_neighbors < 0, a NaN radius, both or neither
 * of n_neighbors and radius: TDA_E_INVALID.  N > 8192, L * N * N > 2^28,
 * float64 POINT clouds: TDA_E_UNSUPPORTED.  Last, a host distance matrix with
 * an entry that is not finite and >= 0: TDA_E_INVALID.
 * Added to ABI 8 (new symbols only; no existing struct changed).
 */
#define TDA_GEO_MAX_OUT (1ll << 28)

typedef struct tda_geodesic_args {
    const void *x;          /* (L, N, D) points or (L, N, N) distances, host or device */
    int32_t dtype;          /* TDA_F32 | TDA_F64 (TDA_F64: distance matrices only)  */
    int32_t x_on_device;    /* 1: x is a device pointer on `device`                 */
    int64_t L, N, D;        /* D ignored when is_dist                               */
    int32_t is_dist;        /* 1: x holds (L, N, N) distance matrices (upper used)  */
    int32_t device;         /* HIP device ordinal                                   */
    void *stream;           /* device input is read after it; NULL = null stream    */
    int32_t n_neighbors;    /* k >= 1: the kNN graph; 0: not given                  */
    int32_t graph_only;     /* 1: return W, skip the closure                        */
    double radius;          /* >= 0 (+inf allowed): the radius graph; < 0: not given */
} tda_geodesic_args;

typedef struct tda_geodesic_result {
    int64_t L, N;
    const float *dist;           /* host [L][N][N]: G, or W with graph_only          */
    const int32_t *n_components; /* host [L]; -1 with graph_only                     */
    const int64_t *n_edges;      /* host [L]                                         */
    int32_t device;
    double device_ms;            /* device time of the call (HIP events)             */
} tda_geodesic_result;

int tda_geodesic(const tda_geodesic_args *args, tda_geodesic_result **out);
void tda_geodesic_free(tda_geodesic_result *r);

/*
 * The permutation test between groups of diagrams (Robinson and Turner 2017,
 * "Hypothesis testing for topological data analysis") on the GPU.  Inputs, all
 * on the host: w, an (S, S) float64 matrix of the q-th powers of the pairwise
 * distances; obs[S], the observed group codes in [0, G); lab[B][S], B
 * relabellings, each a permutation of obs.  With n_g the size of group g the
 * weight is c_g = 1 / (2 n_g (n_g - 1)): one rounded division of 1.0 by the
 * product, which is exact in float64.  For a labelling l:
 *     col_j = sum over i = 0, 1, ..., S-1 in that order, starting from +0.0,
 *             of w[i][j] where l_i == l_j        (one rounded addition each;
 *             an unselected i adds nothing or +0.0: the same bits, as col_j
 *             is never -0.0)
 *     t_j   = c[l_j] * col_j                     (one rounded product, never
 *             fused with an addition)
 *     T(l)  = 64 partial sums, the k-th over t_j for j = k, k+64, k+128, ...
 *             in that order from +0.0 (a lane without a column holds +0.0),
 *             then added pairwise: lanes k and k^1, then k^2, k^4, k^8, k^16,
 *             k^32
 * the statistic sigma^2 = sum_g c_g sum_{i, j in g} d(X_i, X_j)^q of the
 * paper over ordered pairs, in the reduction shape of tda_heat_kernel.  The
 * call returns t_obs = T(obs), null[b] = T(lab[b]), count = #{b : null[b] <=
 * t_obs} and pvalue = (1 + count) / (B + 1) (one float64 division; the form
 * of Phipson and Smyth 2010, never 0).
 * Promised, bit for bit:
 *  1. T depends on the partition only.  col_j selects by equality with l_j, so
 *     it is a function of the SET of diagrams grouped with j and of nothing
 *     else; c[l_j] depends on the size of that set only; the order of every
 *     addition is fixed by i and j, never by a group code.  Two labellings
 *     that split the diagrams into the same sets, two equal-sized groups
 *     swapped included, give the same bits, and such a row of lab always
 *     counts as <= t_obs.
 *  2. null[b] depends on neither B, the row's position in lab, the launch
 *     shape, which kernel ran, nor the run (no atomics, no order left open).
 *  3. Everything equals the numpy restatement tests/perm_ref.py.
 * Not promised: independence of the ORDER of the diagrams.  Permuting the
 * rows and columns of w and the labels together permutes the additions.  The
 * bound, as for tda_heat_kernel: every term is non-negative, so every partial
 * sum is at most the final one and an addition's error is at most u (u =
 * 2^-53) times the part of T that passes through it.  A term w[i][j] passes
 * through at most n - 2 inexact additions of col_j (n the size of j's group,
 * at most S - 2: the diagonal term +0.0 and the first addition onto +0.0 are
 * exact), one product, ceil(S / 64) - 1 inexact lane additions and 6
 * butterfly additions.  To first order in u,
 *     |T - T_exact| <= (n_max + 3 + ceil(S / 64)) u T
 *                   <= S u T + 7 u T   for S <= 384 (ceil(S / 64) <= 6),
 * and at most S u T + 33 u T at S = 2048.  Two orders of the same data differ
 * by at most twice that.
 * Checked on the host, before any device work, in this order: a NULL pointer,
 * S < 2, B < 1, G < 2 or reserved != 0: TDA_E_INVALID.  S > TDA_PERM_MAX_S,
 * G > TDA_PERM_MAX_GROUPS or B * S > TDA_PERM_MAX_TABLE: TDA_E_UNSUPPORTED.
 * Then TDA_E_INVALID, the message naming the first offending index, for a w
 * entry that is not finite or is negative, a diagonal entry that is not +0.0,
 * w[i][j] and w[j][i] that differ in bits, an obs code >= G, a group with
 * fewer than 2 members, and a row of lab whose label histogram is not that of
 * obs.  After that the kernels read in bounds by construction.
 * The call runs on a stream and a per-device workspace of its own (no slot's,
 * nothing captured into a graph), which holds w, the weights, the table with
 * obs as one more row (B * S + S bytes) and the B + 1 statistics, and
 * synchronises before it returns.
 * Added to ABI 8 (new symbols only; no existing struct changed).
 */
#define TDA_PERM_MAX_S 2048
#define TDA_PERM_MAX_GROUPS 64
#define TDA_PERM_MAX_TABLE (1ll << 27)

typedef struct tda_perm_args {
    const double *w;     /* HOST (S, S): symmetric in bits, +0.0 diagonal, finite, >= 0 */
    const uint8_t *obs;  /* HOST [S]: observed group codes in [0, G)                    */
    const uint8_t *lab;  /* HOST [B][S]: every row a permutation of obs                 */
    int64_t S;           /* diagrams, 2 .. TDA_PERM_MAX_S                               */
    int64_t B;           /* relabellings, >= 1, B * S <= TDA_PERM_MAX_TABLE             */
    int32_t G;           /* groups, 2 .. TDA_PERM_MAX_GROUPS, each of >= 2 members      */
    int32_t device;      /* HIP device ordinal                                          */
    int32_t reserved;    /* must be 0                                                   */
} tda_perm_args;

typedef struct tda_perm_result {
    int64_t S, B;
    double t_obs;        /* T(obs)                                                      */
    const double *null;  /* host [B]: T(lab[b])                                         */
    int64_t count;       /* #{b : null[b] <= t_obs}                                     */
    double pvalue;       /* (1 + count) / (B + 1)                                       */
    int32_t device;
    double device_ms;    /* device time of the call (HIP events)                        */
} tda_perm_result;

int tda_permutation_test(const tda_perm_args *args, tda_perm_result **out);
void tda_perm_free(tda_perm_result *r);

/*
 * The other spectral metrics of the reference's metrics.py, on the Gram
 * kernels and the Jacobi kernel of tda_effective_dim (same workspace, same
 * ordering after the caller's stream, same limits: min(N, D) <= 1024 and
 * N <= 8192 for the N rows of one matrix).
 *
 * tda_matrix_entropy: matrix-based Renyi entropy (matrix_entropy,
 * metrics.py:344-399) of every matrix for n_alpha orders at once.  With the
 * eigenvalues lambda_i of the f64 Gram matrix clamped at 0,
 *     p_i = lambda_i / (sum lambda + eps)
 *     |alpha - 1| < eps:  -sum xlogy(p_i, p_i)
 *     otherwise:          log(sum p_i^alpha) / (1 - alpha)
 * in f64, as float32 into out[item][a] (host).  The reference takes the
 * spectrum of the N x N matrix Z Z^T; the library diagonalises the smaller
 * side, m = min(N, D): for N > D the N - m eigenvalues it leaves out are exact
 * zeros, which add nothing for alpha > 0.  Orders alpha <= 0 are refused
 * (TDA_E_INVALID): there the reference's own float32 noise eigenvalues decide
 * its answer.  1 <= n_alpha <= 16.
 *
 * tda_effective_dim_windows: compute_fixed_window_ed (metrics.py:47-109), the
 * effective dimensionality of tda_effective_dim over n_windows non-overlapping
 * windows of S / n_windows rows, as float32 into out[b][w] (host).
 *
 * Windows: with S % W == 0 the (B, S, D) input is read in place as
 * (B * W, S / W, D); otherwise the first W * (S / W) rows of every item are
 * staged with one 2-D copy.  n_windows > S is taken as n_windows = S (every
 * row its own window; the output then has S columns); n_windows < 0, or 0 for
 * tda_effective_dim_windows: TDA_E_INVALID.  Errors arrive before any device
 * work.  Added to ABI 8 (new symbols only; no existing struct changed).
 */
typedef struct tda_spectral_args {
    const void *x;          /* (B, S, D) row-major, host or device               */
    int32_t dtype;          /* TDA_F32 | TDA_F64                                 */
    int32_t x_on_device;    /* 1: x is a device pointer on `device`              */
    int64_t B, S, D;        /* B items of S rows (tokens) by D                   */
    int64_t n_windows;      /* 0: one matrix per item (N = S); W >= 1: W windows of
                               S / W rows each, the last S % W rows of an item dropped */
    int32_t n_alpha;        /* matrix entropy only: orders per call, 1 .. 16     */
    const double *alphas;   /* matrix entropy only: host [n_alpha], each > 0     */
    double eps;             /* matrix entropy only: metrics.py's eps (1e-10)     */
    int32_t device;
    void *stream;           /* device input is read after it; NULL = null stream  */
} tda_spectral_args;

int tda_matrix_entropy(const tda_spectral_args *args, float *out);        /* out[B * max(W, 1)][n_alpha] */
int tda_effective_dim_windows(const tda_spectral_args *args, float *out); /* out[B][W] */

/*
 * Native sweep pipeline: consecutive sweeps of a layer loop in flight at once,
 * without a host thread of the caller per call.  The pipe owns `depth` worker
 * threads, one per workspace slot (the top `depth` slots of the device; slot 0
 * is left to plain calls), coalesces up to `coalesce` consecutive sweeps into
 * one tda_rips_batch call (their arrays as x_parts) and hands every sweep its
 * own layers of the call's result.  The caller makes one short call per sweep
 * (tda_pipe_submit) and one blocking call per result (tda_pipe_wait); a
 * binding whose interpreter has a global lock never takes it in a worker.
 *
 * The pending batch is dispatched when it holds `coalesce` sweeps, when a
 * sweep with another (L, N, D), dtype, residence or tmpl_id arrives, when one
 * of its tickets is waited on, and at flush / destroy.  Call n runs on worker
 * n % depth, so the calls of one slot stay ordered.
 *
 * tda_pipe_submit: *tmpl gives every argument of the call but x, dtype,
 * x_on_device, L, N, D, slot, x_parts and n_parts, which the pipe fills
 * (TDA_FLAG_ONE_STREAM is the caller's to set in tmpl->flags: each worker then
 * holds one hardware queue).  The template is copied when a batch starts;
 * sweeps share a call only under one tmpl_id, so equal ids must mean equal
 * contents.  Device input must be complete (TDA_FLAG_INPUT_READY in
 * tmpl->flags): a worker does not order itself after any caller stream.  x and
 * tmpl->labels must stay valid until the ticket's tda_pipe_wait has returned.
 * Host input is checked for NaN / infinity by the worker, before the call: the
 * call then fails with TDA_E_INVALID, "Input contains NaN or infinity.".
 *
 * tda_pipe_wait with TDA_PIPE_BLOCK: blocks until the ticket's call has run.
 * Returns the call's code (with its message in tda_last_error() of the waiting
 * thread); every ticket of a failed call reports the same error.  On success
 * *res is the call's result, shared by its *n_sweeps tickets, of which layers
 * [*lo, *hi) are the ticket's; *call identifies the call (tickets of one call
 * agree).  TDA_PIPE_POLL never blocks and dispatches nothing; TDA_PIPE_DISPATCH
 * dispatches the ticket's batch if it is still pending and does not block
 * either: both return TDA_PIPE_BUSY (with *res NULL) while the call has not run.
 * The result stays valid until the LAST of the call's tickets is released,
 * which frees it; never pass it to tda_rips_free.  tda_pipe_release returns the
 * number of the call's tickets still unreleased (>= 0) or TDA_E_INVALID.
 * tda_pipe_destroy dispatches what is pending, lets the workers finish, joins
 * them and frees every result still held; all tickets die with the pipe.
 * Submit, wait and release may be called from any threads.
 * Added to ABI 8 (new symbols only; no existing struct changed).
 */
typedef struct tda_pipe tda_pipe;

#define TDA_PIPE_POLL 0
#define TDA_PIPE_BLOCK 1
#define TDA_PIPE_DISPATCH 2
#define TDA_PIPE_BUSY 1

int tda_pipe_create(int32_t depth, int32_t coalesce, tda_pipe **out);
int tda_pipe_submit(tda_pipe *pipe, const tda_rips_args *tmpl, int64_t tmpl_id, const void *x, int64_t L, int64_t N, int64_t D,
                    int32_t dtype, int32_t x_on_device, uint64_t *ticket);
int tda_pipe_flush(tda_pipe *pipe);
int tda_pipe_wait(tda_pipe *pipe, uint64_t ticket, tda_rips_result **res, int64_t *lo, int64_t *hi, int32_t *n_sweeps,
                  uint64_t *call, int32_t mode);
int tda_pipe_release(tda_pipe *pipe, uint64_t ticket);
void tda_pipe_destroy(tda_pipe *pipe);

/*
 * Representative H1 cocycles (ripser.py's do_cocycles=True for dimension 1, coeff 2) of L small
 * layers on the GPU.  Input: L square float32 distance matrices (L, N, N) on the host, zero
 * diagonal; only the strict upper triangle is read, as in tda_rips_batch.  thresh = +inf (or
 * FLT_MAX) means the enclosing radius min_i max_j d(i, j); num_edges = #{i < j : d <= thresh}.
 *
 * Definition.  Edges and triangles carry their colex indices (edge {i > j}: C(i,2) + j, triangle
 * {a > b > c}: C(a,3) + C(b,2) + c) and diameters (the largest distance inside); only simplices of
 * diameter <= thresh exist.  H0 deaths are the edges Kruskal accepts over the edges in (diam asc,
 * index desc) order.  The remaining edges are the columns, in (diam desc, index asc) order; the
 * H0 deaths are skipped (clearing).  R = delta V is reduced over Z/2 from left to right: a column
 * starts as the coboundary of its edge (V_e = {e}); its pivot is its minimal triangle by (diam
 * asc, index desc); while an earlier column owns that pivot, that column is added, R to R and V
 * to V.  A column left with a pivot owns it and dies there; a column reduced to zero is essential.
 * The cocycle of a pair is V_e at that moment: a set of edges, each of length >= the birth, the
 * birth edge among them.  Under these rules V_e is unique, and ripser's emergent- and
 * apparent-pair shortcuts (which only skip additions that would not happen) leave it unchanged:
 * it is the set of edges ripser.py records.  ORDER: a cocycle's edges are listed in column order,
 * so the birth edge comes last; ripser.py lists them in the pop order of its heap, which is not
 * reproduced (compare cocycles as sets).
 *
 * Output, per layer, in ripser's emission order for H1 (columns by birth desc, birth-edge index
 * asc): the pairs with death > birth, and the essential classes as (birth, +inf), with
 * birth_idx / death_idx as in tda_rips_result (death_idx = -1 for essential classes), and one
 * CSR of cocycles over the pairs of all layers.  Every output is an integer or a copied f32.
 *
 * Limits: 0 <= N <= TDA_CC_MAX_N (N <= 2 gives empty results); N above: TDA_E_UNSUPPORTED.
 * A NULL pointer, L < 1, N < 0, reserved != 0, a NaN thresh, a NaN or negative distance in a
 * strict upper triangle: TDA_E_INVALID.  All of this is checked before any device work
 * (csrc/cc_plan.h cc_check).  Layers run in rounds so that the device workspace stays within
 * TDA_CC_WS_BYTES (csrc/cc_plan.h cc_plan).
 *
 * THE ENTRY IS NOT IN THE LIBRARY YET: this comment, the limits and the argument struct are what
 * the host plan (csrc/cc_plan.h) and the reference (tests/cc_ref.py) are written against; the
 * result struct and the functions come with the device side.
 */
#define TDA_CC_MAX_N 64
#define TDA_CC_WS_BYTES (1ull << 30)

typedef struct tda_cc_args {
    const float *dist;   /* HOST (L, N, N) f32 distance matrices (strict upper triangle read) */
    int64_t L, N;
    float thresh;        /* +inf: enclosing radius                                            */
    int32_t device;      /* HIP device ordinal                                                */
    int32_t reserved;    /* must be 0                                                         */
} tda_cc_args;

#ifdef __cplusplus
}
#endif
#endif /* TDA_RIPS_H */
