/*
 * tda_dgm.h -- distances between persistence diagrams on the MI355X (gfx950).
 * Part of libtda_rips.so: error codes, tda_last_error() and tda_device_ok()
 * are those of tda_rips.h.  Added to ABI 8 (new symbols only; no existing
 * struct changed).
 *
 * tda_sliced_wasserstein: the sliced Wasserstein distance (Carriere, Cuturi,
 * Oudot 2017; persim.sliced_wasserstein [upstream]) of P pairs out of S
 * diagrams in one call.  For diagrams A (n1 points) and B (n2 points) of
 * (birth, death) pairs, after dropping every point with a non-finite
 * coordinate (the essential classes):
 *     pi(p)   = ((b + d) / 2, (b + d) / 2)            the diagonal projection
 *     theta_i = -pi/2 + i * (pi / M),  u_i = (cos theta_i, sin theta_i)
 *     V1_i    = {p . u_i : p in A} u {pi(q) . u_i : q in B}
 *     V2_i    = {q . u_i : q in B} u {pi(p) . u_i : p in A}
 *     SW(A,B) = (1 / M) * sum_{i < M} sum_k |sort(V1_i)[k] - sort(V2_i)[k]|
 * (= (1/pi) * sum_i (pi/M) * ...), everything in float64, the directions
 * summed in increasing i.  Two empty diagrams give 0.  The result is a pure
 * function of the two point multisets and M: SW(A, A) is exactly 0,
 * SW(A, B) == SW(B, A) bit for bit, and a pair's value does not depend on
 * what else the call holds.
 *
 * Limits: n1 + n2 <= TDA_SW_MAX_POINTS finite points for every requested
 * pair and 1 <= M <= TDA_SW_MAX_DIRECTIONS, else TDA_E_UNSUPPORTED;
 * P * M <= TDA_SW_MAX_WORK per call (the (P, M) scratch buffer), else
 * TDA_E_UNSUPPORTED: split the call.  Bad offsets or pair indices:
 * TDA_E_INVALID.  All argument errors arrive before any device work.
 *
 * tda_bottleneck: the bottleneck distance (the distance of the stability
 * theorem; persim.bottleneck [upstream]) of P pairs out of S diagrams in one
 * call.  For diagrams A (n1 points) and B (n2 points), after dropping every
 * point with a non-finite coordinate:
 *     c(p, q) = max(|b_p - b_q|, |d_p - d_q|)     p in A, q in B   (L-infinity)
 *     c(p)    = |d_p - b_p| / 2                   the distance to the diagonal
 *     d_B(A, B) = min over partial matchings m of A with B of
 *                 max(c(p, m(p)) for matched p, c(p) for unmatched p in A,
 *                     c(q) for unmatched q in B)
 * Two empty diagrams give 0, one empty diagram gives the other's largest
 * c(p) (half its maximum persistence).  Everything is float64 and exact: the
 * value is one of the costs above, each a single correctly rounded operation
 * on the inputs.  It is a pure function of the two point multisets:
 * d_B(A, A) is 0.0, d_B(A, B) == d_B(B, A) bit for bit, and a pair's value
 * depends neither on the order of the rows nor on what else the call holds.
 *
 * Limits: at most TDA_BN_MAX_POINTS finite points in each diagram of a
 * requested pair, and at most TDA_SW_MAX_WORK diagrams and pairs per call, else
 * TDA_E_UNSUPPORTED.  points, offsets, pairs and the error codes are those of
 * tda_sliced_wasserstein; reserved must be 0 (TDA_E_INVALID).  All argument
 * errors arrive before any device work.  TDA_E_CAPACITY: a pair's matching
 * ran into one of the kernel's loop bounds (an internal error; no result).
 *
 * tda_wasserstein: the 1-Wasserstein distance with the Euclidean ground metric
 * (persim.wasserstein(dgm1, dgm2, matching=False) [upstream]) of P pairs out of
 * S diagrams in one call, and on request the matching itself.  For diagrams A
 * (n1 points) and B (n2 points), after dropping every point with a non-finite
 * coordinate:
 *     c(p, q) = sqrt((b_p - b_q)*(b_p - b_q) + (d_p - d_q)*(d_p - d_q))   p in A, q in B
 *     c(p)    = (d_p - b_p) * 0.70710678118654752440    the L2 distance to the diagonal
 *     W(A, B) = min over partial matchings m of A with B of
 *               sum of c(p, m(p)) over matched p + sum of c(p) over unmatched p in A
 *                                                + sum of c(q) over unmatched q in B
 * Everything is float64.  Each cost is that sequence of individually rounded
 * operations (two subtractions, two products, one addition, one correctly
 * rounded sqrt; no fused multiply-add), so c(p, q) is numpy's
 * np.sqrt(db*db + dd*dd) bit for bit.  Two empty diagrams give exactly 0.0, one
 * empty diagram gives the sum of the other's c(p).
 *
 * What is promised, with K = n1 + n2, u = 2^-53 and cmax the pair's largest cost:
 *   1. the matching is a valid partial matching (an exact solver: successive
 *      shortest augmenting paths with float64 duals), and its cost lies within
 *      4 K^2 u cmax of the optimum;
 *   2. dist is the sum of the float64 costs of that matching, added in one fixed
 *      order: within K u dist of their exact sum;
 *   3. bit for bit: W(A, B) == W(B, A) (each pair is solved in one canonical
 *      orientation: the longer diagram first, at equal counts the
 *      lexicographically smaller point array), and a pair's value and matching
 *      are the same alone, among other pairs of any sizes, in any position of
 *      the pair list and from run to run.
 * Not promised bit for bit: independence of the order of a diagram's rows (the
 * values of two orders agree within bound 1), and W(A, A) being exactly 0 (it
 * is at most bound 1).
 *
 * With TDA_WS_WANT_MATCHING, match holds for pair p, from match_off[p] on, one
 * entry per finite point of the pair's first diagram as the caller named it, in
 * the caller's row order with the non-finite rows dropped: the index of its
 * partner among the second diagram's finite points, or -1 for the diagonal.
 * The points of the second diagram that no entry names go to the diagonal.
 *
 * Limits: at most TDA_WS_MAX_POINTS finite points in each diagram of a
 * requested pair, at most TDA_SW_MAX_WORK diagrams and pairs per call and, with
 * the matching, at most TDA_SW_MAX_WORK entries of match, else
 * TDA_E_UNSUPPORTED.  points, offsets, pairs and the error codes are those of
 * tda_bottleneck; a bit of flags other than TDA_WS_WANT_MATCHING is
 * TDA_E_INVALID.  All argument errors arrive before any device work.
 * TDA_E_CAPACITY: a pair's solver ran into one of the kernel's loop bounds (an
 * internal error; no result).
 */
#ifndef TDA_DGM_H
#define TDA_DGM_H

#include "tda_rips.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDA_SW_MAX_POINTS 4096
#define TDA_SW_MAX_DIRECTIONS 1024
#define TDA_SW_MAX_WORK (1ll << 27)

typedef struct tda_sw_args {
    const double *points;   /* host (total, 2) f64 (birth, death); non-finite rows are skipped */
    const int64_t *offsets; /* host [S + 1] non-decreasing row boundaries, offsets[0] = 0      */
    int64_t S;              /* diagrams                                                        */
    const int32_t *pairs;   /* host (P, 2) diagram indices, or NULL: every i < j, row-major    */
    int64_t P;              /* pairs in `pairs`; ignored when pairs is NULL                    */
    int32_t M;              /* directions, 1 .. TDA_SW_MAX_DIRECTIONS                          */
    int32_t device;         /* HIP device ordinal                                              */
} tda_sw_args;

typedef struct tda_sw_result {
    int64_t P;          /* pairs computed (S (S - 1) / 2 when pairs was NULL)   */
    const double *dist; /* host [P]                                             */
    double device_ms;   /* device time of the call (HIP events, copies included) */
} tda_sw_result;

int tda_sliced_wasserstein(const tda_sw_args *args, tda_sw_result **out);
void tda_sw_free(tda_sw_result *r);

#define TDA_BN_MAX_POINTS 512

typedef struct tda_bn_args {
    const double *points;   /* host (total, 2) f64 (birth, death); non-finite rows are skipped */
    const int64_t *offsets; /* host [S + 1] non-decreasing row boundaries, offsets[0] = 0      */
    int64_t S;              /* diagrams                                                        */
    const int32_t *pairs;   /* host (P, 2) diagram indices, or NULL: every i < j, row-major    */
    int64_t P;              /* pairs in `pairs`; ignored when pairs is NULL                    */
    int32_t device;         /* HIP device ordinal                                              */
    int32_t reserved;       /* must be 0                                                       */
} tda_bn_args;

typedef struct tda_bn_result {
    int64_t P;          /* pairs computed (S (S - 1) / 2 when pairs was NULL)   */
    const double *dist; /* host [P]                                             */
    double device_ms;   /* device time of the call (HIP events, copies included) */
} tda_bn_result;

int tda_bottleneck(const tda_bn_args *args, tda_bn_result **out);
void tda_bn_free(tda_bn_result *r);

#define TDA_WS_MAX_POINTS 512
#define TDA_WS_WANT_MATCHING 1

typedef struct tda_ws_args {
    const double *points;   /* host (total, 2) f64 (birth, death); non-finite rows are skipped */
    const int64_t *offsets; /* host [S + 1] non-decreasing row boundaries, offsets[0] = 0      */
    int64_t S;              /* diagrams                                                        */
    const int32_t *pairs;   /* host (P, 2) diagram indices, or NULL: every i < j, row-major    */
    int64_t P;              /* pairs in `pairs`; ignored when pairs is NULL                    */
    int32_t device;         /* HIP device ordinal                                              */
    int32_t flags;          /* 0 or TDA_WS_WANT_MATCHING                                       */
} tda_ws_args;

typedef struct tda_ws_result {
    int64_t P;                /* pairs computed (S (S - 1) / 2 when pairs was NULL)             */
    const double *dist;       /* host [P]                                                       */
    double device_ms;         /* device time of the call (HIP events, copies included)          */
    const int64_t *match_off; /* host [P + 1] into match, or NULL without TDA_WS_WANT_MATCHING  */
    const int32_t *match;     /* host [match_off[P]]: partner in the second diagram or -1; NULL */
} tda_ws_result;

int tda_wasserstein(const tda_ws_args *args, tda_ws_result **out);
void tda_ws_free(tda_ws_result *r);

#ifdef __cplusplus
}
#endif
#endif
