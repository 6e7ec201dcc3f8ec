/*
 * tda_dgm.h -- distances between persistence diagrams, their vectorisations
 * (landscapes, images, persistence curves), the heat kernel and the persistence Fisher
 * distance, on the MI355X (gfx950).
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
 *
 * tda_landscape: the persistence landscape (Bubenik 2015; persim.landscapes
 * [upstream]) of S diagrams, sampled exactly on a grid, in one call.  For a
 * diagram A, after dropping every row with a non-finite coordinate, and a grid
 * value t:
 *     f_p(t)   = max(0, min(t - b_p, d_p - t))             one tent per point
 *     lambda_k(t) = the k-th largest of {f_p(t) : p in A}, k = 1 .. K; 0 when A has fewer than k points
 *     values[s][k - 1][g] = lambda_k(grid[g])
 * Everything is float64.  Each value is one correctly rounded subtraction of two
 * inputs (t - b_p or d_p - t) or +0.0, never -0.0: the result is exact, equal bit
 * for bit to a numpy restatement.  A row with d <= b contributes zeros only.
 * This is the exact landscape at the grid values: nothing is snapped to the grid
 * (persim's PersLandscapeApprox moves the bars to the grid first and so differs).
 * grid holds G finite values in any order; the library forms no grid value itself.
 *
 * Limits: at most TDA_VEC_MAX_POINTS finite points per diagram, 1 <= K <=
 * TDA_PL_MAX_DEPTH, 1 <= G <= TDA_PL_MAX_STEPS, S * K * G <= TDA_VEC_MAX_OUT and
 * S <= TDA_SW_MAX_WORK, else TDA_E_UNSUPPORTED.  Bad offsets, grid == NULL, a
 * non-finite grid value, K < 1, G < 1, reserved != 0: TDA_E_INVALID.  All argument
 * errors arrive before any device work.
 *
 * tda_persistence_image: the persistence image (Adams et al. 2017;
 * persim.PersistenceImager [upstream], with its default skew = True) of S diagrams
 * in one call.  Finite rows only, in birth-persistence coordinates (b_p, pi_p),
 * pi_p the float64 difference d_p - b_p:
 *     w_p      = pi_p ^ weight_power for pi_p > 0, else 0       (1 for power 0, pi_p for power 1)
 *     r        = 0.70710678118654752440 / sigma                  1 / (sigma sqrt(2))
 *     gx_p[i]  = (erf((x_edges[i + 1] - b_p) r) - erf((x_edges[i] - b_p) r)) / 2
 *     gy_p[j]  = the same with y_edges and pi_p
 *     values[s][i][j] = sum over p of w_p gx_p[i] gy_p[j]         p in the order of the finite rows
 * i is the birth axis (W pixels), j the persistence axis (H pixels): a Gaussian of
 * standard deviation sigma in both axes (covariance sigma^2 I, which is what
 * persim's kernel_params["sigma"] holds), integrated over each pixel.
 *
 * Accuracy: for every pixel |values - exact| <= C(n) u sum_p w_p, with n the
 * diagram's finite points, u = 2^-53, the exact value that of the formulas above
 * on the float64 b_p, pi_p and edges, and
 *     C(n) = 2 E + 9 + n,    E = TDA_PI_ERF_ULP = 16.
 * Derivation (first order in u; every step rounds up, which covers the u^2 terms):
 *   1. the argument z = (edge - b) r is a rounded subtraction, r (a rounded
 *      constant and a rounded division) and a rounded product: a relative error of
 *      4 u, and |z erf'(z)| <= 0.49, so erf moves by at most 1.96 u <= 2 u;
 *   2. the device erf is within E ulp, and an ulp of a value below 1 is at most u:
 *      each erf value is within (2 + E) u of the exact one;
 *   3. g = (e1 - e0) / 2 adds half of two such errors each way and one rounding of
 *      a value <= 1: |g^ - g| <= (3 + E) u, with 0 <= g <= 1;
 *   4. a term w gx gy: the weight is within one ulp, at most 2 u w (the host's pow;
 *      exact for the powers 0 and 1), w gx is rounded once, the product with gy is
 *      exact inside the fused multiply-add: with gx, gy <= 1 the term is within
 *      (2 (3 + E) + 3) u w;
 *   5. the n terms are non-negative up to those errors and are added one by one,
 *      each addition rounding a partial sum that is at most the total: n u sum w.
 * E: the ROCm install documents no bound for the device erf (no table of ulp
 * errors ships with it), so E is the OpenCL conformance bound for double erf, 16
 * ulp, which the device math library is built to meet.  C is not fitted to
 * observed errors.
 *
 * Limits: TDA_VEC_MAX_POINTS as above, 1 <= W, H <= TDA_PI_MAX_PIXELS, S * W * H
 * <= TDA_VEC_MAX_OUT, else TDA_E_UNSUPPORTED.  Edges that are NULL, non-finite or
 * not strictly increasing, sigma not finite or <= 0, weight_power not finite or
 * < 0, W or H < 1, reserved != 0: TDA_E_INVALID, before any device work.
 *
 * Promised by both, bit for bit: a diagram's output is the same alone, among other
 * diagrams of any sizes (whatever size classes the call then holds), at any
 * position in the call and from run to run; the image's sum over p runs in the
 * order of the finite rows whatever the image shape's tiling.  An empty diagram
 * gives +0.0 everywhere.
 *
 * tda_heat_kernel: the persistence scale-space kernel (Reininghaus, Huber, Bauer, Kwitt
 * 2015) of P pairs out of S diagrams in one call, the kernel of every diagram with itself,
 * and the distance it induces (persim.heat(dgm1, dgm2, sigma) [upstream]).  For diagrams F
 * (n1 rows) and G (n2 rows), after dropping every row with a non-finite coordinate, and
 * sigma > 0:
 *     c8      = 1 / (8 sigma)                       host, one rounded division (8 sigma is exact)
 *     cn      = 1 / (8 pi sigma)                    host, the rounded constant 8 pi, one product, one division
 *     r2(p,q) = (b_p - b_q)^2 + (d_p - d_q)^2
 *     m2(p,q) = (b_p - d_q)^2 + (d_p - b_q)^2       q mirrored at the diagonal
 *     t(p,q)  = exp(-c8 r2(p,q)) - exp(-c8 m2(p,q))
 *     k(F,G)  = cn * sum_{p in F} sum_{q in G} t(p,q)
 *     heat(F,G) = sqrt(max(0, (k(F,F) + k(G,G)) - 2 k(F,G)))      exactly this order of float64 operations
 * Everything is float64.  r2 and m2 are two rounded subtractions, two rounded products and
 * one rounded addition each (no fused multiply-add), -c8 r2 is one rounded product.  An
 * empty diagram gives k = +0.0 against anything, two empty diagrams are at distance 0.0.
 * It is a kernel in the Hilbert-space sense: the Gram matrix of any list of diagrams is
 * positive semi-definite up to bound 3 below.
 *
 * The result: kern[P] = k of each pair, self[S] = k(F_s, F_s) of every diagram of the call
 * (the Gram matrix's diagonal), dist[P] = heat, formed on the host from kern and self.
 *
 * The order of the sum is a function of (n1, n2) alone.  Every pair is evaluated in one
 * canonical orientation (the diagram with more finite points is F and, at equal counts, the
 * one whose point array comes first lexicographically), and then, with R = 64 rows and
 * Q = 256 columns:
 *     part[rb][cc] = the rows p = 64 rb .. 64 rb + 63 (a row beyond n1 counts +0.0), each summed
 *                    over q = 256 cc .. min(256 cc + 255, n2 - 1) in that order, starting from
 *                    +0.0, then added pairwise over the row index: lanes l and l ^ 1, then
 *                    l ^ 2, l ^ 4, l ^ 8, l ^ 16, l ^ 32;
 *     sum          = with the parts numbered k = rb * ceil(n2 / 256) + cc: 64 partial sums, the
 *                    l-th over k = l, l + 64, ... in that order from +0.0, added pairwise in
 *                    the same way;
 *     k            = cn * sum                       one rounded product
 * whatever the launch shape and whatever else the call holds.
 *
 * What is promised, with u = 2^-53:
 *   1. bit for bit, symmetry and identity: k(F, G) == k(G, F) and heat(F, G) == heat(G, F);
 *      kern of a pair (s, s) == self[s], and so heat(F, F) is exactly 0.0;
 *   2. bit for bit, independence of the call: a pair's kern, a diagram's self and so dist are
 *      the same alone, among other pairs of any sizes, at any position in the pair list,
 *      with or without an explicit `pairs`, and from run to run;
 *   3. accuracy: |kern - exact| <= C(n1, n2) u cn, the exact value that of the formulas above
 *      on the float64 inputs, c8 and cn, n1 >= n2 the pair's two counts, and
 *          C(n1, n2) = n1 n2 (2 E + 8 + D(n1, n2)),    E = TDA_HK_EXP_ULP = 3,
 *          D(n1, n2) = min(n2, 256) + 12 + ceil(ceil(n1 / 64) ceil(n2 / 256) / 64);
 *      self[s] is within C(n, n) u cn.
 *      Derivation (first order in u; every step rounds up, which covers the u^2 terms):
 *        a. r2 (and m2): each difference carries a relative error u, its square 3 u, the sum
 *           of the two non-negative squares 4 u, the product with c8 5 u: the argument
 *           z = -c8 r2 has a relative error of at most 6 u;
 *        b. |z| e^z <= 1 / e, so the exponential moves by at most 6 u / e <= 3 u;
 *        c. the device exp is within E ulp, and an ulp of a value <= 1 is at most u: each
 *           exponential is within (3 + E) u of the exact one;
 *        d. a term t is the rounded difference of two such values, |t| <= 1: within
 *           (2 (3 + E) + 1) u = (2 E + 7) u; the n1 n2 terms together: (2 E + 7) n1 n2 u;
 *        e. the sum: an addition rounds a partial sum, which is at most the number of terms
 *           below it, so the additions together err by at most u times the sum, over the
 *           terms, of the number of additions a term passes through.  That number is at
 *           most D: min(n2, 256) in its row's chunk, 6 over the rows, ceil(parts / 64) over
 *           the parts of a lane and 6 over the lanes: D n1 n2 u;
 *        f. the product with cn rounds a value of at most n1 n2: n1 n2 u.
 *      E: the ROCm install documents no bound for the device's double exp (no table of ulp
 *      errors ships with it), so E is the OpenCL conformance bound for double exp, 3 ulp,
 *      which the device math library is built to meet (as TDA_PI_ERF_ULP was chosen).  C is
 *      not fitted to observed errors.
 *      The squared distance q = (k(F,F) + k(G,G)) - 2 k(F,G) before the clamp: within
 *          B2 = (C(n1, n1) + C(n2, n2) + 2 C(n1, n2)) u cn + 2 u (self_F + self_G + 2 |kern|)
 *      of the exact one (three bounds of kind 3, the doubling exact, and the two host
 *      roundings, each of a value of at most self_F + self_G + 2 |kern|).  dist is the correctly
 *      rounded square root of the clamped value, so |dist - exact| <= sqrt(B2) + u dist.
 *   4. not promised bit for bit: independence of the order of a diagram's rows.  Two row
 *      orders agree within bound 3.  What steps a to f derive for them: a term is a function
 *      of its two points alone, so both orders add the same n1 n2 terms, bit for bit, and
 *      differ by the roundings of steps e and f only, at most 2 (D + 1) n1 n2 u cn; that is
 *      below twice bound 3 but, D being at least 14, not below bound 3 itself.  Bound 3 is
 *      what the tests hold two row orders to, and it is the stricter of the two.
 *
 * Limits: at most TDA_HK_MAX_POINTS finite points per diagram, at most TDA_SW_MAX_WORK
 * diagrams and pairs per call, and at most TDA_SW_MAX_WORK parts (above) over the call's
 * P + S evaluations (the call's scratch, 8 bytes per part), else TDA_E_UNSUPPORTED.  TDA_E_INVALID, in this order: args NULL,
 * S < 0, offsets NULL, reserved != 0, sigma not finite, not > 0, or such that c8 or cn is
 * not a finite normal number, bad offsets, points NULL, P < 0; then TDA_E_UNSUPPORTED for
 * too many diagrams or pairs, TDA_E_INVALID for a pair index outside [0, S), and
 * TDA_E_UNSUPPORTED for a diagram beyond the point limit (whether a pair names it or not:
 * every diagram has a self) and for too many parts.  All argument errors arrive before any
 * device work.
 *
 * tda_persistence_fisher: the persistence Fisher distance (Le and Yamada 2018; gudhi's
 * PersistenceFisherDistance / PersistenceFisherKernel [upstream]) of P pairs out of S diagrams
 * in one call.  Both diagrams of a pair are smoothed into densities on a common support, and
 * the distance is the Fisher information (geodesic) distance between the two densities on the
 * sphere.  For diagrams F (n1 rows) and G (n2 rows), after dropping every row with a
 * non-finite coordinate, and sigma > 0:
 *     c2        = 1 / (2 sigma sigma)       host: one rounded product, an exact doubling, one rounded division
 *     pi(b, d)  = (m, m), m = (b + d) * 0.5      one rounded addition, the halving exact
 *     U         = F_0 .. F_{n1-1}, pi(G_0) .. pi(G_{n2-1})        M = n1 + n2 source points
 *     V         = G_0 .. G_{n2-1}, pi(F_0) .. pi(F_{n1-1})
 *     Z         = U then V                                         2 M evaluation points
 *     r2(z, w)  = (z.b - w.b)^2 + (z.d - w.d)^2    two rounded subtractions, two rounded products, one rounded addition
 *     e(z, w)   = +0.0 if -c2 r2 < -TDA_PF_CUT (= -708), else exp(-c2 r2)     -c2 r2 one rounded product
 *     rhoU(z)   = sum over w in U of e(z, w);   rhoV(z) likewise over V
 *     a = sum_z rhoU(z);   b = sum_z rhoV(z);   h = sum_z sqrt(rhoU(z) * rhoV(z))
 *     affinity  = min(1, h / sqrt(a * b))          host, this order
 *     fisher    = arccos(affinity)                 host (libm)
 * Everything is float64 and nothing is contracted to a fused multiply-add.  The product
 * rhoU(z) * rhoV(z) is rounded once and its square root is the correctly rounded one: the
 * device's __dsqrt_rn (IEEE round to nearest even).  exp(-708) = 3.3e-308 is a normal number,
 * so the cut keeps every term either +0.0 or normal.  The Gaussian's constant
 * 1 / (sigma sqrt(2 pi)) of the upstream formula cancels in the normalisation and is not
 * computed.  The kernel exp(-fisher / bandwidth) is formed by the caller.  Two empty diagrams
 * are at distance +0.0 (a = b = h = +0.0); one empty diagram is an ordinary case (U = F,
 * V = pi(F)).  The values are bounded by pi / 2.
 *
 * The result, per pair: a, b, h and dist = fisher, formed on the host from the three sums.
 * Every pair is evaluated in one canonical orientation (that of tda_heat_kernel: the diagram
 * with more finite points is F and, at equal counts, the one whose point array comes first
 * lexicographically); where that exchanged the two diagrams, a and b are exchanged back, so
 * that a belongs to the U of the pair's first diagram as the caller named it.  h and dist do
 * not depend on the naming.
 *
 * The order of the sums is a function of (n1, n2) alone, in the canonical orientation, with
 * L = TDA_PF_LANES = 64:
 *     rhoU(z), rhoV(z) = from +0.0, over the sources w = U_0 .. U_{M-1} (V_0 .. V_{M-1}) in that
 *                        order, one rounded addition per source (a term cut to +0.0 is added
 *                        like any other);
 *     part[k]          = for each of a, b and h: the values of z = 64 k .. 64 k + 63 (a z beyond
 *                        2 M counts +0.0), added pairwise over the lane index l = z - 64 k:
 *                        lanes l and l ^ 1, then l ^ 2, l ^ 4, l ^ 8, l ^ 16, l ^ 32;
 *     a, b, h          = the ceil(2 M / 64) <= 64 parts, part k in lane k (a lane without a part
 *                        counts +0.0), added pairwise in the same way
 * whatever the launch shape and whatever else the call holds.  The sources are staged
 * TDA_PF_CHUNK = 128 of U and of V at a time; the chunk does not enter the order.
 *
 * What is promised, with u = 2^-53:
 *   1. bit for bit, symmetry and identity: fisher(F, G) == fisher(G, F), h likewise, and
 *      a(F, G) == b(G, F); fisher(F, F) is exactly +0.0 for two diagrams with the same finite
 *      rows, named by one index or by two.  Why: with F = G the sequences U and V hold the
 *      same bits in the same order, so rhoU(z) == rhoV(z) =: x at every z, with x in [1, 2 M]
 *      (the term e(z, z) is exp(-0.0) = 1).  For a binary format and a correctly rounded
 *      square root, sqrt(fl(x x)) == x when nothing over- or underflows, so every h term is the
 *      a term and the b term, the three sums run in one order, and h == a == b.  On the host
 *      sqrt(fl(a a)) == a for the same reason, the quotient is 1 and arccos(1) is +0.0;
 *   2. bit for bit, independence of the call: a pair's a, b, h and dist are the same alone,
 *      among other pairs of any sizes, at any position in the pair list, with or without an
 *      explicit `pairs`, and from run to run;
 *   3. accuracy: |affinity - exact| <= B(n1, n2), the exact value that of the formulas above
 *      (the cut included) on the float64 inputs and c2, and
 *          T         = 6 TDA_PF_CUT + 2 E + 2 = 4256,       E = TDA_PF_EXP_ULP = 3,
 *          R(n1, n2) = T + (n1 + n2),
 *          B(n1, n2) = (2 R(n1, n2) + 30) u + 3 (n1 + n2) 2^-510.
 *      Derivation (first order in u; every step rounds up, which covers the u^2 terms):
 *        a. the argument: each difference carries a relative error u, its square 3 u, the sum
 *           of the two non-negative squares 4 u, the product with c2 5 u: t = -c2 r2 has a
 *           relative error of at most 6 u.  A term that is kept has |t| <= 708, so
 *           exp(t) moves by a factor within 1 +- 6 * 708 u;
 *        b. the device exp is within E ulp, and an ulp is at most 2 u of the value: a kept term
 *           is within a relative T u of the exact one (the + 2 for the second order);
 *        c. a term whose exact argument lies within rounding of -708 may appear or vanish:
 *           an additive error of at most exp(-708 (1 - 6 u)) <= 2^-1021 per term, M 2^-1021 per
 *           density.  It is carried separately (step f);
 *        d. a density is a sum of M non-negative terms in series, M - 1 additions: a relative
 *           M u.  So rhoU and rhoV are within a relative R u of the exact ones (and step c);
 *        e. sqrt(rhoU rhoV): one rounded product, one correctly rounded root:
 *           (R + R + 1) / 2 + 1 <= R + 2 relative.  Every z lies in U or in V, so one of the
 *           two densities holds the term e(z, z) = 1: the product is at least 3.3e-308 or is
 *           +0.0, never subnormal;
 *        f. step c under the root: at a z of U, rhoU >= 1 takes it as a relative error far below
 *           u^2, and sqrt(rhoU (rhoV + d)) - sqrt(rhoU rhoV) <= sqrt(rhoU d) <= sqrt(2 M M 2^-1021);
 *           over the 2 M values of z: at most 3 M^2 2^-510 added to h;
 *        g. a, b and h are sums of non-negative values through 6 + 6 pairwise additions:
 *           a and b within R + 12, h within R + 14 relative;
 *        h. the host: a b rounded, its root, the quotient: the denominator within
 *           ((R + 12) + (R + 12) + 1) / 2 + 1 <= R + 14.5, the quotient within
 *           (R + 14) + (R + 14.5) + 1 <= 2 R + 30, relative to an exact value of at most 1
 *           (Cauchy-Schwarz); min(1, .) moves nothing away from it.  Step f divided by
 *           sqrt(a b) >= M: 3 M 2^-510.
 *      E is the OpenCL conformance bound for double exp, as TDA_HK_EXP_ULP and for the same
 *      reason.  B is not fitted to observed errors; at sigma where no argument comes near the
 *      cut it is loose by the factor 6 * 708 of step a.  The largest share of B seen in the
 *      tests is 2.3e-4 (one ulp of the affinity).
 *      The distance: with A the affinity computed,
 *          |fisher - exact| <= arccos(max(-1, A - B)) - arccos(min(1, A + B)) + 4 u
 *      (arccos is decreasing, the exact affinity lies in [A - B, A + B], and 4 u covers the
 *      library arccos, which is taken to be within one ulp of a value of at most pi / 2).
 *      This is loose near A = 1, as any such distance is: about sqrt(2 B) at A = 1.
 *   4. not promised bit for bit: independence of the order of a diagram's rows.  A term is a
 *      function of its two points alone, so two row orders add the same terms, bit for bit, and
 *      differ by the roundings of steps d, e, g and h only: at most 2 (2 M + 30) u, which is
 *      below B as long as 2 M + 30 <= 2 T, that is for every M the entry accepts.  B is what
 *      the tests hold two row orders to.
 *
 * Limits: at most TDA_PF_MAX_POINTS = 1024 finite points in a diagram that a pair names (no
 * self is evaluated, so a larger diagram that no pair names is accepted), at most
 * TDA_SW_MAX_WORK diagrams and pairs per call, and at most TDA_SW_MAX_WORK parts (above) over
 * the call's pairs (the call's scratch, 24 bytes per part), else TDA_E_UNSUPPORTED.
 * TDA_E_INVALID, in this order: args NULL, S < 0, offsets NULL, reserved != 0, sigma not
 * finite, not > 0, or such that c2 is not a finite normal number, bad offsets, points NULL,
 * P < 0; then TDA_E_UNSUPPORTED for too many diagrams or pairs, TDA_E_INVALID for a pair index
 * outside [0, S), and TDA_E_UNSUPPORTED for a named diagram beyond the point limit and for too
 * many parts.  All argument errors arrive before any device work.  Coordinates so large that
 * b + d overflows are outside the definition (pi(p) is then infinite and a density may be NaN).
 *
 * tda_persistence_curve: persistence curves (Chung and Lawson 2019) of S diagrams on a grid, in
 * one call: the Betti curve, the lifespan curve, the entropy summary function (Atienza,
 * Gonzalez-Diaz, Soriano-Trigueros 2020), the silhouette (Chazal et al. 2014) and any other sum of
 * one term per point.  For a diagram A, a coefficient c_p per row and a grid value t:
 *     K_p(t) = 1 where b_p <= t and t < d_p, else 0                 TDA_PC_INDICATOR
 *     K_p(t) = max(0, min(t - b_p, d_p - t))                       TDA_PC_TENT (the landscape's tent)
 *     acc    = +0.0; for p in row order: if K_p(t) > 0: acc = acc + (c_p * K_p(t))
 *     values[s][g] = acc                                           at t = grid[g]
 * Everything is float64.  The tent is one rounded subtraction, the product is rounded and the sum
 * is rounded (no fused multiply-add); a point outside its support adds nothing, not even a zero.
 * With coef == NULL every c_p is 1 and the term is K_p(t) itself (no product).  So every value
 * equals a numpy restatement bit for bit.
 *
 * Rows kept: those with a finite b and a finite d.  The indicator with TDA_PC_KEEP_ESSENTIAL also
 * keeps the rows with a finite b and d = +inf (a Betti number counts the essential classes, and
 * t < +inf needs no arithmetic); the flag with the tent is TDA_E_INVALID.  Every other row is
 * dropped with its coefficient.
 *
 * With TDA_PC_NORMALIZE, values[s][g] = acc / W_s: W_s the sum of the kept c_p in row order from
 * +0.0 (the number n of kept rows when coef is NULL), one rounded division; a quotient that is a
 * zero of either sign is +0.0, and a diagram with W_s == 0 or without a kept row is +0.0
 * everywhere.  No value is -0.0, with or without the flag.
 *
 * Promised bit for bit: a value depends on its diagram, its grid value, kernel and flags alone --
 * not on the other diagrams, the diagram's place in the call, the grid value's place in the grid,
 * a size class or the launch shape -- and is the same from run to run.  grid holds G finite values
 * in any order.
 *
 * Limits: at most TDA_VEC_MAX_POINTS kept rows per diagram, G <= TDA_PL_MAX_STEPS, S * G <=
 * TDA_VEC_MAX_OUT and S <= TDA_SW_MAX_WORK, else TDA_E_UNSUPPORTED.  The checks, in this order:
 * args NULL, reserved != 0, an unknown kernel, an unknown bit of flags, TDA_PC_KEEP_ESSENTIAL with
 * the tent, G < 1, grid NULL (TDA_E_INVALID), G > TDA_PL_MAX_STEPS (TDA_E_UNSUPPORTED), a
 * non-finite grid value, S < 0, offsets NULL, bad offsets, points NULL (TDA_E_INVALID), too many
 * diagrams (TDA_E_UNSUPPORTED), a non-finite coefficient on a kept row (TDA_E_INVALID), a diagram
 * beyond the point limit, S * G beyond the output limit (TDA_E_UNSUPPORTED).  All argument errors
 * arrive before any device work.
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

#define TDA_VEC_MAX_POINTS 4096     /* finite points of one diagram          */
#define TDA_VEC_MAX_OUT (1ll << 24) /* doubles of one call's result, S * F   */
#define TDA_PL_MAX_DEPTH 64
#define TDA_PL_MAX_STEPS 4096
#define TDA_PI_MAX_PIXELS 256       /* per axis                              */
#define TDA_PI_ERF_ULP 16           /* E of the accuracy bound C(n)          */

typedef struct tda_pl_args {
    const double *points;   /* host (total, 2) f64 (birth, death); non-finite rows are skipped */
    const int64_t *offsets; /* host [S + 1] non-decreasing row boundaries, offsets[0] = 0      */
    int64_t S;              /* diagrams                                                        */
    const double *grid;     /* host [G] finite grid values, any order                          */
    int32_t G;              /* 1 .. TDA_PL_MAX_STEPS                                           */
    int32_t K;              /* depth, 1 .. TDA_PL_MAX_DEPTH                                    */
    int32_t device;         /* HIP device ordinal                                              */
    int32_t reserved;       /* must be 0                                                       */
} tda_pl_args;

typedef struct tda_pl_result {
    int64_t S;            /* diagrams                                              */
    int64_t F;            /* values per diagram, K * G                             */
    const double *values; /* host [S][K][G]                                        */
    double device_ms;     /* device time of the call (HIP events, copies included) */
} tda_pl_result;

int tda_landscape(const tda_pl_args *args, tda_pl_result **out);
void tda_pl_free(tda_pl_result *r);

typedef struct tda_pi_args {
    const double *points;   /* host (total, 2) f64 (birth, death); non-finite rows are skipped */
    const int64_t *offsets; /* host [S + 1] non-decreasing row boundaries, offsets[0] = 0      */
    int64_t S;              /* diagrams                                                        */
    const double *x_edges;  /* host [W + 1] finite, strictly increasing: the birth axis        */
    const double *y_edges;  /* host [H + 1] finite, strictly increasing: the persistence axis  */
    int32_t W, H;           /* pixels per axis, 1 .. TDA_PI_MAX_PIXELS                         */
    double sigma;           /* finite, > 0                                                     */
    double weight_power;    /* finite, >= 0                                                    */
    int32_t device;         /* HIP device ordinal                                              */
    int32_t reserved;       /* must be 0                                                       */
} tda_pi_args;

typedef struct tda_pi_result {
    int64_t S;            /* diagrams                                              */
    int64_t F;            /* values per diagram, W * H                             */
    const double *values; /* host [S][W][H]                                        */
    double device_ms;     /* device time of the call (HIP events, copies included) */
} tda_pi_result;

int tda_persistence_image(const tda_pi_args *args, tda_pi_result **out);
void tda_pi_free(tda_pi_result *r);

#define TDA_PC_INDICATOR 0      /* kernel: 1 on [b, d)                              */
#define TDA_PC_TENT 1           /* kernel: max(0, min(t - b, d - t))                */
#define TDA_PC_NORMALIZE 1      /* flags: divide by the sum of the coefficients     */
#define TDA_PC_KEEP_ESSENTIAL 2 /* flags: keep (finite b, +inf) rows; indicator only */

typedef struct tda_pc_args {
    const double *points;   /* host (total, 2) f64 (birth, death); see "Rows kept"                    */
    const int64_t *offsets; /* host [S + 1] non-decreasing row boundaries, offsets[0] = 0             */
    int64_t S;              /* diagrams                                                               */
    const double *coef;     /* host [total] f64, one per row of points, or NULL: every c_p = 1        */
    const double *grid;     /* host [G] finite grid values, any order                                 */
    int32_t G;              /* 1 .. TDA_PL_MAX_STEPS                                                  */
    int32_t kernel;         /* TDA_PC_INDICATOR or TDA_PC_TENT                                        */
    int32_t flags;          /* 0 or TDA_PC_NORMALIZE | TDA_PC_KEEP_ESSENTIAL                          */
    int32_t device;         /* HIP device ordinal                                                     */
    int32_t reserved;       /* must be 0                                                              */
} tda_pc_args;

typedef struct tda_pc_result {
    int64_t S;            /* diagrams                                              */
    int64_t F;            /* values per diagram, G                                 */
    const double *values; /* host [S][G]                                           */
    double device_ms;     /* device time of the call (HIP events, copies included) */
} tda_pc_result;

int tda_persistence_curve(const tda_pc_args *args, tda_pc_result **out);
void tda_pc_free(tda_pc_result *r);

#define TDA_HK_MAX_POINTS 4096 /* finite points of one diagram   */
#define TDA_HK_EXP_ULP 3       /* E of the accuracy bound C(n1, n2) */

typedef struct tda_hk_args {
    const double *points;   /* host (total, 2) f64 (birth, death); non-finite rows are skipped */
    const int64_t *offsets; /* host [S + 1] non-decreasing row boundaries, offsets[0] = 0      */
    int64_t S;              /* diagrams                                                        */
    const int32_t *pairs;   /* host (P, 2) diagram indices, or NULL: every i < j, row-major    */
    int64_t P;              /* pairs in `pairs`; ignored when pairs is NULL                    */
    double sigma;           /* finite, > 0, 1 / (8 sigma) and 1 / (8 pi sigma) finite normal   */
    int32_t device;         /* HIP device ordinal                                              */
    int32_t reserved;       /* must be 0                                                       */
} tda_hk_args;

typedef struct tda_hk_result {
    int64_t P;          /* pairs computed (S (S - 1) / 2 when pairs was NULL)    */
    const double *kern; /* host [P]: k of each pair                              */
    const double *self; /* host [S]: k(F_s, F_s) of every diagram of the call    */
    const double *dist; /* host [P]: heat of each pair                           */
    double device_ms;   /* device time of the call (HIP events, copies included) */
} tda_hk_result;

int tda_heat_kernel(const tda_hk_args *args, tda_hk_result **out);
void tda_hk_free(tda_hk_result *r);

#define TDA_PF_MAX_POINTS 1024 /* finite points of a diagram that a pair names          */
#define TDA_PF_EXP_ULP 3       /* E of the accuracy bound B(n1, n2)                      */
#define TDA_PF_CUT 708         /* a term whose argument is below -708 is +0.0            */
#define TDA_PF_LANES 64        /* evaluation points of a part: enters the order of sums  */
#define TDA_PF_CHUNK 128       /* sources staged at a time: does not enter the order     */

typedef struct tda_pf_args {
    const double *points;   /* host (total, 2) f64 (birth, death); non-finite rows are skipped */
    const int64_t *offsets; /* host [S + 1] non-decreasing row boundaries, offsets[0] = 0      */
    int64_t S;              /* diagrams                                                        */
    const int32_t *pairs;   /* host (P, 2) diagram indices, or NULL: every i < j, row-major    */
    int64_t P;              /* pairs in `pairs`; ignored when pairs is NULL                    */
    double sigma;           /* finite, > 0, 1 / (2 sigma^2) a finite normal number             */
    int32_t device;         /* HIP device ordinal                                              */
    int32_t reserved;       /* must be 0                                                       */
} tda_pf_args;

typedef struct tda_pf_result {
    int64_t P;          /* pairs computed (S (S - 1) / 2 when pairs was NULL)          */
    const double *a;    /* host [P]: sum_z rhoU(z), U that of the pair's first diagram  */
    const double *b;    /* host [P]: sum_z rhoV(z)                                      */
    const double *h;    /* host [P]: sum_z sqrt(rhoU(z) rhoV(z))                        */
    const double *dist; /* host [P]: fisher of each pair                                */
    double device_ms;   /* device time of the call (HIP events, copies included)       */
} tda_pf_result;

int tda_persistence_fisher(const tda_pf_args *args, tda_pf_result **out);
void tda_persistence_fisher_free(tda_pf_result *r);

/* The Frechet mean (2-Wasserstein barycenter; Turner, Mileyko, Mukherjee, Harer 2014) of S diagrams:
 * the argument struct and the limits of an entry that is NOT in the library yet
 * (DESIGN.md section 7).  What exists is its host plan, csrc/fm_plan.h (the argument checks in the
 * order below, the finite points, the start, the launch class of a step), and the CPU restatement of
 * the definition, tests/fm_ref.py.  Neither a result struct nor a function is declared here until
 * the device side ships.
 *     F(Y)       = (1 / S) sum_j W2^2(Y, X_j)
 *     W2^2(Y, X) = min over partial matchings of the sum of the costs paid
 *     c(p, q)    = db db + dd dd,   c(p) = (pers pers) 0.5      each operation rounded on its own
 * A step matches Y against every X_j, replaces every y that has k >= 1 partners (taken in increasing
 * j, sums left to right from the first partner) by ((k mb + (S - k) w) / S, (k md + (S - k) w) / S)
 * with mb = sb / k, md = sd / k, w = (mb + md) 0.5, drops a y without a partner, and appends, for j
 * and within j for i increasing, that update (k = 1) of every point of X_j no y took.  The iteration
 * ends when a step returns its input bit for bit, or after max_iter steps.
 * The plan's checks, in this order: args NULL, S < 0, offsets NULL, reserved != 0, an unknown bit of
 * flags, max_iter < 1 (TDA_E_INVALID), max_iter > TDA_FM_MAX_ITER (TDA_E_UNSUPPORTED), S < 1
 * (TDA_E_INVALID), S > TDA_FM_MAX_DIAGRAMS (TDA_E_UNSUPPORTED), the layout of offsets and points,
 * init_index outside {-1} u [0, S), init_n < 0 or init_points NULL (TDA_E_INVALID), then a diagram
 * or a start with more than TDA_FM_MAX_POINTS finite points (TDA_E_UNSUPPORTED). */
#define TDA_FM_MAX_POINTS 512    /* finite points of one diagram and of Y at every step (= TDA_WS_MAX_POINTS) */
#define TDA_FM_MAX_DIAGRAMS 4096 /* S at most                                                                 */
#define TDA_FM_MAX_ITER 1024     /* max_iter at most                                                          */
#define TDA_FM_WANT_MATCHING 1

typedef struct tda_fm_args {
    const double *points;      /* host (total, 2) f64 (birth, death); non-finite rows are skipped     */
    const int64_t *offsets;    /* host [S + 1] non-decreasing row boundaries, offsets[0] = 0          */
    int64_t S;                 /* diagrams, 1 .. TDA_FM_MAX_DIAGRAMS                                  */
    int64_t init_index;        /* Y_0 = the finite points of diagram init_index, or -1: init_points   */
    const double *init_points; /* host (init_n, 2) f64: the caller's start (init_index == -1)         */
    int64_t init_n;            /* its rows, >= 0; non-finite rows are skipped                         */
    int32_t max_iter;          /* steps at most, 1 .. TDA_FM_MAX_ITER                                 */
    int32_t device;            /* HIP device ordinal                                                  */
    int32_t flags;             /* 0 or TDA_FM_WANT_MATCHING                                           */
    int32_t reserved;          /* must be 0                                                           */
} tda_fm_args;

#ifdef __cplusplus
}
#endif
#endif
