"""The sizes at which a persistence call changes its kernels, and the clouds run on both sides of them.

HIP-free (numpy only).  Two files import it:

* tests/test_rips_plan_cpu.py checks PLAN_BORDERS against the host plan program: the plan of
  (L = 1, N, D = 3, maxdim = 2) changes in the fields below at exactly these N and takes these values
  at N - 1 and at N;
* tests/test_size_borders.py runs the kernels at the sizes that follow from it (DENSE_NS,
  FORCED_CHAIN_NS) and at the borders of the enqueue code, and compares with the oracle.

So a constant that moves (kChainKs, kChainFastMaxK, kLdsMax, kP1MaxWaves in csrc/rips_shapes.h)
fails the CPU test, which prints where the plan changes now: move PLAN_BORDERS there, and the GPU
cases follow.
"""
import numpy as np

CHAIN_GENERAL, CHAIN_FAST, CHAIN_TABLE = 0, 1, 2  # csrc/rips_shapes.h: k_h1_chain's MODE
K_LDS_MAX = 160 * 1024

# the fields of a Plan the borders are read from (tests/rips_plan_main.cpp prints them by these names)
PLAN_FIELDS = ("dense", "dK", "cmode", "p1_waves", "par", "par2", "wide", "packed")
# (first N of the new plan, {field: (value at N - 1, value at N)}): every N in 3 .. PLAN_SCAN_MAX at
# which one of PLAN_FIELDS changes, with the fields that change -- and, where it is the LDS size that
# decides, that size (chain_lds, p1_lds: bytes, not part of the scan)
PLAN_BORDERS = (
    (3, {"dense": (0, 1), "dK": (0, 1), "cmode": (CHAIN_GENERAL, CHAIN_TABLE), "p1_waves": (1, 2)}),
    (25, {"dK": (1, 2)}),
    (31, {"dK": (2, 3)}),
    (35, {"dK": (3, 4)}),
    (38, {"dK": (4, 6)}),
    (43, {"dK": (6, 9)}),
    # K = 12: the coboundary table no longer fits (it would at K = 9: 161,856 bytes at N = 49), FAST by default
    (50, {"dK": (9, 12), "cmode": (CHAIN_TABLE, CHAIN_FAST), "chain_lds": (161856, 141344)}),
    # the rank tables no longer fit either (FAST would need 166,064 bytes): GENERAL
    (53, {"cmode": (CHAIN_FAST, CHAIN_GENERAL), "chain_lds": (157488, 94384)}),
    (54, {"dK": (12, 16)}),
    (60, {"dK": (16, 21), "p1_lds": (151104, 159920)}),  # the last N with two waves in k_h2_phase1, 3,920 bytes below the limit
    (61, {"p1_waves": (2, 1), "p1_lds": (159920, 95808)}),
    # off the dense path: k_reduce_par for H1 and H2
    (65, {"dense": (1, 0), "dK": (21, 0), "par": (0, 1), "par2": (0, 1)}),
    (569, {"wide": (0, 1)}),     # C(N, 4) >= 2^32: edge-code H2 keys
    (1025, {"packed": (1, 0)}),  # k_reduce_par keys without packed vertices
)
PLAN_SCAN_MAX = 1100
P1_TWO_WAVES_AT_61 = 169248  # what two waves of k_h2_phase1 would need at N = 61: above K_LDS_MAX


def plan_below(border):
    """The PLAN_FIELDS values of the plan at N = border - 1, read off PLAN_BORDERS."""
    state = {k: v[0] for k, v in PLAN_BORDERS[0][1].items()}
    state.update(par=0, par2=0, wide=0, packed=1)
    for n, f in PLAN_BORDERS:
        if n >= border:
            break
        state.update({k: v[1] for k, v in f.items() if k in PLAN_FIELDS})
    return state


_dense = [(n, f) for n, f in PLAN_BORDERS if 24 < n <= 65]
# both sides of every border of the dense path
DENSE_NS = tuple(sorted({m for n, _ in _dense for m in (n - 1, n)}))
# the top N of each (K, mode) class whose default is TABLE or FAST: TDA_CHAIN=fast / general force another variant there
FORCED_CHAIN_NS = tuple(n - 1 for n, f in _dense if ("dK" in f or "cmode" in f) and plan_below(n)["cmode"] != CHAIN_GENERAL)
# the last N with two waves by default: what TDA_P1_WAVES=1 makes of the plan there is held on the CPU only
# (the graph key does not carry the waves, so a GPU case could replay the default's graph)
P1_NS = tuple(n - 1 for n, f in _dense if f.get("p1_waves") == (2, 1))
DENSE_L = 4

# ---- the enqueue code's own borders (csrc/rips_enqueue.h), which no Plan field shows
L_BORDER_N, L_BORDERS = 25, (16, 17, 64, 65)  # c.order 5 / 2 / 3, k_prep_tables blocks per layer, grids divided by L
# 128/129 k_apparent's LDS staging and the tile kernel; 190/191 one-wave Prim / Borůvka; 256/257 H0 block size, wcap_g
MID_NS, MID_L = (128, 129, 190, 191, 256, 257), 2
# (N, thresh): wide H2 keys from 569, unpacked k_reduce_par keys from 1025; one torus(N, seed 0) layer.
# The oracle (one core) on it, measured when the thresholds were chosen:
BIG_CASES = (
    (568, 2.0),   # 0.88 s; 39,844 of 161,028 edges; pairs 567 / 39,277 / 1,161,594; column additions 5,627 (H1), 7,323 (H2)
    (569, 2.0),   # 0.83 s; 40,041 of 161,596 edges; pairs 568 / 39,473 / 1,172,856; column additions 5,530, 8,193
    (1024, 1.4),  # 1.11 s; 50,231 of 523,776 edges; pairs 1,023 / 49,206 / 995,300; column additions 8,110, 2,656
    (1025, 1.4),  # 0.93 s; 50,501 of 524,800 edges; pairs 1,024 / 49,475 / 1,020,080; column additions 9,123, 2,557
)


# ---- clouds
def normal_cloud(n, seed):
    return np.random.default_rng(seed).standard_normal((n, 3)).astype(np.float32)


def tie_cloud(n, seed):
    """Small integer coordinates: many equal edge lengths (and equal points: 64 lattice sites)."""
    return np.random.default_rng(seed).integers(0, 4, (n, 3)).astype(np.float32)


def dense_layers(n):
    """[(generator name, seed)] of the four layers at N = n: two normal clouds, two tie-heavy ones.
    The seeds are the first from 1000 n on for which the oracle both pairs columns and adds columns
    in H1 and in H2 (n_all_pairs > 0, n_adds > 0): at N = 24 normal seeds 24000 and 24002 add none in H2."""
    normal = (24001, 24003) if n == 24 else (1000 * n, 1000 * n + 1)
    return [("normal_cloud", s) for s in normal] + [("tie_cloud", s) for s in (1000 * n, 1000 * n + 1)]


# layer l of an L-border call: normal (l even) / tie-heavy (l odd) cloud of L_BORDER_N points with this
# seed; chosen from 25500 on by the same rule as above
L_SEEDS = (25500, 25501, 25502, 25503, 25504, 25505, 25507, 25508, 25509, 25510, 25511, 25512, 25513, 25514, 25515, 25516, 25517, 25518,
           25521, 25522, 25523, 25524, 25526, 25527, 25528, 25529, 25531, 25532, 25533, 25534, 25535, 25536, 25537, 25538, 25539, 25540,
           25541, 25542, 25543, 25544, 25546, 25547, 25548, 25549, 25550, 25551, 25553, 25554, 25555, 25556, 25558, 25559, 25560, 25561,
           25562, 25563, 25564, 25565, 25566, 25567, 25568, 25569, 25570, 25571, 25572)


def l_border_layers(L):
    return [(("normal_cloud", "tie_cloud")[l & 1], L_SEEDS[l]) for l in range(L)]


def mid_layers(n):
    """A torus (synthetic.torus(n, seed 0)) and a normal cloud.  No H1 or H2 class of theirs lives longer
    than MID_MAX_LIFE of the threshold (the GPU file asserts it of the oracle's diagrams), below the
    column caps' 0.5: no cap-miss re-run."""
    return [("torus", 0), ("normal_cloud", 1000 * n + 2)]


MID_MAX_LIFE = 0.32  # the longest: 0.3125 of the threshold, on the torus at N = 256
