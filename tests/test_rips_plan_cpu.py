"""The host plan of a persistence call (csrc/rips_plan.h, make_plan) on the CPU.

tests/rips_plan_main.cpp includes only rips_plan.h; it is compiled with g++ under the address and
undefined-behaviour sanitizers and run as a program of its own, once per environment.  Three checks:

* the pin: the plans of PIN_CASES reproduce tests/golden/rips_plan.txt byte for byte.  The file was
  recorded by this program when make_plan had just been moved out of rips.hip, bodies untouched.
  To record it again: python tests/test_rips_plan_cpu.py | <the program> > tests/golden/rips_plan.txt
* invariants of every plan (alignment, regions that do not overlap, LDS sizes, reducer selection),
  from sizes restated here, for the pin's cases and for random shapes;
* a test knob forces the field it is named for at the shapes where the GPU tests set it, and
  changes nothing without TDA_TEST_OVERRIDES=1;
* the knobs of tests/test_retry_paths.py: TDA_PAR_POOL_SHIFT changes the four pool capacities of
  k_reduce_par (their growing parts only) and the offsets behind them, nothing else;
  TDA_PAR_STEPS_H1 / _H2 set the step limit of one k_reduce_par launch and leave step_limit() alone;
* the size borders of tests/size_borders.py, which tests/test_size_borders.py runs on a device: the
  plan changes kernel, instantiation, LDS layout or key format at exactly the N listed there (the
  dense borders are in this test and not in the pin's NS: the pin would outgrow its size rule);
* the H0 shape (h0_shape: block size, LDS carves, sort chunk, Borůvka rounds, elder-rule variant) of every
  N = 65 .. 8192 against tests/large_n.py, which tests/test_large_n.py runs on a device, and the dynamic LDS
  of k_h0, k_bor_hook, k_twonn and k_silhouette against their limits at every N.
"""
import math
import os
import random
import subprocess
import sys

import pytest

import large_n as ln
import size_borders as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tda-multimodal_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "rips_plan.txt")

F32, F64 = 0, 1
K_LDS_MAX, K_DENSE_MAX_N = 160 * 1024, 64
CHAIN_KS = (1, 2, 3, 4, 6, 9, 12, 16, 21)
SIZEOF = {"Pair": 24, "LayerStats": 608, "BorCtl": 16, "ParCtl": 128}
NS = (1, 2, 3, 8, 24, 64, 65, 144, 145, 190, 191, 256, 257, 568, 569, 1024, 1025, 2048)


def case(L, N, D=3, maxdim=1, dtype=F32, is_dist=0, want64=0, force_global=0, scale=0, force_big=0, no_par=0):
    return (L, N, D, maxdim, dtype, is_dist, want64, force_global, scale, force_big, no_par)


def pin_cases():
    """The cross product of the pin, thinned: every N at every maxdim for L = 1 and 32; the other axes at a few N each."""
    cs = [case(L, n, maxdim=md) for L in (1, 32) for md in (0, 1, 2) for n in NS]
    cs += [case(L, n, D, 1, dt) for L, n in ((1, 8), (32, 144), (1, 145), (32, 1024)) for D in (32, 4096) for dt in (F32, F64)]
    cs += [case(1, n, n, 2, dt, is_dist=1) for n in (8, 65, 257) for dt in (F32, F64)]
    cs += [case(L, n, D, 1, F64, want64=1) for L, n, D in ((1, 24, 3), (32, 24, 32), (1, 145, 3), (32, 145, 4096))]
    cs += [case(L, n, maxdim=2, scale=s) for L, n in ((32, 64), (1, 256), (1, 1025)) for s in (1, 2, 3, 4)]
    cs += [case(L, n, maxdim=md, force_global=1) for L, n in ((32, 8), (1, 64)) for md in (1, 2)]
    cs += [case(1, n, maxdim=md, force_global=1, force_big=1, scale=s) for n, s in ((64, 0), (65, 1), (256, 2)) for md in (1, 2)]
    cs += [case(L, n, maxdim=2, no_par=k) for L, n in ((32, 65), (1, 257), (1, 569)) for k in (1, 2)]
    cs += [case(1, 2048, maxdim=2, scale=4, no_par=1)]
    return cs


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rips_plan") / "rips_plan")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, "-o", out, os.path.join(ROOT, "tests", "rips_plan_main.cpp")], check=True)
    return out


def run_text(exe, cases, knobs=None, gate=True):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TDA_")}
    env.update(knobs or {})
    if gate:
        env["TDA_TEST_OVERRIDES"] = "1"
    text = "".join(" ".join(map(str, c)) + "\n" for c in cases)
    return subprocess.run([exe], input=text, capture_output=True, text=True, check=True, env=env).stdout


def parse(text, n_cases):
    """-> (sizes of the first line, one dict per case: name -> int or list of ints)"""
    blocks = text.split("\ncase ")
    head = dict((k, int(v)) for k, v in (t.split("=") for t in blocks[0].split()[1:]))
    plans = []
    for b in blocks[1:]:
        p = {}
        for tok in b.split("\n", 1)[1].split():
            if "=" in tok:
                k, v = tok.split("=")
                p[k] = [int(x) for x in v.split(",")] if "," in v else int(v)
        plans.append(p)
    assert len(plans) == n_cases
    return head, plans


def plans_of(exe, cases, knobs=None, gate=True):
    return parse(run_text(exe, cases, knobs, gate), len(cases))[1]


def test_pin(exe):
    got = run_text(exe, pin_cases())
    with open(GOLDEN) as f:
        assert got == f.read()
    assert os.path.getsize(GOLDEN) <= max(os.path.getsize(os.path.join(os.path.dirname(GOLDEN), f)) for f in os.listdir(os.path.dirname(GOLDEN))
                                          if f != "rips_plan.txt")


def test_pin_holds_every_boundary():
    cs = pin_cases()
    for md in (0, 1, 2):
        assert {c[1] for c in cs if c[3] == md} >= set(NS)
    assert {c[0] for c in cs} == {1, 32} and {c[2] for c in cs} >= {3, 32, 4096} and {c[4] for c in cs} == {F32, F64}
    assert {c[8] for c in cs} == {0, 1, 2, 3, 4} and {c[10] for c in cs} == {0, 1, 2}
    assert any(c[5] for c in cs) and any(c[6] for c in cs) and any(c[7] for c in cs) and any(c[9] for c in cs)
    assert case(32, 2048, maxdim=2) in cs  # the sparse pivot bitmap, far above 2 GB


def region_sizes(c, p):
    """Bytes of the regions whose size follows from the printed capacities (restated, not read from make_plan)."""
    L, N, D, maxdim, dtype, is_dist = c[:6]
    S = SIZEOF
    sz = {
        "o_x": L * N * (N if is_dist else max(D, 1)) * (8 if dtype == F64 else 4),
        "o_gpart": L * p["dist.dsplit"] * N * N * 8, "o_npart": L * p["dist.dsplit"] * N * 8,
        "o_dist": L * N * N * 4, "o_d64": L * N * N * 8, "o_rowmax": L * N * 4,
        "o_stats": L * S["LayerStats"], "o_mst": L * p["mst_words"] * 4,
        "o_p1used": L * 8, "o_p1next": L * 4, "o_res1": L * p["piv_words"][1] * 4, "o_necnt": L * 4, "o_clr2": L * p["clr_cap"] * 8,
        "o_tmp": L * 2 * p["max_rcap"] * 8, "o_rmk": L * 2 * p["rmap_stride"] * 8, "o_rmv": L * 2 * p["rmap_stride"] * 4,
        "o_vlen": L * p["max_rcap"] * 4, "o_vpool": L * p["vpool_cap"] * 8, "o_voff": L * p["max_rcap"] * 8,
        "o_h0s": L * 2 * N * 8 + 64, "o_bcomp": L * N * 4, "o_bcheap": L * N * 8, "o_bctl": L * S["BorCtl"],
        "o_fk": L * 2 * p["sstride"] * 8, "o_fv": L * 2 * p["sstride"] * 4, "o_pptr": 32, "o_pcap": 32, "o_outoff": L * 32,
        "o_pctl": S["ParCtl"], "o_pitem": (L + 1) * 8, "o_pokey": L * p["ostride"] * 8, "o_poval": L * p["ostride"] * 8,
        "o_prec": p["rec_cap"] * 32, "o_prpool": p["rpool_cap"] * 8, "o_pbpool": p["bpool_cap"] * 8, "o_prq": p["rq_cap"] * 8,
        "o_dsort": L * p["ecap"] * 8, "o_dtmp": L * p["ecap"] * 8, "o_dcode": L * N * N * 4,
    }
    for d in range(1, maxdim + 1):
        sz["o_piv%d" % d] = L * p["piv_words"][d] * 4
        sz["o_resid%d" % d] = L * p["rcap"][d] * 8
    for d in range(maxdim + 1):
        sz["o_pairs%d" % d] = L * p["pcap"][d] * S["Pair"]
    return sz


def check_invariants(c, p, knobs_set=False):
    L, N, D, maxdim = c[:4]
    offs = {}
    for k, v in p.items():
        if k.startswith("o_"):
            offs.update({"%s%d" % (k, i): x for i, x in enumerate(v)} if isinstance(v, list) else {k: v})
    assert p["o_x"] == 0
    live = {k: v for k, v in offs.items() if v != 0 or k == "o_x"}
    for k, v in live.items():
        assert v % 256 == 0, (c, k)
    sz = region_sizes(c, p)
    for k in ["o_dist", "o_stats", "o_mst"] + ["o_%s%d" % (n, d) for n in ("piv", "resid", "pairs") for d in range(1, maxdim + 1)] + ["o_pairs0"]:
        assert k in live and k in sz, (c, k)
    order = sorted(live.items(), key=lambda kv: kv[1])
    for (k, v), (k2, v2) in zip(order, order[1:] + [("total", p["total"])]):
        assert v + sz.get(k, 1) <= v2, (c, k, k2)
    # the memset range
    assert p["memset_lo"] <= p["o_stats"] < p["memset_hi"], c
    for d in range(1, maxdim + 1):
        if d == 2 and p["piv2_sparse"]:
            assert p["o_piv"][2] >= p["memset_hi"], c
        else:
            assert p["memset_lo"] <= p["o_piv"][d] and p["o_piv"][d] + sz["o_piv%d" % d] <= p["memset_hi"], c
    # LDS
    for k in ("chain_lds", "p1_lds", "prep_lds", "rcfg.bytes"):
        assert p[k] <= K_LDS_MAX, (c, k)
    if p["dense"]:
        assert 3 <= N <= K_DENSE_MAX_N and p["dK"] in CHAIN_KS and 64 * 32 * p["dK"] >= math.comb(N, 3), c
    # reducer selection
    assert not p["par2"] or p["par"], c
    assert not p["par"] or p["big"], c
    assert not p["big"] or not p["lds_mode"], c
    if not knobs_set:
        assert bool(p["wide"]) == (bool(p["big"]) and maxdim >= 2 and N > 568), c


def test_struct_sizes_and_limits(exe):
    head, _ = parse(run_text(exe, []), 0)
    assert head == dict(SIZEOF, kLdsMax=K_LDS_MAX, kDenseMaxN=K_DENSE_MAX_N)


def test_invariants_of_the_pin(exe):
    cs = pin_cases()
    for c, p in zip(cs, plans_of(exe, cs)):
        check_invariants(c, p)


def random_cases(n, seed):
    rng = random.Random(seed)
    cs = []
    for _ in range(n):
        N = rng.choice([rng.randint(1, 70), rng.randint(1, 300), rng.randint(1, 2048)])
        dt = rng.choice((F32, F64))
        is_dist = rng.random() < 0.2
        cs.append(case(rng.randint(1, 64), N, N if is_dist else rng.choice((1, 3, 31, 32, 100, 1050, 4096)), rng.randint(0, 2), dt, int(is_dist),
                       int(not is_dist and dt == F64 and rng.random() < 0.3), int(rng.random() < 0.2), rng.randint(0, 4), int(rng.random() < 0.2),
                       rng.randint(0, 2)))
    return cs


def test_invariants_of_random_shapes(exe):
    cs = random_cases(400, 7)
    for c, p in zip(cs, plans_of(exe, cs)):
        check_invariants(c, p)


def test_dist_sel_does_not_depend_on_L(exe):
    base = [case(1, n, D, 1, dt) for n in (17, 40, 144, 145, 200, 1024) for D in (3, 32, 260, 1050, 4096) for dt in (F32, F64)]
    ref = plans_of(exe, base)
    for L in (2, 32, 64):
        for a, b in zip(ref, plans_of(exe, [(L,) + c[1:] for c in base])):
            assert [a[k] for k in ("dist.mfma", "dist.dsplit", "dist.gram_layer")] == [b[k] for k in ("dist.mfma", "dist.dsplit", "dist.gram_layer")]


# (knobs, [(L, N, D, maxdim, dtype)] where tests/test_gpu_parity.py or tests/test_distance_paths.py set them -- or, for the
# three knobs no GPU test sets (TDA_PAR=0, TDA_P1_WAVES=1, TDA_PIV2_SPARSE=0), a shape of the neighbouring test --, the fields forced)
SWEEP48, GRID144_8, GRID144_6, TORUS256, TORUS300, ADV324 = (32, 48, 3, 2, F32), (8, 144, 3, 2, F32), (6, 144, 3, 2, F32), (1, 256, 3, 2, F32), \
    (1, 300, 3, 2, F32), (1, 324, 3, 2, F32)
FORCED = [
    ({"TDA_REDUCE": "wave"}, [GRID144_8, TORUS256], {"big": 0, "par": 0, "lds_mode": 0}),
    # (big = 1 is all TDA_REDUCE=big forces: par and par2 stay 1 at these shapes, as without the knob, so H1 and H2 run on
    # k_reduce_par and the serial radix heap itself is reached only with TDA_PAR=0 / TDA_PAR2=0 or after an abort)
    ({"TDA_REDUCE": "big"}, [GRID144_8, TORUS256], {"big": 1}),
    ({"TDA_REDUCE": "par", "TDA_PAR_STRICT": "1"}, [GRID144_6, TORUS256, ADV324], {"par": 1, "par2": 1}),
    ({"TDA_PAR": "0"}, [TORUS300, GRID144_8], {"par": 0, "par2": 0, "serial_tables": 1}),
    ({"TDA_PAR2": "0"}, [(1, 600, 3, 2, F32), TORUS300], {"par": 1, "par2": 0, "serial_tables": 1}),
    ({"TDA_PAR2": "1"}, [(1, 500, 3, 2, F32), TORUS300], {"par": 1, "par2": 1}),
    ({"TDA_H2_WIDE": "1", "TDA_PAR2": "1"}, [TORUS300], {"wide": 1, "par2": 1}),
    ({"TDA_H2_WIDE": "1", "TDA_PAR2": "0"}, [TORUS300], {"wide": 1, "par2": 0}),
    ({"TDA_H2_WIDE": "0"}, [TORUS300], {"wide": 0}),
    ({"TDA_CHAIN": "general"}, [SWEEP48, (3, 48, 2, 2, F32), (3, 48, 3, 2, F32)], {"dense": 1, "cmode": 0, "fast": 0}),
    ({"TDA_CHAIN": "fast"}, [SWEEP48, (3, 48, 2, 2, F32), (3, 48, 3, 2, F32)], {"dense": 1, "cmode": 1, "fast": 1}),
    ({"TDA_CHAIN": "auto"}, [SWEEP48], {"dense": 1, "cmode": 2, "fast": 1}),
    ({"TDA_P1_WAVES": "1"}, [SWEEP48], {"dense": 1, "p1_waves": 1}),
    ({"TDA_PIV2_SPARSE": "1"}, [TORUS300], {"piv2_sparse": 1}),
    ({"TDA_PIV2_SPARSE": "0"}, [(1, 2048, 3, 2, F32)], {"piv2_sparse": 0}),
    ({"TDA_DIST": "scalar"}, [(3, 145, 257, 1, F32), (3, 145, 257, 1, F64), (2, 63, 64, 2, F32), (2, 130, 37, 2, F64)], {"dist.mfma": 0, "dist.dsplit": 1, "dist.gram_layer": 0}),
    ({"TDA_DIST": "mfma"}, [(2, 200, 3, 2, F32), (2, 200, 3, 2, F64), (2, 5, 33, 2, F32)], {"dist.mfma": 1}),
    ({"TDA_DIST": "tiles"}, [(3, 63, 100, 1, F32), (3, 40, 1050, 1, F32)], {"dist.mfma": 1, "dist.gram_layer": 0}),
    ({"TDA_DIST": "tiles", "TDA_DIST_SPLIT": "3"}, [(3, 130, 224, 1, F32)], {"dist.mfma": 1, "dist.dsplit": 3, "dist.gram_layer": 0}),
    ({"TDA_DIST_SPLIT": "5"}, [(3, 40, 1050, 1, F32)], {"dist.mfma": 1, "dist.dsplit": 5, "dist.gram_layer": 1}),
    ({"TDA_DIST_SPLIT": "7"}, [(3, 65, 260, 1, F64)], {"dist.mfma": 1, "dist.dsplit": 7, "dist.gram_layer": 0}),
]
# what the same shapes get with no knob: the forced value is another one wherever the knob is not the default's name
DEFAULTS = {"p1_waves": 2, "cmode": 2}


@pytest.mark.parametrize("knobs,shapes,want", FORCED, ids=lambda x: ",".join("%s=%s" % kv for kv in x.items()) if isinstance(x, dict) and any(
    k.startswith("TDA_") for k in x) else None)
def test_forced_variant_names_what_it_runs(exe, knobs, shapes, want):
    cs = [case(*s) for s in shapes]
    plain = plans_of(exe, cs)
    for c, p, q in zip(cs, plans_of(exe, cs, knobs), plain):
        for k, v in want.items():
            assert p[k] == v, (knobs, c, k)
        check_invariants(c, p, knobs_set=True)
        for k, v in DEFAULTS.items():
            if k in want and q["dense"]:
                assert q[k] == v, (c, k)
    assert plans_of(exe, cs, knobs, gate=False) == plain  # no gate: the knobs change nothing


# ---- the knobs of tests/test_retry_paths.py
PAR_RESERVE = 512 * 65 * 3840  # kParGrid * kParLv * chunk_start(4): every workgroup's first bucket chunks
POOL_CAPS = ("rec_cap", "rpool_cap", "bpool_cap", "rq_cap")
POOL_SHAPES = [case(2, 256, maxdim=2, scale=s) for s in range(5)] + [case(1, 300, maxdim=2, scale=s) for s in (0, 2)] + \
    [case(1, 256, maxdim=1), case(4, 256, maxdim=2, no_par=1), case(1, 1025, maxdim=2, scale=1), case(1, 256, 256, 2, F64, is_dist=1)]


@pytest.mark.parametrize("k", [1, 3, 9, 17, 30])
def test_pool_shift_changes_the_four_capacities_and_what_lies_behind(exe, k):
    knobs = {"TDA_PAR_POOL_SHIFT": str(k)}
    plain = plans_of(exe, POOL_SHAPES)
    for c, p, q in zip(POOL_SHAPES, plans_of(exe, POOL_SHAPES, knobs), plain):
        scale = c[8]
        assert q["par"] == 1
        # the growing part shifted, after the << scale; the fixed parts as they were
        assert p["rec_cap"] == ((q["rec_cap"] - (4096 << scale)) >> k) + (4096 << scale), c
        assert p["rpool_cap"] == q["rpool_cap"] >> k, c
        assert p["bpool_cap"] == ((q["bpool_cap"] - PAR_RESERVE) >> k) // 256 * 256 + PAR_RESERVE, c
        assert p["rq_cap"] == max(1, q["rq_cap"] >> k), c
        assert all(p[f] < q[f] for f in POOL_CAPS), c
        # nothing else but the offsets carved behind the first pool that shrank, and the total
        behind = {f for f, v in q.items() if f.startswith("o_") and (max(v) if isinstance(v, list) else v) > q["o_prec"]} | {"total"}
        changed = {f for f in q if p[f] != q[f]}
        assert set(POOL_CAPS) <= changed <= set(POOL_CAPS) | behind, (c, sorted(changed - behind))
        assert {"o_prpool", "o_pbpool", "o_prq", "total"} <= changed, c
        check_invariants(c, p, knobs_set=True)
    assert plans_of(exe, POOL_SHAPES, knobs, gate=False) == plain  # no gate: the knob changes nothing
    # no parallel reducer in the plan: nothing to change
    serial = [case(32, 48, maxdim=2), case(1, 256, maxdim=2, no_par=2), case(1, 300, maxdim=0)]
    assert plans_of(exe, serial, knobs) == plans_of(exe, serial)


@pytest.mark.parametrize("k", [1, 6, 13, 30])
def test_invariants_of_random_shapes_with_the_pool_shift(exe, k):
    cs = random_cases(200, 11 + k)
    assert any(p["par"] for p in plans_of(exe, cs))
    for c, p in zip(cs, plans_of(exe, cs, {"TDA_PAR_POOL_SHIFT": str(k)})):
        check_invariants(c, p)


def knob_line(exe, knobs=None, gate=True):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TDA_")}
    env.update(knobs or {})
    if gate:
        env["TDA_TEST_OVERRIDES"] = "1"
    err = subprocess.run([exe], input="", capture_output=True, text=True, check=True, env=env).stderr
    return dict((k, int(v)) for k, v in (t.split("=") for t in err.split()[1:]))


def test_par_step_knobs_set_one_launch_each(exe):
    plain = dict(step_limit=1 << 26, par_steps_h1=1 << 26, par_steps_h2=1 << 26, par_pool_shift=0)
    assert knob_line(exe) == plain
    assert knob_line(exe, {"TDA_PAR_STEPS_H1": "4"}) == dict(plain, par_steps_h1=4)
    assert knob_line(exe, {"TDA_PAR_STEPS_H2": "4"}) == dict(plain, par_steps_h2=4)
    assert knob_line(exe, {"TDA_STEP_LIMIT": "99", "TDA_PAR_STEPS_H2": "7"}) == dict(plain, step_limit=99, par_steps_h1=99, par_steps_h2=7)
    assert knob_line(exe, {"TDA_PAR_POOL_SHIFT": "5"}) == dict(plain, par_pool_shift=5)
    assert knob_line(exe, {"TDA_PAR_STEPS_H1": "4", "TDA_PAR_STEPS_H2": "4", "TDA_PAR_POOL_SHIFT": "5", "TDA_STEP_LIMIT": "9"}, gate=False) == plain
    # the serial kernels' step limit (rcfg) does not follow the parallel knobs
    cs = [case(1, 256, maxdim=2)]
    assert plans_of(exe, cs, {"TDA_PAR_STEPS_H1": "4", "TDA_PAR_STEPS_H2": "4"}) == plans_of(exe, cs)


# ---- the size borders that tests/test_size_borders.py runs on a device (tests/size_borders.py)
def border_case(n, L=1):
    return case(L, n, maxdim=2)


def test_size_borders_are_where_the_plan_changes(exe):
    """Every N in 3 .. PLAN_SCAN_MAX at which the plan of (L = 1, N, D = 3, maxdim = 2) changes a field of
    PLAN_FIELDS is a border of PLAN_BORDERS, with the fields and the values on both sides named there,
    and the other way round.  A moved constant fails here, and the message says where the plan
    changes now: the sizes tests/size_borders.py, and through it the GPU file, must move to."""
    ns = list(range(2, sb.PLAN_SCAN_MAX + 1))
    plans = dict(zip(ns, plans_of(exe, [border_case(n) for n in ns])))
    found = []
    for n in ns[1:]:
        diff = {k: (plans[n - 1][k], plans[n][k]) for k in sb.PLAN_FIELDS if plans[n - 1][k] != plans[n][k]}
        if diff:
            found.append((n, diff))
    want = [(n, {k: v for k, v in f.items() if k in sb.PLAN_FIELDS}) for n, f in sb.PLAN_BORDERS]
    fd, wd = dict(found), dict(want)
    assert found == want, "the plan changes at N = %s, tests/size_borders.py says %s; move these:\n%s" % (
        [n for n, _ in found], [n for n, _ in want],
        "\n".join("  N = %d: the plan changes %r, the file says %r" % (n, fd.get(n), wd.get(n)) for n in sorted(set(fd) | set(wd)) if fd.get(n) != wd.get(n)))
    # the LDS sizes that decide a border, as literals
    for n, f in sb.PLAN_BORDERS:
        for k in ("chain_lds", "p1_lds"):
            if k in f:
                assert (plans[n - 1][k], plans[n][k]) == f[k], (n, k)
    # what the list is read for: the state on the lower side, and the sizes the GPU file runs
    for n, _ in sb.PLAN_BORDERS:
        assert sb.plan_below(n) == {k: plans[n - 1][k] for k in sb.PLAN_FIELDS}, n
    # the sizes that follow from PLAN_BORDERS, restated: after PLAN_BORDERS has moved these literals move too
    moved = "derived from PLAN_BORDERS; if PLAN_BORDERS was moved on purpose, restate this literal here"
    assert sb.DENSE_NS == (24, 25, 30, 31, 34, 35, 37, 38, 42, 43, 49, 50, 52, 53, 54, 59, 60, 61, 64, 65), moved
    assert sb.FORCED_CHAIN_NS == (24, 30, 34, 37, 42, 49, 52) and sb.P1_NS == (60,), moved
    assert [n for n, _ in sb.BIG_CASES] == [568, 569, 1024, 1025]


def test_size_borders_lds_margins(exe):
    """N = 60 is the last size whose two k_h2_phase1 waves fit: 159,920 of 163,840 bytes.  At 61 two
    waves would need 169,248, so the plan has one; TABLE stops fitting at K = 12 and FAST at N = 53."""
    p49, p50, p52, p53, p60, p61 = plans_of(exe, [border_case(n) for n in (49, 50, 52, 53, 60, 61)])
    assert sb.K_LDS_MAX == K_LDS_MAX == 163840
    assert p60["p1_waves"] == 2 and p60["p1_lds"] == 159920 <= K_LDS_MAX
    shared = 16 + (4 * 61 * 61 + 15) // 16 * 16 + 2 * p61["n2p"]  # the matrix and the class table; n2p is a multiple of 8
    two = shared + 2 * (p61["p1_lds"] - shared)
    assert p61["p1_waves"] == 1 and two == sb.P1_TWO_WAVES_AT_61 > K_LDS_MAX
    assert (p49["cmode"], p49["chain_lds"]) == (sb.CHAIN_TABLE, 161856) and p49["chain_lds"] <= K_LDS_MAX
    assert (p50["cmode"], p50["chain_lds"]) == (sb.CHAIN_FAST, 141344)
    assert (p52["cmode"], p52["chain_lds"]) == (sb.CHAIN_FAST, 157488) and (p53["cmode"], p53["chain_lds"]) == (sb.CHAIN_GENERAL, 94384)
    # the L of the GPU cases changes no field of the borders
    keys = sb.PLAN_FIELDS + ("chain_lds", "p1_lds")
    ns = sb.DENSE_NS + sb.MID_NS
    one = plans_of(exe, [border_case(n) for n in ns])
    for L in (sb.DENSE_L, sb.MID_L) + sb.L_BORDERS:
        for n, p, q in zip(ns, one, plans_of(exe, [border_case(n, L) for n in ns])):
            assert [q[k] for k in keys] == [p[k] for k in keys], (L, n)


def test_size_borders_forced_variants(exe):
    """What the knobs of tests/test_size_borders.py force at its sizes.  TDA_CHAIN=fast is honoured
    while FAST fits (cmode 1 up to N = 52) and silently gives GENERAL from 53 on: the forced `fast`
    tie case of tests/test_gpu_parity.py at N = 64 (D = 4) runs GENERAL."""
    cs = [border_case(n, sb.DENSE_L) for n in sb.FORCED_CHAIN_NS]
    plain = plans_of(exe, cs)
    fast, general = plans_of(exe, cs, {"TDA_CHAIN": "fast"}), plans_of(exe, cs, {"TDA_CHAIN": "general"})
    for c, q, f, g in zip(cs, plain, fast, general):
        assert q["cmode"] == sb.plan_below(c[1] + 1)["cmode"] != sb.CHAIN_GENERAL, c
        assert f["cmode"] == sb.CHAIN_FAST and f["fast"] == 1 and g["cmode"] == sb.CHAIN_GENERAL and g["fast"] == 0, c
        assert f["dK"] == g["dK"] == q["dK"] and f["dense"] == g["dense"] == 1, c
        check_invariants(c, f, knobs_set=True)
        check_invariants(c, g, knobs_set=True)
    # forced fast is another variant than the default's everywhere but at 52, where FAST is the default
    assert [c[1] for c, q, f in zip(cs, plain, fast) if f["cmode"] == q["cmode"]] == [52]
    at52, at53, tie64 = plans_of(exe, [border_case(52), border_case(53), case(2, 64, 4, 2)], {"TDA_CHAIN": "fast"})
    assert at52["cmode"] == sb.CHAIN_FAST and at53["cmode"] == sb.CHAIN_GENERAL and tie64["cmode"] == sb.CHAIN_GENERAL and tie64["dense"] == 1
    cs = [border_case(n, sb.DENSE_L) for n in sb.P1_NS]
    for c, q, p in zip(cs, plans_of(exe, cs), plans_of(exe, cs, {"TDA_P1_WAVES": "1"})):
        assert q["p1_waves"] == 2 and p["p1_waves"] == 1 and p["p1_lds"] < q["p1_lds"], c
        check_invariants(c, p, knobs_set=True)
        # the knob moves these two fields only.  Neither is part of a captured graph's key (fill_graph_key
        # in csrc/rips.hip), so on a device such a call can replay the two-wave graph of the default
        # call of its shape: the GPU file has no TDA_P1_WAVES case (left out)
        assert {k for k in q if q[k] != p[k]} == {"p1_waves", "p1_lds"}, c


# ---- the H0 shape above the dense path and the side metrics' LDS (tests/large_n.py, run by tests/test_large_n.py)
def h0_scan(exe, lo, hi):
    """-> (the limits line, {N: fields}) of `<program> h0 lo hi`"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("TDA_")}
    lines = subprocess.run([exe, "h0", str(lo), str(hi)], capture_output=True, text=True, check=True, env=env).stdout.splitlines()
    rows = [dict((k, int(v)) for k, v in (t.split("=") for t in ln_.split())) for ln_ in lines[1:]]
    assert [r["N"] for r in rows] == list(range(lo, hi + 1))
    return dict((k, int(v)) for k, v in (t.split("=") for t in lines[0].split()[1:])), {r["N"]: r for r in rows}


def test_large_n_h0_borders_are_where_the_shape_changes(exe):
    """Every N in 66 .. 8192 at which h0_shape changes a field of H0_FIELDS is a border of H0_BORDERS, with
    the values on both sides named there, and the other way round.  A moved constant fails here, and the
    message says where the shape changes now: the sizes tests/large_n.py, and through it the GPU file,
    must move to."""
    lo, hi = ln.H0_SCAN
    assert (lo, hi) == (K_DENSE_MAX_N + 1, ln.MAX_N)
    _, rows = h0_scan(exe, lo, hi)
    found = []
    for n in range(lo + 1, hi + 1):
        diff = {k: (rows[n - 1][k], rows[n][k]) for k in ln.H0_FIELDS if rows[n - 1][k] != rows[n][k]}
        if diff:
            found.append((n, diff))
    want = [(n, {k: v for k, v in f.items() if k in ln.H0_FIELDS}) for n, f in ln.H0_BORDERS]
    fd, wd = dict(found), dict(want)
    assert found == want, "the H0 shape changes at N = %s, tests/large_n.py says %s; move these:\n%s" % (
        [n for n, _ in found], [n for n, _ in want],
        "\n".join("  N = %d: the shape changes %r, the file says %r" % (n, fd.get(n), wd.get(n)) for n in sorted(set(fd) | set(wd)) if fd.get(n) != wd.get(n)))
    for n, f in ln.H0_BORDERS:
        assert (rows[n - 1]["lds"], rows[n]["lds"]) == f["lds"], (n, "lds")
        assert ln.h0_below(n) == {k: rows[n - 1][k] for k in ln.H0_FIELDS}, n
    # the sizes that follow from H0_BORDERS, restated: after H0_BORDERS has moved this literal moves too
    assert ln.H0_NS == (1024, 1025, 2026, 2027, 4096, 4097, 4098, 6122, 6123, 8170, 8171, 8191, 8192), \
        "derived from H0_BORDERS; if H0_BORDERS was moved on purpose, restate this literal here"
    # the chunk is a power of two, what the kernel is told (ilog2) is that chunk, and the merge passes of block_sort
    # (more keys than the chunk) run exactly where tests/large_n.py says: two chunks from 6123, four from 8171
    for n, r in rows.items():
        assert r["ch"] == 1 << r["chunk_log2"] and r["rounds"] == max(1, (n - 1).bit_length()), n
        chunks = -(-(n - 1) // r["ch"])
        assert chunks == (1 if n <= 6122 else 2 if n <= 8170 else 4), (n, chunks)
    assert {c[0] for c in ln.H0_THRESH_CASES} == {6122, 6123}


def test_large_n_lds_fits_at_every_n(exe):
    """The dynamic LDS of the four launches that grow with N, at every N = 65 .. 8192, against the limits
    restated here from the attributes csrc/rips.hip sets (init_device): a moved constant, or a carve that
    grew, fails and names the N."""
    limits, rows = h0_scan(exe, *ln.H0_SCAN)
    assert limits == dict(kLdsMax=160 * 1024, kBorHookLdsMax=150 * 1024, kTnLdsMax=8192 * 4, kSilLdsMax=128 * 1024, kSilMaxK=32, kSilT=256,
                          kTnT=1024, kH0BorWQ=16, kH0WaveMaxN=190)
    assert (ln.K_LDS_MAX, ln.BOR_HOOK_LDS_MAX, ln.TWONN_LDS_MAX, ln.SIL_LDS_MAX, ln.SIL_MAX_K, ln.SIL_T, ln.TWONN_T) == \
        (160 * 1024, 150 * 1024, 8192 * 4, 128 * 1024, 32, 256, 1024)
    for n, r in rows.items():
        # k_h0: 16 | best n x 8 | par n (even) x 4 | red 40 x 8 | hooks n x 4, rounded up to 16; the chunk; the staged matrix
        base = (16 + 8 * n + 4 * ((n + 1) & ~1) + 320 + 4 * n + 15) // 16 * 16
        assert r["base"] == base and r["lds"] == base + 8 * r["ch"] + (4 * n * n if r["dlds"] else 0), n
        assert r["lds"] <= K_LDS_MAX, "k_h0 at N = %d: %d bytes of LDS" % (n, r["lds"])
        # the chunk is the largest that fits (no staged matrix), 16384 keys at most
        if not r["dlds"]:
            assert r["ch"] == 16384 or base + 16 * r["ch"] > K_LDS_MAX, n
        else:
            assert r["ch"] >= n - 1, n  # the LDS path never merges
        assert r["hl"] == 8 * ((n + 3) & ~3) + 8 * n, n
        assert r["hl"] <= 150 * 1024, "k_bor_hook at N = %d: %d bytes of LDS" % (n, r["hl"])
        assert r["pw2"] >= max(n, 64) and r["pw2"] & (r["pw2"] - 1) == 0 and r["pw2"] < 2 * max(n, 64) and r["tn_lds"] == 4 * r["pw2"], n
        assert r["pw2"] * 4 <= 8192 * 4, "k_twonn at N = %d: %d bytes of LDS" % (n, r["tn_lds"])
        assert r["sil_lds"] == 32 * 2048 + 4 * n, n
        assert 32 * 2048 + 4 * n <= 128 * 1024, "k_silhouette at N = %d: %d bytes of LDS" % (n, r["sil_lds"])
    top = rows[ln.MAX_N]
    assert (top["lds"], top["hl"], top["sil_lds"], top["tn_lds"]) == (ln.H0_LDS_AT_8192, ln.BOR_HOOK_LDS_AT_8192, ln.SIL_LDS_AT_8192, ln.TWONN_LDS_MAX)
    # k_twonn's strided loops take pw2 / kTnT trips: one up to n = 1024, eight at 8192 -- the sizes the GPU file runs
    assert [rows[n]["pw2"] // 1024 for n in ln.TWONN_NS] == [1, 1, 2, 2, 4, 8, 8]


if __name__ == "__main__":
    sys.stdout.write("".join(" ".join(map(str, c)) + "\n" for c in pin_cases()))
