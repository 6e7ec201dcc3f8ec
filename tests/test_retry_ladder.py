"""The retry ladder of a persistence call (csrc/rips_retry.h, next_attempt) as a table (CPU).

tests/retry_ladder_main.cpp includes only rips_retry.h (and, through it, the error flags of
rips_err.h); it is compiled with g++ and run once for all cases.  The expected outcomes are
written out from the ladder as run_pipeline had it before it became a function (an if-chain on
the call's error flags that re-entered the pipeline), `parent_ladder` below restates that chain.
"""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tda-multimodal_amd", "csrc")

RESID, PAIR, WORK, VPOOL, OUT, SPILL, STEP, PAR, PAR2, CAP_MISS = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
MAX_PAR_SCALE = 4


def run_cases(exe, cases):
    """cases: (errs, code, (fg, scale, fb, no_par, no_cap), big, strict, wave) -> [(what, attempt)]"""
    text = "".join("%d %d %d %d %d %d %d %d %d %d\n" % (e, code, *map(int, at), int(big), int(strict), int(wave))
                   for e, code, at, big, strict, wave in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    rows = []
    for line in out[1:1 + len(cases)]:
        f = line.split()
        rows.append((f[0], (bool(int(f[1])), int(f[2]), bool(int(f[3])), int(f[4]), bool(int(f[5])))))
    assert len(rows) == len(cases)
    return out[0], rows


@pytest.fixture(scope="module")
def ladder(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ladder") / "retry_ladder")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "retry_ladder_main.cpp")], check=True)
    return exe


def test_flag_values(ladder):
    head, _ = run_cases(ladder, [])
    assert [int(x) for x in head.split()] == [RESID, PAIR, WORK, VPOOL, OUT, SPILL, STEP, PAR, PAR2, CAP_MISS, MAX_PAR_SCALE]


# (name, errs, ParCtl code, attempt (force_global, scale, force_big, no_par, no_cap), plan.big, strict, wave, expected)
F, T = False, True
ROWS = [
    ("zero is done", 0, 0, (T, 1, T, 1, T), T, F, F, ("done", None)),
    ("par, capacity code, scale 3 -> 4", PAR, 21, (F, 3, T, 0, F), T, F, F, ("retry", (F, 4, T, 0, F))),
    ("par, capacity code, scale 4: no_par 2", PAR, 21, (F, 4, T, 0, F), T, F, F, ("retry", (F, 4, T, 2, F))),
    ("par, capacity code, scale 4, strict: fail", PAR, 21, (F, 4, T, 0, F), T, T, F, ("fail", None)),
    ("par, capacity code below the limit, strict: still larger pools", PAR, 22, (F, 0, F, 0, F), T, T, F, ("retry", (F, 1, F, 0, F))),
    ("capacity code 41", PAR2, 41, (F, 1, F, 0, T), T, F, F, ("retry", (F, 2, F, 0, T))),
    ("capacity code 53", PAR, 53, (T, 2, T, 1, F), T, F, F, ("retry", (T, 3, T, 1, F))),
    ("par2 alone, no_par 0 -> 1", PAR2, 7, (F, 0, F, 0, F), T, F, F, ("retry", (F, 0, F, 1, F))),
    ("par2 alone, no_par 2 stays", PAR2, 7, (F, 0, F, 2, F), T, F, F, ("retry", (F, 0, F, 2, F))),
    ("par and par2: no_par 2", PAR | PAR2, 7, (F, 0, F, 1, F), T, F, F, ("retry", (F, 0, F, 2, F))),
    ("non-capacity code at scale 0: no_par at once", PAR, 81, (F, 0, F, 0, T), T, F, F, ("retry", (F, 0, F, 2, T))),
    ("non-capacity code, strict: fail", PAR, 81, (F, 0, F, 0, F), T, T, F, ("fail", None)),
    ("par wins over an LDS spill", PAR | SPILL, 7, (F, 0, F, 0, F), T, F, F, ("retry", (F, 0, F, 2, F))),
    ("LDS spill: global tables, force_big dropped", SPILL, 0, (F, 1, T, 1, T), F, F, F, ("retry", (T, 1, F, 1, T))),
    ("LDS spill, force_global set: falls through to the scale rule", SPILL, 0, (T, 0, F, 0, F), F, F, F, ("retry", (T, 1, F, 0, F))),
    ("LDS spill, force_global set, scale 2: fail", SPILL, 0, (T, 2, F, 0, F), F, F, F, ("fail", None)),
    ("work cap off the big path: radix heap from scale 0", WORK, 0, (F, 1, F, 2, F), F, F, F, ("retry", (T, 0, T, 2, F))),
    ("work cap, big: scale rule, force_big = big", WORK, 0, (F, 0, F, 2, F), T, F, F, ("retry", (F, 1, T, 2, F))),
    ("work cap, TDA_REDUCE=wave: scale rule", WORK, 0, (T, 1, F, 0, F), F, F, T, ("retry", (T, 2, F, 0, F))),
    ("work + pool cap, big, scale 1 -> 2", WORK | VPOOL, 0, (T, 1, T, 0, F), T, F, F, ("retry", (T, 2, T, 0, F))),
    ("pool cap at scale 2: fail", VPOOL, 0, (F, 2, F, 0, F), T, F, F, ("fail", None)),
    ("pool cap after parallel retries raised scale to 3: fail", VPOOL, 0, (F, 3, F, 1, F), T, F, F, ("fail", None)),
    ("residual cap fails at once", RESID, 0, (F, 0, F, 0, F), T, F, F, ("fail", None)),
    ("residual cap beside a work cap, big: fail", RESID | WORK, 0, (F, 0, F, 0, F), T, F, F, ("fail", None)),
    ("pair cap: fail", PAIR, 0, (F, 0, F, 0, F), F, F, F, ("fail", None)),
    ("step limit: fail", STEP, 0, (F, 0, F, 0, F), T, F, F, ("fail", None)),
    ("output cap left over: fail", OUT, 0, (F, 0, F, 0, F), T, F, F, ("fail", None)),
]


def test_table(ladder):
    _, got = run_cases(ladder, [r[1:7] for r in ROWS])
    for row, (what, nxt) in zip(ROWS, got):
        exp_what, exp_next = row[7]
        assert what == exp_what, row[0]
        if exp_next is not None:
            assert nxt == exp_next, row[0]


def parent_ladder(errs, code, at, big, strict, wave):
    """The if-chain at the end of the old run_pipeline, restated (its `scale < 2` guard included)."""
    fg, scale, fb, no_par, no_cap = at
    if errs & (PAR | PAR2):
        np_next = 2 if errs & PAR else max(no_par, 1)
        if code in (21, 22, 41, 53) and scale < MAX_PAR_SCALE:
            return "retry", (fg, scale + 1, fb, no_par, no_cap)
        if strict:
            return "fail", None
        return "retry", (fg, scale, fb, np_next, no_cap)
    if (errs & SPILL) and not fg:
        return "retry", (True, scale, False, no_par, no_cap)
    if (errs & WORK) and not big and not wave:
        return "retry", (True, 0, True, no_par, no_cap)
    if (errs & ~SPILL) == (errs & (WORK | VPOOL)) and errs and scale < 2:
        return "retry", (fg, scale + 1, big, no_par, no_cap)
    if errs:
        return "fail", None
    return "done", None


def test_every_combination(ladder):
    bits = (RESID, WORK, VPOOL, SPILL, PAR, PAR2)
    flags = [sum(b for b, on in zip(bits, m) if on) for m in itertools.product((0, 1), repeat=len(bits))]
    cases = [(e, code, (fg, scale, fb, no_par, (scale + no_par) % 2 == 1), big, strict, wave)
             for e in flags for code in (0, 21, 81) for fg in (F, T) for scale in range(5) for fb in (F, T)
             for no_par in range(3) for big in (F, T) for strict in (F, T) for wave in (F, T)
             if (e & (PAR | PAR2)) or code == 0]
    _, got = run_cases(ladder, cases)
    for case, (what, nxt) in zip(cases, got):
        exp_what, exp_next = parent_ladder(*case)
        assert what == exp_what and (exp_next is None or nxt == exp_next), case
