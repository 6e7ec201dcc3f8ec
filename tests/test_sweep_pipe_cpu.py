"""The queue of the native sweep pipeline (csrc/sweep_pipe.h) with a stand-in batch call (CPU).

tests/sweep_pipe_main.cpp includes only sweep_pipe.h (plain C++17: no HIP, no Python) and drives
it with a batch call that sleeps and reports what it was given.  It is compiled with g++ and run
three times: plain, under the thread sanitizer, and under the address and undefined-behaviour
sanitizers -- each a stand-alone executable.  The program checks: tickets resolve to their own
[lo, hi) in submission order; the four dispatch triggers (full batch, a change of shape / dtype /
residence / argument template in the middle, a wait, flush with a partial last batch); round-robin
slot assignment on the top slots; an error (a NaN in host input, a refused call) reaches every
ticket of its call and only those; a result is freed exactly once, with its last ticket; destroy
with unreleased tickets and a pending batch; two submitting threads; several threads blocked on one
ticket, the first of which releases it (and with it the call) while the others still wait.
"""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tda-multimodal_amd", "csrc")
CASES = ["order_and_slots", "key_changes_and_flush", "errors", "destroy", "two_threads", "waiters_on_one_ticket"]


# the sanitizer runtimes are linked statically: the programs then run whatever else the loader brings in first
@pytest.mark.parametrize("name,flags", [("plain", ["-O1"]), ("tsan", ["-O1", "-g", "-fsanitize=thread", "-static-libtsan"]),
                                        ("asan_ubsan", ["-O1", "-g", "-fsanitize=address,undefined",
                                                        "-fno-sanitize-recover=undefined", "-static-libasan",
                                                        "-static-libubsan"])])
def test_sweep_pipe(tmp_path, name, flags):
    exe = str(tmp_path / ("sweep_pipe_" + name))
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", *flags, "-pthread", "-I" + CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "sweep_pipe_main.cpp")], check=True)
    cmd = [exe]
    if name == "tsan" and shutil.which("setarch"):
        # this compiler's thread sanitizer refuses the address layouts of kernels with more mmap
        # randomisation than it knows ("unexpected memory mapping"): run that one program, and only
        # it, with a fixed layout
        cmd = ["setarch", platform.machine(), "-R", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.split("\n")[:-1] == ["ok " + c for c in CASES] + ["all ok"]
    assert "Sanitizer" not in r.stderr, r.stderr[-4000:]
