"""Workspace lifetime (csrc/ws_life.h) with a stand-in runtime (CPU).

tests/ws_life_main.cpp includes only ws_life.h (plain C++17: no HIP, no Python) and drives its
buffer type, graph cache, launch path and lock scopes with a runtime that allocates with malloc,
logs every call, fails a chosen call, and aborts when an allocation, free or graph destruction
runs beside another thread's open capture or a launch runs between another thread's
instantiation and its first launch.  It is compiled with g++ and run three times: plain, under
the thread sanitizer, and under the address and undefined-behaviour sanitizers -- each a
stand-alone executable.  The program checks: a growth that fails at its free, its allocation or
its device-pointer fetch leaves the buffer empty, for every memory kind, and the next growth
works (the sequences ws_prepare and grow_hout had before kept a freed pointer under its old
capacity: this case fails against them); a baked buffer's growth destroys the slot's graphs before
the free and bumps the generation, an unbaked one's does not, a growth that fits calls nothing;
the sizes each workspace buffer asks for (1.5x, 2x, the floors 1<<16, 1<<12, 64, none); the cache
(hit, sixteen kept, the seventeenth destroys the sixteen after its own instantiation and before
its own launch, a key one field apart misses, -0.0 against 0.0 included, equal fields over
differently filled memory are equal bytes); a failed enqueue, capture end or instantiation
caches nothing, destroys the graph once and is captured again by the next call; a hit is
record, launch, record under the shared side of the launch lock, graphs off run the enqueue once
and cache nothing; and eight threads, one per slot, that start together and make 5000 calls each
from fixed seeds (88 % replays of a steady key, new keys, eager calls, growths of a baked and of
an unbaked buffer, a reserve with a further allocation in one hold of the allocation scope):
neither rule fires, the thread sanitizer reports nothing, every allocation is freed once.  5000
calls per thread: about 0.15 s under the thread sanitizer on eight cores.
"""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tda-multimodal_amd", "csrc")
CASES = ["grow_failure_leaves_empty", "baked_growth_drops_first", "growth_policy", "cache_hit_miss_evict", "capture_failures",
         "replay_and_eager", "threads"]


# the sanitizer runtimes are linked statically: the programs then run whatever else the loader brings in first
@pytest.mark.parametrize("name,flags", [("plain", ["-O1"]), ("tsan", ["-O1", "-g", "-fsanitize=thread", "-static-libtsan"]),
                                        ("asan_ubsan", ["-O1", "-g", "-fsanitize=address,undefined",
                                                        "-fno-sanitize-recover=undefined", "-static-libasan",
                                                        "-static-libubsan"])])
def test_ws_life(tmp_path, name, flags):
    exe = str(tmp_path / ("ws_life_" + name))
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", *flags, "-pthread", "-I" + CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "ws_life_main.cpp")], check=True)
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
