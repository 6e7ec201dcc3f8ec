"""A plain ``bench.py --gpus 1 --steps K --warmup W`` run does what its headline
figure needs and nothing else; everything next to it sits behind ``--full``.
``--dump-outputs DIR`` writes the last timed step's diagrams."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_dump_outputs_files(tmp_path):
    import bench

    inf = np.inf
    last = [[np.array([[0.0, 0.5], [0.0, inf]]), np.array([[0.7, 0.9]])],
            [np.array([[0.0, 0.25], [0.0, 0.75], [0.0, inf]]), np.zeros((0, 2))]]
    bench.dump_outputs(str(tmp_path), last, 1)
    got = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert all(a.dtype == np.float64 and a.size > 0 and np.isfinite(a).all() for a in got.values())
    assert sorted(got) == ["dgm0", "dgm1", "dgms_counts"]
    assert got["dgms_counts"].tolist() == [[2, 1], [3, 0]]
    # layer, birth, death (the birth where it is infinite), infinite
    assert got["dgm0"].tolist() == [[0, 0.0, 0.5, 0], [0, 0.0, 0.0, 1], [1, 0.0, 0.25, 0], [1, 0.0, 0.75, 0], [1, 0.0, 0.0, 1]]
    assert got["dgm1"].tolist() == [[0, 0.7, 0.9, 0]]


def test_dump_outputs_writes_no_empty_file(tmp_path):
    import bench

    bench.dump_outputs(str(tmp_path), [[np.array([[0.0, np.inf]]), np.zeros((0, 2)), np.zeros((0, 2))]], 2)
    assert sorted(os.listdir(tmp_path)) == ["dgm0.npy", "dgms_counts.npy"]
    assert np.load(tmp_path / "dgms_counts.npy").tolist() == [[1, 0, 0]]


def test_dump_outputs_caps_the_size(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    rows = np.stack([np.zeros(500), np.arange(1.0, 501.0)], axis=1)
    for d in ("a", "b"):  # the same seeded sample twice
        bench.dump_outputs(str(tmp_path / d), [[rows]], 0)
    a = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sum(x.nbytes for x in a.values()) <= 4096
    assert 0 < len(a["dgm0.npy"]) < 500 and (np.diff(a["dgm0.npy"][:, 2]) > 0).all()
    for f, x in a.items():
        assert np.array_equal(x, np.load(tmp_path / "b" / f))


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last(tmp_path, oracle):
    import bench

    # the run itself is what is checked: a process of its own, as the benchmark is started
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["metric"] == bench.METRIC and out["unit"] == "layers/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f32" and out["steps"] == 3 and out["warmup"] == 1
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(32 / (out["ms_per_step"] * 1e-3))
    # nothing that takes a run of its own
    assert out["cpu_baseline"] is None and out["roofline"] is None and out["pipeline"]["sequential"] is None
    assert not {"workloads", "summary", "stages_ms", "speedup_vs_cpu"} & set(out)
    # step i runs sweep i % 8: the last of 3 steps ran variant 2
    X = bench.make_workload("sweep48_host", variant=2)
    exp = [oracle.rips(x, maxdim=2)["dgms"] for x in X]
    counts = np.load(tmp_path / "dgms_counts.npy")
    assert counts.tolist() == [[len(d) for d in layer] for layer in exp]
    for k in range(3):
        rows = np.concatenate([np.asarray(layer[k], dtype=np.float64).reshape(-1, 2) for layer in exp])
        if not len(rows):
            assert not os.path.exists(tmp_path / f"dgm{k}.npy")
            continue
        got = np.load(tmp_path / f"dgm{k}.npy")
        inf = ~np.isfinite(rows[:, 1])
        assert np.array_equal(got[:, 0], np.repeat(np.arange(32.0), counts[:, k].astype(int)))
        assert np.array_equal(got[:, 1], rows[:, 0]) and np.array_equal(got[:, 3], inf.astype(np.float64))
        assert np.array_equal(got[:, 2], np.where(inf, rows[:, 0], rows[:, 1]))
