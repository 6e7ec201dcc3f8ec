"""What reaches the library from the cloud entries (no device): ripser_batch and its options,
parts and n_perm, greedy_perm_batch, hausdorff_resamples, h0_subsamples, the spectral metrics,
TwoNN, umap_batch and a native SweepPipeline submit, for every input form, with every refusal's
type, message and place in the order of checks.  Recorded with the stand-in library of
tests/cloud_call.py and compared, field for field, with tests/golden/cloud_call_args.json, which
was recorded before these entries shared their input and call paths."""
import json
import os

import pytest

import cloud_call
from conftest import GOLDEN


OWN = ("ValueError", "NotImplementedError", "returned")  # what the project itself raises here, message and all


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "cloud_call_args.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def recorded(pkg, built_lib):
    mp = pytest.MonkeyPatch()
    try:
        pkg._lib.hostviews()  # the real one: the ripser family's finite check runs in it
        return json.loads(json.dumps(cloud_call.record(pkg, mp.setattr)))
    finally:
        mp.undo()


def test_the_grid_is_the_recorded_one(golden, recorded):
    assert sorted(recorded) == sorted(golden)
    assert len(golden) > 400 and sum(len(v["calls"]) for v in golden.values()) > 350
    assert {v["outcome"][0] for v in golden.values()} - set(OWN) == {"TypeError", "RuntimeError"}


def test_every_call_and_refusal_is_as_recorded(golden, recorded):
    """An error of another type is torch's own (a bfloat16 or requires_grad tensor to numpy): its type is
    compared, not its wording, which is torch's to change."""
    wrong = []
    for name in sorted(golden):
        g, r = golden[name], recorded.get(name)
        if r is None or (r["outcome"] != g["outcome"] if g["outcome"][0] in OWN else r["outcome"][0] != g["outcome"][0]):
            wrong.append((name, "outcome", g["outcome"], r and r["outcome"]))
            continue
        if [c[0] for c in r["calls"]] != [c[0] for c in g["calls"]]:
            wrong.append((name, "symbols", [c[0] for c in g["calls"]], [c[0] for c in r["calls"]]))
            continue
        for (sym, ga), (_, ra) in zip(g["calls"], r["calls"]):
            if ga != ra:
                diff = {k: (ga.get(k), ra.get(k)) for k in sorted(set(ga) | set(ra)) if ga.get(k) != ra.get(k)} if ga and ra else (ga, ra)
                wrong.append((name, sym, diff))
    assert not wrong, f"{len(wrong)} of {len(golden)} cases differ; the first: {wrong[:5]}"


def test_the_grid_reaches_what_it_is_meant_to(golden):
    """The fixture itself: the cases that must reach the library do, with the fields the issue names."""
    def only(name):
        (call,) = golden[name]["calls"]
        return call

    refusal = ["ValueError", cloud_call.REFUSAL]
    sym, a = only("ripser_batch/points/np_f32")
    assert sym == "tda_rips_batch" and golden["ripser_batch/points/np_f32"]["outcome"] == refusal
    assert (a["dtype"], a["x_on_device"], a["L"], a["N"], a["D"], a["stream"], a["x_parts"]) == (0, 0, 2, 5, 3, "NULL", "NULL")
    for fm in ("np_f64", "np_f16", "np_i64", "torch_f64", "torch_f16"):  # the ripser family: f32 and f64 kept, else f64
        assert only(f"ripser_batch/points/{fm}")[1]["dtype"] == 1
        assert only(f"effective_dim/points/{fm}")[1]["dtype"] == 0  # the metrics: everything to f32
    # a nested list is input in parts to ripser_batch (each part then 2-D), one array to the metrics
    assert golden["ripser_batch/points/list"] == {"calls": [], "outcome": ["ValueError", "X must be (L, N, D)"]}
    assert only("effective_dim/points/list")[1]["x"] == only("effective_dim/points/np_f64")[1]["x"]
    for fm in ("np_f32_strided", "np_f32_fortran", "torch_f32", "torch_grad"):
        assert only(f"ripser_batch/points/{fm}")[1]["x"] == a["x"]  # the same bytes whatever the form
    assert only("umap_batch/points/np_f64")[1]["dtype"] == 1 and only("umap_batch/points/np_f16")[1]["dtype"] == 0
    two = golden["ripser_batch_n_perm/option/all"]["calls"]
    assert [c[0] for c in two] == ["tda_greedy_perm", "tda_rips_batch", "tda_greedy_free"]
    assert two[1][1]["x"] == {"device_pointer": cloud_call.SUB_DEV} and two[1][1]["is_dist"] == 1 and two[1][1]["N"] == 3
    parts = only("ripser_batch/parts/two_f32")[1]
    assert parts["x"] == "NULL" and parts["n_parts"] == 2 and len(parts["x_parts"]) == 2 and parts["L"] == 4 and parts["x_parts"][0] == a["x"]
    create, submit = golden["sweep_pipeline/option/labels"]["calls"]
    assert (create[0], submit[0]) == ("tda_pipe_create", "tda_pipe_submit") and submit[1]["x"] == a["x"]
    assert submit[1]["template"]["n_label_sets"] == 2 and submit[1]["template"]["labels"] != "NULL" and submit[1]["template"]["x"] == "NULL"
    assert golden["intrinsic_dim/no_call_below_6"]["calls"] == []
    # messages differ between modules by their final full stop; a refusal before the library records no call
    assert golden["refuse/nan/ripser_batch"] == {"calls": [], "outcome": ["ValueError", "Input contains NaN or infinity."]}
    assert golden["refuse/nan/effective_dim"] == {"calls": [], "outcome": ["ValueError", "Input contains NaN or infinity"]}
    assert golden["refuse/order/ed_nan_and_too_large"]["outcome"][1] == "Input contains NaN or infinity"
    assert golden["refuse/order/entropy_nan_and_too_large"]["outcome"][0] == "NotImplementedError"
    assert golden["refuse/not_square_and_nan/ripser_batch"]["outcome"][1] == "Input contains NaN or infinity."
    assert golden["refuse/not_square_and_nan/greedy_perm_batch"]["outcome"][1] == "Distance matrix is not square"
    assert golden["refuse/order/ndim2_and_bad_n_perm"]["outcome"][1] == "n_perm must be an integer"
