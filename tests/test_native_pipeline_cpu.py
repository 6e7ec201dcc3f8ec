"""What SweepPipeline's native path owns on the Python side (no GPU needed).

A native worker reads a sweep's array (the NaN scan, then the library's copy) whenever its call
runs, whether or not anybody still holds the future -- so the pipeline, not the future, keeps the
array until the call has run.  Without a device the calls fail at the device check, after the
scan; with one they run: the tests assert neither, only who is alive when.
"""
import gc
import importlib
import weakref

import numpy as np
import pytest


@pytest.fixture(scope="module", autouse=True)
def torch_device_first():
    """Where there is a device these calls run on it: torch ships its own HIP runtime and must
    initialise its device before the library does ("torch and the HIP runtime"),
    or the GPU tests that follow in the same process find none."""
    import torch

    if torch.cuda.is_available():
        torch.cuda.init()


def private_sweep(seed):
    """A sweep whose only owner is the pipeline: non-contiguous, so submit() makes its own copy
    (2 MB: a mapping of its own, which goes back to the system when freed)."""
    return np.full((4, 512, 512), 1.0 + seed, np.float32)[:, :, ::2]


def settle(fut):
    try:
        fut.result()
    except RuntimeError:  # no device here
        pass


def test_dropped_futures_leave_their_arrays_with_the_pipeline(pkg, built_lib):
    rp = importlib.import_module("tda-multimodal_amd.ripser")
    pipe = pkg.SweepPipeline(depth=1, coalesce=4, maxdim=0)
    futs = [pipe.submit(private_sweep(i)) for i in range(3)]  # a pending batch: nothing runs yet
    assert all(type(f) is rp._NativeFuture for f in futs)
    tickets = [f._ticket for f in futs]
    alive = [weakref.ref(pipe._keeps[t][0]) for t in tickets]
    del futs
    gc.collect()
    # dropped unread while their call is still to run: parked, arrays held
    assert sorted(pipe._orphans) == sorted(tickets)
    assert all(a() is not None for a in alive) and all(t in pipe._keeps for t in tickets)
    last = pipe.submit(private_sweep(3))  # completes the batch: the worker now reads all four arrays
    settle(last)  # its call is the dropped ones' call
    pipe._reap()
    gc.collect()
    assert pipe._orphans == [] and pipe._keeps == {} and pipe._calls == {}
    assert all(a() is None for a in alive)
    pipe.close()


def test_results_ignored_in_a_loop_and_a_pipeline_never_closed(pkg, built_lib):
    pipe = pkg.SweepPipeline(depth=2, coalesce=2, maxdim=0)
    for i in range(9):  # a warm-up whose results nobody reads, arrays owned by nobody else
        pipe.submit(private_sweep(i))
    held = [weakref.ref(k) for k, _ in pipe._keeps.values()]
    assert held  # the odd one is pending at least
    settle(pipe.submit(private_sweep(9)))
    del pipe  # never closed: the pipe runs what is queued and joins its workers before the arrays go
    gc.collect()
    assert all(a() is None for a in held)


def test_templates_hold_the_arguments_they_are_keyed_by(pkg, built_lib):
    """Per-submit arrays are keyed by identity: a template keeps the object, so a later object
    at a recycled address gets a template of its own, and the table stays bounded."""
    X = np.zeros((2, 6, 3), np.float32)
    with pkg.SweepPipeline(depth=1, coalesce=2, maxdim=0) as pipe:
        for i in range(3 * pipe._MAX_TEMPLATES):
            lab = [np.arange(6) % (2 + i % 2)]  # a fresh list each time, freed after the submit
            f = pipe.submit(X, labels=lab)
            t = pipe._keeps[f._ticket][1]
            assert t.given["labels"] is lab
            assert t.lab.tolist() == [(np.arange(6) % (2 + i % 2)).tolist()]
            assert len(pipe._tmpl) <= pipe._MAX_TEMPLATES
            del f, lab
