"""GPU tests of the device branch of the shared input path (_cloud.prepare / fill_head): what a CPU
test cannot see.  For every cloud entry, a CUDA tensor gives bit for bit what the same data gives as
a numpy array -- contiguous f32, f16 (to f64 for the ripser family, to f32 for the metrics) and a
strided view -- also when the tensor is still being written on a non-default torch stream, and the
call runs on the tensor's own device whatever the ``device`` argument says.  Ordinary calls only.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L, N, D = 2, 48, 3
B, SN, SD = 2, 16, 8


@pytest.fixture(scope="module")
def gpu(pkg, built_lib):
    import torch  # a process that hands torch CUDA tensors to the library initialises torch's device first

    torch.cuda.init()
    assert pkg.lib().tda_device_ok(0) == 1, "no gfx950 device visible"
    return pkg


IDX = np.random.default_rng(5).integers(0, N, size=(6, 20), dtype=np.int32)


def _np(v):
    return v.detach().cpu().numpy() if type(v).__module__.startswith("torch") else np.asarray(v)


def _rips(p, X):
    res = p.ripser_batch(X, maxdim=1, want_dist=True)
    return [a.tobytes() for r in res for a in (*r.dgms, r.dist)]


def _greedy(p, X):
    g = p.greedy_perm_batch(X, 12)
    return [g.idx_perm.tobytes(), g.lambdas.tobytes(), g.dperm2all.tobytes()]


ENTRIES = {  # name -> (call -> list of bytes, shape of its input)
    "ripser_batch": (_rips, (L, N, D)),
    "greedy_perm_batch": (_greedy, (L, N, D)),
    "hausdorff_resamples": (lambda p, X: [p.hausdorff_resamples(X, IDX).tobytes()], (L, N, D)),
    "h0_subsamples": (lambda p, X: [p.h0_subsamples(X, IDX).tobytes()], (L, N, D)),
    "effective_dim": (lambda p, X: [_np(p.compute_effective_dimensionality(X)).tobytes()], (B, SN, SD)),
    "entropy_profile": (lambda p, X: [_np(p.matrix_entropy_profile(X, [1.0, 2.0])).tobytes()], (B, SN, SD)),
    "fixed_window_ed": (lambda p, X: [_np(p.compute_fixed_window_ed(X, 2)).tobytes()], (B, SN, SD)),
}
FORMS = ("f32", "f16", "strided")


def host_form(shape, form):
    """The data (multiples of 1/64, exact in f16) as the numpy array of that form."""
    base = np.random.default_rng(sum(shape)).integers(-128, 128, size=shape).astype(np.float32) / 64.0
    if form == "f16":
        return base.astype(np.float16)
    if form == "strided":
        wide = np.full(shape[:-1] + (2 * shape[-1],), 7.0, np.float32)
        wide[..., ::2] = base
        return wide[..., ::2]
    return base


def device_form(X):
    """The same array as a CUDA tensor of the same dtype and strides."""
    import torch

    if X.flags.c_contiguous:
        return torch.from_numpy(X).cuda()
    t = torch.from_numpy(np.ascontiguousarray(X.base)).cuda()[..., ::2]
    assert not t.is_contiguous() and t.shape == X.shape
    return t


def outcome(call, p, X):
    try:
        return call(p, X)
    except (ValueError, NotImplementedError) as e:  # f16 points are f64 points: greedy, resample and sh0 refuse them on both sides
        return [type(e).__name__, str(e)]


_HOST = {}


def host_result(p, name, form):
    """The host call's result, computed once per (entry, form) and left unchanged."""
    if (name, form) not in _HOST:
        call, shape = ENTRIES[name]
        _HOST[name, form] = outcome(call, p, host_form(shape, form))
    return _HOST[name, form]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(ENTRIES))
def test_device_and_host_input_agree(gpu, name, form):
    call, shape = ENTRIES[name]
    want = host_result(gpu, name, form)
    got = outcome(call, gpu, device_form(host_form(shape, form)))
    assert got == want
    refused = name in ("greedy_perm_batch", "hausdorff_resamples", "h0_subsamples") and form == "f16"
    assert (want[0] == "NotImplementedError") == refused


@pytest.mark.parametrize("name", list(ENTRIES))
def test_a_tensor_still_being_written_on_another_stream(gpu, name):
    """The call is ordered after torch's current stream: the cloud is written into the tensor by the
    last of a few kernels enqueued on a side stream, and the entry is called there without a wait.
    (With ``stream`` left NULL for device input four of the seven cases fail and three pass:
    DESIGN.md 6.37.)"""
    import torch

    call, shape = ENTRIES[name]
    want = host_result(gpu, name, "f32")
    src = device_form(host_form(shape, "f32"))
    t = torch.full(shape, 3.0, device="cuda")  # what a call that does not wait would read
    m = torch.ones((4096, 4096), device="cuda")  # eight products of these: milliseconds of work ahead of the copy
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(8):
            m = (m @ m) * (1.0 / 4096)  # stays all ones
        t.copy_(src + m[0, 0] * 0.0)
        got = outcome(call, gpu, t)
    torch.cuda.synchronize()
    assert got == want


def test_device_input_runs_on_the_tensors_device_whatever_the_argument(gpu):
    """``device`` is where host input goes; a CUDA tensor brings its own (there is no device 5 here)."""
    Xd = device_form(host_form((L, N, D), "f32"))
    res = gpu.ripser_batch(Xd, maxdim=1, want_dist=True, device=5)
    assert [a.tobytes() for r in res for a in (*r.dgms, r.dist)] == host_result(gpu, "ripser_batch", "f32")
    assert gpu.greedy_perm_batch(Xd, 12, device=5).idx_perm.tobytes() == host_result(gpu, "greedy_perm_batch", "f32")[0]
    assert gpu.hausdorff_resamples(Xd, IDX, device=5).tobytes() == host_result(gpu, "hausdorff_resamples", "f32")[0]
    assert gpu.h0_subsamples(Xd, IDX, device=5).tobytes() == host_result(gpu, "h0_subsamples", "f32")[0]


def test_umap_device_input(gpu):
    """The fuzzy graph of a CUDA tensor is the host call's, byte for byte (the layout is pinned bit
    for bit nowhere); the tensor's device wins over the argument; f16 on the device is refused."""
    import torch

    X = np.random.default_rng(3).standard_normal((2, 32, 3)).astype(np.float32)
    _, want = gpu.umap_batch(X, return_graph=True, random_state=0)
    _, got = gpu.umap_batch(torch.from_numpy(X).cuda(), return_graph=True, random_state=0)
    assert got.tobytes() == want.tobytes() and want.any()
    _, got = gpu.umap_batch(torch.from_numpy(X).cuda(), return_graph=True, random_state=0, device=5)
    assert got.tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="^X must be float32 or float64$"):
        gpu.umap_batch(torch.from_numpy(X).cuda().half(), return_graph=True, random_state=0)
