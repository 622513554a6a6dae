"""-m gpu: _op.enqueue / _op.workspace against the call they replace.  Every case spells the old call out longhand - the entry point
under torch.cuda.device(dev) with .data_ptr() arguments and torch.cuda.current_stream(dev).cuda_stream - and asks the helper for the same
bits: without a workspace (gm_cov_to_scale_rot), with one (gm_knn), with an optional NULL (gm_sh_colors), on a side stream, on a device
that is not the current one, and a call the C side refuses on its arguments alone."""
import math

import pytest
import torch

from gaussianmesh_amd import _lib, _op

pytestmark = pytest.mark.gpu


def _covariances(dev):
    """three symmetric positive definite matrices: a diagonal one, a rotated one, one with two equal eigenvalues"""
    c, s = math.cos(0.7), math.sin(0.7)
    rz = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]], dtype=torch.float64)
    r = rz @ rx
    d = lambda *v: torch.diag(torch.tensor(v, dtype=torch.float64))
    cov = torch.stack([d(0.25, 1.0, 4.0), r @ d(0.04, 0.5, 2.0) @ r.T, r @ d(0.3, 0.3, 1.5) @ r.T])
    return ((cov + cov.transpose(1, 2)) * 0.5).float().contiguous().to(dev)


def _cov_outputs(dev):
    return torch.full((3, 3), math.nan, device=dev), torch.full((3, 4), math.nan, device=dev)


def _cov_longhand(dev, cov):
    scales, rots = _cov_outputs(dev)
    with torch.cuda.device(dev):
        assert _lib.lib().gm_cov_to_scale_rot(3, cov.data_ptr(), scales.data_ptr(), rots.data_ptr(), torch.cuda.current_stream(dev).cuda_stream) == 0
    torch.cuda.synchronize(dev)
    assert bool(torch.isfinite(scales).all()) and bool(torch.isfinite(rots).all())
    return scales, rots


@pytest.mark.parametrize("dev", [torch.device("cuda", 0), torch.device("cuda")], ids=["cuda:0", "cuda without an index"])
def test_without_a_workspace(dev):
    cov = _covariances(dev)
    want = _cov_longhand(dev, cov)
    scales, rots = _cov_outputs(dev)
    _op.enqueue(dev, "gm_cov_to_scale_rot", 3, cov, scales, rots)
    torch.cuda.synchronize(dev)
    assert torch.equal(scales, want[0]) and torch.equal(rots, want[1])


def test_with_a_workspace():
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    pts = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.5, 0.5, 3.0]], device=dev)
    want = torch.zeros((4,), device=dev)
    with torch.cuda.device(dev):
        nbytes = lib.gm_knn_workspace_bytes(4)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        assert lib.gm_knn(4, pts.data_ptr(), want.data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream) == 0
    got = torch.zeros((4,), device=dev)
    ws2 = _op.workspace(dev, "gm_knn_workspace_bytes", 4)
    assert ws2.dtype is torch.uint8 and ws2.device == dev and ws2.numel() == nbytes
    _op.enqueue(dev, "gm_knn", 4, pts, got, workspace=ws2)
    torch.cuda.synchronize(dev)
    assert bool((want > 0).all()) and torch.equal(got, want)


def test_with_an_optional_null():
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    pos, campos = torch.randn((2, 3), generator=g).to(dev), torch.tensor([0.5, -2.0, 4.0], device=dev)
    shs = (torch.randn((2, 16, 3), generator=g) * 0.3).to(dev)
    want, got = torch.full((2, 3), math.nan, device=dev), torch.full((2, 3), math.nan, device=dev)
    with torch.cuda.device(dev):
        assert _lib.lib().gm_sh_colors(2, 3, 16, pos.data_ptr(), campos.data_ptr(), None, shs.data_ptr(), want.data_ptr(),
                                       torch.cuda.current_stream(dev).cuda_stream) == 0
    _op.enqueue(dev, "gm_sh_colors", 2, 3, 16, pos, campos, None, shs, got)
    torch.cuda.synchronize(dev)
    assert bool(torch.isfinite(want).all()) and torch.equal(got, want)


def test_on_a_side_stream():
    """Issued inside torch.cuda.stream(s) and read after s.synchronize() alone.  The default stream is kept busy meanwhile (a spin of a
    few milliseconds at most), so a call that went to it instead of s would not have run yet and the outputs would still be NaN."""
    dev = torch.device("cuda", 0)
    cov = _covariances(dev)
    want = _cov_longhand(dev, cov)
    scales, rots = _cov_outputs(dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    torch.cuda._sleep(2_000_000)
    with torch.cuda.stream(s):
        _op.enqueue(dev, "gm_cov_to_scale_rot", 3, cov, scales, rots)
        s.synchronize()
        got = scales.cpu(), rots.cpu()
    torch.cuda.synchronize(dev)
    assert torch.equal(got[0], want[0].cpu()) and torch.equal(got[1], want[1].cpu())


def test_on_a_device_that_is_not_current():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    dev = torch.device("cuda", 1)
    torch.cuda.set_device(0)
    cov = _covariances(dev)
    want = _cov_longhand(dev, cov)
    scales, rots = _cov_outputs(dev)
    assert torch.cuda.current_device() == 0
    _op.enqueue(dev, "gm_cov_to_scale_rot", 3, cov, scales, rots)
    assert torch.cuda.current_device() == 0
    torch.cuda.synchronize(dev)
    assert torch.equal(scales, want[0]) and torch.equal(rots, want[1])


def test_a_refused_call_surfaces():
    """gm_knn(5, NULL, NULL, NULL, 0, stream) returns 1 before any GPU work (test_abi.py).  The NULL workspace and its size go in as plain
    arguments: workspace=None means an entry point without one, and gm_knn's C signature needs the two slots filled."""
    dev = torch.device("cuda", 0)
    with pytest.raises(_lib.GmeshError):
        _op.enqueue(dev, "gm_knn", 5, None, None, None, 0, workspace=None)
    torch.cuda.synchronize(dev)
