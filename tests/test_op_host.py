"""gaussianmesh_amd._op on the host: the pointer, the refusal and the conversions the operator modules share.  No device is touched."""
import numpy as np
import pytest
import torch

from gaussianmesh_amd import _lib, _op


def test_ptr():
    t = torch.arange(6.0)
    assert _op.ptr(None) is None
    assert _op.ptr(t) == t.data_ptr()
    assert _op.ptr(t[2:]) == t.data_ptr() + 2 * t.element_size()


@pytest.mark.parametrize("x", [torch.zeros(3), None, np.zeros(3, np.float32), torch.device("cpu")], ids=["cpu tensor", "None", "numpy", "cpu device"])
def test_need_cuda_refuses(x):
    with pytest.raises(_lib.GmeshError) as e:
        _op.need_cuda(x, "X", "Y")
    assert str(e.value) == "X needs Y on a HIP (cuda) device; there is no CPU path"


def test_need_cuda_accepts_a_cuda_device():
    assert _op.need_cuda(torch.device("cuda", 0), "X", "Y") is None          # (constructed, never used)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
def test_on_device(dtype):
    base = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    for a in (base.t(), base.t().numpy()):                                   # neither is contiguous
        out = _op.on_device(a, dtype, torch.device("cpu"))
        assert out.dtype is dtype and out.is_contiguous() and out.device.type == "cpu"
        assert torch.equal(out, base.t().to(dtype))


def test_f32():
    base = torch.arange(12, dtype=torch.float64).reshape(3, 4).requires_grad_()
    out = _op.f32(base.t())
    assert out.dtype is torch.float32 and out.is_contiguous() and not out.requires_grad
    assert torch.equal(out, base.detach().t().float())


def test_host_round_trip():
    a = np.arange(6, dtype=np.int32).reshape(2, 3)
    assert _op.host(a) is a
    back = _op.host(torch.from_numpy(a.copy()).requires_grad_(False))
    assert isinstance(back, np.ndarray) and back.dtype == a.dtype and np.array_equal(back, a)
    assert np.array_equal(_op.host(torch.tensor([1.5, 2.5], requires_grad=True)), np.array([1.5, 2.5], np.float32))
    assert np.array_equal(_op.host([[1, 2], [3, 4]]), np.array([[1, 2], [3, 4]]))
