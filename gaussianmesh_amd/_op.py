"""The one place where an operator module hands torch tensors to libgmesh_hip.so: which device is made current, which stream is passed,
where a workspace is allocated, how None becomes NULL - and the refusal and the conversions the modules share.  _lib stays ctypes-only;
the rasterizer's frame path spells its own calls out and takes ptr / on / raw_stream from here."""
import numpy as np
import torch

from . import _lib


def ptr(t):
    return None if t is None else t.data_ptr()


class on:
    """`with torch.cuda.device(d)` for the usual case that d already is the current device: one C call instead of the context
    manager's four (a pipelined render loop enters it three times per frame)."""
    __slots__ = ("guard",)

    def __init__(self, device):
        self.guard = None if torch.cuda.current_device() == device.index else torch.cuda.device(device)

    def __enter__(self):
        if self.guard is not None:
            self.guard.__enter__()

    def __exit__(self, *a):
        if self.guard is not None:
            return self.guard.__exit__(*a)


def raw_stream(device):
    """torch.cuda.current_stream(device).cuda_stream without the Stream object; torch.device("cuda"), which names no index (the default
    of ArapSolver, SurfaceGraph and TsdfVolume), is the current device here as it is there"""
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device() if device.index is None else device.index)


def enqueue(device, name, *args, workspace=None, stream=None):
    """_lib.check(lib.<name>(*args, [workspace pointer, workspace bytes,] stream)) with `device` current.  A tensor among args goes as
    its data pointer, everything else (None, numbers, ctypes arrays and pointers) as it is; workspace: a uint8 tensor; stream: a raw
    handle, by default torch's current stream of `device`.  For the entry points that end `..., void* stream` (with a workspace:
    `..., void* workspace, size_t workspace_bytes, void* stream`); the caller keeps the tensors alive, as with a call spelled out."""
    call = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    if workspace is not None:
        call += (workspace.data_ptr(), workspace.numel())
    with on(device):
        _lib.check(getattr(_lib.lib(), name)(*call, raw_stream(device) if stream is None else stream))


def workspace(device, size_name, *size_args):
    """a fresh uint8 tensor of lib.<size_name>(*size_args) bytes on `device`"""
    with on(device):
        return torch.empty((getattr(_lib.lib(), size_name)(*size_args),), dtype=torch.uint8, device=device)


def need_cuda(x, who, what):
    """x: a tensor, a device, or anything else (refused)"""
    device = x.device if torch.is_tensor(x) else x
    if not isinstance(device, torch.device) or device.type != "cuda":
        raise _lib.GmeshError("%s needs %s on a HIP (cuda) device; there is no CPU path" % (who, what))


def f32(t):
    return t.detach().contiguous().float()


def on_device(a, dtype, device):
    """a tensor or host array as a contiguous tensor of `dtype` on `device`"""
    return (a.detach().to(device=device, dtype=dtype) if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=device)).contiguous()


def host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
