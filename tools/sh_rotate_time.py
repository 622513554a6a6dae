#!/usr/bin/env python
"""Time of gm_sh_rotate (deform.rotate_sh's C call on preallocated buffers) at N = 1 M rows, M = 16, degree 3, out of place and in place:
HIP events, median after warm-ups.  Next to it the same arithmetic stated in torch on the device - sample SH(A^T d_j) . c at the 32
directions, multiply by the pseudo-inverse - as the yardstick, and the bytes the call has to move (192 B in + 192 B out + 36 B of rot
per row) over its time.  Asserts nothing; prints the largest difference between the two.
    python tools/sh_rotate_time.py [--rows N]"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
import numpy as np
import torch
from gaussianmesh_amd import _lib
import sh_rotate_ref as ref

dev = torch.device("cuda:0")
lib = _lib.lib()
N = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else 1000000
M, DEG, K = 16, 3, 32


def median_ms(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), float(min(out)), float(max(out))


def torch_basis(d):
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    C0, C1, C2, C3 = ref.C0, ref.C1, ref.C2, ref.C3
    return torch.stack([C0 * torch.ones_like(x), -C1 * y, C1 * z, -C1 * x, C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy),
                        C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy), C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
                        C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy), C3[6] * x * (xx - 3 * yy)], -1)


g = torch.Generator(device=dev); g.manual_seed(0)
shs = torch.randn((N, M, 3), device=dev, generator=g) * torch.tensor([0.5] + [0.1] * (M - 1), device=dev)[None, :, None]
q = torch.nn.functional.normalize(torch.randn((3, N, 4), device=dev, generator=g), dim=2)
r, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)
w = torch.distributions.Dirichlet(torch.ones(3, device=dev)).sample((N,))
rot = (w.t()[:, :, None] * Rm).sum(0).contiguous()                      # [N,9]: blends of three rotations, as gm_deform writes them
out = torch.empty_like(shs)
inplace = shs.clone()
st = torch.cuda.current_stream(dev).cuda_stream
D64 = ref.fibonacci_directions(K).astype(np.float32).astype(np.float64)
D = torch.tensor(D64, dtype=torch.float32, device=dev)
P = torch.tensor(np.linalg.pinv(ref.basis(D64)), dtype=torch.float32, device=dev)      # [16, K]


def call(src, dst):
    return lambda: _lib.check(lib.gm_sh_rotate(N, DEG, M, src.data_ptr(), rot.data_ptr(), dst.data_ptr(), st))


def torch_statement():
    dr = torch.einsum("nji,kj->nki", rot.view(N, 3, 3), D)             # A^T d_j
    f = torch.einsum("nkj,njc->nkc", torch_basis(dr), shs)             # the samples [N,K,3]
    return torch.einsum("jk,nkc->njc", P, f)


moved = N * (2 * M * 3 * 4 + 36)
for label, fn in (("gm_sh_rotate, out of place", call(shs, out)), ("gm_sh_rotate, in place", call(inplace, inplace))):
    med, lo, hi = median_ms(fn, 30, 5)
    print("%-28s N %d M %d deg %d: median %.4f ms (min %.4f, max %.4f) | %.1f MB moved -> %.2f TB/s" % (label, N, M, DEG, med, lo, hi, moved / 1e6,
                                                                                                       moved / med / 1e9), flush=True)
med, lo, hi = median_ms(torch_statement, 5, 2)
print("%-28s N %d M %d deg %d: median %.4f ms (min %.4f, max %.4f)" % ("torch, the same arithmetic", N, M, DEG, med, lo, hi), flush=True)
call(shs, out)()
print("largest |gm_sh_rotate - torch| = %.3g" % float((out - torch_statement()).abs().max()))
