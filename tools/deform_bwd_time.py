#!/usr/bin/env python
"""Time of gm_deform_shade_bwd (the C call on preallocated buffers) at the C3 workload: N = 1 M rows bound to the 100 x 75 torus
(7.5 k vertices), degree 3, every optional output off (the pose-fitting call) and on.  HIP events, median after warm-ups.  Next to it
the bytes the call has to move over its time - per row 12 tri + 12 w + 36 cov + 12 pos + 192 shs + 12 + 24 + 12 upstream read and 84
workspace written by the row kernel, 4 entry + 4 w + 84 workspace read per corner (x 3) by the vertex kernel; the 7.5 k-vertex tables stay
in L2 - and the same algebra stated in torch autograd (index_add_ behind the gathers) on the device as the yardstick.  Asserts nothing;
prints the largest difference between the two.
    python tools/deform_bwd_time.py [--rows N]"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
from gaussianmesh_amd import _lib, scenes
from gaussianmesh_amd.deform import DeformBinding
from gaussianmesh_amd.renderer import eval_sh_torch

dev = torch.device("cuda:0")
lib = _lib.lib()
N = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else 1000000
M, DEG = 16, 3


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


T = lambda a, dt=torch.float32: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
verts, faces = scenes.torus_mesh(100, 75)
V1, Rv, Sv = scenes.twist_bend_frame(verts, t=9)
cl = scenes.bind_cloud_to_mesh(N, verts, faces, seed=1)
Vm = verts.shape[0]
tri, w = T(cl["tri"], torch.int32), T(cl["weights"])
cov, pos, shs = T(scenes.cov3d_from_scale_rot(cl["scales"], cl["rots"])).reshape(N, 9), T(cl["means"]), T(cl["shs"])
dV, Rv, Sv = T(V1 - verts), T(Rv).reshape(Vm, 9), T(Sv).reshape(Vm, 9)
campos = T([4.0, 1.0, -3.0])
g = torch.Generator(device=dev); g.manual_seed(0)
g_pos, g_cov6, g_rgb = (torch.randn((N, k), device=dev, generator=g) for k in (3, 6, 3))
binding = DeformBinding(tri, w, Vm)
f = dict(dtype=torch.float32, device=dev)
g_dV, g_Rv, g_Sv = torch.empty((Vm, 3), **f), torch.empty((Vm, 9), **f), torch.empty((Vm, 9), **f)
g_shs, g_cov, g_rest = torch.empty((N, M, 3), **f), torch.empty((N, 9), **f), torch.empty((N, 3), **f)
ws = torch.empty((lib.gm_deform_shade_bwd_workspace_bytes(N, Vm),), dtype=torch.uint8, device=dev)
st = torch.cuda.current_stream(dev).cuda_stream
P = lambda t: None if t is None else t.data_ptr()


def call(optional):
    o = (g_shs, g_cov, g_rest) if optional else (None, None, None)
    return lambda: _lib.check(lib.gm_deform_shade_bwd(N, DEG, M, Vm, *[P(t) for t in (tri, w, dV, Rv, Sv, cov, pos, shs, campos, binding.inc_offsets,
                                                                                    binding.inc_entries, g_pos, g_cov6, g_rgb, g_dV, g_Rv, g_Sv) + o],
                                                      ws.data_ptr(), ws.numel(), st))


def torch_statement():
    """the forward in torch on leaf tables, loss = <g, outputs>, autograd: the gathers' backward is index_add_"""
    a, b, c = (t.clone().requires_grad_(True) for t in (dV, Rv, Sv))
    t64 = tri.long()
    blend = lambda tab: (w[:, 0:1] * tab[t64[:, 0]] + w[:, 1:2] * tab[t64[:, 1]]) + w[:, 2:3] * tab[t64[:, 2]]
    d, Rb, Sb = blend(a), blend(b).view(N, 3, 3), blend(c).view(N, 3, 3)
    RS = Rb.transpose(1, 2) @ Sb
    O = RS @ cov.view(N, 3, 3) @ RS.transpose(1, 2)
    cov6 = torch.stack([O[:, 0, 0], O[:, 0, 1], O[:, 0, 2], O[:, 1, 1], O[:, 1, 2], O[:, 2, 2]], 1)
    npos = pos + d
    v = npos - campos
    xyz = (Rb @ (v / v.norm(dim=1, keepdim=True))[:, :, None])[:, :, 0]
    rgb = torch.clamp_min(eval_sh_torch(DEG, shs, xyz) + 0.5, 0.0)
    ((npos * g_pos).sum() + (cov6 * g_cov6).sum() + (rgb * g_rgb).sum()).backward()
    return a.grad, b.grad, c.grad


rows_read = 12 + 12 + 36 + 12 + 192 + 12 + 24 + 12
for label, optional, extra in (("gm_deform_shade_bwd, tables only", False, 0), ("gm_deform_shade_bwd, all outputs", True, 192 + 36 + 12)):
    moved = N * (rows_read + 84 + extra + 3 * (4 + 4 + 84))
    med, lo, hi = median_ms(call(optional), 30, 5)
    print("%-34s N %d Vm %d deg %d: median %.4f ms (min %.4f, max %.4f) | %.1f MB moved -> %.2f TB/s" % (label, N, Vm, DEG, med, lo, hi, moved / 1e6,
                                                                                                         moved / med / 1e9), flush=True)
med, lo, hi = median_ms(torch_statement, 5, 2)
print("%-34s N %d Vm %d deg %d: median %.4f ms (min %.4f, max %.4f)" % ("torch autograd, the same algebra", N, Vm, DEG, med, lo, hi), flush=True)
call(False)()
ref = torch_statement()
print("largest |gm_deform_shade_bwd - torch| / max|torch|: " + ", ".join("%s %.3g" % (n, float((a - b).abs().max() / b.abs().max()))
                                                                         for n, a, b in zip(("g_dV", "g_Rv", "g_Sv"), (g_dV, g_Rv, g_Sv), ref)))
