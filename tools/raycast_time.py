#!/usr/bin/env python
"""Time of the first-hit ray cast behind mesh_pick (gm_ray_mesh, the whole launch chain: face records, cast, finish), HIP events, median
after warm-ups, at the three shapes its callers have:
    a pick:       1 ray x torus_mesh(300, 200) (120 000 faces)
    a selection:  one ray per vertex (60 000) x the same mesh
    a frame:      1920 x 1080 pixel rays x torus_mesh(100, 75) (15 000 faces)
and next to each the same formula stated in torch on the device, chunked over the rays so that a chunk's [rays, faces] temporaries stay
near 64 MB each - the yardstick the kernel has to beat.  The two are compared (faces and t bits) at every shape.
    python tools/raycast_time.py [--quick]        (--quick: the frame at 480 x 270)"""
import math, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
from gaussianmesh_amd import _lib, scenes
from gaussianmesh_amd.mesh_pick import camera_rays
from gaussianmesh_amd.renderer import Camera

dev = torch.device("cuda:0")
lib = _lib.lib()
PAIRS = 1 << 24            # ray-face pairs per chunk of the torch statement


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


def kernel_chain(O, D, V, F):
    """the C call alone on preallocated buffers (no allocation, no copy inside the timed window)"""
    R, Vm, nF = O.shape[0], V.shape[0], F.shape[0]
    t = torch.empty(R, device=dev); face = torch.empty(R, dtype=torch.int32, device=dev); uv = torch.empty((R, 2), device=dev)
    nbytes = lib.gm_ray_mesh_workspace_bytes(R, nF)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    fn = lambda: _lib.check(lib.gm_ray_mesh(R, O.data_ptr(), D.data_ptr(), Vm, V.data_ptr(), nF, F.data_ptr(), 0.0, math.inf, t.data_ptr(),
                                            face.data_ptr(), uv.data_ptr(), ws.data_ptr(), nbytes, st))
    return fn, (t, face, uv), nbytes


def torch_chain(O, D, V, F):
    """gm_ray_mesh's formula in torch, per component as the definition writes it; per chunk of rays the smallest accepted t and the first
    face that has it (a hit at t = +inf aside, which these inputs do not have)"""
    R = O.shape[0]
    A = V[F[:, 0].long()]
    E1, E2 = V[F[:, 1].long()] - A, V[F[:, 2].long()] - A
    ax, ay, az = (A[:, k][None] for k in range(3))
    e1x, e1y, e1z = (E1[:, k][None] for k in range(3))
    e2x, e2y, e2z = (E2[:, k][None] for k in range(3))
    t_out = torch.empty(R, device=dev); f_out = torch.empty(R, dtype=torch.int64, device=dev)
    step = max(1, PAIRS // F.shape[0])
    inf = torch.tensor(math.inf, device=dev)

    def run():
        for s in range(0, R, step):
            o, d = O[s:s + step], D[s:s + step]
            ox, oy, oz = (o[:, k:k + 1] for k in range(3))
            dx, dy, dz = (d[:, k:k + 1] for k in range(3))
            px, py, pz = dy * e2z - dz * e2y, dz * e2x - dx * e2z, dx * e2y - dy * e2x
            det = (e1x * px + e1y * py) + e1z * pz
            sx, sy, sz = ox - ax, oy - ay, oz - az
            qx, qy, qz = sy * e1z - sz * e1y, sz * e1x - sx * e1z, sx * e1y - sy * e1x
            inv = 1.0 / det
            u = ((sx * px + sy * py) + sz * pz) * inv
            v = ((dx * qx + dy * qy) + dz * qz) * inv
            t = ((e2x * qx + e2y * qy) + e2z * qz) * inv
            hit = (u >= 0) & (v >= 0) & ((u + v) <= 1) & (t >= 0)
            best, k = torch.min(torch.where(hit, t + 0.0, inf), dim=1)
            t_out[s:s + step] = best
            f_out[s:s + step] = torch.where(best < inf, k, -1)
    return run, (t_out, f_out)


t32 = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
quick = "--quick" in sys.argv
big = tuple(t32(x, dt) for x, dt in zip(scenes.torus_mesh(300, 200), (torch.float32, torch.int32)))
mid = tuple(t32(x, dt) for x, dt in zip(scenes.torus_mesh(100, 75), (torch.float32, torch.int32)))
W, H = (480, 270) if quick else (1920, 1080)
cam = Camera(scenes.look_at_camera((4, 3, 5), (0, 0, 0), W, H), dev)
eye = cam.camera_center.reshape(1, 3)
pix = torch.stack(torch.meshgrid(torch.arange(W, device=dev), torch.arange(H, device=dev), indexing="xy"), -1).reshape(-1, 2).float()
frame_o, frame_d = camera_rays(cam, pix)
aimed = (eye.contiguous(), (big[0][:1] - eye).contiguous())          # the pick: towards vertex 0 of the torus (the frame's centre looks through its hole)
shapes = [("pick: 1 ray x 120k faces", aimed[0], aimed[1], big, (50, 5), (20, 3)),
          ("selection: 60k vertex rays x 120k faces", eye.expand(big[0].shape[0], 3).contiguous(), (big[0] - eye).contiguous(), big, (10, 2), (3, 1)),
          ("frame: %d x %d rays x 15k faces" % (W, H), frame_o, frame_d, mid, (5, 1), (2, 1))]
for label, O, D, (V, F), kreps, treps in shapes:
    kfn, (kt, kface, _), nbytes = kernel_chain(O, D, V, F)
    tfn, (tt, tface) = torch_chain(O, D, V, F)
    k = median_ms(kfn, *kreps)
    t = median_ms(tfn, *treps)
    same_face = int((kface.long() == tface).sum()); same_t = int((kt.view(torch.int32) == tt.view(torch.int32)).sum())
    pairs = O.shape[0] * F.shape[0]
    print("%-42s gm_ray_mesh median %.3f ms (min %.3f, max %.3f; %.1f G pairs/s, workspace %.1f MB) | torch median %.3f ms (min %.3f, max %.3f) | "
          "%.1f x | hits %d, same face %d / %d, same t bits %d" % ((label,) + k + (pairs / k[0] / 1e6, nbytes / 1e6) + t + (t[0] / k[0], int((kface >= 0).sum()),
                                                                    same_face, O.shape[0], same_t)), flush=True)
