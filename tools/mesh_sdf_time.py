#!/usr/bin/env python
"""Time of a mesh's signed-distance grid (mesh_sdf.grid_values: whole calls, slabs, allocations and sample positions included), split
into its closest-face part (gm_closest_face) and its winding part (gm_mesh_winding) on the same samples, with a chunked torch
float64 statement of the same sum next to the winding part as the baseline.  HIP events around each call after a synchronize,
2 warm-ups, then 5 repetitions (3 where one takes seconds): median, min and max.
    lattices 64^3 and 128^3  x  tori of 1 k, 15 k and 120 k faces (scenes.torus_mesh 25 x 20, 100 x 75, 300 x 200)
The torch baseline evaluates 2 atan2(det, den) per (sample, face) in float64 with torch operators, 2^24 pairs at a time, and sums over
the faces (torch's own order: it is a baseline for time, not for bits); at 128^3 x 120 k it is extrapolated from 1/16 of the samples.
Last: the share of the grid in what `edit_sequence --dynamics --obstacle_mesh` does before its first simulated step
(SdfGrid.from_mesh of a 15 k-face obstacle at the CLI's default resolution 128 against loading the 64-pixel test scene's object).
    python tools/mesh_sdf_time.py [--quick]"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
from gaussianmesh_amd import _lib, mesh_sdf, scenes
from gaussianmesh_amd.dynamics import SdfGrid
from gaussianmesh_amd.mesh_bind import closest_faces

dev = torch.device("cuda:0")
quick = "--quick" in sys.argv
t = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)


def timed(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), float(min(out)), float(max(out))


def slabs(total, F):
    """grid_values' slabs of the lattice"""
    chunks = (F + mesh_sdf.WN_CHUNK - 1) // mesh_sdf.WN_CHUNK
    slab = max(256, mesh_sdf.SLAB_PARTIAL_BYTES // (8 * chunks) // 256 * 256)
    return [(s, min(s + slab, total)) for s in range(0, total, slab)]


def torch_winding(P, V, F, pairs=1 << 24):
    """sum_f 2 atan2(det, den) / (4 pi) in float64 with torch operators, `pairs` (sample, face) pairs at a time"""
    A, B, C = (V[F[:, k].long()].double() for k in range(3))
    out = torch.empty(P.shape[0], dtype=torch.float64, device=P.device)
    rows = max(1, pairs // F.shape[0])
    for s in range(0, P.shape[0], rows):
        p = P[s:s + rows].double()[:, None, :]
        a, b, c = A[None] - p, B[None] - p, C[None] - p
        la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
        det = (a * torch.linalg.cross(b, c, dim=-1)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        out[s:s + rows] = (2.0 * torch.atan2(det, den)).sum(dim=1) / (4.0 * np.pi)
    return out


fmt = lambda r: "median %9.3f ms (min %9.3f, max %9.3f)" % r
meshes = [("1k", scenes.torus_mesh(25, 20)), ("15k", scenes.torus_mesh(100, 75)), ("120k", scenes.torus_mesh(300, 200))]
sides = (64,) if quick else (64, 128)
for side in sides:
    for label, (V, F) in meshes:
        V, F = V.astype(np.float32), F
        Vd, Fd = t(V), t(F, torch.int32)
        nF, total = len(F), side ** 3
        lo, hi = V.min(axis=0) - 1.0, V.max(axis=0) + 1.0
        voxel = float((hi - lo).max()) / side
        shape = (side, side, side)
        pairs = total * nF
        reps = 3 if pairs > 5e10 else 5
        whole = timed(lambda: mesh_sdf.grid_values(Vd, Fd, lo, voxel, shape, device=dev), reps)
        parts = slabs(total, nF)
        pts = [mesh_sdf.lattice_points(lo, voxel, shape, s, e, dev) for s, e in parts]
        close = timed(lambda: [closest_faces(p, Vd, Fd) for p in pts], reps)
        wind = timed(lambda: [mesh_sdf.winding_numbers(p, Vd, Fd) for p in pts], reps)
        print("%3d^3 x %4s faces (%d slab%s): grid_values %s | closest-face part %s | winding part %s = %.1f G pairs/s"
              % (side, label, len(parts), "" if len(parts) == 1 else "s", fmt(whole), fmt(close), fmt(wind), pairs / wind[0] / 1e6), flush=True)
        every = 16 if pairs > 1e11 else 1
        allp = torch.cat(pts)[::every].contiguous()
        base = timed(lambda: torch_winding(allp, Vd, Fd), 3, 1)
        w_t, w_k = torch_winding(allp, Vd, Fd), torch.cat([mesh_sdf.winding_numbers(p, Vd, Fd) for p in pts])[::every]
        print("      torch float64 baseline of the winding part%s: %s, %.1f x the kernels; max |w_torch - w| = %.2g"
              % (" (1/16 of the samples, x 16)" if every > 1 else "", fmt(tuple(x * every for x in base)), base[0] * every / wind[0],
                 float((w_t - w_k).abs().max())), flush=True)

# the share of the grid in edit_sequence --obstacle_mesh's setup: SdfGrid.from_mesh (host checks, the lattice, the kernels, the prepare
# kernel) against loading the object the CLI simulates
import tempfile
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
from gaussianmesh_amd.edittool import ObjectVisualTool
from test_gpu_arap import _scene64
V, F = meshes[1][1]
with tempfile.TemporaryDirectory() as d:
    _scene64(d)
    def load():
        tool = ObjectVisualTool()
        tool.get_camera(d)
        tool.add_gaussian(os.path.join(d, "object.ply"), os.path.join(d, "rest.obj"), "Object")
        torch.cuda.synchronize()
    def grid(res):
        SdfGrid.from_mesh(V, F, resolution=res)
        torch.cuda.synchronize()
    for fn, arg in ((load, ()), (grid, (128,))):
        fn(*arg)
    wall = lambda fn, *a: (lambda t0: (fn(*a), time.perf_counter() - t0)[1])(time.perf_counter())
    tl = sorted(wall(load) for _ in range(5))
    for res in (64, 128):
        tg = sorted(wall(grid, res) for _ in range(5))
        print("edit_sequence --obstacle_mesh setup, wall clock, median of 5 (min, max): loading the object %.1f ms (%.1f, %.1f); SdfGrid.from_mesh of 15 k "
              "faces at resolution %d: %.1f ms (%.1f, %.1f) = %.0f %% of the two" % (1e3 * tl[2], 1e3 * tl[0], 1e3 * tl[4], res, 1e3 * tg[2], 1e3 * tg[0], 1e3 * tg[4],
                                                                                      100.0 * tg[2] / (tg[2] + tl[2])))
