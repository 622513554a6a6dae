#!/usr/bin/env python
"""Device time of one ArapSolver.solve at its defaults (gm_arap_solve: one init launch, then two launches per outer iteration), HIP events,
median of 20 after 5 warm-ups, on preallocated buffers (out=...), from the rest pose:
    the C3 torus torus_mesh(100, 75) (7.5 k vertices) and torus_mesh(300, 200) (60 k vertices),
    handles: the ring |atan2(z, x)| < 0.25 held, the ring ||atan2(z, x)| - pi| < 0.25 rotated by 0.6 about z and lifted by 0.8.
Beside each: the CG steps the solves took and their final residuals (one extra call with want_stats, outside the timed window), the
same at 400 steps / 1e-10, and the time of a solve with 1 CG step per outer iteration (the launches and local steps alone).
    python tools/arap_time.py"""
import math, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
from gaussianmesh_amd import _lib, scenes
from gaussianmesh_amd.arap import ArapSolver

dev = torch.device("cuda:0")


def median_ms(fn, reps=20, warm=5):
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


def ring_handles(V0):
    ang = np.arctan2(V0[:, 2].astype(np.float64), V0[:, 0].astype(np.float64))
    still, moved = np.nonzero(np.abs(ang) < 0.25)[0], np.nonzero(np.abs(np.abs(ang) - math.pi) < 0.25)[0]
    c, s = math.cos(0.6), math.sin(0.6)
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    target = V0[moved].astype(np.float64) @ Rz.T + np.array([0.0, 0.8, 0.0])
    return np.concatenate([still, moved]), np.concatenate([V0[still].astype(np.float64), target], 0).astype(np.float32)


def main():
    for label, (nu, nv) in (("7.5k", (100, 75)), ("60k", (300, 200))):
        verts, faces = scenes.torus_mesh(nu, nv)
        V0 = verts.astype(np.float32)
        handles, targets = ring_handles(V0)
        solver = ArapSolver(V0, faces, handles, device=dev)
        tg = torch.as_tensor(targets, device=dev)
        out = torch.empty((len(V0), 3), dtype=torch.float32, device=dev)
        print("torus_mesh(%d, %d): %d vertices, %d handles, workspace %.2f MB" % (nu, nv, len(V0), len(handles), _lib.lib().gm_arap_workspace_bytes(len(V0)) / 1e6), flush=True)
        print("  solve, defaults (4 outer, <= 64 CG steps, 1e-6)   median %.3f ms (min %.3f, max %.3f)" % median_ms(lambda: solver.solve(tg, out=out)), flush=True)
        print("  solve, 4 outer, 1 CG step each                    median %.3f ms (min %.3f, max %.3f)" % median_ms(lambda: solver.solve(tg, out=out, cg_iterations=1)), flush=True)
        for kw in (dict(), dict(cg_iterations=400, cg_tolerance=1e-10), dict(outer_iterations=10, cg_iterations=1000, cg_tolerance=1e-6)):
            st = solver.solve(tg, want_stats=True, **kw)[1].cpu().numpy()
            print("  %s: CG steps per outer iteration (x y z) %s, final |r|/|b| at most %.2e, E %.6g -> %.6g" % (
                kw or "defaults", [tuple(int(v) for v in row[2:5]) for row in st], st[:, 5:8].max(), st[0, 0], st[-1, 1]), flush=True)


if __name__ == "__main__":
    main()
