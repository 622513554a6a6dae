#!/usr/bin/env python
"""Device time of one ArapSolver.solve at its defaults, HIP events, median of 20 after 5 warm-ups, on preallocated buffers (out=...), from
the rest pose, for either global step or both in one process (--global_step column | grid | both; column = gm_arap_solve: one init
launch, then two launches per outer iteration; grid = gm_arap_solve_grid: rows over the whole chip, two launches per CG step):
    the C3 torus torus_mesh(100, 75) (7.5 k vertices) and torus_mesh(300, 200) (60 k vertices),
    handles: the ring |atan2(z, x)| < 0.25 held, the ring ||atan2(z, x)| - pi| < 0.25 rotated by 0.6 about z and lifted by 0.8.
Beside each: the CG steps the solves took and their final residuals (one extra call with want_stats, outside the timed window), the
same at 400 steps / 1e-10, and the time of a solve with 1 CG step per outer iteration (the launches and local steps alone).
Then a warm-started drag: ten frames of a handle path (the moved ring at 1/10, 2/10, ... of its rotation and lift), each frame solved at
the defaults from the previous frame's solution, timed as one window; beside it the CG steps each frame's last outer iteration took.
And a solve with the handles at rest, which converges before its first step: on the grid path the price of a solve's launches when
every product / update pair returns after reading the carried state.
With --sizes a list of NUxNV tori instead of the two above (the crossover between the two global steps).
With --batch B1,B2,... instead of all the above: a 32-frame drag (the moved ring at 1/32, 2/32, ... of its path) through
ArapSolver.solve_sequence at each batch size, on torus_mesh(32, 32), (100, 75) and (300, 200) unless --sizes says otherwise and for both
global steps unless --global_step names one: milliseconds per frame (the whole drag as one window of device events, median of 20 after 5
warm-ups, over 32) and, from a separate untimed pass with want_stats, the final energy of every frame.  The baseline beside them is
the same 32 frames through the chain of solve() calls, each warm-started from the frame before: the code path without batches.
    python tools/arap_time.py [--global_step both] [--sizes 16x16,40x25,...] [--batch 1,2,4,8,16]"""
import argparse, math, os, sys
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


def ring_handles(V0, fraction=1.0):
    ang = np.arctan2(V0[:, 2].astype(np.float64), V0[:, 0].astype(np.float64))
    still, moved = np.nonzero(np.abs(ang) < 0.25)[0], np.nonzero(np.abs(np.abs(ang) - math.pi) < 0.25)[0]
    c, s = math.cos(0.6 * fraction), math.sin(0.6 * fraction)
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    target = V0[moved].astype(np.float64) @ Rz.T + np.array([0.0, 0.8 * fraction, 0.0])
    return np.concatenate([still, moved]), np.concatenate([V0[still].astype(np.float64), target], 0).astype(np.float32)


def batch_report(sizes, paths, batches, frames=32):
    for nu, nv in sizes:
        verts, faces = scenes.torus_mesh(nu, nv)
        V0 = verts.astype(np.float32)
        handles = ring_handles(V0)[0]
        solver = ArapSolver(V0, faces, handles, device=dev)
        pos = torch.as_tensor(np.stack([ring_handles(V0, (t + 1) / float(frames))[1] for t in range(frames)], 0), device=dev)
        out = torch.empty((len(V0), 3), dtype=torch.float32, device=dev)
        print("torus_mesh(%d, %d): %d vertices, %d handles, %d workgroups of 256 rows, %d-frame drag" % (
            nu, nv, len(V0), len(handles), (len(V0) + 255) // 256, frames), flush=True)
        for path in paths:
            g = dict(global_step=path)

            def chain(stats=False):
                cur, energy = None, []
                for t in range(frames):
                    cur = solver.solve(pos[t], init=cur, out=out, want_stats=stats, **g)
                    if stats:
                        energy.append(cur[1][-1, 1]); cur = cur[0]
                return energy
            base = median_ms(chain)
            e_base = torch.stack(chain(True)).cpu().numpy()
            print(" global_step=%s" % path, flush=True)
            print("  baseline: chain of solve(), warm-started   %8.3f ms / frame (drag median %.3f ms, min %.3f, max %.3f)" % ((base[0] / frames,) + base), flush=True)
            print("    final E per frame: %s" % " ".join("%.6g" % e for e in e_base), flush=True)
            for B in batches:
                m = median_ms(lambda: solver.solve_sequence(pos, batch=B, **g))
                e = solver.solve_sequence(pos, batch=B, want_stats=True, **g)[1][:, -1, 1].cpu().numpy()
                rel = e / e_base
                print("  solve_sequence(batch=%-2d)                   %8.3f ms / frame (drag median %.3f ms, min %.3f, max %.3f)  baseline / this %.2fx" % (
                    (B, m[0] / frames) + m + (base[0] / m[0],)), flush=True)
                print("    final E per frame: %s" % " ".join("%.6g" % v for v in e), flush=True)
                print("    E / baseline's E per frame: mean %.4f, max %.4f (frame %d); sum over the drag %.4f" % (
                    rel.mean(), rel.max(), int(rel.argmax()), e.sum() / e_base.sum()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--global_step", choices=("column", "grid", "both"), default=None)
    ap.add_argument("--sizes", type=str, default=None)
    ap.add_argument("--batch", type=str, default=None)
    args = ap.parse_args()
    if args.batch is not None:
        sizes = [tuple(int(v) for v in item.split("x")) for item in (args.sizes or "32x32,100x75,300x200").split(",")]
        return batch_report(sizes, ("column", "grid") if args.global_step in (None, "both") else (args.global_step,), [int(b) for b in args.batch.split(",")])
    args.global_step, args.sizes = args.global_step or "column", args.sizes or "100x75,300x200"
    paths = ("column", "grid") if args.global_step == "both" else (args.global_step,)
    for nu, nv in (tuple(int(v) for v in item.split("x")) for item in args.sizes.split(",")):
        verts, faces = scenes.torus_mesh(nu, nv)
        V0 = verts.astype(np.float32)
        handles, targets = ring_handles(V0)
        solver = ArapSolver(V0, faces, handles, device=dev)
        tg = torch.as_tensor(targets, device=dev)
        rest_tg = torch.as_tensor(V0[handles], device=dev)
        path_tg = [torch.as_tensor(ring_handles(V0, (k + 1) / 10.0)[1], device=dev) for k in range(10)]
        out = torch.empty((len(V0), 3), dtype=torch.float32, device=dev)
        nbytes = {"column": _lib.lib().gm_arap_workspace_bytes(len(V0)), "grid": _lib.lib().gm_arap_grid_workspace_bytes(len(V0))}
        print("torus_mesh(%d, %d): %d vertices, %d handles, %d workgroups of 256 rows" % (nu, nv, len(V0), len(handles), (len(V0) + 255) // 256), flush=True)
        medians = {}
        for path in paths:
            g = dict(global_step=path)

            def drag(stats=False):
                cur, steps = None, []
                for t in path_tg:
                    cur = solver.solve(t, init=cur, out=out, want_stats=stats, **g)
                    if stats:
                        steps.append(cur[1]); cur = cur[0]
                return steps
            print(" global_step=%s, workspace %.2f MB" % (path, nbytes[path] / 1e6), flush=True)
            m = medians[path] = [median_ms(lambda: solver.solve(tg, out=out, **g)), median_ms(lambda: solver.solve(tg, out=out, cg_iterations=1, **g)),
                                 median_ms(drag), median_ms(lambda: solver.solve(rest_tg, out=out, **g))]
            print("  solve, defaults (4 outer, <= 64 CG steps, 1e-6)   median %.3f ms (min %.3f, max %.3f)" % m[0], flush=True)
            print("  solve, 4 outer, 1 CG step each                    median %.3f ms (min %.3f, max %.3f)" % m[1], flush=True)
            print("  warm-started drag, 10 frames at the defaults      median %.3f ms (min %.3f, max %.3f)" % m[2], flush=True)
            print("    CG steps of each frame's last outer iteration (x y z): %s" % [tuple(int(v) for v in st[-1, 2:5].tolist()) for st in drag(True)], flush=True)
            print("  solve at the rest pose (0 CG steps: converged at once) median %.3f ms (min %.3f, max %.3f)" % m[3], flush=True)
            for kw in (dict(), dict(cg_iterations=400, cg_tolerance=1e-10), dict(outer_iterations=10, cg_iterations=1000, cg_tolerance=1e-6)):
                st = solver.solve(tg, want_stats=True, **kw, **g)[1].cpu().numpy()
                print("  %s: CG steps per outer iteration (x y z) %s, final |r|/|b| at most %.2e, E %.6g -> %.6g" % (
                    kw or "defaults", [tuple(int(v) for v in row[2:5]) for row in st], st[:, 5:8].max(), st[0, 0], st[-1, 1]), flush=True)
        if len(paths) == 2:
            print(" column / grid: defaults %.2fx, 1 CG step %.2fx, drag %.2fx" % tuple(medians["column"][k][0] / medians["grid"][k][0] for k in range(3)), flush=True)


if __name__ == "__main__":
    main()
