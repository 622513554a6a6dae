#!/usr/bin/env python
"""Device time of PoseInterpolator.between as whole calls, HIP events, median of 20 after 5 warm-ups, on a preallocated out=, at
T = 1, 8 and 64 in-betweens (evenly spaced in (0, 1)) of two key pairs:
    rest -> a twist about y (0.2 .. 0.8 rad) with a 1.3x stretch,   that twist -> the rest pose turned 179 degrees about its centroid,
on torus_mesh(37, 29) (1073 vertices) and the C3 torus torus_mesh(100, 75) (7.5 k vertices), anchors=None (the centroid rule).
Beside each: the largest CG step count any (frame, coordinate) used at the defaults and the largest final residual (one extra call
with want_stats, outside the timed window), and the same at 2000 steps / 1e-6: the steps the tolerance alone asks for.
Then what the parent commit offers for in-betweens: ArapSolver.solve_sequence at its defaults (batch=4) over the same number of frames,
handles as in tools/arap_time.py (one ring held, the opposite ring at k / T of its rotation and lift) - a full ARAP solve per frame.
    python tools/pose_interp_time.py [--sizes 37x29,100x75] [--frames 1,8,64]"""
import argparse, math, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
from gaussianmesh_amd import scenes
from gaussianmesh_amd.arap import ArapSolver
from gaussianmesh_amd.pose_interp import PoseInterpolator

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


def rotation_y(angle):
    c, s = math.cos(angle), math.sin(angle)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def twisted(V):
    d = V - V.mean(0)
    phi = 0.5 + 0.3 * d[:, 1] / np.abs(d[:, 1]).max()
    return np.stack([np.cos(phi) * d[:, 0] + np.sin(phi) * d[:, 2], 1.3 * d[:, 1], -np.sin(phi) * d[:, 0] + np.cos(phi) * d[:, 2]], 1) + V.mean(0)


def ring_handles(V0, fraction=1.0):
    ang = np.arctan2(V0[:, 2].astype(np.float64), V0[:, 0].astype(np.float64))
    still, moved = np.nonzero(np.abs(ang) < 0.25)[0], np.nonzero(np.abs(np.abs(ang) - math.pi) < 0.25)[0]
    c, s = math.cos(0.6 * fraction), math.sin(0.6 * fraction)
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    target = V0[moved].astype(np.float64) @ Rz.T + np.array([0.0, 0.8 * fraction, 0.0])
    return np.concatenate([still, moved]), np.concatenate([V0[still].astype(np.float64), target], 0).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="37x29,100x75")
    ap.add_argument("--frames", type=str, default="1,8,64")
    args = ap.parse_args()
    counts = [int(v) for v in args.frames.split(",")]
    for nu, nv in (tuple(int(v) for v in item.split("x")) for item in args.sizes.split(",")):
        verts, faces = scenes.torus_mesh(nu, nv)
        V0 = verts.astype(np.float32)
        c = V0.astype(np.float64).mean(0)
        keys = {"rest": V0, "twist": twisted(V0.astype(np.float64)).astype(np.float32),
                "turn179": ((V0.astype(np.float64) - c) @ rotation_y(math.radians(179.0)).T + c + [0.4, 0.3, -0.2]).astype(np.float32)}
        keys = {k: torch.as_tensor(v, device=dev) for k, v in keys.items()}
        interp = PoseInterpolator(V0, faces, device=dev)
        handles = ring_handles(V0)[0]
        solver = ArapSolver(V0, faces, handles, device=dev)
        print("torus_mesh(%d, %d): %d vertices, %d faces" % (nu, nv, len(V0), len(faces)), flush=True)
        for a, b in (("rest", "twist"), ("twist", "turn179")):
            print(" %s -> %s" % (a, b), flush=True)
            for T in counts:
                ts = np.arange(1, T + 1) / (T + 1.0)
                out = torch.empty((T, len(V0), 3), dtype=torch.float32, device=dev)
                m = median_ms(lambda: interp.between(keys[a], keys[b], ts, out=out))
                st = interp.between(keys[a], keys[b], ts, want_stats=True)[1].cpu().numpy()
                st2 = interp.between(keys[a], keys[b], ts, cg_iterations=2000, want_stats=True)[1].cpu().numpy()
                print("  between, T = %-2d, defaults   median %8.3f ms (min %.3f, max %.3f)  %7.3f ms / frame   CG steps at most %d, |r|/|b| at most %.2e;"
                      " uncapped at 1e-6: at most %d steps" % ((T,) + m + (m[0] / T, int(st[:, :3].max()), st[:, 3:].max(), int(st2[:, :3].max()))), flush=True)
        print(" ArapSolver.solve_sequence at its defaults (4 outer iterations, <= 64 CG steps, batch=4), %d handles" % len(handles), flush=True)
        for T in counts:
            pos = torch.as_tensor(np.stack([ring_handles(V0, (t + 1) / float(T))[1] for t in range(T)], 0), device=dev)
            m = median_ms(lambda: solver.solve_sequence(pos))
            print("  solve_sequence, T = %-2d       median %8.3f ms (min %.3f, max %.3f)  %7.3f ms / frame" % ((T,) + m + (m[0] / T,)), flush=True)


if __name__ == "__main__":
    main()
