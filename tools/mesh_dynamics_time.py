#!/usr/bin/env python
"""Device time of MeshDynamics.run as whole calls of 64 steps (one launch chain), HIP events, median of 20 after 5 warm-ups, on a
preallocated out=, every call from the same state (the rest pose at rest; the reset lies outside the timed window), on torus_mesh(37, 29)
(1073 vertices) and the C3 torus torus_mesh(100, 75) (7.5 k vertices): one ring held, the opposite ring at k / 64 of its rotation and
lift in step k (the handles of tools/arap_time.py), at the defaults (stiffness 10, damping 0.02, dt 1 / 30, 3 iterations, <= 64 CG steps
to 1e-6) without and with gravity, and at stiffness 50 with gravity.  Beside each: the CG steps a (step, coordinate) used in its last
iteration, mean and most, and the largest final residual (one extra call with want_stats, outside the timed window).
Then, measured in the same run and alternating with the above, what the package offered for the same drag before:
ArapSolver.solve_sequence at its defaults (4 outer iterations, <= 64 CG steps, batch=4) over the same 64 frames - a quasi-static solve
per frame.  Writes what it prints to --out.
    python tools/mesh_dynamics_time.py [--sizes 37x29,100x75] [--out profiles/mesh_dynamics_time.txt]"""
import argparse, math, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
from gaussianmesh_amd import scenes
from gaussianmesh_amd.arap import ArapSolver
from gaussianmesh_amd.dynamics import MeshDynamics

dev = torch.device("cuda:0")
STEPS = 64


def time_once(fn, prep=None):
    if prep is not None:
        prep()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternating_ms(routes, reps=20, warm=5):
    """routes: [(fn, prep)]; every route once per round, in turn, so that what else the machine does falls on all alike.  Per route
    (median, min, max) ms."""
    for _ in range(warm):
        for fn, prep in routes:
            time_once(fn, prep)
    out = [[] for _ in routes]
    for _ in range(reps):
        for k, (fn, prep) in enumerate(routes):
            out[k].append(time_once(fn, prep))
    return [(float(np.median(o)), float(min(o)), float(max(o))) for o in out]


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
    ap.add_argument("--out", type=str, default=os.path.join(os.path.dirname(__file__), "..", "profiles", "mesh_dynamics_time.txt"))
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say("MeshDynamics.run(64) and ArapSolver.solve_sequence over the same 64 frames, %s; HIP events, median of 20 after 5 warm-ups, alternating"
        % torch.cuda.get_device_name(dev))
    for nu, nv in (tuple(int(v) for v in item.split("x")) for item in args.sizes.split(",")):
        verts, faces = scenes.torus_mesh(nu, nv)
        V0 = verts.astype(np.float32)
        handles = ring_handles(V0)[0]
        pos = torch.as_tensor(np.stack([ring_handles(V0, (t + 1) / float(STEPS))[1] for t in range(STEPS)], 0), device=dev)
        solver = ArapSolver(V0, faces, handles, device=dev)
        out = torch.empty((STEPS, len(V0), 3), dtype=torch.float32, device=dev)
        materials = (("defaults (stiffness 10), no gravity", dict()), ("defaults, gravity (0, -9.8, 0)", dict(gravity=(0.0, -9.8, 0.0))),
                     ("stiffness 50, gravity (0, -9.8, 0)", dict(stiffness=50.0, gravity=(0.0, -9.8, 0.0))))
        dyns = [MeshDynamics(V0, faces, handles=handles, device=dev, **kw) for _, kw in materials]
        routes = [((lambda d=d: d.run(STEPS, pos, out=out)), d.reset) for d in dyns] + [((lambda: solver.solve_sequence(pos)), None)]
        got = alternating_ms(routes)
        say("torus_mesh(%d, %d): %d vertices, %d faces, %d handles" % (nu, nv, len(V0), len(faces), len(handles)))
        for (name, _), d, m in zip(materials, dyns, got):
            d.reset()
            st = d.run(STEPS, pos, want_stats=True)[1].cpu().numpy()
            say("  run(64), %-36s median %8.3f ms (min %.3f, max %.3f)  %7.4f ms / step   CG steps mean %.1f, at most %d; |r|/|b| at most %.2e"
                % ((name + ":",) + m + (m[0] / STEPS, st[:, :3].mean(), int(st[:, :3].max()), st[:, 3:].max())))
        m = got[-1]
        say("  solve_sequence at its defaults (4 outer iterations, <= 64 CG steps, batch=4):"
            "   median %8.3f ms (min %.3f, max %.3f)  %7.4f ms / frame" % (m + (m[0] / STEPS,)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
