#!/usr/bin/env python
"""Device time of MeshDynamics.run against sampled grids that move (gm_mesh_dynamics_fields) as whole calls of 64 steps, beside the same
floor as the one static grid of gm_mesh_dynamics_field, in one process and alternating: HIP events, median of 20 after 5 warm-ups, on a
preallocated out=, every call from the same state (the rest pose at rest, the fields at the identity; the reset lies outside the timed
window).  The drag scenario and the meshes of tools/mesh_dynamics_field_time.py: torus_mesh(37, 29) (1073 vertices) and torus_mesh(100, 75)
(7.5 k vertices), one ring held, the opposite ring dragged, gravity (0, -9.8, 0), the floor a twentieth of the torus's height below it as
a 128^3 grid with friction 0.5, at the defaults and at stiffness 50.  Four routes per material:
  static field     field=grid                                   gm_mesh_dynamics_field
  F = 1, identity  fields=[grid], no poses given                the two 3x3 transforms per candidate, and nothing else
  F = 1, moving    fields=[grid], the floor sliding 0.2 per second sideways and turning 0.1 per second about y: the carried anchor too
  F = 4            the floor and three more floors of their own 128^3 grids 0.1, 0.2 and 0.3 lower, all four moving: 32 gathers per
                   free row and iteration
The poses are a float64 tensor on the device, made once.  Beside each time: the CG steps a (step, coordinate) used in its last iteration,
mean and most, and the rows in contact per step (one extra call outside the timed window).  Writes what it prints to --out.
    python tools/mesh_dynamics_moving_field_time.py [--sizes 37x29,100x75] [--resolution 128] [--out profiles/mesh_dynamics_moving_field_time.txt]"""
import argparse, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
from gaussianmesh_amd import scenes
from gaussianmesh_amd.dynamics import MeshDynamics
from mesh_dynamics_field_time import GRAVITY, STEPS, dev, plane_grid
from mesh_dynamics_time import alternating_ms, ring_handles


def sliding_poses(steps, fields, dt=1.0 / 30.0):
    """[steps,fields,3,4] float64 on the device: every field 0.2 per second along x and 0.1 per second about y, from the identity"""
    out = np.zeros((steps, fields, 3, 4))
    for k in range(steps):
        a = 0.1 * dt * (k + 1)
        out[k, :, :, :3] = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
        out[k, :, 0, 3] = 0.2 * dt * (k + 1)
    return torch.as_tensor(out, dtype=torch.float64, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="37x29,100x75")
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--out", type=str, default=os.path.join(os.path.dirname(__file__), "..", "profiles", "mesh_dynamics_moving_field_time.txt"))
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say("MeshDynamics.run(64) on a floor given as one static %d^3 grid (gm_mesh_dynamics_field) and as moving grids (gm_mesh_dynamics_fields: F = 1 at the "
        "identity, F = 1 moving, F = 4 moving), %s; HIP events, median of 20 after 5 warm-ups, alternating" % (args.resolution, torch.cuda.get_device_name(dev)))
    one, four = sliding_poses(STEPS, 1), sliding_poses(STEPS, 4)
    for nu, nv in (tuple(int(v) for v in item.split("x")) for item in args.sizes.split(",")):
        verts, faces = scenes.torus_mesh(nu, nv)
        V0 = verts.astype(np.float32)
        handles = ring_handles(V0)[0]
        pos = torch.as_tensor(np.stack([ring_handles(V0, (t + 1) / float(STEPS))[1] for t in range(STEPS)], 0), device=dev)
        low, high = float(V0[:, 1].min()), float(V0[:, 1].max())
        height = low - 0.05 * (high - low)
        grids = [plane_grid(V0, height - 0.1 * j, args.resolution) for j in range(4)]
        out = torch.empty((STEPS, len(V0), 3), dtype=torch.float32, device=dev)
        say("torus_mesh(%d, %d): %d vertices, %d faces, %d handles; floor at y = %.3f; grids %d^3, voxel %.4f, %.1f MB each"
            % (nu, nv, len(V0), len(faces), len(handles), height, args.resolution, grids[0].voxel, grids[0].grid.numel() * 4 / 1e6))
        for name, kw in (("defaults (stiffness 10)", dict()), ("stiffness 50", dict(stiffness=50.0))):
            static = MeshDynamics(V0, faces, handles=handles, gravity=GRAVITY, field=grids[0], field_friction=0.5, device=dev, **kw)
            f1 = MeshDynamics(V0, faces, handles=handles, gravity=GRAVITY, fields=grids[:1], field_frictions=[0.5], device=dev, **kw)
            f1m = MeshDynamics(V0, faces, handles=handles, gravity=GRAVITY, fields=grids[:1], field_frictions=[0.5], device=dev, **kw)
            f4 = MeshDynamics(V0, faces, handles=handles, gravity=GRAVITY, fields=grids, field_frictions=[0.5] * 4, device=dev, **kw)
            routes = (("static field", static, None), ("F = 1, identity", f1, None), ("F = 1, moving", f1m, one), ("F = 4, moving", f4, four))
            got = alternating_ms([((lambda m=m, p=p: m.run(STEPS, pos, out=out, **({} if p is None else dict(field_poses=p)))), m.reset) for _, m, p in routes])
            base = got[0][0]
            for (label, m, p), t in zip(routes, got):
                m.reset()
                _, c, st = m.run(STEPS, pos, want_contacts=True, want_stats=True, **({} if p is None else dict(field_poses=p)))
                st = st.cpu().numpy()
                say("  %-24s %-16s median %8.3f ms (min %.3f, max %.3f)  %7.4f ms / step  x %.3f of the static field   CG steps mean %.1f, at most %d; "
                    "rows in contact per step %.1f" % ((name + ":", label) + t + (t[0] / STEPS, t[0] / base, st[:, :3].mean(), int(st[:, :3].max()),
                                                       float((c > 0).sum(dim=1).float().mean())))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
