#!/usr/bin/env python
"""Device time of MeshDynamics.run against a sampled signed-distance grid (gm_mesh_dynamics_field) as whole calls of 64 steps, beside the
same floor as an analytic half-space (gm_mesh_dynamics_contact) and beside no collider at all (gm_mesh_dynamics), in one process and
alternating: HIP events, median of 20 after 5 warm-ups, on a preallocated out=, every call from the same state (the rest pose at rest;
the reset lies outside the timed window).  The drag of tools/mesh_dynamics_contact_time.py on its meshes, torus_mesh(37, 29) (1073
vertices) and torus_mesh(100, 75) (7.5 k vertices): one ring held, the opposite ring at k / 64 of its rotation and lift in step k, gravity
(0, -9.8, 0), at the defaults (stiffness 10, damping 0.02, dt 1 / 30, 3 iterations, <= 64 CG steps to 1e-6) and at stiffness 50.  Three
routes per material:
  analytic floor   a floor a twentieth of the torus's height below it, friction 0.5 (K = 1)
  sampled floor    the same plane as a 128^3 SdfGrid over the torus's box grown by half its longest side (K = 0 and the field): what eight
                   16-byte gathers per free row and iteration cost beside one plane evaluation
  no collider      gm_mesh_dynamics
Beside each time: the CG steps a (step, coordinate) used in its last iteration, mean and most; the rows in contact per step of the two
floors and the largest distance between their meshes (one extra call outside the timed window).  Writes what it prints to --out.
    python tools/mesh_dynamics_field_time.py [--sizes 37x29,100x75] [--resolution 128] [--out profiles/mesh_dynamics_field_time.txt]"""
import argparse, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
from gaussianmesh_amd import scenes
from gaussianmesh_amd.dynamics import MeshDynamics, SdfGrid, floor
from mesh_dynamics_time import alternating_ms, ring_handles

dev = torch.device("cuda:0")
STEPS = 64
GRAVITY = (0.0, -9.8, 0.0)


def plane_grid(V0, height, resolution):
    """the floor y = height as an SdfGrid of resolution^3 samples over V0's box grown by half its longest side"""
    lo, hi = V0.min(0).astype(np.float64), V0.max(0).astype(np.float64)
    side = float((hi - lo).max())
    centre = 0.5 * (lo + hi)
    voxel = np.float32(2.0 * side / resolution)
    origin = (centre - 0.5 * resolution * float(voxel)).astype(np.float32)
    y = origin.astype(np.float64)[1] + (np.arange(resolution) + 0.5) * float(voxel) - height
    values = np.broadcast_to(y[None, :, None], (resolution,) * 3).astype(np.float32)
    return SdfGrid(values, origin, float(voxel), device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="37x29,100x75")
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--out", type=str, default=os.path.join(os.path.dirname(__file__), "..", "profiles", "mesh_dynamics_field_time.txt"))
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say("MeshDynamics.run(64) on a floor given as a half-space (gm_mesh_dynamics_contact), as a %d^3 sampled grid (gm_mesh_dynamics_field) and without "
        "it (gm_mesh_dynamics), %s; HIP events, median of 20 after 5 warm-ups, alternating" % (args.resolution, torch.cuda.get_device_name(dev)))
    for nu, nv in (tuple(int(v) for v in item.split("x")) for item in args.sizes.split(",")):
        verts, faces = scenes.torus_mesh(nu, nv)
        V0 = verts.astype(np.float32)
        handles = ring_handles(V0)[0]
        pos = torch.as_tensor(np.stack([ring_handles(V0, (t + 1) / float(STEPS))[1] for t in range(STEPS)], 0), device=dev)
        low, high = float(V0[:, 1].min()), float(V0[:, 1].max())
        height = low - 0.05 * (high - low)
        grid = plane_grid(V0, height, args.resolution)
        out = torch.empty((STEPS, len(V0), 3), dtype=torch.float32, device=dev)
        say("torus_mesh(%d, %d): %d vertices, %d faces, %d handles; floor at y = %.3f; grid %d^3, voxel %.4f, %.1f MB"
            % (nu, nv, len(V0), len(faces), len(handles), height, args.resolution, grid.voxel, grid.grid.numel() * 4 / 1e6))
        for name, kw in (("defaults (stiffness 10)", dict()), ("stiffness 50", dict(stiffness=50.0))):
            flat = MeshDynamics(V0, faces, handles=handles, gravity=GRAVITY, colliders=[floor(height, friction=0.5)], device=dev, **kw)
            field = MeshDynamics(V0, faces, handles=handles, gravity=GRAVITY, field=grid, field_friction=0.5, device=dev, **kw)
            free = MeshDynamics(V0, faces, handles=handles, gravity=GRAVITY, device=dev, **kw)
            got = alternating_ms([((lambda: flat.run(STEPS, pos, out=out)), flat.reset), ((lambda: field.run(STEPS, pos, out=out)), field.reset),
                                  ((lambda: free.run(STEPS, pos, out=out)), free.reset)])
            for d in (flat, field, free):
                d.reset()
            Xa, ca, sa = flat.run(STEPS, pos, want_contacts=True, want_stats=True)
            Xs, cs, ss = field.run(STEPS, pos, want_contacts=True, want_stats=True)
            _, sf = free.run(STEPS, pos, want_stats=True)
            for label, m, st in (("analytic floor", got[0], sa), ("sampled floor", got[1], ss), ("no collider", got[2], sf)):
                st = st.cpu().numpy()
                say("  %-24s %-15s median %8.3f ms (min %.3f, max %.3f)  %7.4f ms / step   CG steps mean %.1f, at most %d; |r|/|b| at most %.2e"
                    % ((name + ":", label) + m + (m[0] / STEPS, st[:, :3].mean(), int(st[:, :3].max()), st[:, 3:].max())))
            say("  %-24s sampled / analytic %.3f; sampled / no collider %.3f; analytic / no collider %.3f; rows in contact per step: analytic mean %.1f, "
                "sampled mean %.1f; largest distance between the two floors' meshes %.2e"
                % ("", got[1][0] / got[0][0], got[1][0] / got[2][0], got[0][0] / got[2][0], float((ca > 0).sum(dim=1).float().mean()),
                   float((cs > 0).sum(dim=1).float().mean()), float((Xa.double() - Xs.double()).abs().max())))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
