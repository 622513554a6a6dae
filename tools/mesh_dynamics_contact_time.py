#!/usr/bin/env python
"""Device time of MeshDynamics.run with colliders (gm_mesh_dynamics_contact) as whole calls of 64 steps, beside the same run without
colliders (gm_mesh_dynamics), in one process and alternating: HIP events, median of 20 after 5 warm-ups, on a preallocated out=, every
call from the same state (the rest pose at rest; the reset lies outside the timed window).  The drag of tools/mesh_dynamics_time.py on
its meshes, torus_mesh(37, 29) (1073 vertices) and torus_mesh(100, 75) (7.5 k vertices): one ring held, the opposite ring at k / 64 of
its rotation and lift in step k, gravity (0, -9.8, 0), at the defaults (stiffness 10, damping 0.02, dt 1 / 30, 3 iterations, <= 64 CG
steps to 1e-6) and at stiffness 50.  Three routes per material:
  no colliders     gm_mesh_dynamics
  out of reach     a floor and a ball far away: gm_mesh_dynamics_contact's kernels on the states of the first route (the meshes are its
                   meshes bit for bit, which is checked), so the difference is what K = 2 distance evaluations per row, three more
                   columns and the effective diagonal cost
  floor + ball     a floor a twentieth of the torus's height below it (friction 0.5), onto which the free part sags, and a ball 1.2 tube
                   radii wide that rises through the tube a quarter turn from the handles over the 64 steps (friction 0);
                   contact_stiffness at its default
Beside each time: the CG steps a (step, coordinate) used in its last iteration, mean and most, and for the last route the rows in contact
per step (one extra call outside the timed window).  Writes what it prints to --out.
    python tools/mesh_dynamics_contact_time.py [--sizes 37x29,100x75] [--out profiles/mesh_dynamics_contact_time.txt]"""
import argparse, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
from gaussianmesh_amd import scenes
from gaussianmesh_amd.dynamics import MeshDynamics, floor, sphere
from mesh_dynamics_time import alternating_ms, ring_handles

dev = torch.device("cuda:0")
STEPS = 64
GRAVITY = (0.0, -9.8, 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="37x29,100x75")
    ap.add_argument("--out", type=str, default=os.path.join(os.path.dirname(__file__), "..", "profiles", "mesh_dynamics_contact_time.txt"))
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say("MeshDynamics.run(64) with a floor and a moving ball (gm_mesh_dynamics_contact) and without colliders (gm_mesh_dynamics), %s; HIP events, "
        "median of 20 after 5 warm-ups, alternating" % torch.cuda.get_device_name(dev))
    for nu, nv in (tuple(int(v) for v in item.split("x")) for item in args.sizes.split(",")):
        verts, faces = scenes.torus_mesh(nu, nv)
        V0 = verts.astype(np.float32)
        handles = ring_handles(V0)[0]
        pos = torch.as_tensor(np.stack([ring_handles(V0, (t + 1) / float(STEPS))[1] for t in range(STEPS)], 0), device=dev)
        ang = np.arctan2(V0[:, 2].astype(np.float64), V0[:, 0].astype(np.float64))
        ring = V0[np.abs(ang - 0.5 * np.pi) < 0.25].astype(np.float64)                # a quarter turn from both handle rings
        centre = ring.mean(0)
        tube = float(np.linalg.norm(ring - centre, axis=1).max())
        low, high = float(V0[:, 1].min()), float(V0[:, 1].max())
        near = [floor(low - 0.05 * (high - low), friction=0.5), sphere(centre - [0.0, 4.0 * tube, 0.0], 1.2 * tube)]
        far = [floor(low - 1000.0, friction=0.5), sphere(centre - [0.0, 2000.0, 0.0], 1.2 * tube)]
        out = torch.empty((STEPS, len(V0), 3), dtype=torch.float32, device=dev)
        say("torus_mesh(%d, %d): %d vertices, %d faces, %d handles; floor at y = %.3f, ball of radius %.3f" % (nu, nv, len(V0), len(faces), len(handles), near[0][1][3], 1.2 * tube))
        for name, kw in (("defaults (stiffness 10)", dict()), ("stiffness 50", dict(stiffness=50.0))):
            free, idle, hit = (MeshDynamics(V0, faces, handles=handles, gravity=GRAVITY, colliders=c, device=dev, **kw) for c in ((), far, near))
            rows = np.tile(hit.collider_rows, (STEPS, 1, 1))
            rows[:, 1, 1] += (5.0 * tube * np.arange(1, STEPS + 1) / STEPS).astype(np.float32)
            rows = torch.as_tensor(rows, device=dev)
            got = alternating_ms([((lambda: free.run(STEPS, pos, out=out)), free.reset), ((lambda: idle.run(STEPS, pos, out=out)), idle.reset),
                                  ((lambda: hit.run(STEPS, pos, collider_rows=rows, out=out)), hit.reset)])
            for d in (free, idle, hit):
                d.reset()
            Xf, sf = free.run(STEPS, pos, want_stats=True)
            Xi, si = idle.run(STEPS, pos, want_stats=True)
            _, contact, sh = hit.run(STEPS, pos, collider_rows=rows, want_contacts=True, want_stats=True)
            same = bool(torch.equal(Xf, Xi))
            per_step = (contact > 0).sum(dim=1).cpu().numpy()
            for label, m, st in (("no colliders", got[0], sf), ("out of reach", got[1], si), ("floor + ball", got[2], sh)):
                st = st.cpu().numpy()
                say("  %-24s %-13s median %8.3f ms (min %.3f, max %.3f)  %7.4f ms / step   CG steps mean %.1f, at most %d; |r|/|b| at most %.2e"
                    % ((name + ":", label) + m + (m[0] / STEPS, st[:, :3].mean(), int(st[:, :3].max()), st[:, 3:].max())))
            say("  %-24s out of reach / no colliders %.3f (same meshes: %s); floor + ball / no colliders %.3f; rows in contact per step: mean %.1f, "
                "at most %d (floor %d, ball %d rows x steps)"
                % ("", got[1][0] / got[0][0], same, got[2][0] / got[0][0], per_step.mean(), int(per_step.max()), int((contact == 1).sum()), int((contact == 2).sum())))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
