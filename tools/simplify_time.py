#!/usr/bin/env python
"""Time of mesh simplification (mesh_simplify.simplify: csrc/gm_simplify.hip + torch bookkeeping), whole calls with their read-backs,
wall clock around torch.cuda.synchronize(), median of 5 after 1 warm-up: the surface-nets mesh of a sphere field (radius 1.2 in a 3.2
box, gm_surface_nets itself) at 128^3 and 256^3 simplified to 15 k faces.  Per size:
    rounds, total ms, ms a round;
    how many candidates of the first round cost exactly +0 (their keys tie: the edge id decides, and a round selects few of them);
    where a round goes: HIP-event medians of the bookkeeping (torch unique / sort / cumsum), of gm_mesh_collapse_round and of the
    apply step (torch indexing) on the dense mesh's first round, and gm_mesh_quadrics once;
    the one-sided distance from the dense mesh's vertices to the simplified mesh (mesh_bind.closest_faces), max and mean, in voxels;
    at the small size the numpy definition (tests/simplify_ref.py) on the host, for scale, and whether it gives the same mesh.
    python tools/simplify_time.py [--sizes 128 256] [--target_faces 15000] [--out profiles/mesh_simplify_time.txt]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
import numpy as np
import torch
from gaussianmesh_amd import mesh_simplify as ms
from gaussianmesh_amd.mesh_bind import closest_faces
from gaussianmesh_amd.proxy_mesh import TsdfVolume

dev = torch.device("cuda:0")


def event_ms(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def sphere_mesh(N, radius=1.2):
    vol = TsdfVolume([-1.6] * 3, [1.6] * 3, resolution=N, device=dev)
    ax = [torch.tensor(vol.origin[k], device=dev) + (torch.arange(n, device=dev, dtype=torch.float32) + 0.5) * vol.voxel
          for k, n in enumerate((vol.nx, vol.ny, vol.nz))]
    d = torch.sqrt(ax[0][None, None, :] ** 2 + ax[1][None, :, None] ** 2 + ax[2][:, None, None] ** 2) - radius
    vol.tsdf.copy_((d / vol.trunc).clamp(-1.0, 1.0))
    vol.weight.fill_(1.0)
    V, F = vol.extract(keep="all")
    return V, F, vol.voxel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--target_faces", type=int, default=15000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for k, N in enumerate(a.sizes):
        V, F, voxel = sphere_mesh(N)
        torch.cuda.synchronize()
        say("sphere field at %d^3: %d vertices, %d faces -> %d faces" % (N, V.shape[0], F.shape[0], a.target_faces))
        walls = []
        for rep in range(6):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            r = ms.simplify(V, F, target_faces=a.target_faces)
            torch.cuda.synchronize(); walls.append(1e3 * (time.perf_counter() - t0))
        med = float(np.median(walls[1:]))
        st = r.stats
        say(" simplify: %d rounds, median %.1f ms (min %.1f, max %.1f), %.2f ms a round; %d faces, %d vertices, stalled %s, locked %d, max cost %.3g"
            % (st["rounds"], med, min(walls[1:]), max(walls[1:]), med / max(st["rounds"], 1), st["faces"], r.vertices.shape[0], st["stalled"],
               st["locked_vertices"], st["max_cost"]))
        # where the first round goes
        F64 = F.to(torch.int64)
        F32 = F.to(torch.int32).contiguous()
        edges, uses, off, adj = ms._bookkeeping(F64, V.shape[0])
        Q = ms._quadrics(V, F32, off, adj)
        t_book = event_ms(lambda: ms._bookkeeping(F64, V.shape[0]))
        t_quad = event_ms(lambda: ms._quadrics(V, F32, off, adj))
        t_round = event_ms(lambda: ms.collapse_round(V, Q, F32, off, adj, edges, uses, 0.2, float("inf")))
        sel, frm, to, key, count = ms.collapse_round(V, Q, F32, off, adj, edges, uses, 0.2, float("inf"))
        def apply():
            s = sel.bool()
            i, j = frm[s].long(), to[s].long()
            Q2 = Q.clone(); Q2[j] = Q2[i] + Q2[j]
            remap = torch.arange(V.shape[0], dtype=torch.int64, device=dev); remap[i] = j
            live = remap[F64]
            return live[(live[:, 0] != live[:, 1]) & (live[:, 1] != live[:, 2]) & (live[:, 2] != live[:, 0])]
        t_apply = event_ms(apply)
        cand = frm >= 0
        say(" first round (%d edges, %d candidates of which %d cost exactly +0, %d selected = %.2f %% of the vertices): bookkeeping (torch) %.3f ms,"
            " gm_mesh_collapse_round %.3f ms, apply (torch) %.3f ms; gm_mesh_quadrics once %.3f ms"
            % (edges.shape[0], int(cand.sum()), int((cand & ((key >> 32) == 0)).sum()), int(count.item()), 100.0 * int(count.item()) / V.shape[0], t_book,
               t_round, t_apply, t_quad))
        d2, _ = closest_faces(V, r.vertices, r.faces)
        d = torch.sqrt(d2) / voxel
        say(" dense vertices -> simplified mesh: max %.3f voxels, mean %.4f voxels (voxel %.5f)" % (float(d.max()), float(d.mean()), voxel))
        if k == 0:
            import simplify_ref as sr
            vh, fh = V.cpu().numpy(), F.cpu().numpy()
            t0 = time.perf_counter(); ref = sr.simplify_ref(vh, fh, target_faces=a.target_faces); t1 = time.perf_counter()
            same = np.array_equal(ref["faces"], r.faces.cpu().numpy()) and np.array_equal(ref["kept"], r.kept.cpu().numpy())
            say(" numpy definition on the host: %.1f s, %d rounds (same mesh as the device: %s)" % (t1 - t0, ref["rounds"], same))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
