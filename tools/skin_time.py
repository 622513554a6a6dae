#!/usr/bin/env python
"""Device time of the skinning stage as whole calls, HIP events, median of 20 after 5 warm-ups, on torus_mesh(37, 29) (1073 vertices)
and the C3 torus torus_mesh(100, 75) (7.5 k vertices):
  weights   SkinBinding(mesh graph, skeleton) at its defaults for J = 4, 16 and 64 bones: a chain of J + 1 joints round the torus's
            centre circle.  The graph is built before the window (host work, shared); the call uploads the areas and the bones, allocates
            the workspace and runs the four launches.  Beside it the CG steps the slowest bone used and the largest final |r| / |b|.
  pose      SkinBinding.pose on a preallocated out= at T = 1, 8 and 64 frames, both blends, from transforms already on the host (the call
            checks and uploads them); beside it a torch float64 einsum statement of the linear blend on the device.
THE EXPECTATION TO CONFIRM OR REFUTE, as counts: pose moves about Vm T (12 + 32) bytes plus the transforms (0.3 MB at 7.5 k vertices and
T = 1, 21 MB at T = 64: microseconds at HBM rates), so at these sizes it should cost a launch's latency plus the host's check and
upload of the transforms; the weights should cost about one pi_solve-sized PCG - (steps used) x (a step's time, about 31 us at 7.5 k
vertices in PoseInterpolator) - whatever J up to the chip's 256 compute units, since the bones' workgroups run side by side.
    python tools/skin_time.py [--sizes 37x29,100x75] [--bones 4,16,64] [--frames 1,8,64]"""
import argparse, math, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
from gaussianmesh_amd import scenes
from gaussianmesh_amd.mesh_graph import MeshGraph
from gaussianmesh_amd.skinning import Skeleton, SkinBinding

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


def chain(J, radius=2.0):
    ang = 0.1 + np.arange(J + 1) * (2 * math.pi / (J + 1))
    return Skeleton(np.stack([radius * np.cos(ang), np.zeros(J + 1), radius * np.sin(ang)], 1), [-1] + list(range(J)))


def einsum_linear(rest64, ids, w64, M64):
    """the linear blend as torch float64 statements on the device: [T,Vm,3] float32"""
    Mk = M64[:, ids]                                                   # [T,Vm,4,3,4]
    moved = torch.einsum("tvkab,vb->tvka", Mk[..., :3], rest64) + Mk[..., 3]
    return (torch.einsum("vk,tvka->tva", w64, moved) / w64.sum(1)[None, :, None]).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="37x29,100x75")
    ap.add_argument("--bones", type=str, default="4,16,64")
    ap.add_argument("--frames", type=str, default="1,8,64")
    args = ap.parse_args()
    bones, counts = [int(v) for v in args.bones.split(",")], [int(v) for v in args.frames.split(",")]
    for nu, nv in (tuple(int(v) for v in item.split("x")) for item in args.sizes.split(",")):
        verts, faces = scenes.torus_mesh(nu, nv)
        graph = MeshGraph(verts.astype(np.float32), faces, device=dev)
        graph.device_csr
        print("torus_mesh(%d, %d): %d vertices, %d faces" % (nu, nv, graph.Vm, graph.F), flush=True)
        for J in bones:
            skel = chain(J)
            m = median_ms(lambda: SkinBinding(graph, None, skel))
            b = SkinBinding(graph, None, skel)
            st = b.stats.cpu().numpy()
            print(" weights, J = %-3d defaults   median %8.3f ms (min %.3f, max %.3f)   CG steps at most %d, |r|/|b| at most %.2e"
                  % ((J,) + m + (int(st[:, 0].max()), st[:, 1].max())), flush=True)
            if J != bones[len(bones) // 2]:
                continue
            rng = np.random.default_rng(J)
            for T in counts:
                M = skel.bone_transforms(rng.uniform(-0.5, 0.5, (T, J + 1, 3)), rng.uniform(-0.2, 0.2, (T, 3)))
                out = torch.empty((T, graph.Vm, 3), dtype=torch.float32, device=dev)
                for blend in ("dqs", "linear"):
                    m = median_ms(lambda: b.pose(M, blend=blend, out=out))
                    print("  pose %-6s T = %-2d        median %8.3f ms (min %.3f, max %.3f)  %7.3f ms / frame" % ((blend, T) + m + (m[0] / T,)), flush=True)
                rest64, ids, w64, M64 = b.rest.double(), b.bone_ids.long(), b.bone_w.double(), torch.as_tensor(M, device=dev).double()
                m = median_ms(lambda: einsum_linear(rest64, ids, w64, M64))
                err = float((einsum_linear(rest64, ids, w64, M64) - b.pose(M, blend="linear")).abs().max())
                print("  torch float64 einsum, T = %-2d median %8.3f ms (min %.3f, max %.3f)  %7.3f ms / frame   max |difference| %.2e"
                      % ((T,) + m + (m[0] / T, err)), flush=True)


if __name__ == "__main__":
    main()
