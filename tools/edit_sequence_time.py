#!/usr/bin/env python
"""Frames/s of an edit sequence on the C3 scene (1 M Gaussians bound to the torus mesh, analytic twist, 1920 x 1080, orbit cameras):
  1. ObjectVisualTool.render_sequence (K frames per launch chain), without and with the depth / alpha maps;
  2. the per-frame loop of the reference's animation (deform_vertices + render_gaussian: gm_mesh_rs, gm_deform, gm_sh_colors, the
     autograd rasterizer, one host wait on the instance count per frame);
  3. SingleObjectDeform.deform_and_render per frame (gm_mesh_rs + the fused single-frame pair).
Each route renders the same FRAMES frames (mesh t, camera t), is run once to warm up, then REPEATS times between device events with a
synchronisation before and after; the median is printed, with the spread, as one JSON line.  Every route ends with the images on the
device (no file IO).
usage: tools/edit_sequence_time.py [P] [FRAMES] [REPEATS] [K]"""
import json
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch

P = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
FRAMES = int(sys.argv[2]) if len(sys.argv) > 2 else 64
REPEATS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
K = int(sys.argv[4]) if len(sys.argv) > 4 else 4
W, H = 1920, 1080


def build():
    import bench
    from gaussianmesh_amd import deform, edittool, scenes
    from gaussianmesh_amd.renderer import Camera
    host = bench.build_scene(P, W, H, FRAMES)
    T = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")
    o = edittool.SingleObjectDeform.__new__(edittool.SingleObjectDeform)          # the file loader's object, from arrays
    deform.SingleObjectDeform.__init__(o, T(host["pos"]), T(host["cov"]), T(host["opac"]).reshape(-1, 1), T(host["shs"]),
                                       T(host["tri"], torch.int32), T(host["weights"]), T(host["verts"]), name="Object")
    o.device = torch.device("cuda")
    o.faces = T(host["faces"], torch.int32)
    off, adj = deform.vertex_face_adjacency(host["faces"], host["verts"].shape[0])
    o._adjacency = (T(off, torch.int32), T(adj, torch.int32))
    tool = edittool.ObjectVisualTool()
    tool.gaussians_list.append(o)
    cams = []
    for k in range(FRAMES):
        cams.append(Camera(scenes.orbit_camera(k, FRAMES, W, H), "cuda"))
    V1 = [T(host["mesh"][t][:, 0:3]) for t in range(FRAMES)]
    return tool, o, cams, V1


def timed(run):
    run()                                                   # warm-up: workspaces, capacities, allocator
    ms = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    med = ms[len(ms) // 2]
    return dict(fps=round(1000.0 * FRAMES / med, 1), ms_median=round(med, 2), ms_min=round(ms[0], 2), ms_max=round(ms[-1], 2))


def main():
    from gaussianmesh_amd import configure_runtime
    configure_runtime()
    from gaussianmesh_amd.deform import mesh_rs
    tool, o, cams, V1 = build()
    frames = [(cams[t], {"Object": V1[t]}) for t in range(FRAMES)]
    out = dict(P=P, W=W, H=H, frames=FRAMES, repeats=REPEATS, K=K)

    def sequence(aux):
        def run():
            for _ in tool.render_sequence(frames, frames_per_launch=K, aux=aux):
                pass
        return run

    def per_frame():
        for t in range(FRAMES):
            o.deform_vertices(V1[t])
            tool.render_gaussian(cams[t])

    def fused_single():
        for t in range(FRAMES):
            R, S = mesh_rs(o.vertex, V1[t], o.faces, adjacency=o._adjacency)
            o.deform_and_render(V1[t], R, S, cams[t])

    with torch.no_grad():
        out["render_sequence"] = timed(sequence(False))
        out["render_sequence_aux"] = timed(sequence(True))
        out["per_frame_deform_vertices_render_gaussian"] = timed(per_frame)
        out["per_frame_deform_and_render"] = timed(fused_single)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
