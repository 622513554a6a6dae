#!/usr/bin/env python
"""Frames/s of an edit sequence on the C3 scene (1 M Gaussians bound to the torus mesh, analytic twist, 1920 x 1080, orbit cameras):
  1. ObjectVisualTool.render_sequence (K frames per launch chain), without and with the depth / alpha maps;
  2. the per-frame loop of the reference's animation (deform_vertices + render_gaussian: gm_mesh_rs, gm_deform, gm_sh_colors, the
     autograd rasterizer, one host wait on the instance count per frame);
  3. SingleObjectDeform.deform_and_render per frame (gm_mesh_rs + the fused single-frame pair).
With --scene, the scene leg instead: a synthetic plain background of P rows (default 1 M, a shell around the object) plus the torus object
(100 k Gaussians), SceneVisualTool:
  1. SceneVisualTool.render_sequence (K frames per launch chain, rasterizer.forward_scene_batch);
  2. the per-frame loop (deform_vertices + render_gaussian: the rows concatenated, gm_cov_to_scale_rot over all of them, the autograd
     rasterizer, one host wait on the instance count per frame).
Each route renders the same FRAMES frames (mesh t, camera t), is run once to warm up, then REPEATS times between device events with a
synchronisation before and after; the median is printed, with the spread, as one JSON line.  Every route ends with the images on the
device (no file IO).
usage: tools/edit_sequence_time.py [--scene] [P] [FRAMES] [REPEATS] [K]"""
import json
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch

SCENE = "--scene" in sys.argv[1:]
ARGS = [a for a in sys.argv[1:] if a != "--scene"]
P = int(ARGS[0]) if len(ARGS) > 0 else 1_000_000
FRAMES = int(ARGS[1]) if len(ARGS) > 1 else 64
REPEATS = int(ARGS[2]) if len(ARGS) > 2 else 5
K = int(ARGS[3]) if len(ARGS) > 3 else 4
P_OBJECT_IN_SCENE = 100_000
W, H = 1920, 1080


def build(P=P):
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


def build_scene_tool(o):
    """SceneVisualTool around object o: a plain background of P rows on a shell of radius 4.5 .. 7.5 about the object (inside the orbit)"""
    from gaussianmesh_amd import edittool, scenes
    bgc = scenes.make_cloud(P, seed=7, scale_lo=0.02, scale_hi=0.1)
    nb = np.linalg.norm(bgc["means"], axis=1, keepdims=True) + 1e-6
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda")
    tool = edittool.SceneVisualTool.__new__(edittool.SceneVisualTool)
    edittool.ObjectVisualTool.__init__(tool)
    tool.bg_mean3D = T(bgc["means"] / nb * (4.5 + nb))
    tool.bg_cov3D = edittool._covariance(T(np.log(bgc["scales"])), T(bgc["rots"]))
    tool.bg_shs = T(bgc["shs"])
    tool.bg_opacity = T(bgc["opac"])
    tool._scene_seq = None
    tool.gaussians_list.append(o)
    return tool


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
    if SCENE:
        return main_scene()
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


def main_scene():
    _, o, cams, V1 = build(P_OBJECT_IN_SCENE)
    tool = build_scene_tool(o)
    frames = [(cams[t], {"Object": V1[t]}) for t in range(FRAMES)]
    out = dict(scene=True, P_background=P, P_object=P_OBJECT_IN_SCENE, W=W, H=H, frames=FRAMES, repeats=REPEATS, K=K)

    def sequence():
        for _ in tool.render_sequence(frames, frames_per_launch=K):
            pass

    def per_frame():
        for t in range(FRAMES):
            o.deform_vertices(V1[t])
            tool.render_gaussian(cams[t])

    with torch.no_grad():
        out["scene_render_sequence"] = timed(sequence)
        out["scene_per_frame_deform_vertices_render_gaussian"] = timed(per_frame)
    out["speedup"] = round(out["scene_render_sequence"]["fps"] / out["scene_per_frame_deform_vertices_render_gaussian"]["fps"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
