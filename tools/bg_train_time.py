#!/usr/bin/env python
"""Time of one BgTrainer iteration (train_bg_gaussian.py's loop) at 1 M background + 0.3 M object Gaussians, 1920 x 1080: bg_render's
fused route for PlainGaussians against the generic torch route (model.fused = False: torch activations and five concatenations per
call), plus gm_knn_nearest (the neighbour pruning) at that size.  Densification and pruning are off in the timed iterations.
usage: tools/bg_train_time.py [N_bg] [N_obj] [iterations]"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch

NB = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
NO = int(sys.argv[2]) if len(sys.argv) > 2 else 300_000
IT = int(sys.argv[3]) if len(sys.argv) > 3 else 20
W, H = 1920, 1080


def mesh_model(n):
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.renderer import MeshBoundGaussians
    T = lambda a: torch.as_tensor(np.asarray(a, np.float32), device="cuda")
    verts, faces = scenes.torus_mesh(100, 75)
    rng = np.random.default_rng(3)
    cl = scenes.bind_cloud_to_mesh(n, verts, faces, seed=2)
    tri = faces[cl["fid"]]
    v1, v2, v3 = (verts[tri[:, k]].astype(np.float32) for k in range(3))
    nr = np.cross(v2 - v1, v3 - v1); nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    r = ((np.linalg.norm(v2 - v1, axis=1) + np.linalg.norm(v3 - v2, axis=1) + np.linalg.norm(v1 - v3, axis=1)) / 3)[:, None]
    return MeshBoundGaussians(T(rng.normal(size=(n, 3))), T(rng.normal(0, 0.3, size=(n, 1))), T(cl["shs"][:, :1]), T(cl["shs"][:, 1:]),
                              T(np.log(cl["scales"])), T(cl["rots"]), T(rng.normal(size=(n, 1))), T(v1), T(v2), T(v3), T(nr), T(r))


def plain(n, seed, fused):
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.bg_model import PlainGaussians
    b = scenes.make_cloud(n, seed=seed, scale_lo=0.005, scale_hi=0.05, extent=6.0)
    nb = np.linalg.norm(b["means"], axis=1, keepdims=True) + 1e-6
    b["means"] = (b["means"] / nb * (3.0 + nb)).astype(np.float32)
    g = PlainGaussians(3, device="cuda")
    T = lambda a: torch.as_tensor(np.asarray(a, np.float32))
    g._set_params(T(b["means"]), T(b["shs"]), torch.log(T(b["scales"])), T(b["rots"]), torch.logit(T(b["opac"])).reshape(-1, 1))
    g.active_sh_degree, g.fused = 3, fused
    return g


def main():
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.bg_train import BgTrainer
    from gaussianmesh_amd.renderer import Camera, bg_render
    from gaussianmesh_amd.simple_knn import knn_nearest
    from types import SimpleNamespace
    mesh = mesh_model(NO)
    cams = [Camera(scenes.orbit_camera(k, 8, W, H, radius=9.0), "cuda") for k in range(4)]
    bg = torch.zeros(3, device="cuda")
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    with torch.no_grad():
        gts = [bg_render(c, plain(NB, 21, True), pipe, bg, mesh_gaussians=mesh)["render"].detach().clone() for c in cams]
    res = {}
    for route, fused in (("fused", True), ("generic", False), ("fused_again", True)):
        tr = BgTrainer(plain(NB, 9, fused), mesh, remove_neighbor_iterations=(), densify_from_iter=10 ** 9)
        for i in range(3):
            tr.step(cams[i % 4], gts[i % 4], bg)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter(); e0.record()
        for i in range(IT):
            tr.step(cams[i % 4], gts[i % 4], bg)
        e1.record(); torch.cuda.synchronize()
        res[route] = (e0.elapsed_time(e1) / IT, (time.perf_counter() - t0) * 1e3 / IT)
        del tr
        torch.cuda.empty_cache()
    for k, (ms, wall) in res.items():
        print("BgTrainer iteration, %-11s route: %.3f ms (GPU events), %.3f ms wall   [%d bg + %d object, %dx%d]" % (k, ms, wall, NB, NO, W, H))
    q = plain(NB, 9, True)._xyz.detach()
    r = mesh.get_xyz.detach()
    for _ in range(3):
        knn_nearest(q, r)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        d2, _ = knn_nearest(q, r)
    e1.record(); torch.cuda.synchronize()
    print("gm_knn_nearest %d x %d: %.3f ms; %d rows within 0.01 (squared)" % (NB, NO, e0.elapsed_time(e1) / 10, int((d2 < 0.01).sum())))


if __name__ == "__main__":
    main()
