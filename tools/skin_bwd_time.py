#!/usr/bin/env python
"""Device time of the skinning backward and of the pose fit that stands on it, HIP events, median of 20 after 5 warm-ups, on
torus_mesh(37, 29) (1073 vertices) and the C3 torus torus_mesh(100, 75) (7.5 k vertices):
  backward  gm_skin_pose_bwd as skinning._pose_bwd calls it (allocates the output and the workspace, two launches) for J = 4, 16 and 64
            bones (the chain of tools/skin_time.py), T = 1, 8 and 64 frames, both blends; beside it the linear blend's gradient by torch
            float64 autograd on the device (the einsum statement of tools/skin_time.py, backward included) and their largest difference.
  step      one whole SkeletonPoseFitter.step on the fit test's scene (24 x 16 torus, 4000 Gaussians, 96 x 64, five bones), and the
            skinning forward + backward alone (SkeletonPose.vertices() and its backward) as a share of it.
  lr        the fit test's 60 steps from rest at lr = 0.0005 .. 0.1: last / first loss per view and the vertex RMS ratio, or the refusal.
            Beside it, PoseFitter's V1 parameterisation on the same kind of scene is refused at every lr >= 1e-3 of the edge length after
            0.04 of travel (pose_fit.PoseFitter's docstring).
THE EXPECTATIONS TO CONFIRM OR REFUTE, written before the first run: the backward costs a few launch latencies at these sizes (its
traffic is T Vm 96 B of workspace written and read once, 46 MB at 7.5 k vertices and T = 64: tens of microseconds at HBM rates); the
step is bound by the rasterizer and MeshPose.state, not by skinning.
    python tools/skin_bwd_time.py [--sizes 37x29,100x75] [--bones 4,16,64] [--frames 1,8,64] [--out profiles/skin_bwd_time.txt]"""
import argparse, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(__file__))
import numpy as np
import torch
from gaussianmesh_amd import scenes
from gaussianmesh_amd.mesh_graph import MeshGraph
from gaussianmesh_amd.skinning import BLENDS, SkinBinding, _pose_bwd
from skin_time import chain, dev, einsum_linear, median_ms

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def backward_times(args):
    bones, counts = [int(v) for v in args.bones.split(",")], [int(v) for v in args.frames.split(",")]
    for nu, nv in (tuple(int(v) for v in item.split("x")) for item in args.sizes.split(",")):
        verts, faces = scenes.torus_mesh(nu, nv)
        graph = MeshGraph(verts.astype(np.float32), faces, device=dev)
        say("torus_mesh(%d, %d): %d vertices" % (nu, nv, graph.Vm))
        for J in bones:
            skel = chain(J)
            b = SkinBinding(graph, None, skel)
            inc = b.incidence
            rng = np.random.default_rng(J)
            for T in counts:
                M = torch.as_tensor(skel.bone_transforms(rng.uniform(-0.5, 0.5, (T, J + 1, 3)), rng.uniform(-0.2, 0.2, (T, 3))), device=dev)
                g = torch.as_tensor(rng.standard_normal((T, graph.Vm, 3)).astype(np.float32), device=dev)
                for blend in ("dqs", "linear"):
                    m = median_ms(lambda: _pose_bwd(b.rest, b.bone_ids, b.bone_w, M, BLENDS.index(blend), g, inc))
                    say("  J = %-3d T = %-2d backward %-6s median %8.3f ms (min %.3f, max %.3f)" % ((J, T, blend) + m))
                rest64, ids, w64 = b.rest.double(), b.bone_ids.long(), b.bone_w.double()

                def by_autograd():
                    M64 = M.double().requires_grad_(True)
                    return torch.autograd.grad((einsum_linear(rest64, ids, w64, M64) * g).sum(), M64)[0]
                m = median_ms(by_autograd)
                diff = float((by_autograd() - _pose_bwd(b.rest, b.bone_ids, b.bone_w, M, 0, g, inc)).abs().max())
                say("  J = %-3d T = %-2d torch float64 autograd (linear, through a float32 output) median %8.3f ms (min %.3f, max %.3f)   max |difference| %.2e"
                    % ((J, T) + m + (diff,)))


def fit_scene():
    """the scene of tests/test_gpu_skin_bwd.py::test_fit_a_skeleton_pose_from_three_views -> (make an object, skeleton, views, target mesh)"""
    import math
    from gaussianmesh_amd import GaussianRasterizer
    from gaussianmesh_amd.deform import SingleObjectDeform
    from gaussianmesh_amd.renderer import Camera, _settings
    from gaussianmesh_amd.skinning import Skeleton
    W, H = 96, 64
    verts, faces = scenes.torus_mesh(24, 16)
    cl = scenes.bind_cloud_to_mesh(4000, verts, faces, seed=5)
    cov = scenes.cov3d_from_scale_rot(cl["scales"], cl["rots"]).astype(np.float32)
    t = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    radius = float(np.hypot(verts[:, 0], verts[:, 2]).mean())
    ang = 0.2 + np.arange(6) * (2 * math.pi / 6)
    skel = Skeleton(np.stack([radius * np.cos(ang), np.full(6, 0.02), radius * np.sin(ang)], 1), [-1, 0, 1, 2, 3, 4])
    rng = np.random.default_rng(11)
    rot, tr = rng.uniform(-0.4, 0.4, (3, 6, 3))[0], rng.uniform(-0.2, 0.2, (3, 3))[0]

    def make():
        o = SingleObjectDeform(t(cl["means"]), t(cov), t(cl["opac"]), t(cl["shs"]), t(cl["tri"], torch.int32), t(cl["weights"]), t(verts))
        o.attach_skeleton(skel, faces=t(faces, torch.int32))
        return o
    obj = make()
    cams = [Camera(scenes.orbit_camera(k, 3, W, H, radius=6.0), dev) for k in range(3)]
    bg = torch.ones(3, device=dev)
    views = []
    with torch.no_grad():
        obj.pose(rot, tr)
        V1, R, S = obj.deform_state
        for cam in cams:
            pos, rgb, cov6 = obj.deform_and_shade(V1, R, S, cam.camera_center)
            image, _ = GaussianRasterizer(_settings(cam, bg, 1.0, 3, False))(pos, torch.zeros_like(pos), obj.gaussian_o, colors_precomp=rgb, cov3D_precomp=cov6)
            views.append((cam, image.clone()))
    return make, views, V1.clone()


def step_share():
    from gaussianmesh_amd.pose_fit import SkeletonPoseFitter
    make, views, _ = fit_scene()
    fitter = SkeletonPoseFitter(make())
    cam, target = views[0]
    whole = median_ms(lambda: fitter.step(cam, target))
    probe = torch.ones((fitter.obj.vertex.shape[0], 3), device=dev)

    def skinning_alone():
        fitter.optimizer.zero_grad(set_to_none=True)
        (fitter.pose.vertices() * probe).sum().backward()
    skin = median_ms(skinning_alone)
    M = fitter.obj.skin.skeleton.bone_transforms_torch(fitter.pose.rotations[None], fitter.pose.root_translation[None]).detach()

    def kernels_alone():
        Md = M.clone().requires_grad_(True)
        (fitter.obj.skin.pose_differentiable(Md, "dqs")[0] * probe).sum().backward()
    kernels = median_ms(kernels_alone)

    def state_alone():
        V1 = fitter.pose.vertices().detach().requires_grad_(True)
        dV, R, S = fitter.mesh.state(V1)
        (dV.sum() + R.sum() + S.sum()).backward()
    state = median_ms(state_alone)
    say("SkeletonPoseFitter.step (24 x 16 torus, 4000 Gaussians, 96 x 64, 5 bones): median %.3f ms (min %.3f, max %.3f)" % whole)
    say("  forward kinematics + skinning forward + backward alone: median %.3f ms (min %.3f, max %.3f): %.1f %% of the step" % (skin + (100 * skin[0] / whole[0],)))
    say("  of that, gm_skin_pose + gm_skin_pose_bwd from given transforms (the rest is the forward kinematics' torch statements): median %.3f ms (min %.3f, max %.3f): %.1f %% of the step"
        % (kernels + (100 * kernels[0] / whole[0],)))
    say("  MeshPose.state forward + backward alone (with the skinning forward): median %.3f ms (min %.3f, max %.3f): %.1f %% of the step"
        % (state + (100 * state[0] / whole[0],)))


def lr_sweep(rates, steps=60):
    from gaussianmesh_amd.pose_fit import SkeletonPoseFitter
    make, views, target = fit_scene()
    rms = lambda a: float(((a - target) ** 2).sum(1).mean().sqrt())
    say("the fit test's scene, %d steps from rest (PoseFitter on this torus: refused at every lr >= 1e-3 of the edge length after 0.04 of travel)" % steps)
    for lr in rates:
        obj = make()
        fitter = SkeletonPoseFitter(obj, lr=lr)
        try:
            fitter.fit(views, steps)
        except ValueError as e:
            say("  lr = %-6g refused after %d steps: %s" % (lr, len(fitter.losses), e))
            continue
        losses = torch.stack(fitter.losses).cpu().numpy()
        say("  lr = %-6g loss last / first per view %s; vertex RMS %.4f -> %.4f (ratio %.3f)%s" % (
            lr, ", ".join("%.3f" % (losses[steps - 3 + k] / losses[k]) for k in range(3)), rms(obj.vertex), rms(obj.mesh_vertex_current),
            rms(obj.mesh_vertex_current) / rms(obj.vertex), "" if np.isfinite(losses).all() else "  NOT FINITE"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="37x29,100x75")
    ap.add_argument("--bones", type=str, default="4,16,64")
    ap.add_argument("--frames", type=str, default="1,8,64")
    ap.add_argument("--rates", type=str, default="0.0005,0.001,0.002,0.003,0.005,0.01,0.02,0.05,0.1")
    ap.add_argument("--out", type=str, default=os.path.join(os.path.dirname(__file__), "..", "profiles", "skin_bwd_time.txt"))
    args = ap.parse_args()
    backward_times(args)
    step_share()
    lr_sweep([float(v) for v in args.rates.split(",")])
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
