#!/usr/bin/env python
"""arap.ArapEnergy on the device: the time of value_and_grad (gm_arap_energy_grad: three launches) and of smooth_rows with 16 sweeps
(gm_mesh_smooth_rows: 17 launches), and with --sweep the pose fitter's lr x rigidity table under each regularizer.
Time: tori of 7.5 k and 60 k vertices under twist_bend_frame(t=4); whole calls with their allocations, wall clock around
torch.cuda.synchronize() over `--calls` calls in a row (the stream stays full: the device's time per call, not the host's latency),
median of 5 windows after a warm-up one.
Sweep: the scene of tests/test_gpu_pose_fit.py (torus_mesh(24, 16), 4 k bound Gaussians, 96 x 64, three views, target twist_bend_frame
(t=4)), 60 Adam steps from rest per cell; per cell the loss ratio (mean of the last three steps over the first three), the vertex-RMS
ratio to the target pose, and the step at which MeshPose.state() refused (det T <= 0), if it did - the figures of the steps before it then.
    python tools/arap_energy_time.py [--sizes 100x75 300x200] [--calls 200] [--sweep] [--steps 60] [--out profiles/arap_energy_time.txt]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
from gaussianmesh_amd import scenes
from gaussianmesh_amd.arap import ArapEnergy

dev = torch.device("cuda:0")
T = lambda a, dtype=torch.float32: torch.tensor(np.asarray(a), dtype=dtype, device=dev)


def windows(fn, calls):
    out = []
    for rep in range(6):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize(); out.append(1e6 * (time.perf_counter() - t0) / calls)
    return out[1:]


def timing(say, sizes, calls):
    for nu, nv in sizes:
        verts, faces = scenes.torus_mesh(nu, nv)
        energy = ArapEnergy(verts, faces, device=dev)
        V1 = T(scenes.twist_bend_frame(verts, t=4)[0])
        E, g = energy.value_and_grad(V1)
        nnz = len(energy.csr[1])
        say("torus %d x %d: %d vertices, %d directed edges; E / scale = %.4g, max|g| = %.4g" % (nu, nv, energy.Vm, nnz, float(E) / energy.scale, float(g.abs().max())))
        for name, fn in (("value_and_grad", lambda: energy.value_and_grad(V1)), ("energy only", lambda: energy.value_and_grad(V1, want_grad=False)),
                         ("smooth_rows, 16 sweeps", lambda: energy.smooth_rows(g, 1.0, 16)), ("smooth_rows, 0 sweeps", lambda: energy.smooth_rows(g, 1.0, 0))):
            w = windows(fn, calls)
            say("  %-24s median %8.1f us a call (min %.1f, max %.1f; %d calls a window)" % (name, float(np.median(w)), min(w), max(w), calls))


def sweep(say, steps):
    from gaussianmesh_amd import GaussianRasterizer
    from gaussianmesh_amd.deform import SingleObjectDeform
    from gaussianmesh_amd.pose_fit import PoseFitter
    from gaussianmesh_amd.renderer import Camera, _settings
    W, H = 96, 64
    verts, faces = scenes.torus_mesh(24, 16)
    cl = scenes.bind_cloud_to_mesh(4000, verts, faces, seed=5)
    cov = scenes.cov3d_from_scale_rot(cl["scales"], cl["rots"]).astype(np.float32)
    obj = SingleObjectDeform(T(cl["means"]), T(cov), T(cl["opac"]), T(cl["shs"]), T(cl["tri"], torch.int32), T(cl["weights"]), T(verts))
    cams = [Camera(scenes.orbit_camera(k, 3, W, H, radius=6.0), dev) for k in range(3)]
    V1, R, S = (T(a) for a in scenes.twist_bend_frame(verts, t=4))
    bg = torch.ones(3, device=dev)
    views = []
    with torch.no_grad():
        for cam in cams:
            pos, rgb, cov6 = obj.deform_and_shade(V1, R, S, cam.camera_center)
            image, _ = GaussianRasterizer(_settings(cam, bg, 1.0, 3, False))(pos, torch.zeros_like(pos), obj.gaussian_o, colors_precomp=rgb, cov3D_precomp=cov6)
            views.append((cam, image.clone()))
    obj.deform_state = None
    f = T(faces, torch.int32)
    rms = lambda a: float(((a - V1) ** 2).sum(1).mean().sqrt())
    start = rms(obj.vertex)
    say("pose fit sweep, %d steps a cell: loss ratio / vertex-RMS ratio / refusal" % steps)
    for label, opts in (("edge", dict(regularizer="edge")), ("arap", dict(regularizer="arap")), ("arap + 4 sweeps", dict(regularizer="arap", smooth_sweeps=4)),
                        ("arap + 16 sweeps", dict(regularizer="arap", smooth_sweeps=16))):
        for lr in (5e-4, 1e-3, 2e-3, 5e-3):
            cells = []
            for rigidity in (1.0, 10.0, 100.0):
                fitter = PoseFitter(obj, f, lr=lr, rigidity=rigidity, **opts)
                refused = None
                for it in range(steps):
                    try:
                        fitter.step(*views[it % 3])
                    except ValueError:
                        refused = it
                        break
                losses = torch.stack(fitter.losses).cpu().numpy() if fitter.losses else np.zeros(0)
                ratio = losses[-3:].mean() / losses[:3].mean() if len(losses) >= 6 else float("nan")
                cells.append("%.3f / %.3f / %s" % (ratio, rms(fitter.pose.V1.detach()) / start, "not refused" if refused is None else "refused at step %d" % refused))
            say("  %-16s lr %.0e: rigidity 1: %s;  10: %s;  100: %s" % (label, lr, *cells))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["100x75", "300x200"])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--no_time", action="store_true")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    if not a.no_time:
        timing(say, [tuple(int(v) for v in s.split("x")) for s in a.sizes], a.calls)
    if a.sweep:
        sweep(say, a.steps)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
