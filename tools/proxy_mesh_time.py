#!/usr/bin/env python
"""Device time of the proxy-mesh stage (csrc/gm_tsdf.hip), HIP events, median of 20 after 5 warm-ups, on a 128^3 volume with 64 views
of 512 x 512: analytic depth maps of a sphere of radius 1.2 seen from an orbit (alpha 1 on the sphere, 0 beside it).
    fusion: gm_tsdf_integrate with all 64 views in one call, with 8 views a call (from_cloud's default) and with one view a call; beside
            each the bytes of volume read and written per second (the floor of a call is one read and one write of tsdf and weight);
    extraction: gm_surface_nets at a capacity that holds the result (TsdfVolume.extract adds one 8-byte read-back and, for
            keep="largest", the host's component pass, timed on its own);
    the numpy definition (tests/tsdf_ref.py) on the host, for scale: fusion of 2 of the views, extraction of the fused volume.
    python tools/proxy_mesh_time.py [--resolution 128] [--views 64] [--size 512]"""
import argparse, math, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
import numpy as np
import torch
from gaussianmesh_amd import scenes
from gaussianmesh_amd.mesh_pick import camera_rays
from gaussianmesh_amd.proxy_mesh import TsdfVolume, largest_component
from gaussianmesh_amd.renderer import Camera

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


def sphere_maps(cams, radius):
    """(depth, alpha) [K,H,W] of the sphere |p| = radius: the first root of |o + t d| = radius along mesh_pick.camera_rays (t = view depth)"""
    depth, alpha = [], []
    for cam in cams:
        H, W = cam.image_height, cam.image_width
        pix = torch.stack(torch.meshgrid(torch.arange(W, device=dev, dtype=torch.float32), torch.arange(H, device=dev, dtype=torch.float32), indexing="xy"), -1)
        o, d = camera_rays(cam, pix.reshape(-1, 2))
        a, b, c = (d * d).sum(1), (o * d).sum(1), (o * o).sum(1) - radius * radius
        disc = b * b - a * c
        hit = disc > 0
        t = (-b - torch.sqrt(disc.clamp_min(0))) / a
        depth.append(torch.where(hit, t, torch.zeros_like(t)).reshape(H, W))
        alpha.append(hit.float().reshape(H, W))
    return torch.stack(depth), torch.stack(alpha)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    a = ap.parse_args()
    K, S, N = a.views, a.size, a.resolution
    dicts = [scenes.orbit_camera(k, K, S, S, radius=5.0, height=(2.5, -2.5, 0.5)[k % 3]) for k in range(K)]
    cams = [Camera(c, dev) for c in dicts]
    depth, alpha = sphere_maps(cams, 1.2)
    vol = TsdfVolume([-1.6] * 3, [1.6] * 3, resolution=N, device=dev)
    n = vol.nx * vol.ny * vol.nz
    print("volume %d x %d x %d (%.1f MB tsdf + weight), %d views of %d x %d (%.1f MB depth + alpha)" % (
        vol.nx, vol.ny, vol.nz, 8e-6 * n, K, S, S, 8e-6 * K * S * S))

    def fuse(step):
        vol.tsdf.zero_(); vol.weight.zero_()
        for s in range(0, K, step):
            vol.integrate(cams[s:s + step], depth[s:s + step], alpha[s:s + step])
    zero_ms = median_ms(lambda: (vol.tsdf.zero_(), vol.weight.zero_()))[0]
    for step in (K, 8, 1):
        med, lo, hi = median_ms(lambda: fuse(step))
        calls = (K + step - 1) // step
        print(" fusion, %2d views a call (%2d calls): median %.3f ms (min %.3f, max %.3f), %.3f ms without the two fills; %.1f us a view; "
              "volume traffic %.0f GB/s" % (step, calls, med, lo, hi, med - zero_ms, 1e3 * (med - zero_ms) / K, 16e-9 * n * calls / (1e-3 * (med - zero_ms))))
    fuse(8)
    V, F = vol.extract(keep="all")
    nv, nf = V.shape[0], F.shape[0]
    med, lo, hi = median_ms(lambda: vol._surface_nets_enqueue(1.0, nv, nf))
    print(" extraction, %d vertices %d faces: median %.3f ms (min %.3f, max %.3f)" % (nv, nf, med, lo, hi))
    t0 = time.perf_counter(); vol.extract(keep="all"); torch.cuda.synchronize(); t1 = time.perf_counter()
    vh, fh = V.cpu().numpy(), F.cpu().numpy()
    t2 = time.perf_counter(); comps = largest_component(vh, fh)[2]; t3 = time.perf_counter()
    print(" TsdfVolume.extract(keep='all') wall %.3f ms; largest_component on the host %.1f ms (%d components)" % (1e3 * (t1 - t0), 1e3 * (t3 - t2), comps))
    import tsdf_ref as tr
    views, tans = tr.camera_rows(dicts[:2])
    zero = np.zeros((vol.nz, vol.ny, vol.nx), np.float32)
    dh, ah = depth[:2].cpu().numpy(), alpha[:2].cpu().numpy()
    t0 = time.perf_counter(); tr.integrate_ref(zero, zero, dh, ah, views, tans, vol.origin, vol.voxel, vol.trunc); t1 = time.perf_counter()
    D, W = vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy()
    t2 = time.perf_counter(); rV, rF = tr.surface_nets_ref(D, W, vol.origin, vol.voxel, 1.0); t3 = time.perf_counter()
    same = np.array_equal(rV.view(np.uint32), vh.view(np.uint32)) and np.array_equal(rF, fh)
    print(" numpy definition on the host: fusion %.0f ms a view, extraction %.0f ms (same mesh as the device: %s)" % (5e2 * (t1 - t0), 1e3 * (t3 - t2), same))


if __name__ == "__main__":
    main()
