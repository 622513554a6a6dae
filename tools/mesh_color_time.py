#!/usr/bin/env python
"""Time of colouring a proxy mesh (mesh_color.VertexColors: gm_mesh_vertex_normals, gm_mesh_color_integrate, gm_mesh_color_spread of
csrc/gm_mesh_color.hip), whole calls with their allocations, wall clock around torch.cuda.synchronize(), median of 5 after 1 warm-up:
the dense surface-nets mesh of a sphere (radius 1.2 in a 3.2 box) at 128^3, 64 views of 512 x 512 on an orbit ABOVE it - the underside
stays unseen, which is the spread's work - with analytic depth maps and a position-coloured image.  Reported:
    the normals; the 64 views in one call and 8 views a call; resolve without and with the spread (64 and 256 steps, and the slope
    between them: one step launch); the numpy definition (tests/mesh_color_ref.py) on the host, for scale, and whether it gives the
    same bits.
    python tools/mesh_color_time.py [--size 128] [--views 64] [--image 512] [--no_host] [--out profiles/mesh_color_time.txt]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
import numpy as np
import torch
from gaussianmesh_amd import mesh_color as mc, scenes
from gaussianmesh_amd.mesh_pick import camera_rays
from gaussianmesh_amd.proxy_mesh import TsdfVolume
from gaussianmesh_amd.renderer import Camera

dev = torch.device("cuda:0")
RADIUS = 1.2


def sphere_mesh(N):
    vol = TsdfVolume([-1.6] * 3, [1.6] * 3, resolution=N, device=dev)
    ax = [torch.tensor(vol.origin[k], device=dev) + (torch.arange(n, device=dev, dtype=torch.float32) + 0.5) * vol.voxel
          for k, n in enumerate((vol.nx, vol.ny, vol.nz))]
    d = torch.sqrt(ax[0][None, None, :] ** 2 + ax[1][None, :, None] ** 2 + ax[2][:, None, None] ** 2) - RADIUS
    vol.tsdf.copy_((d / vol.trunc).clamp(-1.0, 1.0))
    vol.weight.fill_(1.0)
    V, F = vol.extract(keep="all")
    return V, F, vol.trunc


def sphere_views(K, S):
    """K cameras above the sphere; per view the analytic first hit of every pixel's ray: (cameras, image [K,3,S,S], depth, alpha [K,S,S])"""
    cams = [Camera(scenes.orbit_camera(k, K, S, S, radius=4.0, height=2.5, fovx_deg=50.0), dev) for k in range(K)]
    y, x = torch.meshgrid(torch.arange(S, device=dev, dtype=torch.float32), torch.arange(S, device=dev, dtype=torch.float32), indexing="ij")
    pix = torch.stack([x.reshape(-1), y.reshape(-1)], dim=1)
    image, depth, alpha = [], [], []
    for cam in cams:
        o, d = camera_rays(cam, pix)                                   # directions with view z = 1: t is the view depth
        a, b, c = (d * d).sum(1), 2 * (o * d).sum(1), (o * o).sum(1) - RADIUS ** 2
        disc = b * b - 4 * a * c
        hit = disc > 0
        t = torch.where(hit, (-b - torch.sqrt(disc.clamp(min=0))) / (2 * a), torch.zeros_like(a))
        p = o + d * t[:, None]
        image.append(torch.where(hit[:, None], 0.5 + p / (2 * RADIUS), torch.zeros_like(p)).T.reshape(3, S, S))
        depth.append(t.reshape(S, S))
        alpha.append(hit.to(torch.float32).reshape(S, S))
    return cams, torch.stack(image).contiguous(), torch.stack(depth).contiguous(), torch.stack(alpha).contiguous()


def median_ms(fn, reps=6):
    walls = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(); walls.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(walls[1:])), min(walls[1:]), max(walls[1:]), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--image", type=int, default=512)
    ap.add_argument("--no_host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    V, F, trunc = sphere_mesh(a.size)
    K, S = a.views, a.image
    cams, image, depth, alpha = sphere_views(K, S)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    vc = mc.VertexColors(V, F)
    torch.cuda.synchronize()
    say("sphere at %d^3: %d vertices, %d faces; %d views of %d x %d from above; VertexColors() %.1f ms (the adjacency is built on the host)"
        % (a.size, V.shape[0], F.shape[0], K, S, S, 1e3 * (time.perf_counter() - t0)))
    m = median_ms(lambda: mc._normals(vc.vertices, vc.faces, vc.adjacency))
    say(" gm_mesh_vertex_normals: median %.3f ms (min %.3f, max %.3f)" % m[:3])
    def integrate(step):
        vc.csum.zero_(); vc.wsum.zero_()
        for s in range(0, K, step):
            vc.integrate(cams[s:s + step], image[s:s + step], depth[s:s + step], alpha[s:s + step], depth_tol=trunc)
    for step in (K, 8):
        m = median_ms(lambda: integrate(step))
        say(" integrate, %d views a call: median %.3f ms (min %.3f, max %.3f), %.1f us a view" % ((step,) + m[:3] + (1e3 * m[0] / K,)))
    m = median_ms(lambda: vc.resolve())
    st = vc.stats
    say(" resolve(): median %.3f ms; %d of %d vertices seen" % (m[0], st["seen"], V.shape[0]))
    med = {}
    for n in (64, 256):
        m = median_ms(lambda: vc.resolve(spread=n))
        med[n], st = m[0], vc.stats
        say(" resolve(spread=%d): median %.3f ms (min %.3f, max %.3f); %d filled, %d not reached" % ((n,) + m[:3] + (st["filled"], st["unreached"])))
    say(" slope: %.2f us a spread step launch" % (1e3 * (med[256] - med[64]) / 192))
    if not a.no_host:
        import mesh_color_ref as mr
        import tsdf_ref as tr
        bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)
        Vh, Fh = V.cpu().numpy(), F.cpu().numpy()
        t0 = time.perf_counter(); Nh = mr.vertex_normals_ref(Vh, Fh); t1 = time.perf_counter()
        say(" numpy definition on the host: normals %.2f s (same bits as the device: %s)" % (t1 - t0, np.array_equal(bits(Nh), bits(vc.normals.cpu().numpy()))))
        views = np.stack([c.world_view_transform.cpu().numpy() for c in cams])
        tans = np.array([[np.tan(c.FoVx * 0.5), np.tan(c.FoVy * 0.5)] for c in cams], np.float32)
        integrate(K)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = mr.integrate_ref(np.zeros_like(Vh), np.zeros(len(Vh), np.float32), image.cpu().numpy(), depth.cpu().numpy(), alpha.cpu().numpy(), views, tans,
                               Vh, Nh, 0.5, trunc)
        t1 = time.perf_counter()
        same = np.array_equal(bits(ref[0]), bits(vc.csum.cpu().numpy())) and np.array_equal(bits(ref[1]), bits(vc.wsum.cpu().numpy()))
        say("     %d views: %.2f s, %.1f ms a view (same bits: %s)" % (K, t1 - t0, 1e3 * (t1 - t0) / K, same))
        col, seen = mr.resolve_ref(ref[0], ref[1])
        got = vc.resolve(spread=64).cpu().numpy()
        t0 = time.perf_counter(); sp = mr.spread_ref(Fh, seen, col, 64); t1 = time.perf_counter()
        say("     spread, 64 steps: %.2f s (same bits: %s)" % (t1 - t0, np.array_equal(bits(sp[0]), bits(got))))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
