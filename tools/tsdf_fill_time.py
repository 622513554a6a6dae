#!/usr/bin/env python
"""Time of hole filling (proxy_mesh.TsdfVolume.fill_holes: gm_tsdf_fill of csrc/gm_tsdf_fill.hip), whole calls with their allocations,
wall clock around torch.cuda.synchronize(), median of 5 after 1 warm-up: a sphere field (radius 1.2 in a 3.2 box) as a capture from above
leaves it - free space carved, nothing known deeper than trunc behind the surface, nothing known below the sphere's lower third down to
the grid's bottom - at 96^3 and 128^3, for 64 and 256 iterations, boundary "free".  Per size and count:
    the samples and bricks the fill works on, total ms, us an iteration (the slope between the two counts: one tf_step launch);
    the numpy definition (tests/tsdf_fill_ref.py) on the host, for scale, and whether it gives the same bits;
    border edges of the extracted mesh before and after.
    python tools/tsdf_fill_time.py [--sizes 96 128] [--iterations 64 256] [--no_host] [--out profiles/tsdf_fill_time.txt]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
import numpy as np
import torch
from gaussianmesh_amd.proxy_mesh import TsdfVolume, boundary_edges

dev = torch.device("cuda:0")
BRICK = (32, 4, 2)


def seen_from_above(N, radius=1.2):
    vol = TsdfVolume([-1.6] * 3, [1.6] * 3, resolution=N, device=dev)
    ax = [torch.tensor(vol.origin[k], device=dev) + (torch.arange(n, device=dev, dtype=torch.float32) + 0.5) * vol.voxel
          for k, n in enumerate((vol.nx, vol.ny, vol.nz))]
    x, y, z = ax[0][None, None, :], ax[1][None, :, None], ax[2][:, None, None]
    d = torch.sqrt(x ** 2 + y ** 2 + z ** 2) - radius
    vol.tsdf.copy_((d / vol.trunc).clamp(-1.0, 1.0))
    shadow = (z < -radius / 3) & (x ** 2 + y ** 2 < radius ** 2)       # the column under the sphere: no view from above reaches it
    vol.weight.copy_(((d >= -vol.trunc) & ~shadow).to(torch.float32))
    return vol


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[96, 128])
    ap.add_argument("--iterations", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--no_host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for N in a.sizes:
        vol = seen_from_above(N)
        w = vol.weight.cpu().numpy()
        nz, ny, nx = w.shape
        pad = [(0, -s % b) for s, b in zip((nz, ny, nx), BRICK[::-1])]
        holes = np.pad(w < 1, pad).reshape((nz + pad[0][1]) // BRICK[2], BRICK[2], (ny + pad[1][1]) // BRICK[1], BRICK[1], (nx + pad[2][1]) // BRICK[0], BRICK[0])
        open_bricks = holes.any(axis=(1, 3, 5))
        V, F = vol.extract(keep="all")
        say("sphere seen from above at %d^3: %d of %d samples unobserved, %d of %d bricks hold one; %d border edges without a fill"
            % (N, int((w < 1).sum()), w.size, int(open_bricks.sum()), open_bricks.size, boundary_edges(F.cpu().numpy())))
        med = {}
        for n in a.iterations:
            walls = []
            for rep in range(6):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                vol.fill_holes(n, boundary="free")
                torch.cuda.synchronize(); walls.append(1e3 * (time.perf_counter() - t0))
            med[n] = float(np.median(walls[1:]))
            st = vol.fill_stats
            V, F = vol.extract(keep="all", fill_holes=n, fill_boundary="free")
            say(" %3d iterations: median %.3f ms (min %.3f, max %.3f), %.2f us an iteration; %d filled, %d not reached; %d border edges"
                % (n, med[n], min(walls[1:]), max(walls[1:]), 1e3 * med[n] / n, st["filled_voxels"], st["unreached_voxels"], boundary_edges(F.cpu().numpy())))
            if not a.no_host:
                import tsdf_fill_ref as fr
                D = vol.tsdf.cpu().numpy()
                t0 = time.perf_counter(); ref = fr.fill_ref(D, w, 1.0, n, True); t1 = time.perf_counter()
                same = (np.array_equal(ref[0].view(np.uint32), vol.filled_tsdf.cpu().numpy().view(np.uint32))
                        and np.array_equal(ref[1].view(np.uint32), vol.filled_weight.cpu().numpy().view(np.uint32)))
                say("     numpy definition on the host: %.1f s (same bits as the device: %s)" % (t1 - t0, same))
        ns = sorted(med)
        if len(ns) > 1:
            step = 1e3 * (med[ns[-1]] - med[ns[0]]) / (ns[-1] - ns[0])
            touched = int(open_bricks.sum()) * 256 * 10                # a value and a state byte read and written per sample of an open brick
            say(" slope: %.2f us a step launch; the open bricks' own values and states are %.2f MB a step: %.0f GB/s if that were all it moved"
                % (step, touched / 1e6, touched / step / 1e3))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
