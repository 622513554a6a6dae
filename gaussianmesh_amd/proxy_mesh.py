"""From a trained cloud to its proxy mesh: fuse the rasterizer's depth / opacity maps of the training views into a truncated signed
distance volume (gm_tsdf_integrate) and pull an indexed triangle mesh out of it (gm_surface_nets; both csrc/gm_tsdf.hip).  The mesh
is what train_mesh --input_mesh, SingleObjectDeform, bind_points, ArapSolver, pick and bake start from; the reference sends its users to
a NeuS trainer, MeshLab and MeshFix for it.  Definition, ABI and rules: INTEGRATION.md section T.

    V, F = from_cloud(model, cameras, resolution=96)          # device tensors; io.write_obj(path, V.cpu(), F.cpu())
    python -m gaussianmesh_amd.proxy_mesh --gaussian cloud.ply --cameras cameras.json --out proxy.obj [--vertex_colors]
"""
import argparse
import ctypes as C
import json
import math
import sys
import time
import warnings
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from ._op import enqueue, need_cuda, on_device, workspace
from .arap import components
from .mesh_pick import camera_tuple


def maps_list(x, who, what):
    """a list of [H,W] maps from a list of [H,W] / [1,H,W] tensors or one stacked [K,H,W] / [K,1,H,W] tensor"""
    if torch.is_tensor(x):
        if x.dim() == 4 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() == 2:
            x = x[None]
        if x.dim() != 3:
            raise ValueError("%s: %s must be [K,H,W] or [K,1,H,W]; got %s" % (who, what, tuple(x.shape)))
        return list(x.unbind(0))
    out = []
    for m in x:
        if not torch.is_tensor(m):
            raise _lib.GmeshError("%s needs %s as tensors on a HIP (cuda) device; there is no CPU path" % (who, what))
        m = m[0] if m.dim() == 3 and m.shape[0] == 1 else m
        if m.dim() != 2:
            raise ValueError("%s: every %s map must be [H,W] or [1,H,W]; got %s" % (who, what, tuple(m.shape)))
        out.append(m)
    return out


def largest_component(vertices, faces):
    """(vertices, faces, components): the connected component with the most faces (ties: the one that holds the smallest vertex id),
    its unreferenced vertices dropped and the ids re-numbered in order; components = how many the input had.  Host arrays (numpy)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 0
    rows = np.concatenate([f[:, 0], f[:, 1], f[:, 2], f[:, 1], f[:, 2], f[:, 0]])
    cols = np.concatenate([f[:, 1], f[:, 2], f[:, 0], f[:, 0], f[:, 1], f[:, 2]])
    label = components(len(v), rows, cols)[f[:, 0]]                   # the smallest vertex id of the face's component
    names, counts = np.unique(label, return_counts=True)
    f = f[label == names[np.argmax(counts)]]                          # argmax: the first of the largest, names ascend
    used = np.unique(f)
    remap = np.full(len(v), -1, np.int64)
    remap[used] = np.arange(len(used))
    return v[used], remap[f].astype(np.int32), len(names)


def boundary_edges(faces):
    """edges held by exactly one face (0: the mesh has no border).  Host."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) == 0:
        return 0
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0), axis=1)
    return int((np.unique(e, axis=0, return_counts=True)[1] == 1).sum())


class TsdfVolume:
    """A dense truncated signed distance volume over the box [bounds_min, bounds_max]: tsdf / weight float32 [nz,ny,nx] on the device,
    sample (ix, iy, iz) at origin + (i + 0.5) voxel.  voxel_size, or the longest side / resolution; the other sides take as many voxels
    as cover them (at least 2).  trunc: the truncation distance, 3 voxels unless given."""

    def __init__(self, bounds_min, bounds_max, resolution=96, voxel_size=None, trunc=None, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.GmeshError("TsdfVolume needs a HIP (cuda) device; there is no CPU path")
        lo, hi = np.asarray(bounds_min, np.float64).reshape(3), np.asarray(bounds_max, np.float64).reshape(3)
        if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
            raise ValueError("TsdfVolume: bounds_max must exceed bounds_min on every axis; got %s, %s" % (lo.tolist(), hi.tolist()))
        voxel = float(voxel_size) if voxel_size is not None else float((hi - lo).max()) / int(resolution)
        if not voxel > 0.0 or not math.isfinite(voxel):
            raise ValueError("TsdfVolume: the voxel size must be positive; got %r" % voxel)
        n = np.maximum(np.ceil((hi - lo) / voxel - 1e-6).astype(np.int64), 2)
        if int(n.prod()) > 1 << 28:
            raise ValueError("TsdfVolume: %d x %d x %d samples are more than one dense grid holds (2^28)" % tuple(n))
        self.nx, self.ny, self.nz = (int(x) for x in n)
        self.origin = np.asarray(lo, np.float32)
        self.voxel = float(np.float32(voxel))
        self.trunc = float(np.float32(3.0 * voxel if trunc is None else trunc))
        if not self.trunc > 0.0:
            raise ValueError("TsdfVolume: trunc must be positive; got %r" % trunc)
        self.tsdf = torch.zeros((self.nz, self.ny, self.nx), dtype=torch.float32, device=self.device)
        self.weight = torch.zeros_like(self.tsdf)
        self._origin_c = (C.c_float * 3)(*self.origin.tolist())
        self.views = 0
        self.simplified = None
        self.filled_tsdf = self.filled_weight = None
        self._fill = None

    def integrate(self, cameras, depth, alpha, alpha_min=0.5, carve=True):
        """Fuse views: cameras (renderer.Camera-like objects or scenes.camera_from_RT dicts), depth and alpha the rasterizer's own maps
        (return_aux: depth not normalised) as lists of [H,W] / [1,H,W] tensors or stacked [K,H,W] / [K,1,H,W] tensors.  Views of one
        resolution go into one call each (in the order given: the volume's bits depend on the order of the views, not on the grouping).
        alpha < alpha_min: free space with carve, ignored without.  Only enqueues; nothing waits for the device."""
        cameras = list(cameras)
        depth, alpha = maps_list(depth, "TsdfVolume.integrate", "depth"), maps_list(alpha, "TsdfVolume.integrate", "alpha")
        if not (len(cameras) == len(depth) == len(alpha)):
            raise ValueError("TsdfVolume.integrate: %d cameras, %d depth maps, %d alpha maps" % (len(cameras), len(depth), len(alpha)))
        for d, a in zip(depth, alpha):
            need_cuda(d, "TsdfVolume.integrate", "the depth maps")
            need_cuda(a, "TsdfVolume.integrate", "the alpha maps")
            if d.shape != a.shape:
                raise ValueError("TsdfVolume.integrate: a depth map is %s and its alpha map %s" % (tuple(d.shape), tuple(a.shape)))
        self.filled_tsdf = self.filled_weight = self._fill = None      # a fill is of the volume as it was
        k = 0
        while k < len(cameras):                                        # runs of one resolution, in view order
            e = k + 1
            while e < len(cameras) and depth[e].shape == depth[k].shape:
                e += 1
            H, W = (int(s) for s in depth[k].shape)
            rows, tans = [], []
            for cam in cameras[k:e]:
                view, _, _, cw, ch, tanx, tany = camera_tuple(cam)
                if (cw, ch) != (W, H):
                    raise ValueError("TsdfVolume.integrate: a %d x %d camera with %d x %d maps" % (cw, ch, W, H))
                rows.append(view.detach().to(self.device, torch.float32).reshape(16))
                tans.append((tanx, tany))
            views = torch.stack(rows).contiguous()
            tanfov = torch.tensor(tans, dtype=torch.float32).to(self.device, non_blocking=True)
            dd = torch.stack([m.detach().to(self.device, torch.float32) for m in depth[k:e]]).contiguous()
            aa = torch.stack([m.detach().to(self.device, torch.float32) for m in alpha[k:e]]).contiguous()
            enqueue(self.device, "gm_tsdf_integrate", e - k, H, W, dd, aa, views, tanfov, self.nx, self.ny, self.nz, self._origin_c, self.voxel,
                    self.trunc, float(alpha_min), int(bool(carve)), self.tsdf, self.weight)
            self.views += e - k
            k = e
        return self

    def fill_holes(self, iterations=None, min_weight=1, boundary="none", fill_weight=None):
        """Close the holes no view saw by volumetric diffusion (gm_tsdf_fill; Davis et al. 2002): the samples with weight >= min_weight
        stay as they are and their distances diffuse, one Jacobi step per iteration, into the others, so that an underside nobody
        photographed gets a zero crossing where extract() otherwise ends in a border.  The result goes into self.filled_tsdf /
        self.filled_weight (new device tensors; a filled sample weighs fill_weight, by default min_weight, so the extraction that
        follows takes it; a sample the fill did not reach weighs 0); self.tsdf / self.weight are untouched and can take more views,
        which drops the fill.  iterations: default max(nx, ny, nz).  That is a REACH, not a convergence claim: after n iterations every
        sample within n six-connected steps of a known one has a value, and values further from the sources are less settled.
        boundary="none": the grid's sides contribute nothing - a hole that reaches a side stays open there; "free": the samples beyond
        the grid count as free space (+1), which closes such a hole inside the grid.  Only enqueues; self.fill_stats (iterations,
        filled_voxels, unreached_voxels) reads the counts when it is asked for.  Returns self."""
        if boundary not in ("none", "free"):
            raise ValueError("TsdfVolume.fill_holes: boundary must be 'none' or 'free'; got %r" % (boundary,))
        need_cuda(getattr(self, "tsdf", None), "TsdfVolume.fill_holes", "the volume")
        n = max(self.nx, self.ny, self.nz) if iterations is None else int(iterations)
        if n < 0:
            raise ValueError("TsdfVolume.fill_holes: iterations must not be negative; got %r" % (iterations,))
        self.filled_tsdf, self.filled_weight = torch.empty_like(self.tsdf), torch.empty_like(self.weight)
        counts = torch.empty((2,), dtype=torch.int32, device=self.device)
        ws = workspace(self.device, "gm_tsdf_fill_workspace_bytes", self.nx, self.ny, self.nz)
        enqueue(self.device, "gm_tsdf_fill", self.nx, self.ny, self.nz, self.tsdf, self.weight, float(min_weight), n, int(boundary == "free"),
                float(min_weight if fill_weight is None else fill_weight), self.filled_tsdf, self.filled_weight, counts, workspace=ws)
        self._fill = [n, counts, None]
        return self

    @property
    def fill_stats(self):
        """dict(iterations, filled_voxels, unreached_voxels) of the last fill_holes (the first look waits for the device); None without one"""
        if self._fill is None:
            return None
        if self._fill[2] is None:
            filled, left = (int(c) for c in self._fill[1].cpu())
            self._fill[2] = dict(iterations=self._fill[0], filled_voxels=filled, unreached_voxels=left)
        return dict(self._fill[2])

    def _surface_nets_enqueue(self, min_weight, max_vertices, max_faces, volume=None):
        """gm_surface_nets at the given capacities on (tsdf, weight) = volume, by default the fused pair: (vertex buffer, face buffer,
        device counts); nothing waits"""
        tsdf, weight = (self.tsdf, self.weight) if volume is None else volume
        f = dict(device=self.device)
        V = torch.empty((max_vertices, 3), dtype=torch.float32, **f)
        F = torch.empty((max_faces, 3), dtype=torch.int32, **f)
        counts = torch.empty((2,), dtype=torch.int32, **f)
        ws = workspace(self.device, "gm_surface_nets_workspace_bytes", self.nx, self.ny, self.nz)
        enqueue(self.device, "gm_surface_nets", self.nx, self.ny, self.nz, self._origin_c, self.voxel, tsdf, weight, float(min_weight), max_vertices, V,
                max_faces, F, counts, workspace=ws)
        return V, F, counts

    def _surface_nets(self, min_weight, max_vertices, max_faces, volume=None):
        V, F, counts = self._surface_nets_enqueue(min_weight, max_vertices, max_faces, volume)
        nv, nf = (int(c) for c in counts.cpu())                       # the one host wait
        return V, F, nv, nf

    def extract(self, min_weight=1, keep="largest", target_faces=None, simplify_max_rounds=1024, fill_holes=None, fill_boundary="none"):
        """(vertices float32 [V,3], faces int32 [F,3]) on the device: the zero surface among the samples that at least min_weight views
        observed, by naive surface nets (gm_surface_nets: ids and rows in scan order).  It starts from a capacity guess (a few times
        the largest face of the grid), reads the counts - the one host wait - and runs once more if the guess was short.
        keep="largest": only the connected component with the most faces (ties: the smallest vertex id), unreferenced vertices
        dropped and ids re-numbered in order (on the host: the mesh is small) - a floater would make the mesh unusable, ArapSolver
        refuses a component without a handle; keep="all": everything.  self.stats = vertices / faces / components before the choice.
        target_faces: simplify what was kept to at most that many faces (mesh_simplify.simplify: output vertices are rows of the dense
        mesh) in at most simplify_max_rounds rounds; self.stats then also holds faces_before_simplify, simplify_rounds,
        simplify_stalled, simplify_reached and seconds_simplify (`faces` stays the dense count; the returned F has the final one), and
        self.simplified the whole result (kept, vertex_map; None after an extract without a target).  A run that ends above the target -
        stalled on locked borders, or out of rounds, which a very finely sampled smooth surface can be - is
        returned as it is, with simplify_reached False and a RuntimeWarning.  None: nothing changes.
        fill_holes: an iteration count, or True for fill_holes()'s default: the fill runs first, with this call's min_weight and
        boundary=fill_boundary, and the surface is that of the filled pair; self.stats then also holds fill_iterations, filled_voxels,
        unreached_voxels and seconds_fill (device time between two events; no further host wait).  None: the fused volume as it is."""
        self.simplified = None
        if keep not in ("largest", "all"):
            raise ValueError("TsdfVolume.extract: keep must be 'largest' or 'all'; got %r" % (keep,))
        volume = clock = None
        if fill_holes is not None and fill_holes is not False:
            if fill_boundary not in ("none", "free"):
                raise ValueError("TsdfVolume.extract: fill_boundary must be 'none' or 'free'; got %r" % (fill_boundary,))
            need_cuda(getattr(self, "tsdf", None), "TsdfVolume.extract", "the volume")
            clock = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            clock[0].record(torch.cuda.current_stream(self.device))
            self.fill_holes(None if fill_holes is True else fill_holes, min_weight=min_weight, boundary=fill_boundary)
            clock[1].record(torch.cuda.current_stream(self.device))
            volume = (self.filled_tsdf, self.filled_weight)
        side = max(self.nx * self.ny, self.ny * self.nz, self.nx * self.nz)
        cells = (self.nx - 1) * (self.ny - 1) * (self.nz - 1)
        guess = min(cells, max(4096, 8 * side))
        V, F, nv, nf = self._surface_nets(min_weight, guess, 3 * guess, volume)
        if nv > V.shape[0] or nf > F.shape[0]:
            V, F, nv, nf = self._surface_nets(min_weight, nv, nf, volume)
        V, F = V[:nv], F[:nf]
        self.stats = dict(vertices=nv, faces=nf, components=None, components_dropped=0)
        if volume is not None:                                         # (the counts are there: the wait above was behind the fill)
            st = self.fill_stats
            self.stats.update(fill_iterations=st["iterations"], filled_voxels=st["filled_voxels"], unreached_voxels=st["unreached_voxels"],
                              seconds_fill=clock[0].elapsed_time(clock[1]) * 1e-3)
        if keep == "largest":
            v, f, comps = largest_component(V.cpu().numpy(), F.cpu().numpy())
            self.stats.update(components=comps, components_dropped=max(comps - 1, 0))
            V, F = torch.as_tensor(v, device=self.device), torch.as_tensor(f, device=self.device)
        if target_faces is not None:
            from .mesh_simplify import simplify
            t0 = time.perf_counter()
            self.simplified = simplify(V.contiguous(), F.contiguous(), target_faces=target_faces, max_rounds=simplify_max_rounds)
            torch.cuda.synchronize(self.device)
            st = self.simplified.stats
            self.stats.update(faces_before_simplify=int(F.shape[0]), simplify_rounds=st["rounds"], simplify_stalled=st["stalled"],
                              simplify_reached=st["reached"], seconds_simplify=time.perf_counter() - t0)
            if not st["reached"]:
                warnings.warn("proxy_mesh: simplification ended at %d faces, above target_faces=%d (%s after %d rounds)" % (
                    st["faces"], int(target_faces), "stalled" if st["stalled"] else "out of rounds", st["rounds"]), RuntimeWarning, stacklevel=2)
            V, F = self.simplified.vertices, self.simplified.faces
        return V.contiguous(), F.contiguous()


def default_bounds(pc, resolution, trunc_voxels=3.0, min_opacity=0.5):
    """(bounds_min, bounds_max, voxel): the box of the centres with opacity >= min_opacity, padded by 2 trunc on every side, trunc =
    trunc_voxels voxels of a grid with `resolution` voxels along the padded box's longest side.  Reads the centres (a host wait)."""
    with torch.no_grad():
        xyz, op = pc.get_xyz.detach(), pc.get_opacity.detach().reshape(-1)
        pts = xyz[op >= min_opacity]
        if pts.shape[0] == 0:
            raise ValueError("proxy_mesh: no Gaussian has opacity >= %g: give bounds" % min_opacity)
        lo, hi = pts.min(dim=0).values.cpu().numpy().astype(np.float64), pts.max(dim=0).values.cpu().numpy().astype(np.float64)
    if resolution - 4.0 * trunc_voxels < 2:
        raise ValueError("proxy_mesh: resolution %d leaves no room inside a padding of %g voxels" % (resolution, 2 * trunc_voxels))
    voxel = max(float((hi - lo).max()), 1e-6) / (resolution - 4.0 * trunc_voxels)
    pad = 2.0 * trunc_voxels * voxel
    return lo - pad, hi + pad, voxel


def fuse_cloud(pc, cameras, pipe=None, bg_gaussian=None, resolution=96, bounds=None, views_per_call=8, trunc_voxels=3.0, alpha_min=0.5,
               carve=True, bg_color=None):
    """The TsdfVolume of a trained cloud.  Every camera (renderer.Camera-like, or scenes.camera_from_RT dicts) is rendered with return_aux
    - bg_render for a bg_model.PlainGaussians, render (with bg_gaussian, if given) for a MeshBoundGaussians - and its depth / alpha maps
    are fused, views_per_call views per call.  bounds = (min, max); default: default_bounds()."""
    from .bg_model import PlainGaussians
    from .renderer import Camera, bg_render, render
    need_cuda(pc.get_xyz, "from_cloud", "the cloud")
    dev = pc.get_xyz.device
    pipe = pipe if pipe is not None else SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    bg_color = torch.zeros(3, device=dev) if bg_color is None else bg_color
    cameras = [Camera(c, dev) if isinstance(c, dict) else c for c in cameras]
    if bounds is None:
        lo, hi, voxel = default_bounds(pc, resolution, trunc_voxels)
    else:
        lo, hi = np.asarray(bounds[0], np.float64), np.asarray(bounds[1], np.float64)
        voxel = float((hi - lo).max()) / int(resolution)
    vol = TsdfVolume(lo, hi, voxel_size=voxel, trunc=trunc_voxels * voxel, device=dev)
    plain = isinstance(pc, PlainGaussians)
    step = max(1, int(views_per_call))
    with torch.no_grad():
        for s in range(0, len(cameras), step):
            depth, alpha = [], []
            for cam in cameras[s:s + step]:
                pkg = bg_render(cam, pc, pipe, bg_color, return_aux=True) if plain else render(cam, pc, pipe, bg_color, bg_gaussian=bg_gaussian,
                                                                                               return_aux=True)
                depth.append(pkg["depth"].detach())
                alpha.append(pkg["alpha"].detach())
            vol.integrate(cameras[s:s + step], depth, alpha, alpha_min=alpha_min, carve=carve)
    return vol


def from_cloud(pc, cameras, pipe=None, bg_gaussian=None, resolution=96, bounds=None, views_per_call=8, trunc_voxels=3.0, alpha_min=0.5,
               carve=True, min_weight=1, keep="largest", bg_color=None, target_faces=None, simplify_max_rounds=1024, fill_holes=None,
               fill_boundary="none", vertex_colors=False):
    """The proxy mesh of a trained cloud: (vertices float32 [V,3], faces int32 [F,3]) on the device: fuse_cloud(...).extract(min_weight,
    keep, target_faces, simplify_max_rounds, fill_holes, fill_boundary).  vertex_colors=True: (vertices, faces, colors float32 [V,3]) -
    the same mesh, and the colours of its vertices (the FINAL ones: after keep and after the simplification) from a second rendering of
    the views: mesh_color.color_from_cloud with depth_tol = the volume's trunc and the spread on."""
    vol = fuse_cloud(pc, cameras, pipe=pipe, bg_gaussian=bg_gaussian, resolution=resolution, bounds=bounds, views_per_call=views_per_call,
                     trunc_voxels=trunc_voxels, alpha_min=alpha_min, carve=carve, bg_color=bg_color)
    V, F = vol.extract(min_weight=min_weight, keep=keep, target_faces=target_faces, simplify_max_rounds=simplify_max_rounds, fill_holes=fill_holes,
                       fill_boundary=fill_boundary)
    if not vertex_colors:
        return V, F
    from .mesh_color import color_from_cloud
    colors = color_from_cloud(pc, cameras, V, F, pipe=pipe, bg_gaussian=bg_gaussian, views_per_call=views_per_call, alpha_min=alpha_min,
                              depth_tol=vol.trunc, spread=True, bg_color=bg_color)
    return V, F, colors


def load_model(path, mesh_gaussian, dev):
    from . import io as gio
    t = lambda a: on_device(a, torch.float32, dev)
    if not mesh_gaussian:
        from .bg_model import PlainGaussians
        m = gio.load_plain_gaussians(path)
        pc = PlainGaussians(3, device=dev)
        pc._set_params(t(m["xyz"]), torch.cat([t(m["features_dc"]), t(m["features_rest"])], dim=1), t(m["scaling"]), t(m["rotation"]),
                       t(m["opacity"]).reshape(-1, 1))
        pc.active_sh_degree = pc.max_sh_degree
        return pc
    from .renderer import MeshBoundGaussians
    m = gio.load_mesh_gaussians(path)
    return MeshBoundGaussians(t(m["bc"]), t(m["distance"]), t(m["features_dc"]), t(m["features_rest"]), t(m["scaling"]), t(m["rotation"]),
                              t(m["opacity"]), t(m["v1"]), t(m["v2"]), t(m["v3"]), t(m["normal"]), t(m["radius"]))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m gaussianmesh_amd.proxy_mesh", description="cloud.ply + cameras.json -> proxy.obj")
    ap.add_argument("--gaussian", required=True, help="the trained cloud (a plain 3DGS PLY; with --mesh_gaussian a mesh-bound one)")
    ap.add_argument("--cameras", required=True, help="cameras.json of the training views")
    ap.add_argument("--out", required=True, help="the OBJ to write")
    ap.add_argument("--mesh_gaussian", action="store_true")
    ap.add_argument("--resolution", type=int, default=96)
    ap.add_argument("--bounds", type=float, nargs=6, metavar=("x0", "y0", "z0", "x1", "y1", "z1"))
    ap.add_argument("--trunc_voxels", type=float, default=3.0)
    ap.add_argument("--alpha_min", type=float, default=0.5)
    ap.add_argument("--keep", choices=("largest", "all"), default="largest")
    ap.add_argument("--target_faces", type=int, help="simplify the mesh to at most this many faces (mesh_simplify)")
    ap.add_argument("--simplify_max_rounds", type=int, default=1024)
    ap.add_argument("--fill_holes", type=int, metavar="N", help="close unobserved holes first: N diffusion iterations (gm_tsdf_fill)")
    ap.add_argument("--fill_boundary", choices=("none", "free"), default="none", help="free: beyond the grid is free space")
    ap.add_argument("--vertex_colors", action="store_true", help="colour the final mesh from the views (mesh_color): v x y z r g b records")
    ap.add_argument("--color_spread", type=int, metavar="N", help="steps of the spread over vertices no view coloured (default: min(vertices, 1024))")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("proxy_mesh needs a HIP (cuda) device; there is no CPU path")
    from . import io as gio
    dev = torch.device("cuda")
    t0 = time.perf_counter()
    pc = load_model(a.gaussian, a.mesh_gaussian, dev)
    cams = gio.load_cameras_json(a.cameras)
    if not cams:
        raise SystemExit("proxy_mesh: %s holds no camera" % a.cameras)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    bounds = None if a.bounds is None else (a.bounds[:3], a.bounds[3:])
    vol = fuse_cloud(pc, cams, resolution=a.resolution, bounds=bounds, trunc_voxels=a.trunc_voxels, alpha_min=a.alpha_min)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    V, F = vol.extract(keep=a.keep, target_faces=a.target_faces, simplify_max_rounds=a.simplify_max_rounds, fill_holes=a.fill_holes,
                       fill_boundary=a.fill_boundary)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    colors = color_stats = None
    if a.vertex_colors:                                                # on the final mesh, from a second rendering of the views
        from .mesh_color import colors_and_state
        colors, vc = colors_and_state(pc, cams, V, F, None, None, 8, a.alpha_min, vol.trunc, False, True if a.color_spread is None else a.color_spread,
                                       None)
        colors, color_stats = colors.cpu().numpy(), vc.stats           # (the copy waits for the device)
    t_write = time.perf_counter()
    v, f = V.cpu().numpy(), F.cpu().numpy()
    gio.write_obj(a.out, v, f, colors)
    t4 = time.perf_counter()
    out = dict(vertices=int(v.shape[0]), faces=int(f.shape[0]), components_dropped=int(vol.stats["components_dropped"]),
               boundary_edges=boundary_edges(f), grid=[vol.nx, vol.ny, vol.nz], views=len(cams),
               seconds=dict(load=t1 - t0, render_fuse=t2 - t1, extract=t3 - t2, write=t4 - t_write))
    if a.target_faces is not None:                                     # (extract's time then includes the simplification)
        out.update(faces_before_simplify=vol.stats["faces_before_simplify"], simplify_rounds=vol.stats["simplify_rounds"],
                   simplify_reached=vol.stats["simplify_reached"])
        out["seconds"]["simplify"] = vol.stats["seconds_simplify"]
    if a.fill_holes is not None:                                       # (and the fill)
        out.update(fill_iterations=vol.stats["fill_iterations"], filled_voxels=vol.stats["filled_voxels"],
                   unreached_voxels=vol.stats["unreached_voxels"])
        out["seconds"]["fill"] = vol.stats["seconds_fill"]
    if a.vertex_colors:
        out.update(colored_vertices=color_stats["seen"], spread_vertices=color_stats["filled"], uncolored_vertices=color_stats["unreached"])
        out["seconds"]["color"] = t_write - t3
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
