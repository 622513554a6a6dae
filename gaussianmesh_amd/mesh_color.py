"""Colour on the proxy mesh: the views' own renders fused into one colour per vertex (csrc/gm_mesh_color.hip).  Every view is rendered with
return_aux; a vertex takes the colour of the pixel it projects to when that view's depth map says the view sees it (within depth_tol) and
the vertex faces the camera, weighted by the squared cosine of the viewing angle (gm_mesh_color_integrate); the vertices no view coloured
get a value from their neighbours (gm_mesh_color_spread).  The reference's way of working is to deform the proxy mesh in another program:
with `v x y z r g b` records the artist sees the object, not a grey blob.  Definition, ABI and rules: INTEGRATION.md section X.

    colors = color_from_cloud(model, cameras, V, F)            # float32 [Vm,3] on the device; io.write_obj(path, V, F, colors)
    V, F, colors = proxy_mesh.from_cloud(model, cameras, vertex_colors=True)
    python -m gaussianmesh_amd.mesh_color --gaussian cloud.ply --cameras cameras.json --mesh in.obj --out out.obj
"""
import argparse
import ctypes as C
import json
import math
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from ._op import enqueue, need_cuda, workspace
from .deform import vertex_face_adjacency
from .mesh_bind import mesh_arrays
from .mesh_pick import camera_rays, camera_tuple, first_hits
from .proxy_mesh import maps_list

SPREAD_MAX = 1024                # spread=True: min(Vm, SPREAD_MAX) steps


def _images(x, who):
    """a list of [3,H,W] images from a list of such tensors or one stacked [K,3,H,W] tensor"""
    if torch.is_tensor(x):
        if x.dim() == 3:
            x = x[None]
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("%s: images must be [K,3,H,W]; got %s" % (who, tuple(x.shape)))
        return list(x.unbind(0))
    out = []
    for m in x:
        if not torch.is_tensor(m):
            raise _lib.GmeshError("%s needs the images as tensors on a HIP (cuda) device; there is no CPU path" % who)
        if m.dim() != 3 or m.shape[0] != 3:
            raise ValueError("%s: every image must be [3,H,W]; got %s" % (who, tuple(m.shape)))
        out.append(m)
    return out


def _mesh_on_device(vertices, faces, who):
    """(vertices float32 [Vm,3], faces int32 [F,3]) contiguous on the vertices' device, the face indices checked on the host"""
    need_cuda(vertices, who, "the vertices")
    mesh_arrays(vertices, faces, who)
    dev = vertices.device
    V = vertices.detach().to(torch.float32).contiguous()
    F = (faces.detach() if torch.is_tensor(faces) else torch.as_tensor(np.ascontiguousarray(faces))).to(device=dev, dtype=torch.int32).contiguous()
    return V, F


def _adjacency(faces, Vm, dev):
    off, adj = vertex_face_adjacency(faces, Vm)
    return torch.as_tensor(off, device=dev), torch.as_tensor(adj, device=dev)


def _normals(V, F, adjacency):
    off, adj = adjacency
    N = torch.empty_like(V)
    enqueue(V.device, "gm_mesh_vertex_normals", V.shape[0], F.shape[0], V, F, off, adj, N)
    return N


def vertex_normals(vertices, faces, adjacency=None):
    """gm_mesh_vertex_normals: float32 [Vm,3] on the device, the sum of the cross products (b - a) x (c - a) of the faces at each vertex in
    adjacency order - unnormalised, area-weighted; (0, 0, 0) at a vertex without faces.  adjacency: (offsets, face ids) of
    deform.vertex_face_adjacency as device tensors; None: built here on the host.  vertices on a HIP (cuda) device; no CPU path."""
    V, F = _mesh_on_device(vertices, faces, "vertex_normals")
    if adjacency is None:
        adjacency = _adjacency(F, V.shape[0], V.device)
    for a in adjacency:
        need_cuda(a, "vertex_normals", "the adjacency")
    return _normals(V, F, tuple(a.to(torch.int32).contiguous() for a in adjacency))


class VertexColors:
    """The running colour sums of a mesh: csum float32 [Vm,3] and wsum float32 [Vm] on the device, with the normals and the adjacency
    they need.  integrate() adds views, resolve() turns the sums into colours.  two_sided: a vertex also takes colour from the views its
    normal points away from (a mesh without a consistent winding).  default_depth_tol: 1 % of the bounding box's diagonal (read once,
    here)."""

    def __init__(self, vertices, faces, two_sided=False):
        self.vertices, self.faces = _mesh_on_device(vertices, faces, "VertexColors")
        self.device = self.vertices.device
        self.two_sided = bool(two_sided)
        Vm = self.vertices.shape[0]
        self.adjacency = _adjacency(self.faces, Vm, self.device)
        self.normals = _normals(self.vertices, self.faces, self.adjacency)
        self.csum = torch.zeros((Vm, 3), dtype=torch.float32, device=self.device)
        self.wsum = torch.zeros((Vm,), dtype=torch.float32, device=self.device)
        self.views = 0
        self._stats = None
        if Vm:
            lo, hi = self.vertices.min(dim=0).values.cpu().numpy().astype(np.float64), self.vertices.max(dim=0).values.cpu().numpy().astype(np.float64)
            self.default_depth_tol = float(np.float32(0.01 * float(np.linalg.norm(hi - lo))))
        else:
            self.default_depth_tol = 0.0

    def integrate(self, cameras, images, depth, alpha, alpha_min=0.5, depth_tol=None):
        """Add views: cameras, depth and alpha as TsdfVolume.integrate takes them, images the renders as a list of [3,H,W] tensors or one
        stacked [K,3,H,W].  Views of one resolution go into one call each, in the order given (the sums' bits depend on the order of the
        views, not on the grouping).  depth_tol: how far the depth map may lie from the vertex's own depth; None: default_depth_tol.
        Only enqueues; nothing waits for the device."""
        who = "VertexColors.integrate"
        cameras = list(cameras)
        images, depth, alpha = _images(images, who), maps_list(depth, who, "depth"), maps_list(alpha, who, "alpha")
        if not (len(cameras) == len(images) == len(depth) == len(alpha)):
            raise ValueError("%s: %d cameras, %d images, %d depth maps, %d alpha maps" % (who, len(cameras), len(images), len(depth), len(alpha)))
        for im, d, a in zip(images, depth, alpha):
            need_cuda(im, who, "the images")
            need_cuda(d, who, "the depth maps")
            need_cuda(a, who, "the alpha maps")
            if d.shape != a.shape or tuple(im.shape[1:]) != tuple(d.shape):
                raise ValueError("%s: an image is %s, its depth map %s and its alpha map %s" % (who, tuple(im.shape), tuple(d.shape), tuple(a.shape)))
        tol = self.default_depth_tol if depth_tol is None else float(depth_tol)
        self._stats = None
        Vm = self.vertices.shape[0]
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
                    raise ValueError("%s: a %d x %d camera with %d x %d maps" % (who, cw, ch, W, H))
                rows.append(view.detach().to(self.device, torch.float32).reshape(16))
                tans.append((tanx, tany))
            views = torch.stack(rows).contiguous()
            tanfov = torch.tensor(tans, dtype=torch.float32).to(self.device, non_blocking=True)
            stack = lambda maps: torch.stack([m.detach().to(self.device, torch.float32) for m in maps]).contiguous()
            ii, dd, aa = stack(images[k:e]), stack(depth[k:e]), stack(alpha[k:e])
            enqueue(self.device, "gm_mesh_color_integrate", e - k, H, W, ii, dd, aa, views, tanfov, Vm, self.vertices, self.normals, float(alpha_min),
                    tol, int(self.two_sided), self.csum, self.wsum)
            self.views += e - k
            k = e
        return self

    def resolve(self, min_weight=0.0, spread=None, fallback=(0.5, 0.5, 0.5)):
        """colors float32 [Vm,3] on the device: seen = (wsum > 0) & (wsum >= min_weight), colors = csum / wsum where seen, fallback
        elsewhere.  spread=N: then N steps of gm_mesh_color_spread - an unseen vertex takes the mean of its neighbours that have a value,
        seen ones never move -, True: min(Vm, 1024) steps.  That is a REACH, not a convergence claim: after n steps exactly the vertices
        within n edges of a seen one have a value, and values further from the seen ones are less settled; a component without a seen
        vertex keeps the fallback.  Only enqueues; self.stats (seen, filled, unreached) reads the counts when it is asked for."""
        fb = [float(x) for x in fallback]
        if len(fb) != 3:
            raise ValueError("VertexColors.resolve: fallback must be three numbers; got %r" % (fallback,))
        Vm = self.vertices.shape[0]
        seen = (self.wsum > 0) & (self.wsum >= float(min_weight))
        colors = torch.where(seen[:, None], self.csum / self.wsum[:, None], torch.tensor(fb, dtype=torch.float32, device=self.device)).contiguous()
        counts = None
        if spread is not None and spread is not False:
            n = min(Vm, SPREAD_MAX) if spread is True else int(spread)
            if n < 0:
                raise ValueError("VertexColors.resolve: spread must not be negative; got %r" % (spread,))
            off, adj = self.adjacency
            seen8 = seen.to(torch.uint8)
            has = torch.empty((Vm,), dtype=torch.uint8, device=self.device)
            counts = torch.empty((2,), dtype=torch.int32, device=self.device)
            ws = workspace(self.device, "gm_mesh_color_spread_workspace_bytes", Vm)
            enqueue(self.device, "gm_mesh_color_spread", Vm, self.faces.shape[0], self.faces, off, adj, seen8, n, (C.c_float * 3)(*fb), colors, has,
                    counts, workspace=ws)
        self._stats = [seen.sum(), counts, None]
        return colors

    @property
    def stats(self):
        """dict(seen, filled, unreached) of the last resolve (the first look waits for the device); None without one"""
        if self._stats is None:
            return None
        if self._stats[2] is None:
            seen = int(self._stats[0])
            filled, left = (int(c) for c in self._stats[1].cpu()) if self._stats[1] is not None else (0, self.vertices.shape[0] - seen)
            self._stats[2] = dict(seen=seen, filled=filled, unreached=left)
        return dict(self._stats[2])


def _color_from_cloud(pc, cameras, vertices, faces, pipe, bg_gaussian, views_per_call, alpha_min, depth_tol, two_sided, spread, bg_color):
    """(colors, the VertexColors that made them)"""
    from .bg_model import PlainGaussians
    from .renderer import Camera, bg_render, render
    need_cuda(pc.get_xyz, "color_from_cloud", "the cloud")
    dev = pc.get_xyz.device
    pipe = pipe if pipe is not None else SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    bg_color = torch.zeros(3, device=dev) if bg_color is None else bg_color
    cameras = [Camera(c, dev) if isinstance(c, dict) else c for c in cameras]
    vc = VertexColors(vertices, faces, two_sided=two_sided)
    plain = isinstance(pc, PlainGaussians)
    step = max(1, int(views_per_call))
    with torch.no_grad():
        for s in range(0, len(cameras), step):
            image, depth, alpha = [], [], []
            for cam in cameras[s:s + step]:
                pkg = bg_render(cam, pc, pipe, bg_color, return_aux=True) if plain else render(cam, pc, pipe, bg_color, bg_gaussian=bg_gaussian,
                                                                                               return_aux=True)
                image.append(pkg["render"].detach())
                depth.append(pkg["depth"].detach())
                alpha.append(pkg["alpha"].detach())
            vc.integrate(cameras[s:s + step], image, depth, alpha, alpha_min=alpha_min, depth_tol=depth_tol)
        return vc.resolve(spread=spread), vc


colors_and_state = _color_from_cloud     # (colors, VertexColors): for a caller that also reports vc.stats (the command lines)


def color_from_cloud(pc, cameras, vertices, faces, pipe=None, bg_gaussian=None, views_per_call=8, alpha_min=0.5, depth_tol=None, two_sided=False,
                     spread=True, bg_color=None):
    """The vertex colours of a mesh (vertices [Vm,3] on the device, faces [F,3]) from a trained cloud: float32 [Vm,3] on the device.
    Every camera is rendered as proxy_mesh.fuse_cloud renders it (return_aux) and its render / depth / alpha are integrated,
    views_per_call views per call; then resolve(spread=spread).  depth_tol=None: 1 % of the diagonal of the vertices' bounding box
    (computed on the host: one wait).  The mesh may be any mesh of the object, for instance one made elsewhere."""
    return _color_from_cloud(pc, cameras, vertices, faces, pipe, bg_gaussian, views_per_call, alpha_min, depth_tol, two_sided, spread, bg_color)[0]


def render_preview(camera, vertices, faces, colors, bg_color=None):
    """[3,H,W] float32 on the device: the coloured mesh as the camera sees it, one ray per pixel through gm_ray_mesh (mesh_pick): a pixel
    whose ray hits face (a, b, c) at (u, v) shows (1 - u - v) c_a + u c_b + v c_c, a pixel whose ray misses shows bg_color (black unless
    given).  No shading, no lighting: a preview of where colours, picks and handles lie.  Torch glue; no kernel of its own."""
    need_cuda(vertices, "render_preview", "the vertices")
    dev = vertices.device
    if isinstance(camera, dict):
        from .renderer import Camera
        camera = Camera(camera, dev)
    _, _, _, W, H, _, _ = camera_tuple(camera)
    V, F = _mesh_on_device(vertices, faces, "render_preview")
    col = colors.detach().to(device=dev, dtype=torch.float32) if torch.is_tensor(colors) else torch.as_tensor(np.asarray(colors), dtype=torch.float32, device=dev)
    if col.shape != V.shape:
        raise ValueError("render_preview: one colour per vertex (%s); got %s" % (tuple(V.shape), tuple(col.shape)))
    bg = torch.zeros(3, device=dev) if bg_color is None else torch.as_tensor(bg_color, dtype=torch.float32, device=dev).reshape(3)
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    origins, dirs = camera_rays(camera, torch.stack([x.reshape(-1), y.reshape(-1)], dim=1))
    _, face, uv = first_hits(origins.to(dev).contiguous(), dirs.to(dev).contiguous(), V, F, 0.0, math.inf)
    tri = F[face.clamp(min=0)].long()
    u, v = uv[:, 0:1], uv[:, 1:2]
    shade = ((1.0 - u - v) * col[tri[:, 0]] + u * col[tri[:, 1]]) + v * col[tri[:, 2]]
    out = torch.where((face >= 0)[:, None], shade, bg[None, :])
    return out.reshape(H, W, 3).permute(2, 0, 1).contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m gaussianmesh_amd.mesh_color", description="cloud.ply + cameras.json + mesh.obj -> coloured mesh.obj")
    ap.add_argument("--gaussian", required=True, help="the trained cloud (a plain 3DGS PLY; with --mesh_gaussian a mesh-bound one)")
    ap.add_argument("--cameras", required=True, help="cameras.json of the training views")
    ap.add_argument("--mesh", required=True, help="the OBJ to colour")
    ap.add_argument("--out", required=True, help="the OBJ to write: v x y z r g b")
    ap.add_argument("--mesh_gaussian", action="store_true")
    ap.add_argument("--two_sided", action="store_true", help="also take colour from the views a vertex's normal points away from")
    ap.add_argument("--alpha_min", type=float, default=0.5)
    ap.add_argument("--depth_tol", type=float, help="default: 1 %% of the mesh's bounding-box diagonal")
    ap.add_argument("--spread", type=int, metavar="N", help="steps of the spread over unseen vertices (default: min(vertices, %d))" % SPREAD_MAX)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mesh_color needs a HIP (cuda) device; there is no CPU path")
    from . import io as gio
    from .proxy_mesh import load_model
    dev = torch.device("cuda")
    t0 = time.perf_counter()
    pc = load_model(a.gaussian, a.mesh_gaussian, dev)
    cams = gio.load_cameras_json(a.cameras)
    if not cams:
        raise SystemExit("mesh_color: %s holds no camera" % a.cameras)
    v, f = gio.read_obj(a.mesh)
    V, F = torch.as_tensor(v, dtype=torch.float32, device=dev), torch.as_tensor(f, device=dev)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    colors, vc = _color_from_cloud(pc, cams, V, F, None, None, 8, a.alpha_min, a.depth_tol, a.two_sided, True if a.spread is None else a.spread, None)
    c = colors.cpu().numpy()
    t2 = time.perf_counter()
    gio.write_obj(a.out, v, f, c)
    t3 = time.perf_counter()
    st = vc.stats
    print(json.dumps(dict(vertices=int(v.shape[0]), seen=st["seen"], filled=st["filled"], unreached=st["unreached"],
                          seconds=dict(load=t1 - t0, color=t2 - t1, write=t3 - t2))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
