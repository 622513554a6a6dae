"""From the screen to the proxy mesh: the first hit of a ray on the current mesh (gm_ray_mesh, csrc/gm_raycast.hip) and the thin glue an
editor needs around it - pixels to rays, a pick (face, vertex, point, depth), the vertices visible inside a screen rectangle, and a
pixel offset turned into a world position at a point's own depth.  The reference has no such stage (its meshes come finished from
another program); the rasterizer's depth map is an alpha-blended depth of Gaussians, not a point on the mesh, and names no face."""
import math

import numpy as np
import torch

from ._op import enqueue, f32, need_cuda, workspace
from .mesh_bind import device_mesh, mesh_arrays

OCCLUSION_TOLERANCE = 2.0 ** -10     # visible_vertices: a hit at t >= 1 - 2^-10 is the vertex's own neighbourhood (part of the definition)


def camera_tuple(camera):
    """(view [4,4] stored transposed, proj [4,4], centre [3], W, H, tan(FoVx/2), tan(FoVy/2)) of a camera with the reference's attribute
    names (renderer.Camera) or of a scenes.camera_from_RT dict; the tensors where the camera holds them."""
    if isinstance(camera, dict):
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)
        return t(camera["view"]), t(camera["proj"]), t(camera["campos"]), int(camera["W"]), int(camera["H"]), \
            math.tan(camera["fovx"] * 0.5), math.tan(camera["fovy"] * 0.5)
    c = camera
    return c.world_view_transform, c.full_proj_transform, c.camera_center, int(c.image_width), int(c.image_height), \
        math.tan(c.FoVx * 0.5), math.tan(c.FoVy * 0.5)


def _rows(a, width, device, who, what):
    a = a.detach().to(device=device, dtype=torch.float32) if torch.is_tensor(a) else torch.as_tensor(np.asarray(a), dtype=torch.float32, device=device)
    if a.dim() != 2 or a.shape[1] != width:
        raise ValueError("%s: %s must be [P,%d]; got %s" % (who, what, width, tuple(a.shape)))
    return a


def camera_rays(camera, pixels):
    """(origins, dirs) float32 [P,3] of the rays through pixels [P,2] = (x, y) in the rasterizer's pixel coordinates (an integer value
    is a pixel centre: the inverse of ndc2pix, csrc/gm_pre_body.h).  View-space direction (((2x+1)/W - 1) tan(FoVx/2),
    ((2y+1)/H - 1) tan(FoVy/2), 1), world direction d_view @ world_view_transform[:3,:3].T (the matrix is stored transposed), origin
    camera_center.  Directions are NOT normalised: a hit's t is its view depth.  Torch on the camera's device (CPU tensors work)."""
    view, _, centre, W, H, tanx, tany = camera_tuple(camera)
    pix = _rows(pixels, 2, view.device, "camera_rays", "pixels")
    dv = torch.stack([((2.0 * pix[:, 0] + 1.0) / W - 1.0) * tanx, ((2.0 * pix[:, 1] + 1.0) / H - 1.0) * tany, torch.ones_like(pix[:, 0])], dim=1)
    dirs = dv @ view[:3, :3].T
    return centre.reshape(1, 3).expand(pix.shape[0], 3).contiguous(), dirs.contiguous()


def _view_space(camera, points):
    view, _, _, W, H, tanx, tany = camera_tuple(camera)
    return points @ view[:3, :3] + view[3, :3], W, H, tanx, tany


def screen_offset(camera, points, pixel_offsets):
    """World points [P,3] moved parallel to the image plane by pixel_offsets [P,2], each at its own view depth z: the move in view x
    and y is (dx 2 tan(FoVx/2) / W z, dy 2 tan(FoVy/2) / H z), rotated back to world space and added (a zero offset returns the point
    itself).  Torch on the points' device; nothing waits."""
    view, _, _, W, H, tanx, tany = camera_tuple(camera)
    pts = _rows(points, 3, points.device if torch.is_tensor(points) else view.device, "screen_offset", "points")
    view = view.to(pts.device)
    off = _rows(pixel_offsets, 2, pts.device, "screen_offset", "pixel_offsets")
    if off.shape[0] != pts.shape[0]:
        raise ValueError("screen_offset: one pixel offset per point (%d), got %d" % (pts.shape[0], off.shape[0]))
    z = (pts @ view[:3, 2:3])[:, 0] + view[3, 2]
    mv = torch.stack([off[:, 0] * (2.0 * tanx / W) * z, off[:, 1] * (2.0 * tany / H) * z, torch.zeros_like(z)], dim=1)
    return pts + mv @ view[:3, :3].T


def first_hits(origins, dirs, vd, fd, t_min, t_max, want_uv=True):
    """gm_ray_mesh on device tensors (contiguous float32 / int32, checked by the callers)"""
    dev = origins.device
    R, Vm, F = origins.shape[0], vd.shape[0], fd.shape[0]
    if R and (F == 0 or Vm == 0):
        raise ValueError("ray_mesh_hits: the mesh is empty (%d vertices, %d faces)" % (Vm, F))
    t = torch.empty((R,), dtype=torch.float32, device=dev)
    face = torch.empty((R,), dtype=torch.int32, device=dev)
    uv = torch.empty((R, 2), dtype=torch.float32, device=dev) if want_uv else None
    if R > 0:
        ws = workspace(dev, "gm_ray_mesh_workspace_bytes", R, F)
        enqueue(dev, "gm_ray_mesh", R, origins, dirs, Vm, vd, F, fd, float(t_min), float(t_max), t, face, uv, workspace=ws)
    return t, face.long(), uv


def ray_mesh_hits(origins, dirs, vertices, faces, t_min=0.0, t_max=math.inf, check_faces=True):
    """The first hit of every ray (origins, dirs float [R,3] on a HIP (cuda) device) on the mesh (vertices [Vm,3], faces [F,3]):
    (t float32 [R], face int64 [R], uv float32 [R,2]) on the device.  gm_ray_mesh: Moeller-Trumbore per (ray, face) in float32 without
    contraction, two-sided, no epsilon; a hit needs u >= 0, v >= 0, u + v <= 1 and t_min <= t <= t_max; the smallest t wins, ties to
    the lowest face index - a float32 brute force gives the same bits.  No hit: face -1, t +inf, uv NaN.  The hit point is
    (a + (b - a) u) + (c - a) v.  vertices / faces may be host arrays or tensors on any device; the face indices are checked on the
    host (check_faces=False: the caller has checked this face tensor before; nothing then waits for the device).  No CPU path."""
    for name, x in (("origins", origins), ("dirs", dirs)):
        if not torch.is_tensor(x) or x.dim() != 2 or x.shape[1] != 3:
            raise ValueError("ray_mesh_hits: %s must be a [R,3] tensor; got %s" % (name, tuple(getattr(x, "shape", ()))))
    if origins.shape[0] != dirs.shape[0]:
        raise ValueError("ray_mesh_hits: one direction per origin (%d), got %d" % (origins.shape[0], dirs.shape[0]))
    if not (t_min >= 0.0) or t_max != t_max:
        raise ValueError("ray_mesh_hits: t_min must be >= 0 and neither bound NaN; got %r, %r" % (t_min, t_max))
    if check_faces:
        v, f = mesh_arrays(vertices, faces, "ray_mesh_hits")
        if origins.shape[0] and (f.shape[0] == 0 or v.shape[0] == 0):
            raise ValueError("ray_mesh_hits: the mesh is empty (%d vertices, %d faces)" % (v.shape[0], f.shape[0]))
    need_cuda(origins, "ray_mesh_hits", "the rays")
    dev = origins.device
    vd, fd = device_mesh(vertices, faces, "ray_mesh_hits", dev, check_faces=False)
    o = f32(origins)
    d = dirs.detach().to(dev).contiguous().float()
    return first_hits(o, d, vd, fd, t_min, t_max)


def _camera_device(camera, who):
    dev = camera_tuple(camera)[0].device
    need_cuda(dev, who, "the camera")
    return dev


def pick(camera, pixels, vertices, faces, check_faces=True):
    """What lies under pixels [P,2] of the camera: dict(face int64 [P] (-1: nothing), vertex int64 [P] the corner of the hit face with
    the largest of (1 - u - v, u, v), ties to the first of a, b, c (-1 on a miss), point float32 [P,3] = (a + e1 u) + e2 v (NaN on a
    miss), depth float32 [P] = t, the view depth (+inf on a miss)).  Everything stays on the device; nothing waits for it."""
    dev = _camera_device(camera, "pick")
    origins, dirs = camera_rays(camera, pixels)
    vd, fd = device_mesh(vertices, faces, "pick", dev, check_faces)
    t, face, uv = first_hits(origins, dirs, vd, fd, 0.0, math.inf)
    hit = face >= 0
    tri = fd[face.clamp(min=0)].long()
    a, b, c = vd[tri[:, 0]], vd[tri[:, 1]], vd[tri[:, 2]]
    u, v = uv[:, 0:1], uv[:, 1:2]
    point = (a + (b - a) * u) + (c - a) * v
    weights = torch.cat([1.0 - u - v, u, v], dim=1)
    corner = torch.argmax(torch.where(hit[:, None], weights, torch.zeros_like(weights)), dim=1, keepdim=True)      # the first of the largest
    vertex = torch.where(hit, tri.gather(1, corner)[:, 0], torch.full_like(face, -1))
    return dict(face=face, vertex=vertex, point=point, depth=t)


def visible_vertices(camera, vertices, faces, rect=None, check_faces=True):
    """bool [Vm]: the vertices the camera sees.  One ray per vertex, o = camera_center, d = vertex - o (t = 1 at the vertex); vertex i
    is visible iff its ray hits nothing (a ray can slip between the vertex's own faces), or the hit face has i as a corner, or
    t >= 1 - 2^-10 (the tolerance is part of the definition).  rect = (x0, y0, x1, y1) in pixels: the vertex must also have a view depth
    > 0 and its projected pixel inside the rectangle, edges included."""
    dev = _camera_device(camera, "visible_vertices")
    vd, fd = device_mesh(vertices, faces, "visible_vertices", dev, check_faces)
    centre = camera_tuple(camera)[2].reshape(1, 3)
    origins = centre.expand(vd.shape[0], 3).contiguous()
    t, face, _ = first_hits(origins, (vd - centre).contiguous(), vd, fd, 0.0, math.inf, want_uv=False)
    own = (fd[face.clamp(min=0)].long() == torch.arange(vd.shape[0], device=dev)[:, None]).any(dim=1)
    visible = (face < 0) | own | (t >= 1.0 - OCCLUSION_TOLERANCE)
    if rect is not None:
        x0, y0, x1, y1 = (float(r) for r in rect)
        pv, W, H, tanx, tany = _view_space(camera, vd)
        z = pv[:, 2]
        px = ((pv[:, 0] / (z * tanx) + 1.0) * W - 1.0) * 0.5
        py = ((pv[:, 1] / (z * tany) + 1.0) * H - 1.0) * 0.5
        visible = visible & (z > 0) & (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)
    return visible
