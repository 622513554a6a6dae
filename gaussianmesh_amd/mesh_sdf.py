"""A triangle mesh as a solid: generalized winding numbers (gm_mesh_winding) and signed distances (gm_mesh_signed_distance, which
composes them with gm_closest_face) on the device - the point-in-mesh test for arbitrary points, and the values of a
dynamics.SdfGrid over a mesh (SdfGrid.from_mesh), which is how a simulated mesh collides with another mesh.  The winding number
(Jacobson et al. 2013) is 1 inside a closed mesh, 0 outside, and degrades gracefully where the mesh is open or non-manifold, as
surface-nets proxies simplified and cut by unobserved regions are.  Definition, ABI and rules: include/gmesh_hip.h,
csrc/gm_winding.hip, INTEGRATION.md section AD.  Every (point, face) pair is evaluated: O(N F), a once-per-scene cost."""
import numpy as np
import torch

from ._op import enqueue, f32, host, need_cuda, on_device, workspace
from .mesh_bind import mesh_arrays

WN_CHUNK = 1024                  # faces per partial sum of gm_mesh_winding (csrc/gm_winding.hip)
SLAB_PARTIAL_BYTES = 1 << 28     # grid_values: the partial sums of one slab (8 bytes x points x chunks) stay below this


def _checked(who, points, vertices, faces):
    """the checks every function here shares, before anything is enqueued: (points float32 [N,3], vertices, faces on its device)"""
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("%s: points must be a [N,3] tensor; got %s" % (who, tuple(getattr(points, "shape", ()))))
    v, f = mesh_arrays(vertices, faces, who)
    if points.shape[0] and (f.shape[0] == 0 or v.shape[0] == 0):
        raise ValueError("%s: the mesh is empty (%d vertices, %d faces)" % (who, v.shape[0], f.shape[0]))
    need_cuda(points, who, "the points")
    dev = points.device
    return f32(points), on_device(vertices, torch.float32, dev), on_device(faces, torch.int32, dev)


def winding_numbers(points, vertices, faces):
    """The generalized winding number of the mesh (vertices [Vm,3], faces [F,3] vertex ids) at every row of points [N,3]: float64
    [N] on the points' device.  gm_mesh_winding: per (point, face) the signed solid angle 2 atan2(det, den) of Van Oosterom &
    Strackee in float64 from the float32 inputs, summed in chunks of 1024 faces in face order, the chunk sums in chunk order, over
    4 pi - the same bits in every run and for every batching of the points.  1 inside a closed mesh wound outwards, -1 inside one
    wound inwards, 0 outside.  points on a HIP (cuda) device; vertices / faces may be host arrays or tensors on any device (the
    face indices are checked on the host).  No CPU path."""
    return _winding(*_checked("winding_numbers", points, vertices, faces))


def _winding(p, vd, fd):
    N, Vm, F = p.shape[0], vd.shape[0], fd.shape[0]
    w = torch.empty((N,), dtype=torch.float64, device=p.device)
    if N > 0:
        ws = workspace(p.device, "gm_mesh_winding_workspace_bytes", N, F)
        enqueue(p.device, "gm_mesh_winding", N, p, Vm, vd, F, fd, w, workspace=ws)
    return w


def _signed(p, vd, fd, want_face, want_closest, want_winding):
    """gm_mesh_signed_distance on checked device tensors: (phi, face int32 or None, closest or None, w or None)"""
    dev, N, Vm, F = p.device, p.shape[0], vd.shape[0], fd.shape[0]
    phi = torch.empty((N,), dtype=torch.float32, device=dev)
    face = torch.empty((N,), dtype=torch.int32, device=dev) if want_face else None
    close = torch.empty((N, 3), dtype=torch.float32, device=dev) if want_closest else None
    w = torch.empty((N,), dtype=torch.float64, device=dev) if want_winding else None
    if N > 0:
        ws = workspace(dev, "gm_mesh_signed_distance_workspace_bytes", N, F)
        enqueue(dev, "gm_mesh_signed_distance", N, p, Vm, vd, F, fd, phi, face, close, w, workspace=ws)
    return phi, face, close, w


def signed_distances(points, vertices, faces, want_face=False, want_closest=False, want_winding=False):
    """The signed distance of every row of points [N,3] to the mesh, negative inside: phi float32 [N], followed by whatever was asked
    for, in this order: face int64 [N] and closest float32 [N,3] (mesh_bind.closest_faces' outputs, bit for bit), winding float64
    [N] (winding_numbers').  A tuple when anything was asked for, else phi alone.  gm_mesh_signed_distance:
    phi = s * sqrt(d2) with d2 the float32 squared distance to the closest face, the float32 root correctly rounded, and s = -1 iff
    |w| > 0.5 - the absolute value makes a mesh wound inwards solid inside all the same; +0 on the surface (d2 == 0); NaN where w
    is NaN or no face could claim the point (every face degenerate).  Arguments, checks and errors as winding_numbers."""
    p, vd, fd = _checked("signed_distances", points, vertices, faces)
    phi, face, close, w = _signed(p, vd, fd, want_face, want_closest, want_winding)
    got = (phi,) + ((face.long(),) if want_face else ()) + ((close,) if want_closest else ()) + ((w,) if want_winding else ())
    return got if len(got) > 1 else phi


def inside(points, vertices, faces):
    """bool [N]: |winding_numbers(points, vertices, faces)| > 0.5 - the rows of points inside the mesh, whichever way it is wound."""
    return _winding(*_checked("inside", points, vertices, faces)).abs() > 0.5


def box_lattice(who, lo, hi, resolution, bounds=None, margin=0.5):
    """The lattice SdfGrid.from_mesh and SceneVisualTool.object_field sample, by SceneVisualTool.background_field's rules:
    bounds = (min, max), by default the box (lo, hi) grown on every side by margin times its longest side; the voxel is the bounds'
    longest side / resolution and the other sides take as many voxels as cover them, at least 2 (proxy_mesh.TsdfVolume's count).
    Returns (origin float64 [3], voxel, (nz, ny, nx)).  ValueError for a resolution that is no integer >= 2, a margin that is not
    finite and >= 0, bounds that are not finite with max above min on every axis."""
    if isinstance(resolution, bool) or not isinstance(resolution, (int, np.integer)) or resolution < 2:
        raise ValueError("%s: resolution = %r; an integer >= 2, the voxels along the longest side" % (who, resolution))
    if bounds is None:
        if isinstance(margin, bool) or not isinstance(margin, (int, float, np.integer, np.floating)) or not 0.0 <= margin < float("inf"):
            raise ValueError("%s: margin = %r; a finite number >= 0" % (who, margin))
        lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
        grow = float(margin) * max(float((hi - lo).max()), 1e-6)
        bounds = (lo - grow, hi + grow)
    try:
        bmin, bmax = (np.asarray(host(b), np.float64).reshape(-1) for b in bounds)
    except (TypeError, ValueError):
        bmin = bmax = np.zeros(0)
    if bmin.shape != (3,) or bmax.shape != (3,) or not (np.isfinite(bmin).all() and np.isfinite(bmax).all() and (bmax > bmin).all()):
        raise ValueError("%s: bounds must be (min, max), three finite numbers each, max above min on every axis; got %r" % (who, bounds))
    voxel = float((bmax - bmin).max()) / int(resolution)
    n = np.maximum(np.ceil((bmax - bmin) / voxel - 1e-6).astype(np.int64), 2)
    return bmin, voxel, (int(n[2]), int(n[1]), int(n[0]))


def lattice_points(origin, voxel, shape, start, stop, device):
    """Samples [start, stop) of the lattice of grid_values, in its flat order, as float32 [stop - start, 3] on `device` - computed
    as grid_values' docstring says."""
    nz, ny, nx = shape
    i = torch.arange(start, stop, dtype=torch.int64, device=device)
    idx = torch.stack([i % nx, (i // nx) % ny, i // (nx * ny)], dim=1)
    o = torch.as_tensor(np.asarray(origin, np.float32), device=device)
    return (idx.to(torch.float32) + 0.5) * torch.as_tensor(np.float32(voxel), device=device) + o


def grid_values(vertices, faces, origin, voxel, shape, device="cuda", slab_points=None):
    """signed_distances on the lattice of a dynamics.SdfGrid: float32 [nz,ny,nx] on `device`, sample (ix, iy, iz) at
    origin + (i + 0.5) voxel.  The sample positions are computed in float32, each operation rounded on its own:
        x = fl(fl(fl(float32(ix) + 0.5f) * voxel) + origin_x)       (y and z likewise; origin and voxel rounded to float32 first)
    shape = (nz, ny, nx).  The lattice goes through the kernels in slabs of consecutive samples, so that the winding number's partial
    sums (8 bytes x samples x ceil(F / 1024)) stay below 256 MiB a slab; slab_points overrides the slab's size (a test forces one
    z-layer a slab).  The bits do not depend on the slabbing: every sample's value is signed_distances' at its position.
    The raw values are returned, not an SdfGrid, so that several obstacles, or an obstacle and another volume on the same lattice,
    can be combined with torch.minimum before SdfGrid(values, origin, voxel) prepares them.
    ValueError before anything is enqueued: a mesh mesh_bind.mesh_arrays refuses, an empty mesh, a shape that is not three positive
    integers or holds more than 2^28 samples, an origin that is not three finite numbers, a voxel that is not finite and positive
    (as the float32 they are used as), a slab_points below 1; GmeshError without a device.  No CPU path."""
    who = "grid_values"
    v, f = mesh_arrays(vertices, faces, who)
    if f.shape[0] == 0 or v.shape[0] == 0:
        raise ValueError("%s: the mesh is empty (%d vertices, %d faces)" % (who, v.shape[0], f.shape[0]))
    try:
        dims = tuple(shape)
    except TypeError:
        dims = ()
    if len(dims) != 3 or any(isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1 for n in dims):
        raise ValueError("%s: shape must be (nz, ny, nx), three positive integers; got %r" % (who, shape))
    nz, ny, nx = (int(n) for n in dims)
    if nx * ny * nz > 1 << 28:
        raise ValueError("%s: a lattice of %d x %d x %d samples (at most 2^28 in all)" % (who, nx, ny, nz))
    o = np.asarray(host(origin), np.float64).reshape(-1)
    if o.shape != (3,) or not np.isfinite(o.astype(np.float32)).all():
        raise ValueError("%s: origin must be three finite numbers; got %r" % (who, origin))
    if isinstance(voxel, bool) or not isinstance(voxel, (int, float, np.integer, np.floating)) or not np.isfinite(np.float32(voxel)) or not float(np.float32(voxel)) > 0.0:
        raise ValueError("%s: voxel = %r; finite and positive" % (who, voxel))
    if slab_points is not None and (isinstance(slab_points, bool) or not isinstance(slab_points, (int, np.integer)) or slab_points < 1):
        raise ValueError("%s: slab_points = %r; an integer >= 1" % (who, slab_points))
    dev = torch.device(device)
    need_cuda(dev, who, "a lattice")
    vd, fd = on_device(vertices, torch.float32, dev), on_device(faces, torch.int32, dev)
    total, chunks = nx * ny * nz, (fd.shape[0] + WN_CHUNK - 1) // WN_CHUNK
    slab = max(256, SLAB_PARTIAL_BYTES // (8 * chunks) // 256 * 256) if slab_points is None else int(slab_points)
    out = torch.empty((total,), dtype=torch.float32, device=vd.device)
    for s in range(0, total, slab):
        e = min(s + slab, total)
        out[s:e] = _signed(lattice_points(o, voxel, (nz, ny, nx), s, e, vd.device), vd, fd, False, False, False)[0]
    return out.reshape(nz, ny, nx)
