"""Bind plain points (a 3DGS cloud from any trainer) to a proxy mesh: closest face on the device (gm_closest_face), then the weights
the edit surface needs - the branch of SingleObjectDeform.load_mesh that runs when the Gaussian file carries no face ids
(edittool/__init__.py:68-85 of the reference, edittool.load_mesh here), with the search on the GPU instead of the host."""
import numpy as np
import torch

from . import _lib
from ._op import enqueue, f32, host, need_cuda, on_device, workspace
from .deform import barycentric_weights


def mesh_arrays(vertices, faces, who):
    """(vertices, faces) as host arrays, shapes and index range checked: the device cannot report an index outside [0, Vm)."""
    v, f = host(vertices), host(faces)
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("%s: vertices must be [Vm,3] and faces [F,3]; got %s and %s" % (who, tuple(v.shape), tuple(f.shape)))
    if f.dtype.kind not in "iu":
        raise ValueError("%s: faces must hold integer vertex ids, got %s" % (who, f.dtype))
    if f.shape[0] and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):
        raise ValueError("%s: face index outside [0, %d) (min %d, max %d)" % (who, v.shape[0], int(f.min()), int(f.max())))
    return v, f


def device_mesh(vertices, faces, who, dev, check_faces=True):
    """(vertices float32 [Vm,3], faces int32 [F,3]) on dev.  check_faces: shapes, dtype and the index range on the host
    (mesh_arrays - a host copy, so it waits for the stream); False: the shapes alone, for a caller that checked this face
    tensor before and must not wait (SingleObjectDeform.pick)."""
    if check_faces:
        mesh_arrays(vertices, faces, who)
    vd, fd = on_device(vertices, torch.float32, dev), on_device(faces, torch.int32, dev)
    if vd.dim() != 2 or vd.shape[1] != 3 or fd.dim() != 2 or fd.shape[1] != 3:
        raise ValueError("%s: vertices must be [Vm,3] and faces [F,3]; got %s and %s" % (who, tuple(vd.shape), tuple(fd.shape)))
    return vd, fd


def closest_faces(points, vertices, faces, want_closest=False):
    """For every row of points [N,3] the closest triangle of the mesh (vertices [Vm,3], faces [F,3] vertex ids):
    (d2 float32 [N], face int64 [N]) and with want_closest also the closest point on that face, float32 [N,3].
    gm_closest_face: Ericson's region test per (point, face) in float32 without contraction, the smallest squared distance wins,
    ties go to the lowest face index, a face whose formula gives NaN (no area) never wins - a float32 brute force gives the same
    bits.  A point for which every face gives NaN gets face -1 and d2 = +inf.  points on a HIP (cuda) device; vertices / faces
    may be host arrays or tensors on any device (the face indices are checked on the host).  No CPU path."""
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("closest_faces: points must be a [N,3] tensor; got %s" % (tuple(getattr(points, "shape", ())),))
    v, f = mesh_arrays(vertices, faces, "closest_faces")
    if points.shape[0] and (f.shape[0] == 0 or v.shape[0] == 0):
        raise ValueError("closest_faces: the mesh is empty (%d vertices, %d faces)" % (v.shape[0], f.shape[0]))
    need_cuda(points, "closest_faces", "the points")
    dev = points.device
    p = f32(points)
    vd, fd = on_device(vertices, torch.float32, dev), on_device(faces, torch.int32, dev)
    N, Vm, F = p.shape[0], vd.shape[0], fd.shape[0]
    d2 = torch.empty((N,), dtype=torch.float32, device=dev)
    face = torch.empty((N,), dtype=torch.int32, device=dev)
    close = torch.empty((N, 3), dtype=torch.float32, device=dev) if want_closest else None
    if N > 0:
        ws = workspace(dev, "gm_closest_face_workspace_bytes", N, F)
        enqueue(dev, "gm_closest_face", N, p, Vm, vd, F, fd, d2, face, close, workspace=ws)
    return (d2, face.long(), close) if want_closest else (d2, face.long())


def bind_points(points, vertices, faces, face_id=None):
    """The binding of plain points to a mesh, as the no-face-id branch of edittool.load_mesh computes it: per point the closest
    face (closest_faces, or face_id [N] when the caller has one: a cached binding, a test), the foot of the perpendicular from the
    point onto that face's plane (numpy float64: unit normal n, bias -a.n, distance = -(n.p + bias), intersection = p + distance n)
    and deform.barycentric_weights there.  The query point is the point itself - a plain file has no projected position.
    Returns dict(face_id int64 [N], tri int32 [N,3] the face's vertex ids, weights float32 [N,3], sqr_distance float32 [N] - the
    squared distance to the closest face; NaN rows when face_id was given).  Host arrays.  A point that no face can claim (every
    face without area) raises ValueError naming the first such row."""
    v, f = mesh_arrays(vertices, faces, "bind_points")
    pts = host(points)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("bind_points: points must be [N,3]; got %s" % (tuple(pts.shape),))
    N = pts.shape[0]
    if face_id is None:
        if not torch.is_tensor(points):
            raise _lib.GmeshError("bind_points needs the points as a tensor on a HIP (cuda) device for the search; there is no CPU path")
        d2, fid = closest_faces(points, vertices, faces)
        sqr, fid = d2.cpu().numpy(), fid.cpu().numpy()
        bad = np.nonzero(fid < 0)[0]
        if len(bad):
            raise ValueError("bind_points: point %d has no closest face (every face of the mesh is degenerate for it)" % int(bad[0]))
    else:
        fid = host(face_id).reshape(-1).astype(np.int64)
        if fid.shape[0] != N:
            raise ValueError("bind_points: face_id must have one entry per point (%d), got %d" % (N, fid.shape[0]))
        if N and (int(fid.min()) < 0 or int(fid.max()) >= f.shape[0]):
            raise ValueError("bind_points: face_id outside [0, %d)" % f.shape[0])
        sqr = np.full((N,), np.nan, np.float32)
    vertex = v.astype(np.float64)
    triangles = f.astype(np.int64)
    normals = np.cross(vertex[triangles[:, 1]] - vertex[triangles[:, 0]], vertex[triangles[:, 2]] - vertex[triangles[:, 0]])
    with np.errstate(divide="ignore", invalid="ignore"):
        normals /= np.linalg.norm(normals, axis=1)[:, None]
    bias = -(vertex[triangles[:, 0]] * normals).sum(axis=1)
    gpos = pts.astype(np.float64)
    n_g, b_g = normals[fid], bias[fid]
    distance = -((n_g * gpos).sum(axis=1) + b_g)
    intersection = gpos + distance[:, None] * n_g
    tri = triangles[fid]
    coord = barycentric_weights(intersection, vertex[tri[:, 0]], vertex[tri[:, 1]], vertex[tri[:, 2]])
    return dict(face_id=fid, tri=tri.astype(np.int32), weights=coord.astype(np.float32), sqr_distance=sqr.astype(np.float32))
