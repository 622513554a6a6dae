"""The mesh as the solvers see it: a rest mesh, its triangles and its cotangent edge graph, built once per mesh and handed to the
operators over it - arap.ArapSolver, arap.ArapEnergy, pose_interp.PoseInterpolator, dynamics.MeshDynamics - which add only what is
their own.  Also the one copy of the argument checks those operators share; each takes `who`, so a message begins with the public name
the user called.  mesh_region.SurfaceGraph holds a different graph (float32 lengths, unfolded edges) and stays its own class."""
from functools import cached_property

import numpy as np
import torch

from ._op import host, need_cuda, on_device


def edge_csr(vertices, faces):
    """The weighted edge graph of a triangle mesh as a symmetric CSR: (row_offsets int32 [Vm+1], cols int32 [nnz], weights float64
    [nnz]), columns ascending within each row, no diagonal.  Weights as mesh_rs_kernel forms them (gm_mesh.hip), in float64 from the
    float32 vertices: every face corner c opposite edge (a, b) adds max(0.5 cot(angle at c), 1e-3) to w_ab, cot = (u . w) / |u x w| with
    u = a - c, w = b - c; a face with |u x w| <= 1e-30 adds nothing (an edge that only such faces hold does not appear).  Every weight
    is positive.  Host, numpy only; once per mesh (MeshGraph), like deform.vertex_face_adjacency."""
    v = np.asarray(host(vertices), np.float32).astype(np.float64)
    f = np.asarray(host(faces)).astype(np.int64).reshape(-1, 3)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError("edge_csr: vertices must be [Vm,3]; got %s" % (tuple(v.shape),))
    Vm = v.shape[0]
    if f.shape[0] and (int(f.min()) < 0 or int(f.max()) >= Vm):
        raise ValueError("edge_csr: face index outside [0, %d)" % Vm)
    keys, vals = [], []
    for c in range(3):
        ia, ib, ic = f[:, (c + 1) % 3], f[:, (c + 2) % 3], f[:, c]
        u, w = v[ia] - v[ic], v[ib] - v[ic]
        area2 = np.linalg.norm(np.cross(u, w), axis=1)
        ok = (area2 > 1e-30) & (ia != ib)
        with np.errstate(divide="ignore", invalid="ignore"):
            wt = np.maximum(0.5 * (u * w).sum(axis=1) / area2, 1e-3)
        keys += [ia[ok] * Vm + ib[ok], ib[ok] * Vm + ia[ok]]
        vals += [wt[ok], wt[ok]]
    keys = np.concatenate(keys) if keys else np.zeros(0, np.int64)
    vals = np.concatenate(vals) if vals else np.zeros(0, np.float64)
    uniq, inv = np.unique(keys, return_inverse=True)                   # sorted: rows ascend, columns ascend within a row
    weights = np.bincount(inv.reshape(-1), weights=vals, minlength=len(uniq)).astype(np.float64)
    rows, cols = uniq // Vm, uniq % Vm
    offsets = np.zeros(Vm + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=Vm), out=offsets[1:])
    return offsets.astype(np.int32), cols.astype(np.int32), weights


def components(Vm, rows, cols):
    """Label of the connected component of every vertex (the smallest vertex id in it): min-label propagation with pointer jumping."""
    label = np.arange(Vm, dtype=np.int64)
    while True:
        new = label.copy()
        np.minimum.at(new, rows, label[cols])
        new = new[new]                                                 # a label is a vertex of the same component: jump to its label
        if np.array_equal(new, label):
            return label
        label = new


def vertex_ids(a, Vm, who, what, allow_empty=False, distinct=True):
    """`a` (a list, an array or a tensor) as int64 vertex ids of a mesh of Vm vertices; `what` names them in the message ("handle").
    ValueError for an empty set unless allow_empty, a dtype that is not integer, an id outside [0, Vm) and, with distinct, an id
    given twice."""
    h = np.asarray(host(a)).reshape(-1)
    if h.size == 0:
        if not allow_empty:
            raise ValueError("%s: the %s set is empty" % (who, what))
        return np.zeros(0, np.int64)
    if h.dtype.kind not in "iu":
        raise ValueError("%s: %s ids must be integer vertex ids, got %s" % (who, what, h.dtype))
    h = h.astype(np.int64)
    if int(h.min()) < 0 or int(h.max()) >= Vm:
        raise ValueError("%s: %s id outside [0, %d) (min %d, max %d)" % (who, what, Vm, int(h.min()), int(h.max())))
    if distinct and len(np.unique(h)) != len(h):
        raise ValueError("%s: a %s id is given twice" % (who, what))
    return h


class MeshGraph:
    """rest_vertices [Vm,3], faces [F,3] vertex ids.  On the host: Vm, F, rest_host float32 [Vm,3], faces_host int64 [F,3], csr = (off,
    cols, weights) of edge_csr, rows (the row of every entry of cols), edgeless bool [Vm] (the weights sum to 0: unreferenced, or every
    face at the vertex degenerate; the operators hold these rows) and, on first use, label (components) and vertex_face_adjacency.  On
    the device, uploaded on first use and then shared by every operator of this mesh - nothing writes them: rest float32, off / cols
    int32, w float64, faces int32, vf_off / vf_faces int32.  device="cpu" serves the host half only.
    ValueError, beginning with `who`, for rest_vertices that are not [Vm,3] with Vm > 0; edge_csr's for a face index outside the mesh."""

    def __init__(self, rest_vertices, faces, device="cuda", who="MeshGraph"):
        self.device = torch.device(device)
        v = np.ascontiguousarray(np.asarray(host(rest_vertices), np.float32))
        if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] == 0:
            raise ValueError("%s: rest_vertices must be [Vm,3] with Vm > 0; got %s" % (who, tuple(v.shape)))
        self.rest_host = v
        self.faces_host = np.ascontiguousarray(np.asarray(host(faces)).astype(np.int64).reshape(-1, 3))
        self.Vm, self.F = v.shape[0], self.faces_host.shape[0]
        self.csr = edge_csr(v, self.faces_host)
        off, _, weights = self.csr
        self.rows = np.repeat(np.arange(self.Vm, dtype=np.int64), np.diff(off.astype(np.int64)))
        self.edgeless = np.bincount(self.rows, weights=weights, minlength=self.Vm) <= 0.0

    @classmethod
    def of(cls, x, faces, device="cuda", who="MeshGraph"):
        """x itself when it is a MeshGraph (faces must then be None; its device holds), else MeshGraph(x, faces, device, who)"""
        if not isinstance(x, cls):
            return cls(x, faces, device, who)
        if faces is not None:
            raise ValueError("%s: a MeshGraph carries its faces; pass faces=None with it" % who)
        return x

    @cached_property
    def label(self):
        return components(self.Vm, self.rows, self.csr[1].astype(np.int64))

    @cached_property
    def vertex_face_adjacency(self):
        from .deform import vertex_face_adjacency
        return vertex_face_adjacency(self.faces_host, self.Vm)

    @cached_property
    def device_csr(self):
        """(rest, off, cols, w) on the device"""
        off, cols, weights = self.csr
        if len(cols) == 0:                                             # a mesh without an edge: no row reads them, but the entry points want pointers
            cols, weights = np.zeros(1, np.int32), np.zeros(1, np.float64)
        return tuple(on_device(a, dt, self.device) for a, dt in ((self.rest_host, torch.float32), (off, torch.int32), (cols, torch.int32),
                                                                 (weights, torch.float64)))

    rest, off, cols, w = (property(lambda self, k=k: self.device_csr[k]) for k in range(4))

    @cached_property
    def device_faces(self):
        """(faces, vf_off, vf_faces) on the device"""
        return tuple(on_device(a, torch.int32, self.device) for a in (self.faces_host,) + self.vertex_face_adjacency)

    faces, vf_off, vf_faces = (property(lambda self, k=k: self.device_faces[k]) for k in range(3))

    def need_device(self, who):
        """GmeshError unless this graph lives on a HIP (cuda) device"""
        need_cuda(self.device, who, "the mesh")

    def vertex_ids(self, a, who, what, allow_empty=False, distinct=True):
        return vertex_ids(a, self.Vm, who, what, allow_empty, distinct)

    def require_anchored(self, held, ids, who, what):
        """ValueError if a vertex that `held` (bool [Vm]) leaves free lies in a connected component with none of `ids` in it"""
        has = np.zeros(self.Vm, bool)
        has[self.label[ids]] = True
        loose = np.nonzero(~held & ~has[self.label])[0]
        if len(loose):
            raise ValueError("%s: vertex %d lies in a connected component without %s %s (%d such vertices): the system is singular"
                             % (who, int(loose[0]), "an" if what[0] in "aeiou" else "a", what, len(loose)))

    def rows_f32(self, a, who, name, copy=False):
        """a floating-point [Vm,3] tensor (or host array) as contiguous float32 on the device; copy: never `a`'s own memory"""
        if not torch.is_tensor(a):
            a = torch.as_tensor(np.asarray(a), dtype=torch.float32)
        if a.shape != (self.Vm, 3) or not a.dtype.is_floating_point:
            raise ValueError("%s: %s must be a floating-point [%d,3] tensor; got %s %s" % (who, name, self.Vm, a.dtype, tuple(a.shape)))
        a = a.detach().to(device=self.rest.device, dtype=torch.float32)
        return a.clone(memory_format=torch.contiguous_format) if copy else a.contiguous()

    def out_f32(self, out, shape, who):
        """`out` if it is a contiguous float32 tensor of `shape` on the device (ValueError if not); None: a new one"""
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=self.rest.device)
        if not torch.is_tensor(out) or tuple(out.shape) != tuple(shape) or out.dtype is not torch.float32 or not out.is_contiguous() \
                or out.device != self.rest.device:
            raise ValueError("%s: out must be a contiguous float32 %s tensor on the mesh's device" % (who, list(shape)))
        return out
