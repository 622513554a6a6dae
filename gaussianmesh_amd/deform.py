"""Mesh-driven deformation of bound Gaussians (edit tool), tensor-in form.

Mirrors edittool/__init__.py of the reference:
  SingleObjectDeform (:40-131): attribute names gaussian_pos, gaussian_cov, gaussian_o, gaussian_feature,
  gaussian_deform_pos / gaussian_deform_cov / gaussian_deform_rot, gaussian_triangles, weight_g_pos, vertex.
  deform_gaussian(deform_mesh_path) of the reference reads an OBJ and calls pyACAP.GetRS; pyACAP is an external
  binary that is not in the reference tree, so here the per-vertex (R, S) are an explicit input:
      obj.deform(V1, R, S)   # V1 [Vm,3] deformed vertices, R/S [Vm,3,3]
The arithmetic (gather, barycentric blend, RS cov RS^T, x + dx) runs in one HIP kernel (csrc/gm_deform.hip).
"""
import torch

from . import _lib
from ._op import enqueue, need_cuda, workspace


def _f(t):
    if t.dtype is torch.float32 and t.is_contiguous():
        return t
    return t.detach().contiguous().float()


def barycentric_weights(points, p1, p2, p3):
    """Host-side (numpy, float64) barycentric weights from sub-triangle areas, as the reference computes them once
    per object when a mesh is attached (edittool/general_utils.py:73-88 get_barycentric_coordinate)."""
    import numpy as np
    e1, e2, e3 = points - p1, points - p2, points - p3
    s1 = np.linalg.norm(np.cross(e2, e3), axis=1)
    s2 = np.linalg.norm(np.cross(e1, e3), axis=1)
    s3 = np.linalg.norm(np.cross(e1, e2), axis=1)
    s = s1 + s2 + s3
    return np.stack([s1 / s, s2 / s, s3 / s], axis=1)


def deform_tensors(tri, w, dV, Rv, Sv, cov, pos):
    """gm_deform: returns (pos' [N,3], cov' [N,3,3], rot [N,3,3], cov6 [N,6])."""
    device = pos.device
    need_cuda(device, "deform", "tensors")
    tri = tri.detach().contiguous().to(torch.int32)
    w, dV, Rv, Sv, cov, pos = (_f(t) for t in (w, dV, Rv, Sv, cov, pos))
    N = pos.shape[0]
    f = dict(dtype=torch.float32, device=device)
    pos_o = torch.empty((N, 3), **f); cov_o = torch.empty((N, 3, 3), **f); rot_o = torch.empty((N, 3, 3), **f)
    cov6 = torch.empty((N, 6), **f)
    enqueue(device, "gm_deform", N, tri, w, dV, Rv, Sv, cov, pos, pos_o, cov_o, rot_o, cov6)
    return pos_o, cov_o, rot_o, cov6


def sh_colors(pos, campos, shs, rot=None, deg=3):
    """gm_sh_colors: max(SH_deg(rot^T normalize(pos - campos)) + 0.5, 0)  (edittool/__init__.py:442-448)."""
    device = pos.device
    pos, campos, shs = _f(pos), _f(campos), _f(shs)
    rot = None if rot is None else _f(rot)
    N, M = shs.shape[0], shs.shape[1]
    rgb = torch.empty((N, 3), dtype=torch.float32, device=device)
    enqueue(device, "gm_sh_colors", N, int(deg), M, pos, campos, rot, shs, rgb)
    return rgb


def deform_shade(tri, w, dV, Rv, Sv, cov, pos, shs, campos, deg=3, want_cov_rot=False):
    """gm_deform_shade: fused deform + rotated-direction SH colour.  Returns (pos' [N,3], cov6 [N,6], rgb [N,3]) and, with
    want_cov_rot, also (cov' [N,3,3], rot [N,3,3])."""
    device = pos.device
    need_cuda(device, "deform_shade", "tensors")
    tri = tri.detach().contiguous().to(torch.int32)
    w, dV, Rv, Sv, cov, pos, shs, campos = (_f(t) for t in (w, dV, Rv, Sv, cov, pos, shs, campos))
    N, M = pos.shape[0], shs.shape[1]
    f = dict(dtype=torch.float32, device=device)
    pos_o = torch.empty((N, 3), **f); cov6 = torch.empty((N, 6), **f); rgb = torch.empty((N, 3), **f)
    cov_o = torch.empty((N, 3, 3), **f) if want_cov_rot else None
    rot_o = torch.empty((N, 3, 3), **f) if want_cov_rot else None
    enqueue(device, "gm_deform_shade", N, int(deg), M, tri, w, dV, Rv, Sv, cov, pos, shs, campos, pos_o, cov6, rgb, cov_o, rot_o)
    return (pos_o, cov6, rgb, cov_o, rot_o) if want_cov_rot else (pos_o, cov6, rgb)


class DeformBinding:
    """What ties a cloud to its proxy mesh, as the differentiable pass needs it: tri int32 [N,3], w float32 [N,3], Vm, and the vertex ->
    (row, corner) incidence list in CSR form that gm_deform_shade_bwd sums over - inc_offsets int32 [Vm+1], inc_entries int32 [3N] with
    entry 3 * row + corner, ascending within a vertex.  Built once, on the device: a stable sort of tri.reshape(-1), a bincount and its
    cumsum.  The vertex ids are checked against Vm here (one host wait per binding), since the kernels index the tables with them."""

    def __init__(self, tri, w, Vm):
        need_cuda(tri, "DeformBinding", "tensors")
        self.tri = tri.detach().contiguous().to(torch.int32)
        self.w = _f(w)
        self.Vm = int(Vm)
        N = self.tri.shape[0]
        if self.tri.shape != (N, 3) or self.w.shape != (N, 3):
            raise ValueError("DeformBinding: tri and w must be [N,3]; got %s and %s" % (tuple(self.tri.shape), tuple(self.w.shape)))
        if 3 * N >= 2 ** 31:
            raise ValueError("DeformBinding: 3 N = %d entries do not fit an int32" % (3 * N))
        flat = self.tri.reshape(-1).to(torch.int64)
        if N and (self.Vm < 1 or int(flat.min()) < 0 or int(flat.max()) >= self.Vm):
            raise ValueError("DeformBinding: vertex ids outside 0..%d" % (self.Vm - 1))
        self.inc_entries = torch.sort(flat, stable=True)[1].to(torch.int32)
        off = torch.zeros(self.Vm + 1, dtype=torch.int64, device=self.tri.device)
        if N:
            off[1:] = torch.cumsum(torch.bincount(flat, minlength=self.Vm), 0)
        self.inc_offsets = off.to(torch.int32)


class _DeformShade(torch.autograd.Function):
    """forward: gm_deform_shade; backward: one gm_deform_shade_bwd"""

    @staticmethod
    def forward(ctx, binding, deg, dV, Rv, Sv, cov, pos, shs, campos):
        device = pos.device
        args = tuple(_f(t) for t in (dV, Rv, Sv, cov, pos, shs, campos))
        dV_, Rv_, Sv_, cov_, pos_, shs_, campos_ = args
        N, M = pos_.shape[0], shs_.shape[1]
        f = dict(dtype=torch.float32, device=device)
        pos_o = torch.empty((N, 3), **f); cov6 = torch.empty((N, 6), **f); rgb = torch.empty((N, 3), **f)
        # (rows of M != 16 coefficients take gm_deform_shade's unfused route, which needs the two [N,3,3] intermediates)
        cov_o = torch.empty((N, 3, 3), **f) if M != 16 else None
        rot_o = torch.empty((N, 3, 3), **f) if M != 16 else None
        enqueue(device, "gm_deform_shade", N, int(deg), M, binding.tri, binding.w, dV_, Rv_, Sv_, cov_, pos_, shs_, campos_, pos_o, cov6, rgb,
                cov_o, rot_o)
        ctx.binding, ctx.deg, ctx.shapes = binding, int(deg), (dV.shape, Rv.shape, Sv.shape, cov.shape, pos.shape, shs.shape)
        ctx.save_for_backward(*args)
        ctx.set_materialize_grads(False)                         # an output nobody used arrives as None and goes to the call as NULL
        return pos_o, cov6, rgb

    @staticmethod
    def backward(ctx, g_pos, g_cov6, g_rgb):
        dV, Rv, Sv, cov, pos, shs, campos = ctx.saved_tensors
        b, device = ctx.binding, pos.device
        N, M, Vm = pos.shape[0], shs.shape[1], b.Vm
        f = dict(dtype=torch.float32, device=device)
        need = ctx.needs_input_grad                              # (binding, deg, dV, Rv, Sv, cov, pos, shs, campos)
        g_pos = torch.zeros((N, 3), **f) if g_pos is None else _f(g_pos)
        g_cov6 = None if g_cov6 is None else _f(g_cov6)
        g_rgb = None if g_rgb is None else _f(g_rgb)
        g_dV = torch.empty((Vm, 3), **f); g_Rv = torch.empty((Vm, 9), **f); g_Sv = torch.empty((Vm, 9), **f)
        g_cov = torch.empty((N, 9), **f) if need[5] else None
        g_rest = torch.empty((N, 3), **f) if need[6] else None
        no_upstream = g_cov6 is None and g_rgb is None           # (the rows' gradient is then zero, and the call refuses to be asked for it)
        g_shs = None
        if need[7]:
            g_shs = torch.zeros((N, M, 3), **f) if no_upstream else torch.empty((N, M, 3), **f)
        ws = workspace(device, "gm_deform_shade_bwd_workspace_bytes", N, Vm)
        enqueue(device, "gm_deform_shade_bwd", N, ctx.deg, M, Vm, b.tri, b.w, dV, Rv, Sv, cov, pos, shs, campos, b.inc_offsets, b.inc_entries,
                g_pos, g_cov6, g_rgb, g_dV, g_Rv, g_Sv, None if no_upstream else g_shs, g_cov, g_rest, workspace=ws)
        s = ctx.shapes
        out = (g_dV.reshape(s[0]), g_Rv.reshape(s[1]), g_Sv.reshape(s[2]), None if g_cov is None else g_cov.reshape(s[3]),
               None if g_rest is None else g_rest.reshape(s[4]), None if g_shs is None else g_shs.reshape(s[5]))
        return (None, None) + tuple(g if n else None for g, n in zip(out, need[2:8])) + (None,)


def deform_shade_differentiable(binding, dV, Rv, Sv, cov, pos, shs, campos, deg=3):
    """deform_shade with a backward: (pos' [N,3], cov6 [N,6], rgb [N,3]), bit for bit deform_shade's, as an autograd Function whose
    backward is one gm_deform_shade_bwd (csrc/gm_deform_bwd.hip).  binding: a DeformBinding (its tri and w carry no gradient, nor does
    campos).  Gradients flow to dV [Vm,3], Rv / Sv [Vm,3,3] or [Vm,9], and - where the tensor requires grad - to cov, pos and shs; None
    comes back for the rest.  The vertex sums are deterministic: the same inputs give the same bits."""
    need_cuda(pos.device, "deform_shade_differentiable", "tensors")
    if not isinstance(binding, DeformBinding):
        raise TypeError("deform_shade_differentiable: binding must be a DeformBinding")
    if dV.shape[0] != binding.Vm or Rv.numel() != 9 * binding.Vm or Sv.numel() != 9 * binding.Vm or pos.shape[0] != binding.tri.shape[0]:
        raise ValueError("deform_shade_differentiable: tables of %d vertices and %d rows expected" % (binding.Vm, binding.tri.shape[0]))
    return _DeformShade.apply(binding, int(deg), dV, Rv, Sv, cov, pos, shs, campos)


def pack_cov6(cov):
    """Rest covariances [N,3,3] (or [N,9]) -> [N,6] rows xx xy xz yy yz zz for forward_deformed_begin (GM_STREAM_COV6), or None when
    some matrix is not symmetric BIT FOR BIT: the fused pass reads the mirrored entries from the six, which reproduces the [N,9] call
    exactly only then (the reference multiplies with the full matrix, edittool/__init__.py:300-340)."""
    c = cov.detach().reshape(-1, 3, 3)
    if not (torch.equal(c[:, 0, 1], c[:, 1, 0]) and torch.equal(c[:, 0, 2], c[:, 2, 0]) and torch.equal(c[:, 1, 2], c[:, 2, 1])):
        return None
    return torch.stack((c[:, 0, 0], c[:, 0, 1], c[:, 0, 2], c[:, 1, 1], c[:, 1, 2], c[:, 2, 2]), dim=1).to(torch.float32).contiguous()


def pack_mesh_state(state, verts, out=None):
    """gm_pack_mesh_state: [Vm,21] frame state (V1 | R | S) and rest pose verts [Vm,3] -> gather table [Vm,24]."""
    device = state.device
    need_cuda(device, "pack_mesh_state", "tensors")
    state, verts = _f(state), _f(verts)
    Vm = state.shape[0]
    if state.shape[1] != 21 or verts.shape != (Vm, 3):
        raise ValueError("pack_mesh_state: state must be [Vm,21] and verts [Vm,3]")
    packed = out if out is not None else torch.empty((Vm, 24), dtype=torch.float32, device=device)
    enqueue(device, "gm_pack_mesh_state", Vm, state, verts, packed)
    return packed


def deform_shade_packed(tri, w, packed, cov, pos, shs, campos, deg=3, want_cov_rot=False):
    """gm_deform_shade_packed: deform_shade with the per-vertex (dV, R, S) read from pack_mesh_state()'s table."""
    device = pos.device
    need_cuda(device, "deform_shade", "tensors")
    tri = tri.detach().contiguous().to(torch.int32)
    w, packed, cov, pos, shs, campos = (_f(t) for t in (w, packed, cov, pos, shs, campos))
    N, M = pos.shape[0], shs.shape[1]
    f = dict(dtype=torch.float32, device=device)
    pos_o = torch.empty((N, 3), **f); cov6 = torch.empty((N, 6), **f); rgb = torch.empty((N, 3), **f)
    cov_o = torch.empty((N, 3, 3), **f) if want_cov_rot else None
    rot_o = torch.empty((N, 3, 3), **f) if want_cov_rot else None
    enqueue(device, "gm_deform_shade_packed", N, int(deg), M, tri, w, packed, cov, pos, shs, campos, pos_o, cov6, rgb, cov_o, rot_o)
    return (pos_o, cov6, rgb, cov_o, rot_o) if want_cov_rot else (pos_o, cov6, rgb)


def cov_to_scale_rot(cov):
    """gm_cov_to_scale_rot: (scales [N,3], rotations [N,4]) whose covariance R diag(s^2) R^T equals cov [N,3,3]
    (the SceneVisualTool route: edittool/__init__.py:204-207, rasterised with scales/rotations instead of cov3D_precomp)."""
    device = cov.device
    need_cuda(device, "cov_to_scale_rot", "a tensor")
    cov = _f(cov)
    N = cov.shape[0]
    scales = torch.empty((N, 3), dtype=torch.float32, device=device)
    rots = torch.empty((N, 4), dtype=torch.float32, device=device)
    enqueue(device, "gm_cov_to_scale_rot", N, cov, scales, rots)
    return scales, rots


def rotate_sh(shs, rot, deg=3, out=None):
    """gm_sh_rotate: the SH rows [N,M,3] re-expressed in the unrotated frame - row i becomes the c' with
    SH_deg(d) . c' == SH_deg(rot_i^T d) . c_i for every unit d, so that sh_colors(pos, campos, rotate_sh(shs, rot), rot=None) is
    sh_colors(pos, campos, shs, rot=rot) up to float32 rounding (exact for any 3x3 rot [N,3,3], e.g. deform_tensors' rot_out).
    Coefficients k >= (deg+1)^2 are copied.  out: the result's tensor ([N,M,3] float32, contiguous; may be shs itself: in place)."""
    device = shs.device
    need_cuda(device, "rotate_sh", "tensors")
    shs, rot = _f(shs), _f(rot)
    if shs.dim() != 3 or shs.shape[2] != 3:
        raise ValueError("rotate_sh: shs must be [N,M,3]")
    N, M = shs.shape[0], shs.shape[1]
    if rot.numel() != 9 * N:
        raise ValueError("rotate_sh: rot must be [%d,3,3]" % N)
    if out is None:
        out = torch.empty_like(shs)
    elif out.dtype is not torch.float32 or not out.is_contiguous() or out.shape != shs.shape or out.device != device:
        raise ValueError("rotate_sh: out must be a contiguous float32 tensor of shs' shape on its device")
    enqueue(device, "gm_sh_rotate", N, int(deg), M, shs, rot, out)
    return out


def vertex_face_adjacency(faces, Vm):
    """CSR list of the faces incident to each vertex: (offsets int32 [Vm+1], face ids int32 [3F]), host side, once per mesh."""
    import numpy as np
    f = np.asarray(faces.detach().cpu() if hasattr(faces, "detach") else faces, dtype=np.int64).reshape(-1, 3)
    vid = f.reshape(-1)
    fid = np.repeat(np.arange(f.shape[0], dtype=np.int64), 3)
    order = np.argsort(vid, kind="stable")
    counts = np.bincount(vid, minlength=Vm)
    offsets = np.zeros(Vm + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    return offsets.astype(np.int32), fid[order].astype(np.int32)


def mesh_rs_packed(rest_vertices, deformed_vertices, faces, adjacency, out=None):
    """gm_mesh_rs_packed: the per-vertex gather table [Vm,24] of the fused deformation kernels, straight from the deformed
    mesh (= pack_mesh_state(mesh_rs(..., want_state=True)[2], rest_vertices), bit for bit, in one launch)."""
    device = rest_vertices.device
    need_cuda(device, "mesh_rs_packed", "tensors")
    V0, V1 = _f(rest_vertices), _f(deformed_vertices)
    Vm = V0.shape[0]
    if faces.dtype is not torch.int32 or not faces.is_contiguous():
        faces = faces.detach().contiguous().to(torch.int32)
    off, adj = adjacency
    packed = out if out is not None else torch.empty((Vm, 24), dtype=torch.float32, device=device)
    enqueue(device, "gm_mesh_rs_packed", Vm, faces.shape[0], V0, V1, faces, off, adj, packed)
    return packed


def mesh_rs_packed_batch(rest_vertices, deformed_vertices_list, faces, adjacency, out=None):
    """gm_mesh_rs_packed_batch: the gather tables of up to GM_BATCH_MAX deformed meshes in ONE launch (the frames of a
    rasterizer.forward_deformed_batch); deformed_vertices_list: K tensors [Vm,3]; out: optional [K,Vm,24] tensor, or a list of K
    contiguous [Vm,24] tensors (e.g. one object's rows of combined tables).  Returns the K tables (views of one [K,Vm,24] tensor, or
    the list), each bit for bit what mesh_rs_packed makes of its mesh."""
    device = rest_vertices.device
    need_cuda(device, "mesh_rs_packed_batch", "tensors")
    K = len(deformed_vertices_list)
    if not 1 <= K <= _lib.GM_BATCH_MAX:
        raise ValueError("mesh_rs_packed_batch: 1..%d frames" % _lib.GM_BATCH_MAX)
    V0 = _f(rest_vertices)
    V1 = [_f(v) for v in deformed_vertices_list]
    Vm = V0.shape[0]
    if faces.dtype is not torch.int32 or not faces.is_contiguous():
        faces = faces.detach().contiguous().to(torch.int32)
    off, adj = adjacency
    packed = out if out is not None else torch.empty((K, Vm, 24), dtype=torch.float32, device=device)
    if isinstance(packed, (list, tuple)) and (len(packed) != K or any(t.shape != (Vm, 24) or not t.is_contiguous() for t in packed)):
        raise ValueError("mesh_rs_packed_batch: out must hold K contiguous [Vm,24] tables")
    import ctypes as C
    pv = (C.c_void_p * K)(*[v.data_ptr() for v in V1])
    pp = (C.c_void_p * K)(*[packed[k].data_ptr() for k in range(K)])
    enqueue(device, "gm_mesh_rs_packed_batch", K, Vm, faces.shape[0], V0, pv, faces, off, adj, pp)
    return [packed[k] for k in range(K)]


def rest_mesh_state(vertex):
    """The [Vm,21] frame state (V1 | R | S) of a mesh at rest: its own vertices, R = S = identity (pack_mesh_state's input)."""
    Vm = vertex.shape[0]
    eye = torch.eye(3, dtype=torch.float32, device=vertex.device).reshape(1, 9).expand(Vm, 9)
    return torch.cat([_f(vertex), eye, eye], dim=1)


def plan_sequence(sizes, frames_per_launch=4, emission_policy=None, batchable=True):
    """Route of an edit sequence (edittool.ObjectVisualTool.render_sequence), host only: sizes = the frames' (W, H) in order.  Returns
    [(kind, [frame indices])] in frame order:
      "learn"  - the first frame of a resolution: forward_deformed_begin(...).finish(), which teaches the workspaces their capacity;
      "batch"  - up to frames_per_launch consecutive frames of one resolution: rasterizer.forward_deformed_batch (a change of
                 resolution ends a batch);
      "single" - a frame whose resolution the batch refuses (more than 2048 list tiles under its emission policy, or batchable False,
                 e.g. an empty cloud): the single-frame path, forward_deformed_begin / finish."""
    from .rasterizer import emission_policy_of
    K = int(frames_per_launch)
    if not 1 <= K <= _lib.GM_BATCH_MAX:
        raise ValueError("frames_per_launch: 1..%d, got %r" % (_lib.GM_BATCH_MAX, frames_per_launch))
    plan, learned, run, run_size = [], set(), [], None

    def fits(W, H):                                        # gm_forward_deformed_batch_async: the one-pass tile sort (TileGrid in gm_common.h)
        s = max(emission_policy_of(emission_policy, W, H) - 1, 0)
        gx, gy = (W + 15) // 16, (H + 15) // 16
        return ((gx + (1 << s) - 1) >> s) * ((gy + (1 << s) - 1) >> s) <= 2048

    for i, (W, H) in enumerate(sizes):
        size = (int(W), int(H))
        if run and (size != run_size or len(run) == K):
            plan.append(("batch", run)); run = []
        if not batchable or not fits(*size):
            plan.append(("single", [i]))
        elif size not in learned:
            learned.add(size)
            plan.append(("learn", [i]))
        else:
            run.append(i); run_size = size
    if run:
        plan.append(("batch", run))
    return plan


def mesh_rs(rest_vertices, deformed_vertices, faces, adjacency=None, want_state=False):
    """gm_mesh_rs: per-vertex (R, S) [Vm,3,3] of a deformed proxy mesh, the pair pyACAP.GetRS hands to
    SingleObjectDeform.deform_gaussian (edittool/__init__.py:109-113): cotangent-weighted one-ring least-squares
    deformation gradient per vertex (ACAP / ARAP), polar decomposition; R in pyACAP's row-vector convention (the transpose
    of the rotation).
    adjacency: (offsets, face ids) device int32 tensors from vertex_face_adjacency (built here when None).
    want_state: also return the frame record [Vm,21] = V1 | R | S that pack_mesh_state consumes."""
    device = rest_vertices.device
    need_cuda(device, "mesh_rs", "tensors")
    V0, V1 = _f(rest_vertices), _f(deformed_vertices)
    Vm = V0.shape[0]
    faces = faces.detach().contiguous().to(torch.int32)
    if adjacency is None:
        off, adj = vertex_face_adjacency(faces, Vm)
        adjacency = (torch.tensor(off, device=device), torch.tensor(adj, device=device))
    off, adj = adjacency
    R = torch.empty((Vm, 3, 3), dtype=torch.float32, device=device)
    S = torch.empty((Vm, 3, 3), dtype=torch.float32, device=device)
    state = torch.empty((Vm, 21), dtype=torch.float32, device=device) if want_state else None
    enqueue(device, "gm_mesh_rs", Vm, faces.shape[0], V0, V1, faces, off, adj, R, S, state)
    return (R, S, state) if want_state else (R, S)


class SingleObjectDeform:
    """Tensor-in counterpart of edittool.SingleObjectDeform.

    gaussian_pos [N,3], gaussian_cov [N,3,3], gaussian_o [N,1], gaussian_feature [N,16,3],
    gaussian_triangles int [N,3] (vertex ids of the bound face), weights [N,3] (barycentric, from
    get_barycentric_coordinate), vertex [Vm,3] rest vertices."""

    def __init__(self, gaussian_pos, gaussian_cov, gaussian_o, gaussian_feature, gaussian_triangles, weights, vertex,
                 name=None):
        self.name = name
        self.gaussian_pos = _f(gaussian_pos)
        self.gaussian_cov = _f(gaussian_cov)
        self.gaussian_o = _f(gaussian_o)
        self.gaussian_feature = _f(gaussian_feature)
        self.gaussian_triangles = gaussian_triangles.detach().contiguous().to(torch.int32)
        self.coord = _f(weights)
        self.weight_g_pos = self.coord.unsqueeze(2)
        self.weight_g_rs = self.coord.unsqueeze(2).unsqueeze(3)
        self.vertex = _f(vertex)
        self.number_gaussian = self.gaussian_pos.shape[0]
        self.gaussian_deform_pos = self.gaussian_pos
        self.gaussian_deform_cov = self.gaussian_cov
        self.gaussian_deform_rot = torch.eye(3, device=self.gaussian_pos.device).expand(self.number_gaussian, 3, 3).contiguous()
        self.gaussian_deform_cov6 = None
        self.deform_state = None         # (V1, R, S) of the last deform(); None: the rest pose (edittool render_sequence renders it)
        self.arap = None                 # the ArapSolver of set_handles()
        self.region = None               # set_region_handles(): (picked vertex ids int64 [H], owner int64 [n]) on the device
        self._operators, self._operator_keys = {}, {}    # _operator(): name -> kept operator, name -> (face tensor, key) it was built for

    def get_name(self):
        return self.name

    @property
    def mesh_vertex_current(self):
        """The proxy mesh's vertices as last deformed ([Vm,3], the V1 of deform_state); None: the rest pose.  drag() starts from them."""
        return None if self.deform_state is None else self.deform_state[0]

    @property
    def binding(self):
        """The DeformBinding of this object's cloud (deform_shade_differentiable's first argument), built the first time it is asked for."""
        if getattr(self, "_binding", None) is None:
            self._binding = DeformBinding(self.gaussian_triangles, self.coord, self.vertex.shape[0])
        return self._binding

    def fit_pose(self, views, iterations, faces=None, background=None, **fitter_options):
        """Fit the proxy mesh's pose to images: pose_fit.PoseFitter(self, faces, **fitter_options).fit(views, iterations, background) -
        views a list of (camera, target [3,H,W]) pairs; fitter_options: PoseFitter's lr, rigidity, deg, lambda_dssim, regularizer,
        smooth_sweeps, smooth_lambda.  Leaves the object deformed to the fitted pose (deform_state) and returns the
        fitter (its .losses, its .pose)."""
        from .pose_fit import PoseFitter
        fitter = PoseFitter(self, self._need_faces("fit_pose", faces), **fitter_options)
        fitter.fit(views, iterations, background=background)
        return fitter

    def _set_faces(self, faces):
        self.faces = torch.as_tensor(faces).detach().to(device=self.vertex.device, dtype=torch.int32).contiguous()
        off, adj = vertex_face_adjacency(self.faces, self.vertex.shape[0])
        self._adjacency = (torch.tensor(off, device=self.vertex.device), torch.tensor(adj, device=self.vertex.device))

    def _need_faces(self, who, faces=None):
        """the face tensor, after _set_faces(faces) where faces are given; ValueError where the object has none"""
        if faces is not None:
            self._set_faces(faces)
        if getattr(self, "faces", None) is None:
            raise ValueError("%s: this object has no faces; pass faces=[F,3] here or to set_handles" % who)
        return self.faces

    def _operator(self, name, key, make):
        """The kept operator `name` (_operators[name]); make() builds it anew when `key` or the face tensor is not what it was built for."""
        if name not in self._operators or self._operator_keys[name][0] is not self.faces or self._operator_keys[name][1] != key:
            self._operators[name], self._operator_keys[name] = make(), (self.faces, key)
        return self._operators[name]

    @property
    def mesh_graph(self):
        """The mesh_graph.MeshGraph of the rest mesh, which every operator of this object shares (ArapSolver, PoseInterpolator,
        MeshDynamics, PoseFitter's ArapEnergy): built the first time it is asked for and again when the face tensor changes."""
        from .mesh_graph import MeshGraph
        return self._operator("mesh_graph", None, lambda: MeshGraph(self.vertex, self._need_faces("mesh_graph"), device=self.vertex.device))

    def set_handles(self, vertex_ids, faces=None):
        """Choose the handle vertices of drag(): builds the arap.ArapSolver of this object's rest mesh (its refusals apply).  faces
        [F,3]: the proxy mesh's triangles, for an object built from tensors alone (the file-based object has them)."""
        from .arap import ArapSolver
        self._need_faces("set_handles", faces)
        self.arap = ArapSolver(self.mesh_graph, None, vertex_ids)
        self.region = None
        return self.arap

    def surface_distances(self, vertex_sets, max_distance=None):
        """Distances along the REST mesh (where picks are resolved and ARAP's energy lives) from each of vertex_sets, a list of id
        lists: float32 [B,Vm] on the device, +inf beyond max_distance (mesh_region.SurfaceGraph.distances; one 4-byte read-back per
        64 sweeps).  The graph is built on the host the first time this face tensor is seen and kept."""
        from .mesh_region import SurfaceGraph
        faces = self._need_faces("surface_distances")
        graph = self._operator("surface_graph", None, lambda: SurfaceGraph(self.vertex, faces, device=self.vertex.device))
        return graph.distances(vertex_sets, max_distance=max_distance)

    def set_region_handles(self, handle_vertices, grab_radius, free_radius=None, anchor_vertices=(), faces=None):
        """Choose drag_region()'s handles as surface regions around picked vertices: every vertex within grab_radius (along the rest
        mesh, surface_distances) of handle_vertices[i] moves with pick i; every vertex within grab_radius of an anchor vertex and, with
        free_radius, every vertex farther than free_radius from all picks is held at rest; the others bend
        (mesh_region.region_handles: its order, its refusals).  Distances are computed up to free_radius (grab_radius without it).
        Builds the ArapSolver through set_handles (faces: as there) and returns it; the region ids are arap.handles."""
        from .mesh_region import check_radii, region_handles
        import numpy as np
        grab, free = check_radii("set_region_handles", grab_radius, free_radius)
        hv = np.asarray(handle_vertices.detach().cpu() if torch.is_tensor(handle_vertices) else handle_vertices).reshape(-1)
        av = np.asarray(anchor_vertices.detach().cpu() if torch.is_tensor(anchor_vertices) else anchor_vertices).reshape(-1)
        if hv.size == 0:
            raise ValueError("set_region_handles: the handle set is empty")
        if faces is not None:
            self._set_faces(faces)
        d = self.surface_distances([[v] for v in hv] + [[v] for v in av], max_distance=grab if free is None else free).cpu().numpy()
        ids, owner = region_handles(d[:len(hv)], d[len(hv):] if len(av) else None, grab, free)
        solver = self.set_handles(ids)
        dev = self.vertex.device
        self.region = (torch.as_tensor(hv.astype(np.int64), device=dev), torch.as_tensor(owner.astype(np.int64), device=dev))
        return solver

    def region_targets(self, displacements):
        """The handle positions [n,3] (in the order of arap.handles) that drag_region(displacements) hands to drag()."""
        if self.region is None:
            raise ValueError("drag_region: call set_region_handles(handle_vertices, grab_radius, ...) first")
        picks, owner = self.region
        disp = torch.as_tensor(displacements, dtype=torch.float32, device=self.vertex.device) if not torch.is_tensor(displacements) else \
            displacements.detach().to(device=self.vertex.device, dtype=torch.float32)
        if disp.shape != (len(picks), 3):
            raise ValueError("drag_region: displacements must be [%d,3]; got %s" % (len(picks), tuple(disp.shape)))
        rest = self.vertex.index_select(0, self.arap._handle_idx)
        moved = rest + disp.index_select(0, owner.clamp(min=0))
        return torch.where((owner >= 0)[:, None], moved, rest)                             # (held rows: the rest bits themselves)

    def drag_region(self, displacements, **solve_options):
        """Move the regions of set_region_handles(): the rows grabbed by pick i go to their rest position + displacements[i] ([H,3]: a
        rigid translation of each grabbed patch), the held rows to their rest position; then drag().  No host wait."""
        return self.drag(self.region_targets(displacements), **solve_options)

    def drag_region_pixels(self, camera, pixel_offsets, **solve_options):
        """drag_region() from the screen: pick i's displacement is mesh_pick.screen_offset of the picked vertex's REST position by
        pixel_offsets[i] ([H,2], parallel to the image plane at that vertex's depth) minus that position.  No host wait."""
        from . import mesh_pick
        if self.region is None:
            raise ValueError("drag_region_pixels: call set_region_handles(handle_vertices, grab_radius, ...) first")
        at = self.vertex.index_select(0, self.region[0])
        return self.drag_region(mesh_pick.screen_offset(camera, at, pixel_offsets) - at, **solve_options)

    def deform_vertices(self, deform_vertex):
        """deform() from the deformed vertices alone: their per-vertex (R, S) by gm_mesh_rs first."""
        R, S = mesh_rs(self.vertex, deform_vertex, self._need_faces("deform_vertices"), adjacency=getattr(self, "_adjacency", None))
        return self.deform(deform_vertex, R, S)

    def drag(self, handle_positions, **solve_options):
        """Move the handles of set_handles() to handle_positions [H,3]; the mesh follows as rigidly as it can (ArapSolver.solve, started
        from mesh_vertex_current - the rest pose the first time - so consecutive drags warm-start), and the Gaussians follow the mesh:
        exactly deform_vertices(solver.solve(handle_positions, init=mesh_vertex_current, **solve_options)).  No host wait."""
        if self.arap is None:
            raise ValueError("drag: call set_handles(vertex_ids) first")
        if solve_options.get("want_stats"):
            raise ValueError("drag: want_stats is ArapSolver.solve's; call self.arap.solve for the statistics")
        return self.deform_vertices(self.arap.solve(handle_positions, init=self.mesh_vertex_current, **solve_options))

    def drag_sequence(self, handle_positions, batch=4, **solve_options):
        """A whole drag at once: the meshes [T,Vm,3] with the handles of set_handles() at handle_positions[t] ([T,H,3]), `batch` frames
        per launch chain: exactly self.arap.solve_sequence(handle_positions, init=mesh_vertex_current, batch=batch, **solve_options),
        then deform_vertices of the last frame, which leaves the object as drag(handle_positions[-1]) would.  Inside a run the frames do
        not warm-start from their neighbour (ArapSolver.solve_batch: THE TRADE).  Returns the meshes; no host wait."""
        if self.arap is None:
            raise ValueError("drag_sequence: call set_handles(vertex_ids) first")
        if solve_options.get("want_stats"):
            raise ValueError("drag_sequence: want_stats is ArapSolver.solve_sequence's; call self.arap.solve_sequence for the statistics")
        meshes = self.arap.solve_sequence(handle_positions, init=self.mesh_vertex_current, batch=batch, **solve_options)
        if len(meshes):
            self.deform_vertices(meshes[-1])
        return meshes

    def interpolate_to(self, target_vertices, inbetweens, faces=None, anchors=None, ease="linear", **between_options):
        """The meshes from mesh_vertex_current (the rest pose the first time) to target_vertices [Vm,3] with `inbetweens` frames in
        between, rotation-aware: exactly pose_interp.PoseInterpolator(rest, faces, anchors).sequence([current, target], inbetweens,
        ease=ease, **between_options), [inbetweens + 2, Vm, 3], then deform_vertices of the target, which leaves the object there (in the
        manner of drag_sequence).  The interpolator is built on the first call and kept while faces and anchors stay the same.  faces
        [F,3]: for an object built from tensors alone.  Returns the meshes; no host wait."""
        from .pose_interp import PoseInterpolator
        import numpy as np
        self._need_faces("interpolate_to", faces)
        ids = None if anchors is None else tuple(np.asarray(anchors.detach().cpu() if torch.is_tensor(anchors) else anchors).reshape(-1).tolist())
        interp = self._operator("pose_interp", ids, lambda: PoseInterpolator(self.mesh_graph, None, anchors=None if ids is None else list(ids)))
        current = self.mesh_vertex_current
        meshes = interp.sequence([self.vertex if current is None else current, target_vertices], inbetweens, ease=ease, **between_options)
        self.deform_vertices(meshes[-1])
        return meshes

    def attach_skeleton(self, skeleton, faces=None, **weight_options):
        """Bind this object's rest mesh to a skinning.Skeleton: builds the skinning.SkinBinding (bone-heat weights, one PCG per bone on
        the device; its refusals apply) over the shared mesh_graph and returns it.  weight_options: SkinBinding's heat,
        max_influences, cg_iterations, cg_tolerance, want_full.  The binding is kept while faces, skeleton and options stay the same.
        faces [F,3]: for an object built from tensors alone."""
        from .skinning import SkinBinding
        self._need_faces("attach_skeleton", faces)
        key = (id(skeleton), tuple(sorted(weight_options.items())))
        self.skin = self._operator("skin", key, lambda: SkinBinding(self.mesh_graph, None, skeleton, **weight_options))
        return self.skin

    def pose_sequence(self, rotations, root_translation=None, blend="dqs"):
        """The meshes [T,Vm,3] of the attached skeleton's poses: exactly skin.pose_skeleton(rotations, root_translation, blend) -
        rotations [T,Nj,3,3] matrices or [T,Nj,3] axis-angle vectors, root_translation [T,3] or None -, then deform_vertices of the
        last one, which leaves the object there (in the manner of simulate and interpolate_to).  Returns the meshes; no host wait."""
        if getattr(self, "skin", None) is None:
            raise ValueError("pose_sequence: call attach_skeleton(skeleton) first")
        meshes = self.skin.pose_skeleton(rotations, root_translation, blend=blend)
        self.deform_vertices(meshes[-1])
        self._remember_pose(rotations, root_translation)
        return meshes

    def _remember_pose(self, rotations, root_translation):
        """keeps the last frame's axis-angle parameters for drag_skeleton to start from (matrices are not kept: it starts at rest)"""
        import numpy as np
        host = lambda a: np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
        rot = host(rotations)
        self.skeleton_pose = None
        if rot.ndim == 3 and rot.shape[2] == 3:
            self.skeleton_pose = (rot[-1].copy(), np.zeros(3) if root_translation is None else host(root_translation).reshape(-1, 3)[-1].copy())

    def pose(self, rotations, root_translation=None, blend="dqs"):
        """One pose of the attached skeleton - rotations [Nj,3,3] or [Nj,3], root_translation [3] or None -: leaves the object deformed
        to it and returns what deform_vertices returns."""
        import numpy as np
        if getattr(self, "skin", None) is None:
            raise ValueError("pose: call attach_skeleton(skeleton) first")
        rot = np.asarray(rotations.detach().cpu() if torch.is_tensor(rotations) else rotations, np.float64)[None]
        tr = None if root_translation is None else np.asarray(root_translation.detach().cpu() if torch.is_tensor(root_translation) else root_translation,
                                                              np.float64).reshape(1, 3)
        state = self.deform_vertices(self.skin.pose_skeleton(rot, tr, blend=blend)[0])
        self._remember_pose(rot, tr)
        return state

    def drag_skeleton(self, vertex_ids, targets, iterations=40, damping=0.0, blend="dqs", fit_translation=True):
        """Drag picked vertices and let the attached skeleton follow: skin.solve_ik(vertex_ids, targets, ...) from the current pose
        (the axis-angle parameters of the last pose / pose_sequence / drag_skeleton / fit_skeleton_pose; the rest pose before any), then
        pose(rotations, root_translation, blend), which leaves the object there.  vertex_ids [H] (mesh_pick's, for one), targets [H,3].
        Returns (rotations [Nj,3], root_translation [3], the objective's history) as solve_ik does."""
        if getattr(self, "skin", None) is None:
            raise ValueError("drag_skeleton: call attach_skeleton(skeleton) first")
        start = getattr(self, "skeleton_pose", None) or (None, None)
        rot, tr, history = self.skin.solve_ik(vertex_ids, targets, start[0], start[1], iterations=iterations, damping=damping, blend=blend,
                                              fit_translation=fit_translation)
        self.pose(rot, tr, blend=blend)
        return rot, tr, history

    def fit_skeleton_pose(self, views, iterations, background=None, from_current=True, **fitter_options):
        """Fit the attached skeleton's pose to photographs: pose_fit.SkeletonPoseFitter(self, **fitter_options).fit(views, iterations,
        background) - views: (camera, target [3,H,W]) pairs; fitter_options: lr, blend, deg, lambda_dssim, prior.  from_current: start at
        the current pose (as drag_skeleton does) instead of the rest pose.  Leaves the object at pose(fitted) and returns the fitter
        (its pose, losses and write_pose)."""
        from .pose_fit import SkeletonPoseFitter
        if getattr(self, "skin", None) is None:
            raise ValueError("fit_skeleton_pose: call attach_skeleton(skeleton) first")
        start = (getattr(self, "skeleton_pose", None) if from_current else None) or (None, None)
        fitter = SkeletonPoseFitter(self, rotations=start[0], root_translation=start[1], **fitter_options)
        fitter.fit(views, iterations, background)
        return fitter

    def simulate(self, steps, handle_targets=None, pinned=None, keep_velocity=True, faces=None, collider_rows=None, field_poses=None, **options):
        """`steps` steps of secondary motion (dynamics.MeshDynamics: implicit Euler with the ARAP energy as the potential) from
        mesh_vertex_current (the rest pose the first time): the meshes [steps,Vm,3].  The handles are the ones set_handles /
        set_region_handles chose, scripted to handle_targets [steps,H,3] (in the order of arap.handles); with none chosen the object is
        a free body and handle_targets stays None.  pinned: vertex ids held where they are.  keep_velocity: start from the velocity the
        previous simulate() left (zero the first time); False: from zero.  options: MeshDynamics' mass, density, stiffness, damping,
        gravity, dt, iterations, cg_iterations, cg_tolerance, colliders (dynamics.floor / half_space / sphere, or their tuples, lists or
        dicts) and contact_stiffness; the object is built on the first call and kept while faces, handles, pins and options stay the same
        (colliders are compared by value; field=, a dynamics.SdfGrid, by identity: the operator is reused while the SAME grid object is
        passed; field_friction goes with it; fields=, a list of SdfGrids that move, grid by grid by identity too, field_frictions= by
        value).  collider_rows [steps,K,4]: MeshDynamics.run's, for colliders that move; field_poses [steps,F,3,4]: MeshDynamics.run's,
        the poses of fields= during every step - the fields start every call where the previous call's last pose left them, at the
        identity the first time.  Leaves the object at the last frame through deform_vertices, in the manner of drag_sequence.
        faces [F,3]: for an object built from tensors alone.  Returns the meshes; no host wait."""
        from .dynamics import MeshDynamics
        import numpy as np
        self._need_faces("simulate", faces)
        ids = lambda a: tuple(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a).reshape(-1).tolist())
        hid = () if getattr(self, "arap", None) is None else ids(self.arap.handles)
        pid = () if pinned is None else ids(pinned)
        def frozen(v):                                                 # nested lists, tuples and dicts (colliders) by value
            if isinstance(v, (list, tuple)):
                return tuple(frozen(e) for e in v)
            if isinstance(v, dict):
                return tuple(sorted((k, frozen(e)) for k, e in v.items()))
            if torch.is_tensor(v) or isinstance(v, np.ndarray):
                return tuple(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v).reshape(-1).tolist())
            return v
        opts = tuple(sorted((k, id(v) if torch.is_tensor(v) or isinstance(v, np.ndarray) else frozen(v)) for k, v in options.items()))
        dyn = self._operator("dynamics", (hid, pid, opts), lambda: MeshDynamics(self.mesh_graph, None, pinned=list(pid), handles=list(hid), **options))
        current = self.mesh_vertex_current
        dyn.reset(positions=self.vertex if current is None else current, velocities=getattr(self, "_sim_velocity", None) if keep_velocity else None,
                  field_poses=dyn.field_poses if dyn.NF else None)
        meshes = dyn.run(steps, handle_targets, collider_rows=collider_rows, field_poses=field_poses)
        self._sim_velocity = dyn.velocities
        self.deform_vertices(meshes[-1])
        return meshes

    def _screen_mesh(self, who):
        """(current vertices, faces, check_faces) for the screen-space methods: the face indices are checked on the host the first
        time this face tensor is seen (mesh_pick), afterwards nothing waits for the device."""
        faces = self._need_faces(who)
        check = getattr(self, "_faces_checked", None) is not faces
        current = self.mesh_vertex_current
        return (self.vertex if current is None else current), faces, check

    def pick(self, camera, pixels):
        """mesh_pick.pick on this object's mesh as last deformed (mesh_vertex_current; the rest pose if there is none): what lies under
        pixels [P,2] of the camera, dict(face, vertex, point, depth) on the device.  Its vertex ids are set_handles' ids."""
        from . import mesh_pick
        v, f, check = self._screen_mesh("pick")
        out = mesh_pick.pick(camera, pixels, v, f, check_faces=check)
        self._faces_checked = f
        return out

    def select_visible(self, camera, rect=None):
        """The ids (int64, ascending, on the device) of the vertices of the current mesh that the camera sees
        (mesh_pick.visible_vertices), inside rect = (x0, y0, x1, y1) in pixels if given."""
        from . import mesh_pick
        v, f, check = self._screen_mesh("select_visible")
        mask = mesh_pick.visible_vertices(camera, v, f, rect=rect, check_faces=check)
        self._faces_checked = f
        return torch.nonzero(mask)[:, 0]

    def drag_pixels(self, camera, pixel_offsets, **solve_options):
        """drag() from the screen: the handles of set_handles() move by pixel_offsets [H,2] in the camera's image, each parallel to the
        image plane at its own depth: exactly drag(mesh_pick.screen_offset(camera, current handle positions, pixel_offsets)), the
        current positions being mesh_vertex_current's rows (the rest pose's the first time).  No host wait."""
        from . import mesh_pick
        if self.arap is None:
            raise ValueError("drag_pixels: call set_handles(vertex_ids) first")
        current = self.mesh_vertex_current
        at = (self.vertex if current is None else current).index_select(0, self.arap._handle_idx)
        return self.drag(mesh_pick.screen_offset(camera, at, pixel_offsets), **solve_options)

    def deform(self, deform_vertex, cur_rot, cur_shear):
        dV = _f(deform_vertex) - self.vertex
        pos, cov, rot, cov6 = deform_tensors(self.gaussian_triangles, self.coord, dV, cur_rot.reshape(-1, 3, 3),
                                             cur_shear.reshape(-1, 3, 3), self.gaussian_cov, self.gaussian_pos)
        self.gaussian_deform_pos, self.gaussian_deform_cov, self.gaussian_deform_rot = pos, cov, rot
        self.gaussian_deform_cov6 = cov6
        self.deform_state = (_f(deform_vertex), cur_rot, cur_shear)
        return pos, cov, rot

    def bake(self, deg=3):
        """The object in its current state as a PLAIN Gaussian cloud, a dict on the device: xyz [N,3], scales [N,3], rotations [N,4],
        opacity [N,1], shs [N,M,3] - activated values, ready for GaussianRasterizer(scales=, rotations=, shs=).  Computed from
        deform_state (not from the cached gaussian_deform_* attributes, of which deform_and_shade updates only some):
        deform_tensors -> cov_to_scale_rot(cov') -> rotate_sh(gaussian_feature, rot, deg), so a viewer that evaluates SH at the
        unrotated direction shows the colours the edit path shows.  At rest (deform_state is None) xyz and shs are the object's own
        tensors and (scales, rotations) come from gaussian_cov.  Changes no attribute; only enqueues."""
        if self.deform_state is None:
            pos, cov, shs = self.gaussian_pos, self.gaussian_cov, self.gaussian_feature
        else:
            V1, R, S = self.deform_state
            pos, cov, rot, _ = deform_tensors(self.gaussian_triangles, self.coord, V1 - self.vertex, R.reshape(-1, 3, 3), S.reshape(-1, 3, 3),
                                              self.gaussian_cov, self.gaussian_pos)
            shs = rotate_sh(self.gaussian_feature, rot, deg)
        scales, rotations = cov_to_scale_rot(cov)
        return dict(xyz=pos, scales=scales, rotations=rotations, opacity=self.gaussian_o, shs=shs)

    def deform_and_shade(self, deform_vertex, cur_rot, cur_shear, campos, deg=3):
        """One fused pass for the render loop: updates gaussian_deform_pos / gaussian_deform_cov6 and returns
        (means3D, colors_precomp, cov3D_precomp) for NewGaussianRasterizer (edittool/__init__.py:464-472).  gaussian_deform_cov /
        gaussian_deform_rot are NOT refreshed (the pass never writes them); deform_state records the state, which is what bake() reads."""
        dV = _f(deform_vertex) - self.vertex
        pos, cov6, rgb = deform_shade(self.gaussian_triangles, self.coord, dV, cur_rot.reshape(-1, 3, 3), cur_shear.reshape(-1, 3, 3),
                                      self.gaussian_cov, self.gaussian_pos, self.gaussian_feature, campos, deg)
        self.gaussian_deform_pos, self.gaussian_deform_cov6 = pos, cov6
        self.deform_state = (_f(deform_vertex), cur_rot, cur_shear)
        return pos, rgb, cov6

    def deform_and_render(self, deform_vertex, cur_rot, cur_shear, viewpoint_camera, bg_color=None, workspace=None, begin_only=False):
        """The edit loop's frame in two enqueues (gm_forward_0_deformed_async + gm_forward_1_geom): deformation, rotated-
        direction SH colour and the rasterizer's preprocess run in one kernel, the deformed cloud is never written out.
        viewpoint_camera carries the reference's camera attributes (image_height/width, FoVx/FoVy, world_view_transform,
        full_proj_transform, camera_center).  Returns the image [3,H,W] (white background by default, as
        ObjectVisualTool.render_gaussian), or with begin_only the PendingForward handle for pipelined loops."""
        import math
        from . import rasterizer as Rz
        dev = self.gaussian_pos.device
        state = torch.cat([_f(deform_vertex), _f(cur_rot).reshape(-1, 9), _f(cur_shear).reshape(-1, 9)], dim=1)
        packed = pack_mesh_state(state, self.vertex)
        bg = torch.ones(3, device=dev) if bg_color is None else bg_color
        c = viewpoint_camera
        h = Rz.forward_deformed_begin(bg, self.gaussian_triangles, self.coord, packed, self.gaussian_cov, self.gaussian_pos,
                                      self.gaussian_feature, self.gaussian_o, c.world_view_transform, c.full_proj_transform,
                                      math.tan(c.FoVx * 0.5), math.tan(c.FoVy * 0.5), c.image_height, c.image_width, 3, c.camera_center,
                                      workspace=workspace)
        if begin_only:
            return h
        from .renderer import camera_work_hint
        return h.finish(image_only=True, work_hint=camera_work_hint(c, dev))[1]          # forward-only: no backward state
