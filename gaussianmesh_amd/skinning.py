"""The proxy mesh posed from a skeleton: bone-heat skinning weights and linear / dual-quaternion skinning on the device (gm_skin_weights,
gm_skin_pose, csrc/gm_skin.hip).  A Skeleton is a few joints in a tree; a pose is a rotation per joint and a root translation; forward
kinematics is host work (J x T small matrices, float64) and the surface follows on the device: SkinBinding solves the weights of
Baran & Popovic 2007 once per (mesh, skeleton) - one Jacobi-PCG per bone over the cotangent Laplacian of arap.edge_csr, the solver of
the ARAP global step - and .pose turns [T,J,3,4] bone transforms into the [T,Vm,3] stack of meshes that render_sequence,
SingleObjectDeform.deform_vertices, MeshDynamics' handle_targets and edit_sequence --save_meshes take.  Definition, ABI and rules:
INTEGRATION.md section AE.  The other direction - the gradient of the posed mesh with respect to the bone transforms (gm_skin_pose_bwd),
forward kinematics in torch, inverse kinematics on picked vertices - is skin_pose_differentiable, Skeleton.bone_transforms_torch and
SkinBinding.solve_ik below: INTEGRATION.md section AF.
THE CONVENTION.  joints float [Nj,3] rest positions, parents int [Nj] with parents[0] == -1 and 0 <= parents[k] < k: one root.  Bone b
(b = 0 .. J - 1, J = Nj - 1 >= 1) is the rest segment joints[parents[b + 1]] -> joints[b + 1].  G_0 = rotate by R_0 about joints[0], then
translate; G_k = G_parents[k] o (rotate by R_k about joints[k]).  Bone b moves with G_parents[b + 1]: a leaf joint's rotation moves
nothing."""
import json

import numpy as np
import torch

from . import _lib
from ._op import enqueue, host, need_cuda, on_device, workspace
from .mesh_graph import MeshGraph

BLENDS = ("linear", "dqs")           # GM_SKIN_BLEND_LINEAR, GM_SKIN_BLEND_DQS


def axis_angle_matrices(r):
    """Rotation vectors [...,3] (axis times angle, radians) as matrices [...,3,3], float64, by Rodrigues' formula"""
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r, axis=-1)[..., None, None]
    K = np.zeros(r.shape[:-1] + (3, 3), np.float64)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -r[..., 2], r[..., 1], r[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -r[..., 0], -r[..., 1], r[..., 0]
    small = th < 1e-8
    safe = np.where(small, 1.0, th)
    a = np.where(small, 1.0, np.sin(safe) / safe)
    b = np.where(small, 0.5, 0.5 * (np.sin(0.5 * safe) / (0.5 * safe)) ** 2)
    return np.eye(3) + a * K + b * (K @ K)


def axis_angle_matrices_torch(r):
    """axis_angle_matrices on a float64 tensor [...,3], differentiable everywhere: written in th2 = r . r, with the series of
    sin(th) / th and (1 - cos th) / th^2 below th2 = 1e-8 (their next terms are below 1e-28 there), so the gradient at r = 0 - where
    every fit starts and where a norm's is NaN - is finite"""
    th2 = (r * r).sum(-1)[..., None, None]
    small = th2 < 1e-8
    th = torch.sqrt(torch.where(small, torch.ones_like(th2), th2))
    a = torch.where(small, 1.0 - th2 / 6.0 + th2 * th2 / 120.0, torch.sin(th) / th)
    b = torch.where(small, 0.5 - th2 / 24.0 + th2 * th2 / 720.0, 0.5 * (torch.sin(0.5 * th) / (0.5 * th)) ** 2)
    z = torch.zeros_like(r[..., 0])
    K = torch.stack([torch.stack([z, -r[..., 2], r[..., 1]], -1), torch.stack([r[..., 2], z, -r[..., 0]], -1),
                     torch.stack([-r[..., 1], r[..., 0], z], -1)], -2)
    return torch.eye(3, dtype=r.dtype, device=r.device) + a * K + b * (K @ K)


class Skeleton:
    """joints [Nj,3], parents [Nj] (THE CONVENTION above), names: Nj strings or None.  ValueError naming the joint that breaks the
    convention.  Host data only: joints float32 (what the kernels read), parents int64, J, bones."""

    def __init__(self, joints, parents, names=None):
        j = np.asarray(host(joints))
        p = np.asarray(host(parents))
        if j.ndim != 2 or j.shape[1] != 3 or j.dtype.kind not in "fiu":
            raise ValueError("Skeleton: joints must be [Nj,3] numbers; got %s %s" % (j.dtype, tuple(j.shape)))
        if p.ndim != 1 or p.dtype.kind not in "iu" or len(p) != len(j):
            raise ValueError("Skeleton: parents must be %d integers, one per joint; got %s %s" % (len(j), p.dtype, tuple(p.shape)))
        if len(j) < 2:
            raise ValueError("Skeleton: %d joint(s); a skeleton has at least two (one bone)" % len(j))
        if len(j) - 1 > _lib.GM_SKIN_BONES_MAX:
            raise ValueError("Skeleton: %d bones; at most %d" % (len(j) - 1, _lib.GM_SKIN_BONES_MAX))
        j = j.astype(np.float32)
        for k in range(len(j)):
            if not np.isfinite(j[k]).all():
                raise ValueError("Skeleton: joint %d is not finite" % k)
        if int(p[0]) != -1:
            raise ValueError("Skeleton: joint 0 is the root and must have parent -1; got %d" % int(p[0]))
        for k in range(1, len(p)):
            if not 0 <= int(p[k]) < k:
                raise ValueError("Skeleton: joint %d has parent %d; a parent comes before its child (0 .. %d)" % (k, int(p[k]), k - 1))
        if names is not None:
            names = [str(n) for n in names]
            if len(names) != len(j):
                raise ValueError("Skeleton: %d names for %d joints" % (len(names), len(j)))
        self.joints, self.parents, self.names = np.ascontiguousarray(j), p.astype(np.int64), names
        self.Nj, self.J = len(j), len(j) - 1

    @property
    def bones(self):
        """(a, b): the rest segments' ends, float32 [J,3] each"""
        return np.ascontiguousarray(self.joints[self.parents[1:]]), np.ascontiguousarray(self.joints[1:])

    def joint_transforms(self, rotations, root_translation=None):
        """G_k of every frame and joint: (A float64 [T,Nj,3,3], t float64 [T,Nj,3]), x -> A x + t"""
        who = "Skeleton.bone_transforms"
        R = np.asarray(host(rotations), np.float64)
        if R.ndim == 3 and R.shape[1:] == (self.Nj, 3):
            R = axis_angle_matrices(R)
        if R.ndim != 4 or R.shape[1:] != (self.Nj, 3, 3) or R.shape[0] == 0:
            raise ValueError("%s: rotations must be [T,%d,3,3] matrices or [T,%d,3] axis-angle vectors, T >= 1; got %s" % (who, self.Nj, self.Nj, tuple(R.shape)))
        T = R.shape[0]
        tr = np.zeros((T, 3)) if root_translation is None else np.asarray(host(root_translation), np.float64)
        if tr.shape != (T, 3):
            raise ValueError("%s: root_translation must be [%d,3]; got %s" % (who, T, tuple(tr.shape)))
        if not np.isfinite(R).all() or not np.isfinite(tr).all():
            raise ValueError("%s: rotations and root_translation must be finite" % who)
        c = self.joints.astype(np.float64)
        A, t = np.zeros((T, self.Nj, 3, 3)), np.zeros((T, self.Nj, 3))
        for k in range(self.Nj):
            own = c[k] - R[:, k] @ c[k]                                # rotate about joints[k]: x -> R x + (c - R c)
            if k == 0:
                A[:, 0], t[:, 0] = R[:, 0], own + tr
            else:
                p = self.parents[k]
                A[:, k] = A[:, p] @ R[:, k]
                t[:, k] = np.einsum("tab,tb->ta", A[:, p], own) + t[:, p]
        return A, t

    def bone_transforms(self, rotations, root_translation=None):
        """The rest-to-posed transforms of the J bones, float32 [T,J,3,4] ([A | t] of G_parents[b + 1]), from rotations [T,Nj,3,3]
        (matrices) or [T,Nj,3] (axis-angle vectors) and root_translation [T,3] or None.  Host, float64, rounded once."""
        A, t = self.joint_transforms(rotations, root_translation)
        p = self.parents[1:]
        return np.ascontiguousarray(np.concatenate([A[:, p], t[:, p, :, None]], axis=3).astype(np.float32))

    def bone_transforms_torch(self, rotations, root_translation=None):
        """bone_transforms in torch, differentiable: rotations a floating-point tensor [T,Nj,3] (axis-angle), root_translation [T,3]
        or None -> float64 [T,J,3,4] on the tensor's device (CPU tensors work too), the same convention.  float64 throughout and not
        rounded: skin_pose_differentiable rounds to float32 on its way in.  ValueError for shapes; nothing here reads a value."""
        who = "Skeleton.bone_transforms_torch"
        if not torch.is_tensor(rotations) or not rotations.dtype.is_floating_point or rotations.ndim != 3 or tuple(rotations.shape[1:]) != (self.Nj, 3) \
                or rotations.shape[0] == 0:
            raise ValueError("%s: rotations must be a floating-point tensor [T,%d,3] of axis-angle vectors, T >= 1; got %s"
                             % (who, self.Nj, tuple(rotations.shape) if torch.is_tensor(rotations) else type(rotations).__name__))
        T, dev = rotations.shape[0], rotations.device
        R = axis_angle_matrices_torch(rotations.to(torch.float64))
        if root_translation is None:
            tr = torch.zeros((T, 3), dtype=torch.float64, device=dev)
        elif not torch.is_tensor(root_translation) or tuple(root_translation.shape) != (T, 3) or not root_translation.dtype.is_floating_point:
            raise ValueError("%s: root_translation must be a floating-point tensor [%d,3]" % (who, T))
        else:
            tr = root_translation.to(device=dev, dtype=torch.float64)
        c = torch.as_tensor(self.joints.astype(np.float64), device=dev)
        A, t = [None] * self.Nj, [None] * self.Nj
        for k in range(self.Nj):
            own = c[k] - R[:, k] @ c[k]
            if k == 0:
                A[0], t[0] = R[:, 0], own + tr
            else:
                p = int(self.parents[k])
                A[k] = A[p] @ R[:, k]
                t[k] = torch.einsum("tab,tb->ta", A[p], own) + t[p]
        p = [int(q) for q in self.parents[1:]]
        return torch.cat([torch.stack([A[q] for q in p], 1), torch.stack([t[q] for q in p], 1)[..., None]], 3)

    def write(self, path):
        doc = {"joints": [[float(x) for x in j] for j in self.joints], "parents": [int(p) for p in self.parents]}
        if self.names is not None:
            doc["names"] = list(self.names)
        with open(path, "w") as fh:
            json.dump(doc, fh)

    @classmethod
    def read(cls, path):
        """{"joints": [[x, y, z], ...], "parents": [...], "names": [...] (optional)}; ValueError naming the file and what is wrong"""
        try:
            with open(path) as fh:
                doc = json.load(fh)
        except (OSError, ValueError) as e:
            raise ValueError("Skeleton.read: %s: cannot read it as JSON (%s)" % (path, e))
        if not isinstance(doc, dict) or "joints" not in doc or "parents" not in doc:
            raise ValueError('Skeleton.read: %s: must hold a JSON object with "joints" and "parents"' % path)
        try:
            joints, parents = np.asarray(doc["joints"], np.float64), np.asarray(doc["parents"])
            return cls(joints, parents, doc.get("names"))
        except (TypeError, ValueError) as e:
            raise ValueError("Skeleton.read: %s: %s" % (path, e))


def _transforms(transforms, J, blend, who, checked=True):
    """transforms as float32 [T,J,3,4] on the host plus the blend's number; blend "dqs" refuses a 3 x 3 part that is no rotation
    (checked=False: not looked at)"""
    if blend not in BLENDS:
        raise ValueError('%s: blend must be "dqs" or "linear"; got %r' % (who, blend))
    M = np.asarray(host(transforms))
    if M.ndim != 4 or M.shape[1:] != (J, 3, 4) or M.shape[0] == 0 or M.dtype.kind != "f":
        raise ValueError("%s: transforms must be floating-point [T,%d,3,4], T >= 1; got %s %s" % (who, J, M.dtype, tuple(M.shape)))
    M = np.ascontiguousarray(M.astype(np.float32))
    if not np.isfinite(M).all():
        raise ValueError("%s: transforms must be finite" % who)
    if blend == "dqs" and checked:
        A = M[..., :3].astype(np.float64)
        off = np.abs(A @ A.transpose(0, 1, 3, 2) - np.eye(3)).max(axis=(2, 3))
        bad = np.argwhere((off > 1e-5) | (np.abs(np.linalg.det(A) - 1.0) > 1e-5))
        if len(bad):
            raise ValueError('%s: blend "dqs" needs rotations; the 3 x 3 part of frame %d, bone %d is none within 1e-5 (%d such); use blend="linear"'
                             % (who, int(bad[0][0]), int(bad[0][1]), len(bad)))
    return M, BLENDS.index(blend)


def _weights(who, rest, bone_ids, bone_w, J):
    """the checks skin_vertices and skin_pose_differentiable share -> (rest float32, ids int32, w float32), contiguous on rest's device"""
    if not 1 <= J <= _lib.GM_SKIN_BONES_MAX:
        raise ValueError("%s: %d bones (1 .. %d)" % (who, J, _lib.GM_SKIN_BONES_MAX))
    if rest.ndim != 2 or rest.shape[1] != 3 or rest.shape[0] == 0 or not rest.dtype.is_floating_point:
        raise ValueError("%s: rest must be a floating-point [Vm,3] tensor; got %s %s" % (who, rest.dtype, tuple(rest.shape)))
    Vm, dev = rest.shape[0], rest.device
    ids, w = torch.as_tensor(bone_ids), torch.as_tensor(bone_w)
    if tuple(ids.shape) != (Vm, 4) or ids.dtype.is_floating_point or ids.dtype is torch.bool:
        raise ValueError("%s: bone_ids must be integer [%d,4]; got %s %s" % (who, Vm, ids.dtype, tuple(ids.shape)))
    if tuple(w.shape) != (Vm, 4) or not w.dtype.is_floating_point:
        raise ValueError("%s: bone_w must be floating-point [%d,4]; got %s %s" % (who, Vm, w.dtype, tuple(w.shape)))
    lo, hi = int(ids.min()), int(ids.max())
    if lo < 0 or hi >= J:
        raise ValueError("%s: bone id outside [0, %d) (min %d, max %d)" % (who, J, lo, hi))
    return rest.detach().to(torch.float32).contiguous(), on_device(ids, torch.int32, dev), on_device(w, torch.float32, dev)


def skin_vertices(rest, bone_ids, bone_w, transforms, blend="dqs", out=None, checked=True):
    """gm_skin_pose on weights from anywhere (painted, or imported from another rig): rest [Vm,3] float on the device, bone_ids integer
    [Vm,4] in [0, J), bone_w float [Vm,4] (by falling weight for "dqs": slot 0 sets the sign of the others), transforms [T,J,3,4]
    rest-to-posed (tensor or array; checked on the host) -> [T,Vm,3] float32 on the device.  ValueError for shapes, dtypes, an id outside
    [0, J) and, with blend "dqs", a 3 x 3 part that is no rotation within 1e-5 (checked=False spares that one check, for transforms that
    are rotations by construction); GmeshError without a device."""
    who = "skin_vertices"
    need_cuda(rest, who, "rest")
    M0 = np.asarray(host(transforms))
    if M0.ndim != 4:
        raise ValueError("%s: transforms must be [T,J,3,4]; got %s" % (who, tuple(M0.shape)))
    J = M0.shape[1]
    rest32, ids, w = _weights(who, rest, bone_ids, bone_w, J)
    return _pose(who, rest32, ids, w, J, transforms, blend, out, checked)


def _pose(who, rest, ids, w, J, transforms, blend, out, checked=True):
    M, number = _transforms(transforms, J, blend, who, checked)
    T, Vm, dev = M.shape[0], rest.shape[0], rest.device
    if out is None:
        out = torch.empty((T, Vm, 3), dtype=torch.float32, device=dev)
    elif not torch.is_tensor(out) or tuple(out.shape) != (T, Vm, 3) or out.dtype is not torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError("%s: out must be a contiguous float32 %s tensor on the mesh's device" % (who, [T, Vm, 3]))
    enqueue(dev, "gm_skin_pose", T, Vm, J, rest, ids, w, on_device(M, torch.float32, dev), number, out)
    return out


def bone_incidence(bone_ids, bone_w, J):
    """The bones' incidence lists gm_skin_pose_bwd gathers over: (offsets int32 [J+1], entries int32 [offsets[J]]) on the tensors'
    device.  Every (vertex, slot) with bone_w != 0 appears once, as 4 vertex + slot, under its bone (ids forced into [0, J) as the kernels
    force them), ascending within a bone (a stable sort).  Built with torch; the entries' count is read once (a host wait)."""
    ids, w = torch.as_tensor(bone_ids), torch.as_tensor(bone_w)
    if ids.ndim != 2 or ids.shape[1] != 4 or tuple(w.shape) != tuple(ids.shape) or ids.dtype.is_floating_point or not w.dtype.is_floating_point:
        raise ValueError("bone_incidence: bone_ids must be integer [Vm,4] and bone_w floating-point [Vm,4]; got %s %s, %s %s"
                         % (ids.dtype, tuple(ids.shape), w.dtype, tuple(w.shape)))
    if not 1 <= int(J) <= _lib.GM_SKIN_BONES_MAX:
        raise ValueError("bone_incidence: %d bones (1 .. %d)" % (J, _lib.GM_SKIN_BONES_MAX))
    w = w.to(ids.device)
    flat = ids.reshape(-1).to(torch.int64).clamp(0, int(J) - 1)
    live = torch.nonzero(w.reshape(-1) != 0).reshape(-1)
    bones = flat[live]
    order = torch.sort(bones, stable=True).indices
    offsets = torch.zeros(int(J) + 1, dtype=torch.int64, device=ids.device)
    offsets[1:] = torch.cumsum(torch.bincount(bones, minlength=int(J)), 0)
    return offsets.to(torch.int32), live[order].to(torch.int32).contiguous()


def _pose_bwd(rest, ids, w, M, number, g_out, incidence):
    """gm_skin_pose_bwd: float64 [T,J,3,4]; every argument a contiguous tensor of the kernel's dtype on rest's device"""
    T, J, Vm, dev = M.shape[0], M.shape[1], rest.shape[0], rest.device
    offsets, entries = incidence
    if entries.numel() == 0:                                           # (no weight anywhere: a pointer all the same)
        entries = torch.zeros(1, dtype=torch.int32, device=dev)
    g = torch.empty((T, J, 3, 4), dtype=torch.float64, device=dev)
    ws = workspace(dev, "gm_skin_pose_bwd_workspace_bytes", T, Vm, J, number)
    enqueue(dev, "gm_skin_pose_bwd", T, Vm, J, rest, ids, w, M, number, g_out, offsets, entries, g, workspace=ws)
    return g


class _SkinPose(torch.autograd.Function):
    @staticmethod
    def forward(ctx, transforms, rest, ids, w, number, incidence):
        M = transforms.detach().to(torch.float32).contiguous()
        T, J, Vm = M.shape[0], M.shape[1], rest.shape[0]
        out = torch.empty((T, Vm, 3), dtype=torch.float32, device=rest.device)
        enqueue(rest.device, "gm_skin_pose", T, Vm, J, rest, ids, w, M, number, out)
        ctx.save_for_backward(M, rest, ids, w, *incidence)
        ctx.number, ctx.dtype = number, transforms.dtype
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        M, rest, ids, w, offsets, entries = ctx.saved_tensors
        g = _pose_bwd(rest, ids, w, M, ctx.number, g_out.detach().to(torch.float32).contiguous(), (offsets, entries))
        return g.to(ctx.dtype), None, None, None, None, None


def _device_transforms(who, transforms, J, dev):
    if not torch.is_tensor(transforms) or transforms.dtype not in (torch.float32, torch.float64) or transforms.ndim != 4 \
            or tuple(transforms.shape[1:]) != (J, 3, 4) or transforms.shape[0] == 0:
        raise ValueError("%s: transforms must be a float32 or float64 tensor [T,%d,3,4], T >= 1; got %s"
                         % (who, J, "%s %s" % (transforms.dtype, tuple(transforms.shape)) if torch.is_tensor(transforms) else type(transforms).__name__))
    if transforms.device != dev:
        raise ValueError("%s: transforms must be on the mesh's device %s; got %s" % (who, dev, transforms.device))


def skin_pose_differentiable(rest, bone_ids, bone_w, transforms, blend="dqs", incidence=None):
    """skin_vertices as a torch.autograd.Function: transforms a float32 or float64 tensor [T,J,3,4] on rest's device that may require
    grad -> [T,Vm,3] float32.  Forward: gm_skin_pose on the float32 rounding of the transforms, on the device all the way - no host
    round trip and no host rotation check (the bits of skin_vertices(..., checked=False) on the same float32 transforms).  Backward:
    gm_skin_pose_bwd, float64, returned in the dtype of transforms; nothing flows to rest or the weights.  incidence: bone_incidence's
    pair, built here when None (a host wait; SkinBinding keeps its own).  ValueError for shapes, dtypes and devices; GmeshError without
    a device."""
    who = "skin_pose_differentiable"
    need_cuda(rest, who, "rest")
    if blend not in BLENDS:
        raise ValueError('%s: blend must be "dqs" or "linear"; got %r' % (who, blend))
    if not torch.is_tensor(transforms) or transforms.ndim != 4:
        raise ValueError("%s: transforms must be a tensor [T,J,3,4]" % who)
    J = transforms.shape[1]
    rest32, ids, w = _weights(who, rest, bone_ids, bone_w, J)
    _device_transforms(who, transforms, J, rest32.device)
    if incidence is None:
        incidence = bone_incidence(ids, w, J)
    return _SkinPose.apply(transforms, rest32, ids, w, BLENDS.index(blend), tuple(incidence))


class SkinBinding:
    """The skinning weights of one (mesh, skeleton).  mesh_or_graph: a MeshGraph (faces=None: shared, not rebuilt) or rest vertices [Vm,3]
    with faces [F,3].  heat: the c of h_i = c area_i / d2min_i (1: Baran & Popovic's choice; larger pins a vertex harder to its nearest
    bone); max_influences 1 .. 4 bones kept per vertex.  Holds bone_ids int32 [Vm,4], bone_w float32 [Vm,4] (by falling weight), stats
    float64 [J,2] (CG steps used, final |r| / |b| per bone) and, with want_full, full float64 [J,Vm]: the columns before compaction.
    The defaults (at most 1000 CG steps per bone, relative residual 1e-8) were written down unmeasured; tools/skin_time.py (INTEGRATION.md
    section AE) then saw the tolerance bind at no more than 99 steps at 1073 vertices and 264 at 7.5 k on an MI355X, one PCG's time
    whatever J (0.9 and 8 to 9 ms), so they stay.  Stream-ordered:
    nothing here waits for the device.  ValueError for the options; GmeshError without a device."""

    def __init__(self, mesh_or_graph, faces, skeleton, heat=1.0, max_influences=4, cg_iterations=1000, cg_tolerance=1e-8, want_full=False,
                 device="cuda"):
        who = "SkinBinding"
        if not isinstance(skeleton, Skeleton):
            raise ValueError("%s: skeleton must be a skinning.Skeleton; got %s" % (who, type(skeleton).__name__))
        if isinstance(heat, bool) or not isinstance(heat, (int, float, np.integer, np.floating)) or not np.isfinite(heat) or not heat > 0.0:
            raise ValueError("%s: heat = %r; a finite number > 0" % (who, heat))
        if isinstance(max_influences, bool) or not isinstance(max_influences, (int, np.integer)) or not 1 <= max_influences <= 4:
            raise ValueError("%s: max_influences = %r; an integer in 1 .. 4" % (who, max_influences))
        g = self.mesh = MeshGraph.of(mesh_or_graph, faces, device, who)
        g.need_device(who)
        from .dynamics import vertex_masses
        self.skeleton, self.J, self.Vm, self.device = skeleton, skeleton.J, g.Vm, g.device
        rest, off, cols, w = g.device_csr
        dev = rest.device
        a, b = skeleton.bones
        area = on_device(vertex_masses(g.rest_host, g.faces_host, 1.0), torch.float64, dev)
        self.rest = rest
        self.bone_ids = torch.empty((g.Vm, 4), dtype=torch.int32, device=dev)
        self.bone_w = torch.empty((g.Vm, 4), dtype=torch.float32, device=dev)
        self.full = torch.empty((self.J, g.Vm), dtype=torch.float64, device=dev) if want_full else None
        self.stats = torch.empty((self.J, 2), dtype=torch.float64, device=dev)
        ws = torch.empty((_lib.lib().gm_skin_weights_workspace_bytes(g.Vm, self.J),), dtype=torch.uint8, device=dev)
        enqueue(dev, "gm_skin_weights", g.Vm, self.J, off, cols, w, rest, area, on_device(a, torch.float32, dev), on_device(b, torch.float32, dev),
                float(heat), int(cg_iterations), float(cg_tolerance), int(max_influences), self.bone_ids, self.bone_w, self.full, self.stats,
                workspace=ws)

    def pose(self, transforms, blend="dqs", out=None, checked=True):
        """The meshes [T,Vm,3] float32 on the device under transforms [T,J,3,4] (Skeleton.bone_transforms, or any rest-to-posed
        transforms): blend "dqs" (dual quaternions: a twist keeps its volume) or "linear" (the classic blend, which takes scale and
        shear too).  out: a contiguous float32 [T,Vm,3] tensor on the device.  A frame's bits depend on its transforms alone.
        ValueError for shapes and, with "dqs", a 3 x 3 part that is no rotation within 1e-5 (checked=False spares that check, for
        transforms that are rotations by construction)."""
        return _pose("SkinBinding.pose", self.rest, self.bone_ids, self.bone_w, self.J, transforms, blend, out, checked)

    @property
    def incidence(self):
        """bone_incidence of this binding's weights: built on first use (one host wait) and kept"""
        if getattr(self, "_incidence", None) is None:
            self._incidence = bone_incidence(self.bone_ids, self.bone_w, self.J)
        return self._incidence

    def pose_differentiable(self, transforms, blend="dqs"):
        """pose as a torch.autograd.Function (skin_pose_differentiable): transforms a float32 or float64 tensor [T,J,3,4] on the
        device that may require grad -> [T,Vm,3] float32, the bits of pose() on the same float32 transforms; backward by
        gm_skin_pose_bwd in the dtype of transforms.  No host rotation check: with "dqs" the transforms must be rotations by
        construction (Skeleton.bone_transforms_torch's are)."""
        who = "SkinBinding.pose_differentiable"
        if blend not in BLENDS:
            raise ValueError('%s: blend must be "dqs" or "linear"; got %r' % (who, blend))
        _device_transforms(who, transforms, self.J, self.rest.device)
        return _SkinPose.apply(transforms, self.rest, self.bone_ids, self.bone_w, BLENDS.index(blend), self.incidence)

    def solve_ik(self, vertex_ids, targets, rotations=None, root_translation=None, iterations=40, damping=0.0, blend="dqs", fit_translation=True):
        """Inverse kinematics on picked vertices: the joint rotations [Nj,3] (axis-angle) and root translation [3] that minimise
        1/2 sum |V1[vertex_ids] - targets|^2 + damping |rotations|^2, V1 the skinned mesh, from rotations / root_translation (zeros when
        None) by torch.optim.LBFGS(max_iter=1, history_size=20, line_search_fn="strong_wolfe"), one step per iteration, the gradient
        through bone_transforms_torch and gm_skin_pose_bwd.  fit_translation=False keeps root_translation where it is.  Returns
        (rotations float64 [Nj,3], root_translation float64 [3], history): history[0] the objective at the start, history[k] after k
        steps (floats: the line search waits for the device anyway).  ValueError for shapes, ids outside the mesh, the options."""
        who = "SkinBinding.solve_ik"
        if blend not in BLENDS:
            raise ValueError('%s: blend must be "dqs" or "linear"; got %r' % (who, blend))
        if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 1:
            raise ValueError("%s: iterations = %r; an integer >= 1" % (who, iterations))
        if isinstance(damping, bool) or not isinstance(damping, (int, float, np.integer, np.floating)) or not np.isfinite(damping) or damping < 0.0:
            raise ValueError("%s: damping = %r; a finite number >= 0" % (who, damping))
        dev, Nj = self.rest.device, self.skeleton.Nj
        pick = np.asarray(host(vertex_ids))
        if pick.ndim != 1 or len(pick) == 0 or pick.dtype.kind not in "iu" or pick.min() < 0 or pick.max() >= self.Vm:
            raise ValueError("%s: vertex_ids must be integers [H] in [0, %d), H >= 1" % (who, self.Vm))
        pick = on_device(pick, torch.int64, dev)
        goal = on_device(targets, torch.float64, dev)
        if tuple(goal.shape) != (len(pick), 3) or not bool(torch.isfinite(goal).all()):
            raise ValueError("%s: targets must be finite [%d,3]; got %s" % (who, len(pick), tuple(goal.shape)))
        r = torch.zeros((Nj, 3), dtype=torch.float64, device=dev) if rotations is None else on_device(rotations, torch.float64, dev).clone()
        t = torch.zeros(3, dtype=torch.float64, device=dev) if root_translation is None else on_device(root_translation, torch.float64, dev).reshape(-1).clone()
        if tuple(r.shape) != (Nj, 3) or tuple(t.shape) != (3,):
            raise ValueError("%s: rotations must be [%d,3] axis-angle vectors and root_translation [3]; got %s, %s" % (who, Nj, tuple(r.shape), tuple(t.shape)))
        r.requires_grad_(True)
        t.requires_grad_(bool(fit_translation))
        optimizer = torch.optim.LBFGS([r, t] if fit_translation else [r], max_iter=1, history_size=20, line_search_fn="strong_wolfe")

        def objective():
            V1 = self.pose_differentiable(self.skeleton.bone_transforms_torch(r[None], t[None]), blend)[0]
            return 0.5 * ((V1.index_select(0, pick).to(torch.float64) - goal) ** 2).sum() + damping * (r * r).sum()

        def closure():
            optimizer.zero_grad(set_to_none=True)
            loss = objective()
            loss.backward()
            return loss
        history = []
        for _ in range(int(iterations)):
            history.append(float(optimizer.step(closure).detach()))
        with torch.no_grad():
            history.append(float(objective()))
        return r.detach(), t.detach(), history

    def pose_skeleton(self, rotations, root_translation=None, blend="dqs", out=None):
        """pose(skeleton.bone_transforms(rotations, root_translation), blend)"""
        return self.pose(self.skeleton.bone_transforms(rotations, root_translation), blend, out)
