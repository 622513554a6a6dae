"""Fit a proxy mesh's pose to images: which deformed vertices V1 explain a few photographs of a trained, mesh-bound object?

    MeshPose(rest_vertices, faces)      the parameter V1 [Vm,3]; state() -> differentiable (dV, R, S), the tables of the fused deform pass
    PoseFitter(obj, faces, ...)         step(camera, target, background) -> loss;  fit(views, iterations)
    SkeletonPose(binding, ...)          the parameters of an attached skeleton: rotations [Nj,3], root_translation [3]; vertices() -> V1
    SkeletonPoseFitter(obj, ...)        the same fit over those 3 Nj + 3 numbers: every point of the search space is a skinned mesh

The chain of one step: MeshPose.state() -> deform.deform_shade_differentiable (HIP, csrc/gm_deform_bwd.hip on the way back) ->
GaussianRasterizer(colors_precomp, cov3D_precomp) -> loss.photometric_loss, plus a cotangent-weighted edge-length term, Adam on V1.
The mesh is small (thousands of vertices against a million Gaussians): everything in this module is torch plumbing, none of it a hot path.

MeshPose.state() restates gm_mesh_rs (csrc/gm_mesh.hip) on its well-conditioned branch, in float64: per vertex the cotangent-weighted
least-squares map of the one-ring, T_i = M1_i(V1) M0_i^-1 - linear in V1, so the rest mesh's share (clamped cotangent weights, the 1e-9
normal term, M0^-1) is computed once on the host and T is one index_add of per-edge outer products - then the orthogonal polar factor by
Newton's iteration Q <- (Q + Q^-T) / 2 with an explicit adjugate inverse, R = Q^T, S = sym(Q^T T).  Not torch.linalg.svd: its backward
divides by sigma_i^2 - sigma_j^2 and is infinite at the rest pose, where every fit starts; the iteration's is finite wherever T is
invertible.  The fitter is for proper deformations: det T <= 0 and an iteration that has not converged raise ValueError naming the vertex.
"""
import numpy as np
import torch

NEWTON_ITERATIONS = 16
ORTHOGONALITY_TOL = 1e-9


def _rest_terms(V0, faces):
    """host, float64, once: the directed edges (from, to, row vector w M0^-1 e), the per-corner triples of the normal term, and the
    per-vertex constants; the formulas and conditioning constants of gm_mesh_rs"""
    Vm = V0.shape[0]
    M0 = np.zeros((Vm, 3, 3)); nr = np.zeros((Vm, 3)); wsum = np.zeros(Vm)
    e_from, e_to, e_vec, e_w, corners = [], [], [], [], []
    for c0 in range(3):
        v, a, b = faces[:, c0], faces[:, (c0 + 1) % 3], faces[:, (c0 + 2) % 3]
        ea, eb = V0[a] - V0[v], V0[b] - V0[v]
        ab = eb - ea
        n0 = np.cross(ea, eb)
        l0 = np.linalg.norm(n0, axis=1)
        ok = l0 > 1e-30
        with np.errstate(divide="ignore", invalid="ignore"):
            cot_a = -(ea * ab).sum(1) / l0
            cot_b = (eb * ab).sum(1) / l0
        wa = np.where(ok, np.maximum(0.5 * cot_b, 1e-3), 0.0)
        wb = np.where(ok, np.maximum(0.5 * cot_a, 1e-3), 0.0)
        np.add.at(M0, v, wa[:, None, None] * ea[:, :, None] * ea[:, None, :] + wb[:, None, None] * eb[:, :, None] * eb[:, None, :])
        np.add.at(nr, v, np.where(ok[:, None], n0, 0.0))
        np.add.at(wsum, v, np.where(ok, l0, 0.0))
        for to, vec, wt in ((a, ea, wa), (b, eb, wb)):
            e_from.append(v[ok]); e_to.append(to[ok]); e_vec.append(vec[ok]); e_w.append(wt[ok])
        corners.append(np.stack([v[ok], a[ok], b[ok]], axis=1))
    e_from, e_to, e_vec, e_w = (np.concatenate(x) for x in (e_from, e_to, e_vec, e_w))
    lr = np.linalg.norm(nr, axis=1)
    reg = lr > 1e-30
    lam = np.where(reg, 1e-9 * np.trace(M0, axis1=1, axis2=2), 0.0)
    nru = nr / np.maximum(lr, 1e-300)[:, None]
    M0 = M0 + lam[:, None, None] * nru[:, :, None] * nru[:, None, :]
    has = (wsum > 0) & (np.abs(np.linalg.det(M0)) > 1e-300)
    M0inv = np.tile(np.eye(3), (Vm, 1, 1))
    M0inv[has] = np.linalg.inv(M0[has])
    rows = e_w[:, None] * np.einsum("eij,ej->ei", M0inv[e_from], e_vec)         # w M0^-1 e (M0 is symmetric)
    return dict(e_from=e_from, e_to=e_to, e_row=rows, e_w=e_w, e_len=np.linalg.norm(e_vec, axis=1), corners=np.concatenate(corners),
                lam=lam, lr=lr, reg=reg, n_row=np.einsum("vij,vj->vi", M0inv, nru), has=has)


def _inverse_transpose(Q):
    """(Q^-T, det Q) of [n,3,3] by the adjugate: the cofactor rows are cross products of Q's rows"""
    c0 = torch.linalg.cross(Q[:, 1], Q[:, 2])
    c1 = torch.linalg.cross(Q[:, 2], Q[:, 0])
    c2 = torch.linalg.cross(Q[:, 0], Q[:, 1])
    det = (Q[:, 0] * c0).sum(1)
    return torch.stack([c0, c1, c2], dim=1) / det[:, None, None], det


class MeshPose(torch.nn.Module):
    """The pose of a proxy mesh as a parameter: V1 [Vm,3] float32 (started at the rest pose), on rest_vertices' device - CPU tensors work
    too.  state(V1=None, dtype=float32) -> (dV [Vm,3], R [Vm,3,3], S [Vm,3,3]), differentiable in V1, computed in float64 and returned
    as dtype."""

    def __init__(self, rest_vertices, faces):
        super().__init__()
        V0 = torch.as_tensor(rest_vertices).detach()
        dev = V0.device
        f = np.asarray(faces.detach().cpu() if torch.is_tensor(faces) else faces, np.int64).reshape(-1, 3)
        rt = _rest_terms(V0.cpu().numpy().astype(np.float64), f)
        self.V1 = torch.nn.Parameter(V0.to(torch.float32).clone())
        buf = lambda name, a, dt: self.register_buffer(name, torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev), persistent=False)
        buf("rest", V0.cpu().numpy(), torch.float32)
        for name in ("e_from", "e_to", "corners"):
            buf(name, rt[name], torch.int64)
        for name in ("e_row", "e_w", "e_len", "lam", "lr", "n_row"):
            buf(name, rt[name], torch.float64)
        for name in ("reg", "has"):
            buf(name, rt[name], torch.bool)

    def deformation_gradients(self, V1):
        """T [Vm,3,3] float64 of V1 (float64): the identity for a vertex without a usable one-ring"""
        Vm = V1.shape[0]
        d = V1[self.e_to] - V1[self.e_from]
        T = torch.zeros((Vm, 3, 3), dtype=V1.dtype, device=V1.device).index_add(0, self.e_from, d[:, :, None] * self.e_row[:, None, :])
        v, a, b = self.corners[:, 0], self.corners[:, 1], self.corners[:, 2]
        nd = torch.zeros((Vm, 3), dtype=V1.dtype, device=V1.device).index_add(0, v, torch.linalg.cross(V1[a] - V1[v], V1[b] - V1[v]))
        ld = torch.linalg.vector_norm(nd, dim=1)
        reg = self.reg & (ld > 1e-30)
        scale = torch.sqrt(torch.where(reg, ld / self.lr.clamp_min(1e-300), torch.ones_like(ld)))
        ndu = nd / ld.clamp_min(1e-300)[:, None]
        T = T + torch.where(reg, self.lam * scale, torch.zeros_like(ld))[:, None, None] * ndu[:, :, None] * self.n_row[:, None, :]
        eye = torch.eye(3, dtype=V1.dtype, device=V1.device).expand(Vm, 3, 3)
        return torch.where(self.has[:, None, None], T, eye)

    def state(self, V1=None, dtype=torch.float32):
        V1f = self.V1 if V1 is None else V1
        V1d = V1f.to(torch.float64)
        T = self.deformation_gradients(V1d)
        Q = T
        det = None
        for _ in range(NEWTON_ITERATIONS):
            Qit, d = _inverse_transpose(Q)
            det = d if det is None else det                                   # det T: the first iterate's
            Q = 0.5 * (Q + Qit)
        with torch.no_grad():
            bad = torch.nonzero(~(det > 0))
            if bad.numel():
                raise ValueError("MeshPose: det T <= 0 at vertex %d (a reflected or collapsed one-ring): the fitter is for proper deformations"
                                 % int(bad[0, 0]))
            off = (Q.transpose(1, 2) @ Q - torch.eye(3, dtype=Q.dtype, device=Q.device)).abs().amax(dim=(1, 2))
            bad = torch.nonzero(~(off <= ORTHOGONALITY_TOL))
            if bad.numel():
                raise ValueError("MeshPose: the polar iteration has not converged at vertex %d (|Q^T Q - I| = %.3g after %d iterations)"
                                 % (int(bad[0, 0]), float(off[bad[0, 0]]), NEWTON_ITERATIONS))
        QtT = Q.transpose(1, 2) @ T
        R = Q.transpose(1, 2)
        S = 0.5 * (QtT + QtT.transpose(1, 2))
        dV = V1d - self.rest.to(torch.float64)
        return dV.to(dtype), R.to(dtype), S.to(dtype)

    def edge_length_term(self, V1=None):
        """cotangent-weighted mean of (|e'| - |e|)^2 over the directed one-ring edges: 0 for a rigid motion"""
        V1d = (self.V1 if V1 is None else V1).to(torch.float64)
        length = torch.linalg.vector_norm(V1d[self.e_to] - V1d[self.e_from], dim=1)
        return ((self.e_w * (length - self.e_len) ** 2).sum() / self.e_w.sum()).to(torch.float32)


def _render_state(o, state, camera, background, deg):
    """the differentiable frame of the object o under the tables state = (dV, R, S): image [3,H,W]"""
    from .deform import deform_shade_differentiable
    from .rasterizer import GaussianRasterizer
    from .renderer import _settings
    dV, R, S = state
    pos, cov6, rgb = deform_shade_differentiable(o.binding, dV, R, S, o.gaussian_cov, o.gaussian_pos, o.gaussian_feature, camera.camera_center,
                                                 deg=deg)
    bg = torch.ones(3, device=pos.device) if background is None else background
    image, _ = GaussianRasterizer(_settings(camera, bg, 1.0, deg, False))(pos, torch.zeros_like(pos), o.gaussian_o, colors_precomp=rgb,
                                                                          cov3D_precomp=cov6)
    return image


class PoseFitter:
    """Adam on a MeshPose's V1 against rendered targets.  obj: a deform.SingleObjectDeform (its cloud, its binding); faces [F,3].
    step(camera, target, background=None) -> the loss (a 0-dim tensor; no host wait here - MeshPose.state()'s refusals wait once per
    step): photometric_loss(render, target) + rigidity * edge_length_term.  camera: renderer.Camera's attributes; target [3,H,W];
    background: float [3], white by default as ObjectVisualTool renders.  fit(views, iterations) cycles over (camera, target) pairs and
    then leaves obj deformed to the fitted V1 with gm_mesh_rs's own (R, S) - deform_state - so every existing tool continues from it.
    lr: Adam's step, by default 1e-3 of the rest mesh's (cotangent-weighted) mean edge length.  Adam moves every coordinate by about lr
    per step whatever the gradient's size, and the one-ring fit of a nearly flat ring takes its normal direction from the ring's sagitta
    alone: neighbours that drift apart by that much along the normal turn the fitted map into a reflection, which state() refuses
    (measured on the 24 x 16 torus, edges of 0.27-0.7, sagitta 0.05: refused after 0.04 of travel at every lr >= 1e-3 and every
    rigidity tried, NOTEBOOK.md "Pose fitting"; the edge-length term does not see bending).  Small steps, many of them.
    Two options against that, both off by default (the defaults are bit for bit the fitter described above):
    regularizer: "edge" (the edge-length term) or "arap" - rigidity * arap.ArapEnergy(V1), the ARAP energy over its scale, which is 0
    for a rigid motion and does see bending (gm_arap_energy_grad); ValueError for any other value.
    smooth_sweeps > 0: between backward() and the optimizer's step V1.grad is replaced by ArapEnergy.smooth_rows(V1.grad, smooth_lambda,
    smooth_sweeps) - Jacobi sweeps of (I + smooth_lambda L) y = grad, the Sobolev gradient: neighbours are moved together."""

    def __init__(self, obj, faces, lr=None, rigidity=1.0, deg=3, lambda_dssim=0.2, regularizer="edge", smooth_sweeps=0, smooth_lambda=1.0):
        if regularizer not in ("edge", "arap"):
            raise ValueError('PoseFitter: regularizer must be "edge" or "arap"; got %r' % (regularizer,))
        if int(smooth_sweeps) < 0 or not float(smooth_lambda) >= 0.0:
            raise ValueError("PoseFitter: smooth_sweeps and smooth_lambda must not be negative; got %r, %r" % (smooth_sweeps, smooth_lambda))
        self.obj, self.deg, self.rigidity, self.lambda_dssim = obj, int(deg), float(rigidity), float(lambda_dssim)
        self.regularizer, self.smooth_sweeps, self.smooth_lambda = regularizer, int(smooth_sweeps), float(smooth_lambda)
        self.faces = torch.as_tensor(faces).detach().to(device=obj.vertex.device, dtype=torch.int32).contiguous()
        self.arap = None                                                      # the mesh's ArapEnergy: only when an option asks for it
        if regularizer == "arap" or self.smooth_sweeps > 0:
            from .arap import ArapEnergy
            own = faces is getattr(obj, "faces", None)                        # the object's own faces: its graph is shared, not rebuilt
            self.arap = ArapEnergy(obj.mesh_graph, None) if own else ArapEnergy(obj.vertex, self.faces, device=obj.vertex.device)
        self.pose = MeshPose(obj.vertex, self.faces)
        start = obj.mesh_vertex_current
        if start is not None:
            with torch.no_grad():
                self.pose.V1.copy_(start)
        self.lr = 1e-3 * float((self.pose.e_w * self.pose.e_len).sum() / self.pose.e_w.sum()) if lr is None else float(lr)
        self.optimizer = torch.optim.Adam([self.pose.V1], lr=self.lr)
        self.losses = []

    def render(self, camera, background=None):
        """the differentiable frame of the current pose: image [3,H,W]"""
        return _render_state(self.obj, self.pose.state(), camera, background, self.deg)

    def step(self, camera, target, background=None):
        from .loss import photometric_loss
        self.optimizer.zero_grad(set_to_none=True)
        loss = photometric_loss(self.render(camera, background), target, self.lambda_dssim)
        if self.rigidity:
            loss = loss + self.rigidity * (self.arap(self.pose.V1) if self.regularizer == "arap" else self.pose.edge_length_term())
        loss.backward()
        if self.smooth_sweeps > 0:
            self.pose.V1.grad = self.arap.smooth_rows(self.pose.V1.grad, self.smooth_lambda, self.smooth_sweeps)
        self.optimizer.step()
        self.losses.append(loss.detach())
        return self.losses[-1]

    def fit(self, views, iterations, background=None):
        views = list(views)
        if not views:
            raise ValueError("PoseFitter.fit: no views")
        for it in range(int(iterations)):
            camera, target = views[it % len(views)]
            self.step(camera, target, background)
        V1 = self.pose.V1.detach().clone()
        if getattr(self.obj, "faces", None) is None:
            self.obj._set_faces(self.faces)
        self.obj.deform_vertices(V1)
        return V1


class SkeletonPose(torch.nn.Module):
    """The pose of a skinned mesh as parameters: rotations [Nj,3] (axis-angle, one per joint) and root_translation [3], float64 on the
    binding's device, zero or given.  binding: a skinning.SkinBinding.  vertices() -> V1 [Vm,3] float32, differentiable in both:
    Skeleton.bone_transforms_torch, then SkinBinding.pose_differentiable (gm_skin_pose, gm_skin_pose_bwd on the way back)."""

    def __init__(self, binding, rotations=None, root_translation=None, blend="dqs"):
        super().__init__()
        from .skinning import BLENDS
        if blend not in BLENDS:
            raise ValueError('SkeletonPose: blend must be "dqs" or "linear"; got %r' % (blend,))
        self.binding, self.blend = binding, blend
        dev, Nj = binding.rest.device, binding.skeleton.Nj
        given = lambda a, shape: torch.zeros(shape, dtype=torch.float64, device=dev) if a is None else \
            torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64), device=dev).reshape(shape).clone()
        try:
            self.rotations = torch.nn.Parameter(given(rotations, (Nj, 3)))
            self.root_translation = torch.nn.Parameter(given(root_translation, (3,)))
        except RuntimeError:
            raise ValueError("SkeletonPose: rotations must be [%d,3] axis-angle vectors and root_translation [3]" % Nj)

    def vertices(self):
        M = self.binding.skeleton.bone_transforms_torch(self.rotations[None], self.root_translation[None])
        return self.binding.pose_differentiable(M, self.blend)[0]


class SkeletonPoseFitter:
    """Adam on a SkeletonPose against rendered targets, for an object with an attached skeleton (obj.attach_skeleton; ValueError
    without one).  One step: forward kinematics -> SkinBinding.pose_differentiable -> MeshPose.state(V1) -> deform_shade_differentiable
    -> GaussianRasterizer -> photometric_loss, plus prior * |rotations|^2; step, fit(views, iterations) and losses as PoseFitter has
    them.  fit leaves the object posed by obj.pose(rotations, root_translation, blend) - the ordinary forward path, so its state is
    exactly what pose gives - and returns (rotations [Nj,3], root_translation [3]), float64.  write_pose(path) writes the one-frame
    {"rotations": ..., "root_translation": ...} JSON that edit_sequence --pose_sequence reads.  rotations / root_translation: where the
    fit starts (None: the rest pose).
    lr: Adam's step in radians (and in the mesh's units for the root), 0.002 by default.  Adam moves every one of the 3 Nj + 3 numbers
    by about lr per step whatever the gradient's size, and a chain's rotations compound along it.  A skinned mesh cannot fold the way
    free vertices do, but it can tear where two bones with very different transforms meet: on the fit test's scene (an open chain of
    five bones round the closed 24 x 16 torus) the one-ring maps at the seam between the first and the last bone turn into
    reflections, which MeshPose.state refuses, once the parameters have travelled about 0.25 rad from rest - after 49 steps at
    lr = 0.005, 25 at 0.01, 14 at 0.02 (tools/skin_bwd_time.py, INTEGRATION.md section AF).  The first default, 0.02, was written down
    unmeasured and did not survive that run; 0.003 was the largest lr whose 60 steps converged there (loss ratios 0.42 to 0.65, vertex
    RMS ratio 0.48), and the default 0.002 (0.65 to 0.78, 0.67) keeps a margin below it."""

    def __init__(self, obj, lr=0.002, blend="dqs", deg=3, lambda_dssim=0.2, prior=0.0, rotations=None, root_translation=None):
        if getattr(obj, "skin", None) is None:
            raise ValueError("SkeletonPoseFitter: call attach_skeleton(skeleton) first")
        if not float(lr) > 0.0 or not float(prior) >= 0.0:
            raise ValueError("SkeletonPoseFitter: lr must be positive and prior not negative; got %r, %r" % (lr, prior))
        self.obj, self.deg, self.lambda_dssim, self.prior, self.lr = obj, int(deg), float(lambda_dssim), float(prior), float(lr)
        self.pose = SkeletonPose(obj.skin, rotations, root_translation, blend)
        self.mesh = MeshPose(obj.vertex, obj.faces)
        self.optimizer = torch.optim.Adam([self.pose.rotations, self.pose.root_translation], lr=self.lr)
        self.losses = []

    def render(self, camera, background=None):
        """the differentiable frame of the current pose: image [3,H,W]"""
        return _render_state(self.obj, self.mesh.state(self.pose.vertices()), camera, background, self.deg)

    def step(self, camera, target, background=None):
        from .loss import photometric_loss
        self.optimizer.zero_grad(set_to_none=True)
        loss = photometric_loss(self.render(camera, background), target, self.lambda_dssim)
        if self.prior:
            loss = loss + self.prior * (self.pose.rotations ** 2).sum().to(loss.dtype)
        loss.backward()
        self.optimizer.step()
        self.losses.append(loss.detach())
        return self.losses[-1]

    def fit(self, views, iterations, background=None):
        views = list(views)
        if not views:
            raise ValueError("SkeletonPoseFitter.fit: no views")
        for it in range(int(iterations)):
            camera, target = views[it % len(views)]
            self.step(camera, target, background)
        rotations, root = self.pose.rotations.detach().clone(), self.pose.root_translation.detach().clone()
        self.obj.pose(rotations, root, blend=self.pose.blend)
        return rotations, root

    def write_pose(self, path):
        import json
        doc = {"rotations": [self.pose.rotations.detach().cpu().tolist()], "root_translation": [self.pose.root_translation.detach().cpu().tolist()]}
        with open(path, "w") as fh:
            json.dump(doc, fh)
