"""The plain 3DGS model of the background stage (scene/gaussian_model.py) on torch tensors: PlainGaussians.

Same method names as the reference's GaussianModel.  Differences of representation, not of values:
  * the SH coefficients are ONE parameter `_features` [N,16,3] (`_features_dc` / `_features_rest` are views), and the optimizer is
    model_ops.FusedAdam with the reference's f_dc / f_rest learning rates as the two rates of that one tensor (period 48, split 3);
  * the optimizer state lives in FusedAdam's group dicts ("m", "values", Jittor's names); capture() / restore() carry it;
  * on the GPU the SH rows can share their storage with the joint [background; object] buffer of renderer.bg_render
    (share_feature_storage): every topology edit below keeps that sharing and the optimizer pointed at the current rows.
Densification (densify_and_clone / _split / _prune, prune_points, reset_opacity) runs between iterations, in torch, on CPU or GPU
tensors alike.  The class deliberately has no `activated` method: bg_render() would take that for the mesh-bound model.
"""
import torch

from . import io as gio

_SH_C0 = 0.28209479177387814


def inverse_sigmoid(x):
    """utils/general_utils.py:18-19"""
    return torch.log(x / (1 - x))


def build_rotation(r):
    """utils/general_utils.py:77-98: rotation matrices of (unclamped) normalised quaternions (w, x, y, z)."""
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


class PlainGaussians:
    """scene/gaussian_model.py:GaussianModel.  Raw parameters _xyz [N,3], _features [N,(D+1)^2,3], _scaling [N,3], _rotation [N,4],
    _opacity [N,1]; densification statistics max_radii2D [N], xyz_gradient_accum [N,1], denom [N,1]; screenspace_points [N,3]."""

    SH_GROUP = "f_dc+f_rest"
    _PARAM_OF_GROUP = {"xyz": "_xyz", SH_GROUP: "_features", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}

    def __init__(self, sh_degree=3, device="cuda"):
        self.active_sh_degree = 0
        self.max_sh_degree = sh_degree
        self.device = torch.device(device)
        f = dict(dtype=torch.float32, device=self.device)
        K = (sh_degree + 1) ** 2
        self._set_params(torch.empty((0, 3), **f), torch.empty((0, K, 3), **f), torch.empty((0, 3), **f), torch.empty((0, 4), **f),
                         torch.empty((0, 1), **f))
        self.optimizer = None
        self.percent_dense = 0
        self.spatial_lr_scale = 0
        self.fused = True                        # bg_render's fused route (False: the generic torch route, for comparisons)
        self._share_with = None                  # (mesh model) whose rows follow ours in the joint SH buffer, or None

    # ---- parameters
    def _set_params(self, xyz, features, scaling, rotation, opacity):
        P = lambda t: torch.nn.Parameter(t.detach().to(self.device, torch.float32).contiguous())
        self._xyz, self._features, self._scaling, self._rotation, self._opacity = P(xyz), P(features), P(scaling), P(rotation), P(opacity)
        self._reset_stats()

    def _reset_stats(self):
        N, f = self._xyz.shape[0], dict(dtype=torch.float32, device=self.device)
        self.max_radii2D = torch.zeros((N,), **f)
        self.xyz_gradient_accum = torch.zeros((N, 1), **f)
        self.denom = torch.zeros((N, 1), **f)
        self.screenspace_points = torch.zeros((N, 3), requires_grad=True, **f)

    @property
    def get_number(self):
        return self._xyz.shape[0]

    @property
    def _features_dc(self):
        return self._features[:, :1]

    @property
    def _features_rest(self):
        return self._features[:, 1:]

    @property
    def get_scaling(self):
        return torch.exp(self._scaling)

    @property
    def get_rotation(self):
        return torch.nn.functional.normalize(self._rotation)

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_features(self):
        return self._features

    @property
    def get_opacity(self):
        return torch.sigmoid(self._opacity)

    def get_covariance(self, scaling_modifier=1):
        """build_covariance_from_scaling_rotation (:27-31): strip_symmetric(L L^T), L = R(_rotation) S; [N,6]."""
        from .renderer import strip_symmetric
        L = build_rotation(self._rotation) * (scaling_modifier * self.get_scaling)[:, None, :]
        return strip_symmetric(L @ L.transpose(1, 2))

    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    def create_from_pcd(self, pcd, spatial_lr_scale):
        """:133-170.  pcd: anything with .points [N,3] and .colors [N,3] (BasicPointCloud); scales from distCUDA2 (GPU)."""
        from .simple_knn import distCUDA2
        self.spatial_lr_scale = spatial_lr_scale
        pts = torch.as_tensor(pcd.points, dtype=torch.float32, device=self.device)
        col = (torch.as_tensor(pcd.colors, dtype=torch.float32, device=self.device) - 0.5) / _SH_C0      # RGB2SH
        N, K = pts.shape[0], (self.max_sh_degree + 1) ** 2
        feats = torch.zeros((N, K, 3), dtype=torch.float32, device=self.device)
        feats[:, 0] = col
        dist2 = torch.clamp_min(distCUDA2(pts), 0.0000001)
        scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
        rots = torch.zeros((N, 4), dtype=torch.float32, device=self.device)
        rots[:, 0] = 1
        opac = inverse_sigmoid(0.1 * torch.ones((N, 1), dtype=torch.float32, device=self.device))
        self._set_params(pts, feats, scales, rots, opac)

    # ---- optimizer
    def training_setup(self, training_args):
        """:172-190.  training_args: any object (or dict) with percent_dense, position_lr_*, feature_lr, opacity_lr, scaling_lr,
        rotation_lr.  The f_dc and f_rest groups are the two rates of the one SH tensor (f_rest: feature_lr / 20)."""
        from .model_ops import FusedAdam
        from .train import get_expon_lr_func
        a = training_args if not isinstance(training_args, dict) else type("Args", (), training_args)
        self.percent_dense = a.percent_dense
        self.xyz_gradient_accum = torch.zeros((self._xyz.shape[0], 1), dtype=torch.float32, device=self.device)
        self.denom = torch.zeros((self._xyz.shape[0], 1), dtype=torch.float32, device=self.device)
        K = self._features.shape[1]
        groups = [
            {"params": [self._xyz], "lr": a.position_lr_init * self.spatial_lr_scale, "name": "xyz"},
            {"params": [self._features], "lr": a.feature_lr, "lr_rest": a.feature_lr / 20.0, "period": 3 * K if K > 1 else 0, "split": 3,
             "name": self.SH_GROUP},
            {"params": [self._opacity], "lr": a.opacity_lr, "name": "opacity"},
            {"params": [self._scaling], "lr": a.scaling_lr, "name": "scaling"},
            {"params": [self._rotation], "lr": a.rotation_lr, "name": "rotation"},
        ]
        self.optimizer = FusedAdam(groups, lr=0.0, eps=1e-15)
        self.xyz_scheduler_args = get_expon_lr_func(lr_init=a.position_lr_init * self.spatial_lr_scale,
                                                    lr_final=a.position_lr_final * self.spatial_lr_scale,
                                                    lr_delay_mult=a.position_lr_delay_mult, max_steps=a.position_lr_max_steps)

    def update_learning_rate(self, iteration):
        for g in self.optimizer.param_groups:
            if g["name"] == "xyz":
                lr = self.xyz_scheduler_args(iteration)
                g["lr"] = lr
                return lr

    def _group(self, name):
        return next(g for g in self.optimizer.param_groups if g["name"] == name)

    def _take_optimizer_params(self, params):
        for name, attr in self._PARAM_OF_GROUP.items():
            setattr(self, attr, params[name])
        self._reshare()

    # ---- shared SH storage with the joint buffer of renderer.bg_render
    def share_feature_storage(self, mesh_gaussians):
        """On the GPU: make `_features` a view of the leading rows of the joint [N + Nm, K, 3] SH buffer bg_render uses with
        `mesh_gaussians`, so no per-iteration concatenation of the SH rows is needed.  Kept across topology edits; the optimizer (if
        any) is pointed at the new leaf."""
        self._share_with = (mesh_gaussians,)
        self._reshare()

    def _reshare(self):
        if self._share_with is None or not self._features.is_cuda:
            return
        from .renderer import plain_joint_buffers
        jb = plain_joint_buffers(self, self._share_with[0])
        N = self._features.shape[0]
        if self._features.data_ptr() == jb["shs"].data_ptr() and self._features.shape == jb["shs"][:N].shape:
            return
        with torch.no_grad():
            jb["shs"][:N].copy_(self._features.detach())
        old = self._features
        self._features = torch.nn.Parameter(jb["shs"][:N], requires_grad=old.requires_grad)
        if old.grad is not None:
            self._features.grad = old.grad
        if self.optimizer is not None:
            self.optimizer.rebind(self.SH_GROUP, self._features)

    # ---- PLY / checkpoints
    def save_ply(self, path):
        """:226-244 through io.save_plain_gaussians (the reference's attribute order)."""
        import os
        if os.path.dirname(path):
            os.makedirs(os.path.dirname(path), exist_ok=True)
        n = lambda t: t.detach().cpu().numpy()
        gio.save_plain_gaussians(path, dict(xyz=n(self._xyz), features_dc=n(self._features_dc), features_rest=n(self._features_rest),
                                            opacity=n(self._opacity), scaling=n(self._scaling), rotation=n(self._rotation)))

    def load_ply(self, path):
        """:253-296: the model at its full SH degree."""
        import numpy as np
        m = gio.load_plain_gaussians(path, self.max_sh_degree)
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32)
        self._set_params(t(m["xyz"]), torch.cat([t(m["features_dc"]), t(m["features_rest"])], dim=1), t(m["scaling"]), t(m["rotation"]),
                         t(m["opacity"]).reshape(-1, 1))
        self.active_sh_degree = self.max_sh_degree

    def capture(self):
        """:64-78; the optimizer state is {group name: (exp_avg, exp_avg_sq)} plus the step count."""
        opt = None
        if self.optimizer is not None:
            opt = {"n_step": self.optimizer.n_step,
                   "state": {g["name"]: (g["m"][0].clone(), g["values"][0].clone()) for g in self.optimizer.param_groups}}
        return (self.active_sh_degree, self._xyz.detach().clone(), self._features_dc.detach().clone(), self._features_rest.detach().clone(),
                self._scaling.detach().clone(), self._rotation.detach().clone(), self._opacity.detach().clone(), self.max_radii2D.clone(),
                self.xyz_gradient_accum.clone(), self.denom.clone(), opt, self.spatial_lr_scale)

    def restore(self, model_args, training_args):
        """:80-94."""
        (self.active_sh_degree, xyz, f_dc, f_rest, scaling, rotation, opacity, max_radii2D, xyz_gradient_accum, denom, opt,
         self.spatial_lr_scale) = model_args
        self._set_params(xyz, torch.cat([f_dc, f_rest], dim=1), scaling, rotation, opacity)
        self.max_radii2D = max_radii2D.to(self.device).clone()
        self._reshare()
        self.training_setup(training_args)
        self.xyz_gradient_accum = xyz_gradient_accum.to(self.device).clone()
        self.denom = denom.to(self.device).clone()
        if opt is not None:
            self.optimizer.n_step = opt["n_step"]
            for g in self.optimizer.param_groups:
                m, v = opt["state"][g["name"]]
                g["m"][0], g["values"][0] = m.to(self.device).clone(), v.to(self.device).clone()

    # ---- topology edits (:298-404)
    def reset_opacity(self, keep_grad=False):
        """:246-251: opacity = inverse_sigmoid(min(opacity, 0.01)), both Adam moments of the group zeroed.  keep_grad: the new
        parameter takes over the old one's .grad (the reference's optimizer steps the replaced tensor with the gradient it holds)."""
        with torch.no_grad():
            new = inverse_sigmoid(torch.minimum(self.get_opacity, torch.ones_like(self.get_opacity) * 0.01))
        grad = self._opacity.grad
        self._opacity = self.optimizer.replace("opacity", new)["opacity"]
        if keep_grad and grad is not None:
            self._opacity.grad = grad

    def prune_points(self, mask, keep_grads=False):
        """:320-333: remove the rows where mask is True; parameters and both moments move together, statistics follow.
        keep_grads: the surviving rows keep their .grad (an optimizer step may still follow in this iteration)."""
        valid = mask.logical_not()
        grads = {}
        if keep_grads:
            grads = {g["name"]: g["params"][0].grad for g in self.optimizer.param_groups if g["params"][0].grad is not None}
        self._take_optimizer_params(self.optimizer.resize(keep=valid))
        for g in self.optimizer.param_groups:
            if g["name"] in grads:
                g["params"][0].grad = grads[g["name"]][valid].contiguous()
        self.xyz_gradient_accum = self.xyz_gradient_accum[valid]
        self.denom = self.denom[valid]
        self.max_radii2D = self.max_radii2D[valid]
        self.screenspace_points = torch.zeros((self._xyz.shape[0], 3), dtype=torch.float32, device=self.device, requires_grad=True)

    def densification_postfix(self, new_xyz, new_features, new_opacities, new_scaling, new_rotation):
        """:352-369 (new_features = cat(f_dc, f_rest)): rows appended with zero moments, all statistics reset to zero."""
        d = {"xyz": new_xyz, self.SH_GROUP: new_features, "opacity": new_opacities, "scaling": new_scaling, "rotation": new_rotation}
        self._take_optimizer_params(self.optimizer.resize(new_rows=d))
        self._reset_stats()

    def densify_and_split(self, grads, grad_threshold, scene_extent, N=2, samples=None, generator=None):
        """:371-393.  The gradient is zero-padded to the current row count (the clones appended by densify_and_clone are never split).
        The positions are R(q) s + xyz with s ~ Normal(0, get_scaling) per axis: s = get_scaling * samples, samples [N * n_selected, 3]
        standard normal - given, or drawn with torch.randn(generator=generator).  Rows: the selection repeated N times, block after block."""
        n_init = self._xyz.shape[0]
        padded = torch.zeros((n_init,), dtype=torch.float32, device=self.device)
        padded[:grads.shape[0]] = grads.squeeze()
        sel = torch.logical_and(padded >= grad_threshold, torch.max(self.get_scaling, dim=1).values > self.percent_dense * scene_extent)
        with torch.no_grad():
            stds = self.get_scaling[sel].repeat(N, 1)
            if samples is None:
                samples = torch.randn(stds.shape, generator=generator, dtype=torch.float32,
                                      device=generator.device if generator is not None else self.device).to(self.device)
            elif tuple(samples.shape) != tuple(stds.shape):
                raise ValueError("densify_and_split: samples must be %s, got %s" % (tuple(stds.shape), tuple(samples.shape)))
            s = stds * samples.to(self.device, torch.float32)
            rots = build_rotation(self._rotation[sel]).repeat(N, 1, 1)
            new_xyz = torch.bmm(rots, s.unsqueeze(-1)).squeeze(-1) + self.get_xyz[sel].repeat(N, 1)
            new_scaling = torch.log(self.get_scaling[sel].repeat(N, 1) / (0.8 * N))
            new_rotation = self._rotation[sel].repeat(N, 1)
            new_features = self._features[sel].repeat(N, 1, 1)
            new_opacity = self._opacity[sel].repeat(N, 1)
        self.densification_postfix(new_xyz, new_features, new_opacity, new_scaling, new_rotation)
        prune_filter = torch.cat([sel, torch.zeros((N * int(sel.sum().item()),), dtype=torch.bool, device=self.device)], dim=0)
        self.prune_points(prune_filter)

    def densify_and_clone(self, grads, grad_threshold, scene_extent):
        """:395-406."""
        sel = torch.logical_and(torch.linalg.vector_norm(grads, dim=-1) >= grad_threshold,
                                torch.max(self.get_scaling, dim=1).values <= self.percent_dense * scene_extent)
        with torch.no_grad():
            new = (self._xyz[sel], self._features[sel], self._opacity[sel], self._scaling[sel], self._rotation[sel])
        self.densification_postfix(*new)

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, samples=None, generator=None):
        """:408-421: clone, then split (which sees the clones with zero gradient), then prune on opacity - and, with max_screen_size,
        on screen and world size."""
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        self.densify_and_clone(grads, max_grad, extent)
        self.densify_and_split(grads, max_grad, extent, samples=samples, generator=generator)
        prune_mask = (self.get_opacity < min_opacity).squeeze(1)
        if max_screen_size:
            big_vs = self.max_radii2D > max_screen_size
            big_ws = self.get_scaling.max(dim=1).values > 0.1 * extent
            prune_mask = torch.logical_or(torch.logical_or(prune_mask, big_vs), big_ws)
        self.prune_points(prune_mask)

    def add_densification_stats(self, viewspace_point_tensor_grad, update_filter):
        """:423-427 (max_radii2D is the training loop's, train_bg_gaussian.py:141-146; on the GPU model_ops.densify_stats does both)."""
        f = update_filter[:self._xyz.shape[0]]
        self.xyz_gradient_accum[f] += torch.linalg.vector_norm(viewspace_point_tensor_grad[f, :2], dim=-1, keepdim=True)
        self.denom[f] += 1
