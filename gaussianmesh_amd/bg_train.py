"""The background stage of the training pipeline, train_bg_gaussian.py:56-150, on this package's operators:

    bg_render(cam, bg model, mesh_gaussians=frozen object)  ->  loss = (1 - l) L1 + l (1 - SSIM)  ->  backward  ->  Adam step

BgTrainer drives a bg_model.PlainGaussians: the exponential position schedule, one SH degree more every 1000 iterations, an optional
random background colour, the densification statistics of the first N rows (one fused kernel), densify_and_prune every
`densification_interval` iterations past densify_from_iter (500: the value the reference's loop forces, train_bg_gaussian.py:142),
opacity resets, and the neighbour pruning that removes background Gaussians lying on the object (:129-137).  An iteration that
densifies takes no optimizer step (the reference's update_flag); its gradients are still dropped.
"""
from types import SimpleNamespace

import torch

from .loss import photometric_loss
from .renderer import bg_render
from .train import DEFAULT_OPT

# arguments/__init__.py OptimizationParams as train_bg_gaussian.py uses them: percent_dense and random_background besides the
# common ones; densification_interval as the loop sets it
BG_DEFAULT_OPT = dict(DEFAULT_OPT, percent_dense=0.01, random_background=False, densification_interval=500)


class BgTrainer:
    """gaussians: a PlainGaussians (its optimizer is made here, training_setup); mesh_gaussians: the frozen object cloud
    (renderer.MeshBoundGaussians or anything with get_xyz / get_scaling / get_rotation / get_opacity / get_features).

    Neighbour pruning (remove_neighbor_iterations, default [1000, 10000]): background rows whose nearest object Gaussian
    (simple_knn.knn_nearest) is closer than `min_distance` are removed.  The reference compares jittor.misc.knn's distance with
    0.01; the pytorch3d knn_points call it replaced returns SQUARED distances, and so - to our reading - does jittor.misc.knn.
    squared=True (default) therefore compares the squared distance with min_distance, i.e. prunes within sqrt(0.01) = 0.1;
    squared=False compares the Euclidean distance, pruning within 0.01.

    Order within one iteration: render, loss, backward, statistics, neighbour pruning, densification, opacity reset, optimizer step
    (skipped when the iteration densified), zero_grad.  The reference prunes neighbours before it takes the statistics, with the
    statistics' row filter of the pre-pruning cloud applied to the pruned one; here the statistics are taken first, on the rows they
    belong to, and follow the pruning.  Rows that survive a pruning or an opacity reset keep their gradient for this iteration's step,
    as the reference's optimizer does with the gradients it holds."""

    def __init__(self, gaussians, mesh_gaussians, spatial_lr_scale=1.0, extent=None, white_background=False, remove_neighbor_iterations=(1000, 10000),
                 min_distance=0.01, squared=True, generator=None, **opt):
        o = dict(BG_DEFAULT_OPT); o.update(opt)
        self.opt = SimpleNamespace(**o)
        self.g = gaussians
        self.mesh = mesh_gaussians
        self.extent = float(spatial_lr_scale if extent is None else extent)
        self.white_background = bool(white_background)
        self.remove_neighbor_iterations = set(int(i) for i in remove_neighbor_iterations)
        self.min_distance, self.squared = float(min_distance), bool(squared)
        self.generator = generator
        gaussians.spatial_lr_scale = spatial_lr_scale
        if gaussians._xyz.is_cuda and getattr(gaussians, "fused", True):
            gaussians.share_feature_storage(mesh_gaussians)       # before the optimizer captures the SH parameter
        gaussians.training_setup(self.opt)
        self.pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
        self.iteration = 0
        self.pruned_neighbors = 0

    def schedule(self, iteration):
        """What train_bg_gaussian.py:72-150 does at `iteration` (1-based) besides render / loss / backward."""
        o = self.opt
        before_until = iteration < o.densify_until_iter
        densify = before_until and iteration > o.densify_from_iter and iteration % o.densification_interval == 0
        return {"oneup": iteration % 1000 == 0, "stats": before_until, "neighbors": iteration in self.remove_neighbor_iterations,
                "densify": densify,
                "reset_opacity": before_until and (iteration % o.opacity_reset_interval == 0 or
                                                   (self.white_background and iteration == o.densify_from_iter)),
                "optimizer_step": iteration < o.iterations and not densify}

    def neighbor_mask(self):
        """Rows of the background cloud within min_distance of the object's Gaussians (see the class docstring for `squared`)."""
        from .simple_knn import knn_nearest
        d2, _ = knn_nearest(self.g.get_xyz.detach(), self.mesh.get_xyz.detach())
        return (d2 if self.squared else torch.sqrt(d2)) < self.min_distance

    def remove_neighbors(self, keep_grads=True):
        mask = self.neighbor_mask()
        self.pruned_neighbors += int(mask.sum().item())
        self.g.prune_points(mask, keep_grads=keep_grads)
        return mask

    def step(self, camera, gt_image, background):
        """One iteration of the loop, schedule included.  Returns (loss, render package, plan); plan["rows"] = rows afterwards."""
        g, o = self.g, self.opt
        it = self.iteration + 1
        plan = self.schedule(it)
        g.update_learning_rate(it)
        if plan["oneup"]:
            g.oneupSHdegree()
        bg = torch.rand((3,), generator=self.generator, device=background.device) if o.random_background else background
        pkg = bg_render(camera, g, self.pipe, bg, mesh_gaussians=self.mesh)
        loss = photometric_loss(pkg["render"], gt_image, o.lambda_dssim)
        loss.backward()
        N = g._xyz.shape[0]
        if plan["stats"]:
            vg = g.screenspace_points.grad
            if vg is None:
                vg = torch.zeros((N, 3), dtype=torch.float32, device=g.device)
            if g._xyz.is_cuda:
                from .model_ops import densify_stats
                densify_stats(pkg["radii"][:N], vg, g.max_radii2D, g.xyz_gradient_accum, g.denom)
            else:
                vis = pkg["visibility_filter"][:N]
                g.max_radii2D[vis] = torch.maximum(g.max_radii2D[vis], pkg["radii"][:N][vis].float())
                g.add_densification_stats(vg, vis)
        if plan["neighbors"]:
            self.remove_neighbors(keep_grads=plan["optimizer_step"])
        if plan["densify"]:
            g.densify_and_prune(o.densify_grad_threshold, 0.005, self.extent, None, generator=self.generator)
        if plan["reset_opacity"]:
            g.reset_opacity(keep_grad=plan["optimizer_step"])
        if plan["optimizer_step"]:
            g.optimizer.step()
        g.optimizer.zero_grad(set_to_none=True)
        self.iteration = it
        plan["rows"] = g._xyz.shape[0]
        return loss.detach(), pkg, plan
