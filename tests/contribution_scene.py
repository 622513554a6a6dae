"""The scene of the mask-lifting tests: a torus of opaque Gaussians (THE OBJECT) inside a far shell of background Gaussians, seen from
views on two circles around it, and the torus's own rendered opacity per view (what a data set's masks are made of).

The lifting can only tell a background Gaussian from the object where some view sees it next to the object instead of through it, so
the shell keeps the candidates that have such a view: projected at least 8 pixels inside the frame, with no object opacity (< 0.01)
anywhere in the 17 x 17 pixels around - the far background has little parallax, the ones right behind the object stay behind it."""
import math

import numpy as np
import torch


def view_dicts(n_views, W, H, fovx_deg, radius=7.0, height=2.0):
    from gaussianmesh_amd import scenes
    return [scenes.look_at_camera((radius * math.cos(2 * math.pi * k / n_views), height * (1 if k % 2 else -1), radius * math.sin(2 * math.pi * k / n_views)),
                                  (0, 0, 0), W, H, fovx_deg=fovx_deg) for k in range(n_views)]


def render_alpha(pc, n, cam, W, H):
    """(colour [3,H,W], opacity [H,W]) of the first n rows of pc, on black"""
    from gaussianmesh_amd import rasterizer as R
    with torch.no_grad():
        h = R.rasterize_forward_begin(torch.zeros(3, device="cuda"), pc.get_xyz[:n].contiguous(), None, pc.get_opacity[:n].contiguous(),
                                      pc.get_scaling[:n].contiguous(), pc.get_rotation[:n].contiguous(), 1.0, None, cam.world_view_transform,
                                      cam.full_proj_transform, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), H, W,
                                      pc.get_features[:n].contiguous(), 3, cam.camera_center, aux=True)
        out = h.finish()
    return out[1], out[7][0]


def _plain(xyz, scaling, seed):
    from gaussianmesh_amd.bg_model import PlainGaussians, inverse_sigmoid
    P = len(xyz)
    rot = np.zeros((P, 4), np.float32); rot[:, 0] = 1.0
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32))
    pc = PlainGaussians(3, device="cuda")
    pc._set_params(t(xyz), t(np.random.default_rng(seed).normal(0, 0.3, size=(P, 16, 3))), t(scaling), t(rot), inverse_sigmoid(torch.full((P, 1), 0.95)))
    pc.active_sh_degree = 3
    return pc


def torus_in_shell(W, H, n_views, fovx_deg, nu, nv, obj_scale, candidates, shell_scale, seed=0):
    """Returns (pc, n_obj, cameras, alphas): a PlainGaussians whose first n_obj rows are the torus, renderer.Camera's, and the torus's
    opacity map per view, float32 [H,W]."""
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.renderer import Camera
    verts, _ = scenes.torus_mesh(nu, nv)
    n_obj = len(verts)
    dicts = view_dicts(n_views, W, H, fovx_deg)
    cams = [Camera(c, "cuda") for c in dicts]
    obj = _plain(verts, np.full((n_obj, 3), math.log(obj_scale)), seed)
    alphas = [render_alpha(obj, n_obj, cam, W, H)[1] for cam in cams]
    d = np.random.default_rng(seed + 1).normal(size=(candidates, 3))
    shell = 20.0 * d / np.linalg.norm(d, axis=1, keepdims=True)
    clear = np.zeros(candidates, bool)
    for c, a in zip(dicts, alphas):
        near = torch.nn.functional.max_pool2d(a[None, None], 17, 1, 8)[0, 0].cpu().numpy()
        ph = np.concatenate([shell, np.ones((candidates, 1))], 1) @ np.asarray(c["proj"], np.float64)
        w = np.maximum(ph[:, 3], 1e-9)
        px = np.rint(((ph[:, 0] / w + 1.0) * W - 1.0) * 0.5).astype(np.int64); py = np.rint(((ph[:, 1] / w + 1.0) * H - 1.0) * 0.5).astype(np.int64)
        ok = (ph[:, 3] > 0.2) & (px >= 8) & (px < W - 8) & (py >= 8) & (py < H - 8)
        ok[ok] = near[py[ok], px[ok]] < 0.01
        clear |= ok
    xyz = np.concatenate([verts, shell[clear]])
    scaling = np.concatenate([np.full((n_obj, 3), math.log(obj_scale)), np.full((int(clear.sum()), 3), math.log(shell_scale))])
    return _plain(xyz, scaling, seed), n_obj, cams, alphas
