"""GPU: the background stage - gm_plain_activate_fwd / _bwd, gm_knn_nearest, bg_render's fused route for bg_model.PlainGaussians and
bg_train.BgTrainer - against float64 autograd, a float32 brute force, the generic torch route of bg_render, and a hand-written torch
training loop."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, NM, W, H = 1500, 900, 160, 112


def _rel(a, b):
    a = torch.as_tensor(a).double(); b = torch.as_tensor(b).double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


# ---------------------------------------------------------------------------------------------------------------- activation
@pytest.mark.parametrize("joint", [False, True])
def test_plain_activate_matches_float64_autograd(joint):
    from gaussianmesh_amd.model_ops import plain_activate
    import plain_activate_ref as P
    n, extra = 5000, 37
    # near-zero quaternions above the clamp (rows 0-6), one at it and one below it (7, 8), |opacity| > 20 (rows 0-19): drawn by
    # plain_activate_ref.present_test_inputs, which test_plain_activate_ref_host.py reads too
    xyz, scaling, rot, opac, ups = P.present_test_inputs(extra if joint else 0)
    leaves = [t.cuda().requires_grad_(True) for t in (xyz, scaling, rot, opac)]
    ref = [t.detach().double().requires_grad_(True) for t in (xyz, scaling, rot, opac)]
    jb = None
    if joint:
        f = dict(dtype=torch.float32, device="cuda")
        jb = {"xyz": torch.full((n + extra, 3), 7.0, **f), "scales": torch.full((n + extra, 3), 7.0, **f),
              "rots": torch.full((n + extra, 4), 7.0, **f), "opac": torch.full((n + extra, 1), 7.0, **f)}
    out = plain_activate(*leaves, joint=jb)
    want = (ref[0], torch.exp(ref[1]), torch.nn.functional.normalize(ref[2]), torch.sigmoid(ref[3]))
    for o, w in zip(out, want):
        got = o[:n] if joint else o
        assert _rel(got.detach().cpu(), w.detach()) <= 1e-6
        if joint:
            assert torch.equal(o[n:], torch.full_like(o[n:], 7.0))   # the tail is never written
    # element-wise too, for the opacities at |x| > 20 (a normwise error would hide them)
    assert (((out[3][:n] if joint else out[3]).detach().cpu().double() - want[3].detach()).abs() / want[3].detach()).max() <= 1e-6
    assert [tuple(u.shape) for u in ups] == [tuple(o.shape) for o in out]
    ups = [u.cuda() for u in ups]
    sum(((o * u).sum() for o, u in zip(out, ups))).backward()
    sum(((w * u[:n].cpu().double()).sum() for w, u in zip(want, ups))).backward()
    for lf, rf in zip(leaves, ref):
        assert _rel(lf.grad.cpu(), rf.grad) <= 1e-5
    # d opacity where |x| > 20 (x = linspace(-30, 30, 20) in the first rows): element-wise against e / (1 + e)^2, e = exp(-x), for
    # x < -20; for x > 20 the float32 s (1 - s) of torch / Jittor - at most an ulp of s, 0 once s rounds to 1 - as in the loop it replaces
    x64 = ref[3].detach()[:20, 0]
    g64 = ups[3][:20, 0].cpu().double()
    got = leaves[3].grad[:20, 0].cpu().double()
    lo, hi = x64 < -20, x64 > 20
    e = torch.exp(x64[lo])
    want_lo = g64[lo] * e / (1 + e) ** 2
    assert ((got[lo] - want_lo).abs() <= 1e-5 * want_lo.abs()).all()
    assert (got[hi].abs() <= 1.2e-7 * g64[hi].abs()).all()
    # every element of every tensor against float64 (plain_activate_ref.py): the rotation gradient's max-norm is 1.2e12 (row 8, under the
    # clamp), so the norm-wise figures above hold the ordinary rows to ~1e7 absolute - test_plain_activate_ref_host.py shows what passes them
    a = [t.numpy() for t in (xyz, scaling, rot, opac)]
    u = [t[:n].cpu().numpy() for t in ups]
    ref64, s_abs = P.reference(*a, *u)
    dev = {t: (o[:n] if joint else o).detach().cpu().numpy() for t, o in zip(P.FWD, out)}
    dev.update({t: lf.grad.cpu().numpy().reshape(n, -1) for t, lf in zip(P.BWD, leaves)})
    fig = P.check(dev, ref64, s_abs, a[3], u[3])
    print("plain_activate, the 5000 rows of this test, worst ratio / bar: " + P.table(fig))
    assert not P.failures(fig), P.failures(fig)


def test_plain_activate_null_gradients_are_zero():
    from gaussianmesh_amd.model_ops import plain_activate
    t = [torch.randn(100, k, device="cuda", requires_grad=True) for k in (3, 3, 4, 1)]
    out = plain_activate(*t)
    out[1].sum().backward()                                       # only the scales get a gradient
    assert torch.equal(t[0].grad, torch.zeros_like(t[0])) and torch.equal(t[2].grad, torch.zeros_like(t[2]))
    assert torch.equal(t[3].grad, torch.zeros_like(t[3]))
    assert torch.allclose(t[1].grad, torch.exp(t[1].detach()), rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------------- knn
def _brute_np(q, r):
    q = q.astype(np.float32); r = r.astype(np.float32)
    dx = q[:, None, 0] - r[None, :, 0]; dy = q[:, None, 1] - r[None, :, 1]; dz = q[:, None, 2] - r[None, :, 2]
    d2 = (dx * dx + dy * dy) + dz * dz                            # numpy: one rounding per operation, no contraction
    i = np.argmin(d2, axis=1)                                     # first (lowest) index of the minimum
    return d2[np.arange(len(q)), i], i


def _brute_torch(q, r, chunk=512):
    """the same float32 brute force on the device (eager elementwise ops, one rounding each; argmin's first minimum)"""
    d_out, i_out = [], []
    for s in range(0, q.shape[0], chunk):
        a = q[s:s + chunk]
        dx = a[:, None, 0] - r[None, :, 0]; dy = a[:, None, 1] - r[None, :, 1]; dz = a[:, None, 2] - r[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        v, i = d2.min(dim=1)
        i2 = torch.argmin(d2, dim=1)
        assert torch.equal(i, i2) or torch.equal(d2.gather(1, i[:, None]), d2.gather(1, i2[:, None]))
        d_out.append(v); i_out.append(i2)
    return torch.cat(d_out), torch.cat(i_out)


@pytest.mark.parametrize("Pq, Pr, dup", [(1, 1, False), (1, 50, False), (50, 1, False), (300, 2000, False), (777, 333, False),
                                         (1000, 1000, True), (4097, 1025, True), (2000, 70000, False)])
def test_knn_nearest_bit_identical_to_brute_force(Pq, Pr, dup):
    from gaussianmesh_amd.simple_knn import knn_nearest
    rng = np.random.default_rng(Pq * 7 + Pr)
    r = (rng.normal(size=(Pr, 3)) * 2).astype(np.float32)
    q = (rng.normal(size=(Pq, 3)) * 2.5).astype(np.float32)
    if dup:                                                       # duplicate reference points (ties) and queries ON them
        r[Pr // 2:] = r[:Pr - Pr // 2]
        q[: min(Pq, Pr) // 3] = r[: min(Pq, Pr) // 3]
        r[:5] = np.round(r[:5])                                   # and integer points equidistant from integer queries
        q[-5:] = np.round(q[-5:]) + 0.5
    d2, idx = knn_nearest(torch.as_tensor(q).cuda(), torch.as_tensor(r).cuda())
    wd, wi = _brute_np(q, r)
    assert np.array_equal(idx.cpu().numpy(), wi)
    assert np.array_equal(d2.cpu().numpy().view(np.uint32), wd.astype(np.float32).view(np.uint32))


def test_knn_nearest_large_bit_identical():
    """about 200 k x 60 k: against the float32 brute force on the device"""
    from gaussianmesh_amd.simple_knn import knn_nearest
    g = torch.Generator(device="cuda").manual_seed(5)
    r = torch.randn(60000, 3, device="cuda", generator=g) * torch.tensor([2.0, 1.0, 0.5], device="cuda")
    q = torch.randn(200003, 3, device="cuda", generator=g) * 3
    q[:1000] = r[:1000]                                           # exact hits
    d2, idx = knn_nearest(q, r)
    wd, wi = _brute_torch(q, r)
    assert torch.equal(idx, wi)
    assert torch.equal(d2.view(torch.int32), wd.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- scenes
def _camera(k=1, K=6, w=W, h=H, radius=6.5):
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.renderer import Camera
    return Camera(scenes.orbit_camera(k, K, w, h, radius=radius), "cuda")


def _mesh_model(n=NM, seed=3):
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.renderer import MeshBoundGaussians
    T = lambda a: torch.as_tensor(np.asarray(a, np.float32), device="cuda")     # (on the device from the start: screenspace_points too)
    verts, faces = scenes.torus_mesh(24, 16)
    rng = np.random.default_rng(seed)
    cl = scenes.bind_cloud_to_mesh(n, verts, faces, seed=2)
    tri = faces[cl["fid"]]
    v1, v2, v3 = (verts[tri[:, k]].astype(np.float32) for k in range(3))
    nr = np.cross(v2 - v1, v3 - v1); nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    r = ((np.linalg.norm(v2 - v1, axis=1) + np.linalg.norm(v3 - v2, axis=1) + np.linalg.norm(v1 - v3, axis=1)) / 3)[:, None]
    return MeshBoundGaussians(T(rng.normal(size=(n, 3))), T(rng.normal(0, 0.3, size=(n, 1))), T(cl["shs"][:, :1]), T(cl["shs"][:, 1:]),
                              T(np.log(cl["scales"] * 6)), T(cl["rots"]), T(rng.normal(size=(n, 1))), T(v1), T(v2), T(v3), T(nr), T(r))


def _plain(n=N, seed=9, fused=True, sh_degree=3):
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.bg_model import PlainGaussians
    b = scenes.make_cloud(n, seed=seed, scale_lo=0.05, scale_hi=0.3)
    nb = np.linalg.norm(b["means"], axis=1, keepdims=True) + 1e-6
    b["means"] = (b["means"] / nb * (3.0 + nb)).astype(np.float32)
    g = PlainGaussians(3, device="cuda")
    T = lambda a: torch.as_tensor(np.asarray(a, np.float32))
    g._set_params(T(b["means"]), T(b["shs"]), torch.log(T(b["scales"])), T(b["rots"]) * 1.7, torch.logit(T(b["opac"])).reshape(-1, 1))
    g.active_sh_degree = sh_degree
    g.fused = fused
    return g


def _clone_plain(src, fused):
    from gaussianmesh_amd.bg_model import PlainGaussians
    g = PlainGaussians(src.max_sh_degree, device="cuda")
    g._set_params(src._xyz, src._features, src._scaling, src._rotation, src._opacity)
    g.active_sh_degree, g.fused = src.active_sh_degree, fused
    return g


PIPE = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("aux", [False, True])
def test_bg_render_fused_route_matches_generic_route(shared, aux):
    from gaussianmesh_amd.renderer import bg_render
    mesh = _mesh_model()
    a = _plain(fused=True)
    b = _clone_plain(a, fused=False)
    if shared:
        a.share_feature_storage(mesh)
    cam = _camera()
    bg = torch.tensor([0.1, 0.2, 0.3], device="cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    up = torch.randn((3, H, W), device="cuda", generator=g)
    outs = []
    for m in (a, b):
        for _ in range(2):                                        # (a second call: the joint buffers are reused)
            pkg = bg_render(cam, m, PIPE, bg, mesh_gaussians=mesh, return_aux=aux)
            loss = (pkg["render"] * up).sum() + ((pkg["depth"] * 0.1).sum() + pkg["alpha"].sum() if aux else 0.0)
            for p in (m._xyz, m._features, m._scaling, m._rotation, m._opacity):
                p.grad = None
            m.screenspace_points.grad = None
            loss.backward()
        outs.append(pkg)
    pa, pb = outs
    assert hasattr(a, "_plain_joint") and not hasattr(b, "_plain_joint")
    assert pa["radii"].shape[0] == N + NM and torch.equal(pa["radii"], pb["radii"])
    assert (pa["render"] - pb["render"]).abs().max().item() <= 1e-5
    if aux:
        assert _rel(pa["depth"].detach().cpu(), pb["depth"].detach().cpu()) <= 1e-5
        assert (pa["alpha"] - pb["alpha"]).abs().max().item() <= 1e-5
    for name in ("_xyz", "_features", "_scaling", "_rotation", "_opacity"):
        ga, gb = getattr(a, name).grad, getattr(b, name).grad
        assert ga is not None and ga.shape == gb.shape, name
        assert _rel(ga.cpu(), gb.cpu()) <= 1e-4, (name, _rel(ga.cpu(), gb.cpu()))
    # the probe: pc.screenspace_points.grad = the first N rows of the joint probe's gradient, as on the generic route
    assert a.screenspace_points.grad is not None and a.screenspace_points.grad.shape == (N, 3)
    assert torch.equal(a.screenspace_points.grad, pa["viewspace_points"].grad[:N])
    assert _rel(a.screenspace_points.grad.cpu(), b.screenspace_points.grad.cpu()) <= 1e-4
    if shared:
        assert a._features.data_ptr() == a._plain_joint["shs"].data_ptr()


# ---------------------------------------------------------------------------------------------------------------- trainer
def _targets(cams, mesh, n=N):
    """renders of a TARGET cloud (a different draw of the shell) with the object composited: the images the background is fit to"""
    from gaussianmesh_amd.renderer import bg_render
    tgt = _plain(n, seed=21)
    bg = torch.zeros(3, device="cuda")
    with torch.no_grad():
        return [bg_render(c, tgt, PIPE, bg, mesh_gaussians=mesh)["render"].detach().clone() for c in cams]


class _TorchModel:
    """the plain model as separate torch leaves (f_dc and f_rest apart, as the reference's groups) for bg_render's generic route"""

    def __init__(self, src):
        c = lambda t: t.detach().clone().requires_grad_(True)
        self._xyz, self._scaling, self._rotation, self._opacity = c(src._xyz), c(src._scaling), c(src._rotation), c(src._opacity)
        self._features_dc, self._features_rest = c(src._features[:, :1]), c(src._features[:, 1:])
        self.active_sh_degree, self.max_sh_degree = src.active_sh_degree, src.max_sh_degree
        self.screenspace_points = torch.zeros_like(self._xyz, requires_grad=True)

    get_xyz = property(lambda s: s._xyz)
    get_scaling = property(lambda s: torch.exp(s._scaling))
    get_rotation = property(lambda s: torch.nn.functional.normalize(s._rotation))
    get_opacity = property(lambda s: torch.sigmoid(s._opacity))
    get_features = property(lambda s: torch.cat([s._features_dc, s._features_rest], dim=1))


def test_bg_trainer_matches_torch_loop():
    from gaussianmesh_amd.bg_train import BgTrainer
    from gaussianmesh_amd.loss import photometric_loss
    from gaussianmesh_amd.renderer import bg_render
    from gaussianmesh_amd.train import get_expon_lr_func
    mesh = _mesh_model()
    cams = [_camera(k, 6) for k in range(3)]
    gts = _targets(cams, mesh)
    model = _plain(seed=9, sh_degree=0)
    ref = _TorchModel(model)
    tr = BgTrainer(model, mesh, remove_neighbor_iterations=())
    o = tr.opt
    opt = torch.optim.Adam([{"params": [ref._xyz], "lr": o.position_lr_init, "name": "xyz"},
                            {"params": [ref._features_dc], "lr": o.feature_lr}, {"params": [ref._features_rest], "lr": o.feature_lr / 20.0},
                            {"params": [ref._opacity], "lr": o.opacity_lr}, {"params": [ref._scaling], "lr": o.scaling_lr},
                            {"params": [ref._rotation], "lr": o.rotation_lr}], lr=0.0, eps=1e-15)
    sched = get_expon_lr_func(o.position_lr_init, o.position_lr_final, lr_delay_mult=o.position_lr_delay_mult, max_steps=o.position_lr_max_steps)
    bg = torch.zeros(3, device="cuda")
    tiny = {t: torch.zeros_like(t, dtype=torch.bool) for t in (ref._xyz, ref._features_dc, ref._features_rest, ref._opacity, ref._scaling,
                                                                ref._rotation)}
    for it in range(1, 21):
        cam, gt = cams[it % 3], gts[it % 3]
        loss_a, _, plan = tr.step(cam, gt, bg)
        assert not plan["densify"] and plan["optimizer_step"]
        opt.param_groups[0]["lr"] = sched(it)
        ref.screenspace_points.grad = None
        loss_b = photometric_loss(bg_render(cam, ref, PIPE, bg, mesh_gaussians=mesh)["render"], gt, o.lambda_dssim)
        loss_b.backward()
        for t in tiny:
            tiny[t] |= (t.grad != 0) & (t.grad.abs() < 1e-11)
        opt.step(); opt.zero_grad()
        assert abs(loss_a.item() - loss_b.item()) <= 1e-5 * abs(loss_b.item())
    pairs = [(model._xyz, ref._xyz), (model._features[:, :1], ref._features_dc), (model._features[:, 1:], ref._features_rest),
             (model._opacity, ref._opacity), (model._scaling, ref._scaling), (model._rotation, ref._rotation)]
    # Jittor's Adam (FusedAdam, the reference's rule) adds eps to sqrt(v) BEFORE the bias correction, torch.optim.Adam after it: for a
    # gradient near eps (1e-15) the two take different steps.  Elements that ever had 0 < |g| < 1e-11 are left out (eps / sqrt(1 - b2^t) is 3e-14 at step 1).
    for a, b in pairs:
        keep = ~tiny[b]
        assert keep.float().mean().item() > 0.95
        # norm-wise: an element whose gradient is at the noise level of the float32 backward can change sign between two routes
        ka, kb = a.detach()[keep].double(), b.detach()[keep].double()
        assert float((ka - kb).norm() / kb.norm()) <= 1e-4
    assert model.optimizer.n_step == 20


def test_bg_trainer_short_schedule(tmp_path):
    from gaussianmesh_amd.bg_train import BgTrainer
    from gaussianmesh_amd.edittool import SceneVisualTool
    from gaussianmesh_amd.simple_knn import knn_nearest
    mesh = _mesh_model()
    cams = [_camera(k, 6) for k in range(6)]
    gts = _targets(cams, mesh)
    model = _plain(seed=9)
    with torch.no_grad():                                         # perturb, and put some background rows ON the object
        model._xyz.add_(torch.randn_like(model._xyz) * 0.05)
        model._xyz[:40].copy_(mesh.get_xyz[:40] + 0.01)
        model._opacity.add_(torch.randn_like(model._opacity) * 0.5)
    model.active_sh_degree = 0
    gen = torch.Generator(device="cuda").manual_seed(3)
    tr = BgTrainer(model, mesh, remove_neighbor_iterations=[30], generator=gen, densify_from_iter=10, densification_interval=20,
                   opacity_reset_interval=60, densify_grad_threshold=2e-5, iterations=100)
    bg = torch.zeros(3, device="cuda")
    losses, densified = [], 0
    for it in range(1, 101):
        n_step = model.optimizer.n_step
        loss, pkg, plan = tr.step(cams[it % 6], gts[it % 6], bg)
        losses.append(loss.item())
        n = model._xyz.shape[0]
        assert plan["rows"] == n
        if plan["densify"]:                                        # no Adam step on a densifying iteration (update_flag)
            densified += 1
            assert model.optimizer.n_step == n_step
        elif it < 100:
            assert model.optimizer.n_step == n_step + 1
        for grp in model.optimizer.param_groups:
            assert grp["params"][0].shape[0] == n and grp["m"][0].shape[0] == n and grp["values"][0].shape[0] == n
            assert grp["params"][0].grad is None
        assert model.max_radii2D.shape == (n,) and model.xyz_gradient_accum.shape == (n, 1) and model.denom.shape == (n, 1)
        assert model.screenspace_points.shape == (n, 3)
        assert model._features.data_ptr() == model._plain_joint["shs"].data_ptr()
        if it == 30:                                               # neighbour pruning: nothing within sqrt(0.01) = 0.1 survives
            assert tr.pruned_neighbors > 0
            d2, _ = knn_nearest(model._xyz.detach(), mesh.get_xyz.detach())
            assert d2.min().item() >= (0.1 - 2e-3) ** 2           # (this iteration's Adam step moved the survivors by < 1e-3)
        if it == 60:
            assert plan["reset_opacity"]
            assert model.get_opacity.max().item() <= 0.0100001
    assert densified == 5                                          # iterations 20, 40, 60, 80, 100
    assert model.optimizer.param_groups[0]["params"][0] is model._xyz
    jb = model._plain_joint
    assert jb["N"] == model._xyz.shape[0] and jb["xyz"].shape[0] == model._xyz.shape[0] + NM
    assert np.mean(losses[-10:]) < np.mean(losses[:10])
    path = str(tmp_path / "bg" / "point_cloud.ply")
    model.save_ply(path)
    tool = SceneVisualTool(path, device="cuda")
    assert tool.bg_mean3D.shape[0] == model._xyz.shape[0]
    img = tool.render_gaussian(cams[0])
    assert img.shape == (3, H, W) and torch.isfinite(img).all() and (img < 0.999).any()
