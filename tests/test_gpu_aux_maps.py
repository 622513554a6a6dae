"""-m gpu: the depth and opacity maps of the blend (gm_forward_1_aux / gm_backward_aux, aux= / return_aux= in python).

  alpha = 1 - T_final            (the oracle: T_final is the difference of two renders with background 0 and 1)
  depth = sum alpha_i T_i z_i    (the oracle: a render with colors_precomp = view-space z, background 0)
Gradients against oracle/torch_dense.py (float64 autograd), where depth and alpha are renders with colour z and 1 on background 0.
The AUX instantiations must not move anything else: image, radii, instance count, lists and ranges bit for bit with and without them.
"""
import numpy as np
import pytest
import torch

from helpers import assert_grads_elementwise, fuzz_scene, small_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_emission_policy():
    from gaussianmesh_amd import rasterizer as R
    yield
    R.set_default_emission_policy("auto")


def _view_z(sc, cam):
    """p_view.z in float32 (transposed view matrix, as the preprocess)"""
    v = np.asarray(cam["view"], np.float32).reshape(4, 4)
    m = sc["means"].astype(np.float32)
    return (m[:, 0] * v[0, 2] + m[:, 1] * v[1, 2] + m[:, 2] * v[2, 2] + v[3, 2]).astype(np.float32)


def _gpu_frame(sc, cam, bg, D, policy, exact=False, image_only=False, sync_free=False, aux=True, pre_cov=False, pre_col=False, ws=None):
    from gpu_utils import T
    from gaussianmesh_amd import rasterizer as R
    H, W = cam["H"], cam["W"]
    h = R.rasterize_forward_begin(T(bg), T(sc["means"]), T(sc["colors_precomp"]) if pre_col else None, T(sc["opac"]),
                                  None if pre_cov else T(sc["scales"]), None if pre_cov else T(sc["rots"]), 1.0,
                                  T(sc["cov3D_precomp"]) if pre_cov else None, T(cam["view"]), T(cam["proj"]), cam["tanx"], cam["tany"],
                                  H, W, None if pre_col else T(sc["shs"]), D, T(cam["campos"]), workspace=ws, emission_policy=policy, aux=aux)
    if sync_free:
        out = h.finish(sync_free=True, capacity=4 * 1024 * 1024 if ws is None else 0, image_only=image_only)
        ok, nr = h.check()
        assert ok
        out = (nr,) + tuple(out[1:])
    else:
        out = h.finish(image_only=image_only, exact_exponent=exact)
    torch.cuda.synchronize()
    return out


def _reference_maps(oracle, sc, cam, D, pre_cov=False, pre_col=False):
    z0, z1 = np.zeros(3, np.float32), np.ones(3, np.float32)
    kw = dict(D=D, use_precomp_cov=pre_cov, use_precomp_color=pre_col)
    f0 = oracle.forward_full(sc, cam, z0, **kw)
    f1 = oracle.forward_full(sc, cam, z1, **kw)
    alpha = 1.0 - (f1["color"][0].astype(np.float64) - f0["color"][0])
    scz = dict(sc)
    scz["colors_precomp"] = np.repeat(_view_z(sc, cam)[:, None], 3, axis=1)
    fz = oracle.forward_full(scz, cam, z0, D=D, use_precomp_cov=pre_cov, use_precomp_color=True)
    return alpha, fz["color"][0].astype(np.float64), float(np.abs(scz["colors_precomp"][f0["geo"]["radii"] > 0]).max(initial=1.0))


def _gate(got, ref, tol, what):
    """per-pixel gate with room for a decision flip or two (an entry at alpha = 1/255 or T = 1e-4): the 1e-4 colour gate's shape"""
    err = np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref)
    n = int((err > tol).sum())
    print("%-28s max %.3g, %d pixel(s) above %.3g" % (what, err.max(), n, tol))
    assert n <= max(2, int(1e-3 * ref.size)), (what, n)
    return err


def _image_field(img, W, H, name, count, dtype):
    from gaussianmesh_amd import _lib
    from gpu_utils import _view
    return _view(img, _lib.lib().gm_image_field(img.data_ptr(), W, H, name.encode()), count, dtype)


SCENES = {
    "small": lambda: small_scene(P=1500, W=96, H=72, seed=3, D=3, scale_lo=0.05, scale_hi=0.4) + (np.array([0.2, 0.4, 0.6], np.float32), 3, False, False),
    "fuzz7": lambda: fuzz_scene(7)[:6],
    "fuzz10": lambda: fuzz_scene(10)[:6],
}


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("policy", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["small", "fuzz7", "fuzz10"])
def test_alpha_and_depth_maps_vs_oracle(oracle, name, policy, exact):
    sc, cam, bg, D, pre_cov, pre_col = SCENES[name]()
    W, H = cam["W"], cam["H"]
    alpha_ref, depth_ref, zmax = _reference_maps(oracle, sc, cam, D, pre_cov, pre_col)
    nr, color, radii, geom, binning, img, depth, alpha = _gpu_frame(sc, cam, bg, D, policy, exact=exact, pre_cov=pre_cov, pre_col=pre_col)
    assert depth.shape == (1, H, W) and alpha.shape == (1, H, W)
    a, d = alpha.cpu().numpy()[0], depth.cpu().numpy()[0]
    assert np.isfinite(a).all() and np.isfinite(d).all()
    _gate(a, alpha_ref, 1e-4, "alpha %s p%d e%d" % (name, policy, exact))
    _gate(d, depth_ref, 1e-4 * zmax, "depth %s p%d e%d" % (name, policy, exact))
    # a frame that keeps its state: alpha is 1 - final_T bit for bit
    fT = _image_field(img, W, H, "final_T", W * H, torch.float32).reshape(H, W)
    assert np.array_equal(a, (np.float32(1.0) - fT).astype(np.float32))


def test_alpha_and_depth_maps_vs_oracle_c2_size(oracle):
    """the C2-size scene of test_gpu_fullsize.py (100 k Gaussians, 640 x 360)"""
    from gaussianmesh_amd import scenes
    sc = scenes.make_cloud(100_000, seed=3, scale_lo=0.005, scale_hi=0.06)
    cam = scenes.orbit_camera(5, 16, 640, 360)
    bg = np.array([0.3, 0.3, 0.3], np.float32)
    alpha_ref, depth_ref, zmax = _reference_maps(oracle, sc, cam, 3)
    for policy in (2, 3):
        *_, img, depth, alpha = _gpu_frame(sc, cam, bg, 3, policy, exact=True)
        _gate(alpha.cpu().numpy()[0], alpha_ref, 1e-4, "alpha C2 p%d" % policy)
        _gate(depth.cpu().numpy()[0], depth_ref, 1e-4 * zmax, "depth C2 p%d" % policy)


@pytest.mark.parametrize("policy", [0, 1, 2, 3])
def test_aux_moves_nothing_else(policy):
    """aux on and off: image, radii, instance count, lists and ranges bit for bit, image-only and sync-free frames included"""
    from gaussianmesh_amd import _lib, rasterizer as R
    from gpu_utils import _view
    sc, cam = small_scene(P=4000, W=200, H=120, seed=21, D=3, scale_lo=0.03, scale_hi=0.3)
    bg = np.array([0.5, 0.1, 0.8], np.float32)
    W, H = cam["W"], cam["H"]
    for image_only in (False, True):
        for sync_free in (False, True):
            outs = [_gpu_frame(sc, cam, bg, 3, policy, image_only=image_only, sync_free=sync_free, aux=aux) for aux in (False, True)]
            (nr0, c0, r0, g0, b0, i0), (nr1, c1, r1, g1, b1, i1, d1, a1) = outs
            assert nr0 == nr1 and torch.equal(c0, c1) and torch.equal(r0, r1), (image_only, sync_free)
            if not sync_free:
                pairs = [_view(b, _lib.lib().gm_binning_field(b.data_ptr(), nr0, W, H, policy, b"pairs"), 2 * nr0, torch.int32) for b in (b0, b1)]
                assert np.array_equal(pairs[0], pairs[1])
            if not image_only:
                for f in ("final_T", "n_contrib"):
                    assert np.array_equal(_image_field(i0, W, H, f, W * H, torch.int32), _image_field(i1, W, H, f, W * H, torch.int32))
    # ranges of the two frames
    nrs = [_gpu_frame(sc, cam, bg, 3, policy, aux=aux) for aux in (False, True)]
    sh_ = max(policy - 1, 0)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    tiles = ((gx + (1 << sh_) - 1) >> sh_) * ((gy + (1 << sh_) - 1) >> sh_)
    rg = [_image_field(o[5], W, H, "ranges", 2 * tiles, torch.int32) for o in nrs]
    assert np.array_equal(rg[0], rg[1])


def _dense_reference(sc, cam, bg, D, pre, gC, gD, gA):
    from oracle import torch_dense as td
    t64 = lambda a, rg=False: torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=rg)
    means, opac = t64(sc["means"], True), t64(sc["opac"], True)
    m2d = torch.zeros(means.shape[0], 3, dtype=torch.float64, requires_grad=True)
    if pre:
        ref_in = dict(colors_precomp=t64(sc["colors_precomp"], True), cov3D_precomp=t64(sc["cov3D_precomp"], True))
        geo = dict(cov3D_precomp=ref_in["cov3D_precomp"])
    else:
        ref_in = dict(shs=t64(sc["shs"], True), scales=t64(sc["scales"], True), rots=t64(sc["rots"], True))
        geo = dict(scales=ref_in["scales"], rots=ref_in["rots"])
    view = t64(cam["view"])
    common = (opac, view, t64(cam["proj"]), t64(cam["campos"]), cam["W"], cam["H"], cam["tanx"], cam["tany"])
    color, aux = td.render(means, *common, t64(bg), D=D, means2D=m2d, **ref_in)
    ph = torch.cat([means, torch.ones(means.shape[0], 1, dtype=torch.float64)], 1)
    z = (ph @ view.reshape(4, 4))[:, 2:3].expand(-1, 3)
    zero = torch.zeros(3, dtype=torch.float64)
    depth, _ = td.render(means, *common, zero, D=D, means2D=m2d, colors_precomp=z, **geo)
    alpha, _ = td.render(means, *common, zero, D=D, means2D=m2d, colors_precomp=torch.ones_like(z), **geo)
    loss = (color * t64(gC)).sum() + (depth[0] * t64(gD)).sum() + (alpha[0] * t64(gA)).sum()
    loss.backward()
    out = dict(means=means.grad, opac=opac.grad.reshape(-1), m2d=m2d.grad[:, :2])
    out.update({k: v.grad for k, v in ref_in.items()})
    return out, color.detach(), aux


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("terms", ["all", "maps_only", "depth_only"])
def test_map_gradients_vs_dense_autograd(pre, terms):
    from gpu_utils import T, settings
    from gaussianmesh_amd import GaussianRasterizer
    D = 3
    sc, cam = small_scene(P=2000, W=112, H=80, seed=9, D=D, scale_lo=0.05, scale_hi=0.35)
    bg = np.array([0.2, 0.5, 0.9], np.float32)
    W, H = cam["W"], cam["H"]
    rng = np.random.default_rng(4)
    gC = rng.normal(size=(3, H, W)).astype(np.float32) * (0.0 if terms != "all" else 1.0)
    gD = rng.normal(size=(H, W)).astype(np.float32) * 0.2
    gA = rng.normal(size=(H, W)).astype(np.float32) * (0.0 if terms == "depth_only" else 1.0)
    ref, ref_color, ref_aux = _dense_reference(sc, cam, bg, D, pre, gC, gD, gA)
    g_means, g_opac = T(sc["means"], True), T(sc["opac"], True)
    g_m2d = torch.zeros_like(g_means, requires_grad=True)
    if pre:
        g_in = dict(colors_precomp=T(sc["colors_precomp"], True), cov3D_precomp=T(sc["cov3D_precomp"], True))
    else:
        g_in = dict(shs=T(sc["shs"], True), scales=T(sc["scales"], True), rotations=T(sc["rots"], True))
    color, radii, depth, alpha = GaussianRasterizer(settings(cam, bg, D))(g_means, g_m2d, g_opac, **g_in, return_aux=True)
    loss = (depth[0] * T(gD)).sum()
    if terms != "depth_only":
        loss = loss + (alpha[0] * T(gA)).sum()
    if terms == "all":
        loss = loss + (color * T(gC)).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert np.array_equal(radii.cpu().numpy(), ref_aux["radii"].numpy())
    pairs = [("means", g_means.grad, ref["means"]), ("opacity", g_opac.grad.reshape(-1), ref["opac"]), ("means2D", g_m2d.grad[:, :2], ref["m2d"])]
    if pre:
        pairs += [("cov3D", g_in["cov3D_precomp"].grad, ref["cov3D_precomp"])]
        if terms == "all":
            pairs += [("colors", g_in["colors_precomp"].grad, ref["colors_precomp"])]
    else:
        pairs += [("scales", g_in["scales"].grad, ref["scales"]), ("rots", g_in["rotations"].grad, ref["rots"])]
        if terms == "all":
            pairs += [("shs", g_in["shs"].grad, ref["shs"])]
    for what, got, r in pairs:
        got, r = got.cpu().numpy(), r.numpy()
        rel = np.abs(got - r).max() / max(np.abs(r).max(), 1e-30)
        print("%-10s %-10s rel %.3g" % (terms, what, rel))
        assert rel <= 1e-3, (terms, what, rel)
        assert_grads_elementwise(got, r, "%s %s" % (terms, what))


def test_backward_aux_without_maps_is_backward_p(monkeypatch):
    """gm_backward_aux with NULL map gradients == gm_backward_p; the image gradient on two pixels, so float-atomic order moves no sum"""
    from gpu_utils import T
    from gaussianmesh_amd import _lib, rasterizer as R
    sc, cam = small_scene(P=3000, W=128, H=96, seed=5, D=3, scale_lo=0.05, scale_hi=0.4)
    bg = np.array([0.1, 0.2, 0.3], np.float32)
    W, H = cam["W"], cam["H"]
    nr, color, radii, geom, binning, img = _gpu_frame(sc, cam, bg, 3, 2, exact=True, aux=False)
    dpix = np.zeros((3, H, W), np.float32)
    dpix[:, 40, 60] = (0.5, -1.0, 2.0)
    dpix[:, 41, 61] = (1.0, 0.25, -0.5)
    args = (T(bg), T(sc["means"]), radii, None, T(sc["scales"]), T(sc["rots"]), 1.0, None, T(cam["view"]), T(cam["proj"]), cam["tanx"], cam["tany"],
            T(dpix), T(sc["shs"]), 3, T(cam["campos"]), geom, nr, binning, img, False, 2)
    ref = R.rasterize_backward(*args)
    lib = _lib.lib()
    calls = []
    aux = lib.gm_backward_aux

    def via_aux(*a):
        calls.append(1)
        return aux(*a[:-2], None, None, None, *a[-2:])
    monkeypatch.setattr(lib, "gm_backward_p", via_aux)
    got = R.rasterize_backward(*args)
    torch.cuda.synchronize()
    assert calls
    for g, r in zip(got, ref):
        if r is not None:
            assert torch.equal(g, r)


def _deformed_setup(N=6000):
    from gpu_utils import T
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.deform import pack_mesh_state
    verts, faces = scenes.torus_mesh(40, 30)
    cl = scenes.bind_cloud_to_mesh(N, verts, faces, seed=11)
    V1, Rv, Sv = scenes.twist_bend_frame(verts, t=5)
    cov = scenes.cov3d_from_scale_rot(cl["scales"], cl["rots"]).astype(np.float32)
    state = np.concatenate([V1.astype(np.float32), Rv.reshape(-1, 9), Sv.reshape(-1, 9)], axis=1).astype(np.float32)
    W, H = 300, 170
    cams = [scenes.orbit_camera(k, 7, W, H, radius=6.0) for k in (1, 2)]
    packed = pack_mesh_state(T(state), T(verts.astype(np.float32)))
    g = dict(tri=T(cl["tri"], dtype=torch.int32), w=T(cl["weights"]), cov=T(cov), pos=T(cl["means"]), shs=T(cl["shs"]), opac=T(cl["opac"]))
    return g, packed, cams, W, H


def test_deformed_frame_maps_equal_generic_path():
    from gpu_utils import T
    from gaussianmesh_amd import _lib, rasterizer as R
    from gaussianmesh_amd.deform import deform_shade_packed
    g, packed, cams, W, H = _deformed_setup()
    bg = T(np.array([1.0, 1.0, 1.0], np.float32))
    cam = cams[0]
    ct = {k: T(cam[k]) for k in ("view", "proj", "campos")}
    pos, cov6, rgb = deform_shade_packed(g["tri"], g["w"], packed, g["cov"], g["pos"], g["shs"], ct["campos"], deg=3)
    ref = R.rasterize_forward_begin(bg, pos, rgb, g["opac"], None, None, 1.0, cov6, ct["view"], ct["proj"], cam["tanx"], cam["tany"], H, W,
                                    None, 3, ct["campos"], aux=True).finish(image_only=True)
    fb = lambda cam_, **kw: R.forward_deformed_begin(bg, g["tri"], g["w"], packed, g["cov"], g["pos"], g["shs"], g["opac"],
                                                     *(T(cam_[k]) for k in ("view", "proj")), cam_["tanx"], cam_["tany"], H, W, 3,
                                                     T(cam_["campos"]), **kw)
    for sync_free in (False, True):
        h = fb(cam, aux=True)
        out = h.finish(image_only=True, sync_free=sync_free, capacity=4 << 20)
        assert h.check()[0]
        torch.cuda.synchronize()
        assert torch.equal(out[1], ref[1]) and torch.equal(out[2], ref[2])
        assert torch.equal(out[6], ref[6]) and torch.equal(out[7], ref[7])
    assert float(ref[7].max()) > 0.5 and float(ref[6].max()) > 0.0
    # a view stream with a depth plan: aux frames take the partition path (the direct pass writes no depth keys) and stay correct
    plan = R.new_depth_plan(bg.device)
    ws = R.RasterWorkspace()
    fb(cams[1], depth_plan=plan, workspace=ws).finish(sync_free=True, capacity=4 << 20)
    h = fb(cam, depth_plan=plan, workspace=ws, aux=True)
    assert not h.direct
    out = h.finish()
    torch.cuda.synchronize()
    assert torch.equal(out[1][:, :, :], ref[1]) and torch.equal(out[6], ref[6]) and torch.equal(out[7], ref[7])
    # the C ABI on a direct-placement frame: the AUX second half refuses it (status word 3 = 3, background, maps 0)
    h = fb(cam, depth_plan=plan)
    assert h.direct
    h.maps = tuple(torch.full((1, H, W), 7.0, device=bg.device) for _ in range(2))
    out = h.finish(sync_free=True, capacity=4 << 20, image_only=True)
    ok, _ = h.check()
    torch.cuda.synchronize()
    assert not ok and h.refusal == 3
    assert float(out[6].abs().max()) == 0.0 and float(out[7].abs().max()) == 0.0
    assert torch.equal(out[1], bg.reshape(3, 1, 1).expand(3, H, W))
    with pytest.raises(_lib.GmeshError):
        R.forward_deformed_batch(bg, g["tri"], g["w"], [packed], g["cov"], g["pos"], g["shs"], g["opac"],
                                 [dict(view=ct["view"], proj=ct["proj"], campos=ct["campos"], tanx=cam["tanx"], tany=cam["tany"])], H, W, 3,
                                 [R.RasterWorkspace()], aux=True)


def test_render_return_aux_and_backward_through_alpha():
    from types import SimpleNamespace
    from gpu_utils import T
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.renderer import Camera, render
    from test_gpu_bg_route import _mesh_model, W as W_, H as H_
    pc = _mesh_model()
    cam = Camera(scenes.orbit_camera(1, 6, W_, H_, radius=6.5), "cuda")
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    bg = T(np.array([0.0, 0.0, 0.0], np.float32))
    plain = render(cam, pc, pipe, bg)
    out = render(cam, pc, pipe, bg, return_aux=True)
    assert set(out) == set(plain) | {"depth", "alpha"}
    assert "depth" not in plain and "alpha" not in plain
    assert out["depth"].shape == (1, H_, W_) and out["alpha"].shape == (1, H_, W_)
    assert torch.equal(out["render"], plain["render"])
    pc.zero_grad(set_to_none=True)
    out["alpha"].mean().backward()
    torch.cuda.synchronize()
    grads = [p.grad for p in pc.parameters() if p.grad is not None]
    assert grads and any(float(gr.abs().max()) > 0 for gr in grads)


def test_sized_workspace_aux_finish_allocates_nothing():
    from gpu_utils import T
    from gaussianmesh_amd import rasterizer as Rz, scenes
    sc = scenes.make_cloud(20000, seed=6, scale_lo=0.01, scale_hi=0.15)
    cams = [scenes.orbit_camera(k, 8, 320, 200, radius=7.5) for k in range(3)]
    bg = T(np.array([0.1, 0.2, 0.3], np.float32))

    def args(k):
        ct = {n: T(cams[k][n]) for n in ("view", "proj", "campos")}
        return (bg, T(sc["means"]), None, T(sc["opac"]), T(sc["scales"]), T(sc["rots"]), 1.0, None, ct["view"], ct["proj"], cams[k]["tanx"],
                cams[k]["tany"], 200, 320, T(sc["shs"]), 3, ct["campos"])
    ws = Rz.RasterWorkspace()
    Rz.rasterize_forward_begin(*args(0), workspace=ws, aux=True).finish()
    for k in (1, 2):
        ref = Rz.rasterize_forward_begin(*args(k), aux=True).finish()
        h = Rz.rasterize_forward_begin(*args(k), workspace=ws, aux=True)
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        nr, color, radii, geom, binning, img, depth, alpha = h.finish(sync_free=True)
        after = torch.cuda.memory_stats()["allocation.all.allocated"]
        assert nr == -1 and after == before
        ok, count = h.check()
        assert ok and count == ref[0] and torch.equal(color, ref[1]) and torch.equal(depth, ref[6]) and torch.equal(alpha, ref[7])


def test_sh_step_with_an_alpha_gradient_raises():
    from gpu_utils import T, settings
    from gaussianmesh_amd import GaussianRasterizer, _lib
    from gaussianmesh_amd.rasterizer import ShStep
    sc, cam = small_scene(P=500, W=64, H=48, seed=2, D=3)
    bg = np.array([0.0, 0.0, 0.0], np.float32)
    shs = torch.nn.Parameter(T(sc["shs"]))
    ss = ShStep(shs, torch.zeros_like(shs), torch.zeros_like(shs), 1e-3, 1e-4, (0.9, 0.999), 1e-15, 1)
    with ss:
        color, radii, depth, alpha = GaussianRasterizer(settings(cam, bg, 3))(T(sc["means"], True), torch.zeros(500, 3, device="cuda", requires_grad=True),
                                                                              T(sc["opac"], True), shs=shs, scales=T(sc["scales"], True),
                                                                              rotations=T(sc["rots"], True), return_aux=True)
        with pytest.raises(_lib.GmeshError, match="ShStep"):
            (color.sum() + alpha.sum()).backward()
    assert not ss.applied
