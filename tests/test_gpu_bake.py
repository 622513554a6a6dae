"""-m gpu: baking an edit into a plain Gaussian cloud - SingleObjectDeform.bake, the tools' save_baked and edit_sequence --save_baked.
Set-up throughout: torus_mesh(24, 16), 3000 bound Gaussians (scenes.bind_cloud_to_mesh), scenes' analytic twist, a 160 x 96 camera.
The twist is twist_bend_frame(t = 16): its largest amplitude, 0.5 rad per unit height, i.e. up to 0.35 rad on this torus (|y| <= 0.7)."""
import os

import numpy as np
import pytest
import torch

from test_gpu_arap import _drags, _scene64
from test_gpu_edittool import _write_scene

pytestmark = pytest.mark.gpu
TWIST_T = 16


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _camera(k=1):
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.renderer import Camera
    return Camera(scenes.orbit_camera(k, 7, 160, 96, radius=6.5), "cuda")


def _tensor_object(seed=2):
    """the tensor-in object and its twist (V1, R, S) on the device"""
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.deform import SingleObjectDeform
    verts, faces = scenes.torus_mesh(24, 16)
    cl = scenes.bind_cloud_to_mesh(3000, verts, faces, seed=seed)
    cov = scenes.cov3d_from_scale_rot(cl["scales"], cl["rots"])
    o = SingleObjectDeform(_dev(cl["means"]), _dev(cov), _dev(cl["opac"]), _dev(cl["shs"]), _dev(cl["tri"], torch.int32), _dev(cl["weights"]), _dev(verts))
    V1, R, S = scenes.twist_bend_frame(verts, t=TWIST_T)
    return o, (_dev(V1), _dev(R), _dev(S))


def _rasterize(cam, **kw):
    """(image, radii) of NewGaussianRasterizer on a white background, the settings render_deformed uses"""
    from gaussianmesh_amd.rasterizer import NewGaussianRasterizer
    from gaussianmesh_amd.renderer import _settings
    args = dict(shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None)
    args.update(kw)
    return NewGaussianRasterizer(_settings(cam, torch.ones(3, device="cuda"), 1, 3, False))(means2D=torch.zeros_like(args["means3D"]), **args)


def _attributes(o):
    keys = ("gaussian_pos", "gaussian_cov", "gaussian_o", "gaussian_feature", "gaussian_deform_pos", "gaussian_deform_cov", "gaussian_deform_rot",
            "gaussian_deform_cov6", "deform_state")
    return [getattr(o, k) for k in keys]


def test_baked_colour_on_the_same_geometry():
    """5. the baked geometry rendered with the baked SH rows (the rasterizer's own SH, unrotated direction) against the same geometry with
    colors_precomp = the edit path's colour: equal radii, image within 2e-5"""
    from gaussianmesh_amd.deform import sh_colors
    o, (V1, R, S) = _tensor_object()
    _, _, rot = o.deform(V1, R, S)
    b = o.bake()
    assert b["xyz"].shape == (3000, 3) and b["scales"].shape == (3000, 3) and b["rotations"].shape == (3000, 4)
    assert b["opacity"].shape == (3000, 1) and b["shs"].shape == (3000, 16, 3) and all(v.is_cuda for v in b.values())
    assert torch.equal(b["xyz"], o.gaussian_deform_pos)
    cam = _camera()
    geom = dict(means3D=b["xyz"], opacities=b["opacity"], scales=b["scales"], rotations=b["rotations"])
    img_sh, radii_sh = _rasterize(cam, shs=b["shs"], **geom)
    img_pre, radii_pre = _rasterize(cam, colors_precomp=sh_colors(b["xyz"], cam.camera_center, o.gaussian_feature, rot=rot), **geom)
    img_plain, _ = _rasterize(cam, shs=o.gaussian_feature, **geom)
    assert torch.equal(radii_sh, radii_pre) and int((radii_sh > 0).sum()) > 1000
    diff, miss = float((img_sh - img_pre).abs().max()), float((img_plain - img_pre).abs().max())
    print("baked SH vs the edit path's colour: max image difference %.3g (the unrotated original rows: %.3g)" % (diff, miss))
    assert diff <= 2e-5
    assert miss > 2e-3                                       # (what the bake is for: the original rows, unrotated, show other colours)


def test_bake_at_rest_from_the_state_and_without_a_host_wait():
    """6."""
    o, (V1, R, S) = _tensor_object()
    from gaussianmesh_amd.deform import cov_to_scale_rot
    before = _attributes(o)
    b = o.bake()
    assert b["xyz"] is o.gaussian_pos and b["shs"] is o.gaussian_feature and b["opacity"] is o.gaussian_o       # at rest: the object's own rows
    s, q = cov_to_scale_rot(o.gaussian_cov)
    assert torch.equal(b["scales"], s) and torch.equal(b["rotations"], q)
    assert all(x is y for x, y in zip(before, _attributes(o)))
    # deform_and_shade alone leaves gaussian_deform_cov / gaussian_deform_rot at rest: bake() reads the state, not those
    o.deform_and_shade(V1, R, S, _camera().camera_center)
    assert o.gaussian_deform_cov is o.gaussian_cov
    shaded = o.bake()
    p, (V1b, Rb, Sb) = _tensor_object()
    p.deform(V1b, Rb, Sb)
    before = _attributes(p)
    deformed = p.bake()
    assert all(x is y for x, y in zip(before, _attributes(p)))
    assert sorted(shaded) == sorted(deformed) == ["opacity", "rotations", "scales", "shs", "xyz"]
    for k in deformed:
        assert torch.equal(shaded[k], deformed[k]), k
    assert not torch.equal(deformed["shs"], p.gaussian_feature) and bool(torch.isfinite(deformed["shs"]).all())
    for deg in (0, 1, 2):                                     # a lower degree leaves the higher coefficients as they are
        n = (deg + 1) ** 2
        low = p.bake(deg)["shs"]
        assert torch.equal(low[:, n:], p.gaussian_feature[:, n:]) and (deg == 0) == torch.equal(low[:, :n], p.gaussian_feature[:, :n])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = p.bake()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(again[k], deformed[k]) for k in deformed)


def _file_tool(d, cls=None, **kw):
    from gaussianmesh_amd.edittool import ObjectVisualTool
    t = (cls or ObjectVisualTool)(**kw)
    t.add_gaussian(os.path.join(d, "object.ply"), os.path.join(d, "rest.obj"), "Object")
    return t


def _twisted_obj(d, name="twisted.obj"):
    from gaussianmesh_amd import io as gio, scenes
    verts, faces = gio.read_obj(os.path.join(d, "rest.obj"))
    path = os.path.join(d, name)
    gio.write_obj(path, scenes.twist_bend_frame(verts, t=TWIST_T)[0], faces)
    return path


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_saved_file_holds_the_bake_bit_for_bit(tmp_path):
    """7."""
    from gaussianmesh_amd import io as gio
    from gaussianmesh_amd.edittool import SceneVisualTool
    d = str(tmp_path)
    _write_scene(d)
    os.makedirs(os.path.join(d, "b"))
    _write_scene(os.path.join(d, "b"), N=1000, seed=5)
    tool = _file_tool(d)
    tool.add_gaussian(os.path.join(d, "b", "object.ply"), os.path.join(d, "b", "rest.obj"), "Second")
    tool.deform_one_gaussian("Object", _twisted_obj(d))
    A, B = tool.gaussians_list
    one = os.path.join(d, "one.ply")
    A.save_baked(one)
    m, src, b = gio.load_plain_gaussians(one), gio.load_mesh_gaussians(os.path.join(d, "object.ply")), A.bake()
    host = lambda t: t.cpu().numpy()
    assert np.array_equal(_bits(m["xyz"]), _bits(host(b["xyz"])))
    assert np.array_equal(_bits(m["features_dc"]), _bits(host(b["shs"][:, :1]))) and np.array_equal(_bits(m["features_rest"]), _bits(host(b["shs"][:, 1:])))
    assert np.array_equal(_bits(m["rotation"]), _bits(host(b["rotations"])))
    assert np.array_equal(_bits(m["opacity"]), _bits(src["opacity"]))
    assert np.array_equal(_bits(m["scaling"]), _bits(np.log(host(b["scales"]))))
    names, _ = gio.read_ply(one)
    assert names == gio.PLAIN_ATTRS + ["f_dc_%d" % i for i in range(3)] + ["f_rest_%d" % i for i in range(45)] + ["opacity"] + \
        ["scale_%d" % i for i in range(3)] + ["rot_%d" % i for i in range(4)]
    # the tool's file: the objects in list order, or the ones of a name
    both, second = os.path.join(d, "both.ply"), os.path.join(d, "second.ply")
    tool.save_baked(both)
    tool.save_baked(second, name="Second")
    B.save_baked(os.path.join(d, "b_alone.ply"))
    assert open(second, "rb").read() == open(os.path.join(d, "b_alone.ply"), "rb").read()
    mb, m2 = gio.load_plain_gaussians(both), gio.load_plain_gaussians(second)
    for k in m:
        assert np.array_equal(_bits(mb[k]), _bits(np.concatenate([m[k], m2[k]], 0))), k
    # a scene: the same, and with include_background the background's raw rows first, as loaded
    scene = _file_tool(d, SceneVisualTool, bg_gaussian_path=os.path.join(d, "background.ply"))
    scene.deform_one_gaussian("Object", os.path.join(d, "twisted.obj"))
    scene.save_baked(os.path.join(d, "scene_obj.ply"))
    assert open(os.path.join(d, "scene_obj.ply"), "rb").read() == open(one, "rb").read()
    scene.save_baked(os.path.join(d, "scene.ply"), include_background=True)
    ms, bgm = gio.load_plain_gaussians(os.path.join(d, "scene.ply")), gio.load_plain_gaussians(os.path.join(d, "background.ply"))
    nb = len(bgm["xyz"])
    assert nb == 800 and len(ms["xyz"]) == nb + 3000
    for k in m:
        assert np.array_equal(_bits(ms[k][:nb]), _bits(bgm[k])) and np.array_equal(_bits(ms[k][nb:]), _bits(m[k])), k
    scene.load_bg_gaussian(os.path.join(d, "one.ply"))        # the baked object is a background like any other
    assert scene.bg_mean3D.shape == (3000, 3)


def _render_objects(cam, objs):
    """renderer.render_deformed, with the radii"""
    from gaussianmesh_amd.deform import sh_colors
    from gaussianmesh_amd.renderer import strip_symmetric
    cat = lambda xs: torch.cat(xs, dim=0)
    means = cat([o.gaussian_deform_pos for o in objs])
    colors = sh_colors(means, cam.camera_center, cat([o.gaussian_feature for o in objs]), rot=cat([o.gaussian_deform_rot for o in objs]), deg=3)
    return _rasterize(cam, means3D=means, colors_precomp=colors, opacities=cat([o.gaussian_o for o in objs]),
                      cov3D_precomp=strip_symmetric(cat([o.gaussian_deform_cov for o in objs])))


def test_baked_file_bound_to_the_deformed_mesh_renders_the_deformed_object(tmp_path):
    """8. end to end: the baked PLY loaded with add_plain_gaussian against the DEFORMED mesh and rendered at rest, against the original
    tool's render of the deformed object.  The two differ by the covariance -> (scale, quaternion) substitution and one log / exp round
    trip: the bars of test_cov_to_scale_rot - radii differ on at most 2e-3 of the Gaussians, image within 2e-3.
    Control: the same file with the original, unrotated SH rows exceeds the image bar (twist amplitude 0.5 rad per unit height)."""
    from gaussianmesh_amd import io as gio
    from gaussianmesh_amd.edittool import ObjectVisualTool
    d = str(tmp_path)
    _write_scene(d)
    twisted = _twisted_obj(d)
    tool = _file_tool(d)
    tool.deform_one_gaussian("Object", twisted)
    cam = _camera()
    ref_img, ref_radii = _render_objects(cam, tool.gaussians_list)
    assert torch.equal(ref_img, tool.render_gaussian(cam))                       # (the helper IS the tool's render)
    baked = os.path.join(d, "baked.ply")
    tool.save_baked(baked)
    rows = tool.gaussians_list[0].baked_rows()
    src = tool.gaussians_list[0]._loaded
    control = os.path.join(d, "control.ply")
    gio.save_plain_gaussians(control, dict(rows, features_dc=src["features_dc"], features_rest=src["features_rest"]))
    out = {}
    for name, path in (("baked", baked), ("control", control)):
        plain = ObjectVisualTool()
        plain.add_plain_gaussian(path, twisted, "Baked")
        o = plain.gaussians_list[0]
        assert o.deform_state is None and float(o.bind_sqr_distance.max()) < 1.0
        img, radii = _render_objects(cam, plain.gaussians_list)
        assert torch.equal(img, plain.render_gaussian(cam))
        out[name] = (float((radii != ref_radii).float().mean()), float((img - ref_img).abs().max()))
    print("baked file vs the deformed object: radii differ on %.3g of the Gaussians, max image difference %.3g; "
          "control (unrotated SH rows): max image difference %.3g" % (out["baked"] + (out["control"][1],)))
    assert int((ref_radii > 0).sum()) > 1000 and float((ref_img - 1.0).abs().max()) > 0.1
    assert out["baked"][0] <= 2e-3 and out["baked"][1] <= 2e-3
    assert out["control"][1] > 2e-3


def test_cli_save_baked_writes_the_last_frames_state(tmp_path):
    """9. edit_sequence --handle_sequence ... --save_baked writes, byte for byte, tool.save_baked after the last frame's drag"""
    from gaussianmesh_amd.edit_sequence import main
    from gaussianmesh_amd import io as gio
    d = str(tmp_path)
    _scene64(d)
    verts, _ = gio.read_obj(os.path.join(d, "rest.obj"))
    ids, pos = _drags(verts)
    np.savez(os.path.join(d, "handles.npz"), handles=ids, positions=pos)
    out = os.path.join(d, "cli.ply")
    assert main(["--object_gaussian", os.path.join(d, "object.ply"), "--object_origin_mesh", os.path.join(d, "rest.obj"), "--camera_path", d,
                 "--render_path", os.path.join(d, "renders"), "--handle_sequence", os.path.join(d, "handles.npz"), "--save_baked", out]) == 3
    tool = _file_tool(d)
    o = tool.gaussians_list[0]
    o.set_handles(ids)
    for k in range(3):
        o.drag(pos[k])
    tool.save_baked(os.path.join(d, "api.ply"))
    assert open(out, "rb").read() == open(os.path.join(d, "api.ply"), "rb").read()
    rest = os.path.join(d, "rest.ply")
    _file_tool(d).save_baked(rest)
    assert open(out, "rb").read() != open(rest, "rb").read()
    assert sorted(os.listdir(os.path.join(d, "renders"))) == ["%05d.png" % k for k in range(3)]
