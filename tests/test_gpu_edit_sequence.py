"""-m gpu: ObjectVisualTool.render_sequence (edit sequences, K frames per launch chain) and its CLI (python -m
gaussianmesh_amd.edit_sequence) against the single-frame fused path (bit for bit) and the per-frame generic path (the forward gate)."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_edittool import _write_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gate(got, ref, what, tol=1e-4):
    """The forward gate between two routes of one frame: per pixel max-abs <= tol (depth: relative to its size), except for the few
    pixels where an entry's alpha or a pixel's T sits within rounding distance of a threshold (at most max(2, 1e-4 W H) of them)."""
    got, ref = got.detach().float(), ref.detach().float()
    assert got.shape == ref.shape, what
    d = ((got - ref).abs() / ref.abs().clamp(min=1.0)).amax(dim=0)
    n_out = int((d > tol).sum())
    H, W = d.shape
    assert n_out <= max(2, 1e-4 * W * H), "%s: %d pixels beyond %g (max %g)" % (what, n_out, tol, float(d.max()))


def _tools(d, n=2):
    from gaussianmesh_amd.edittool import ObjectVisualTool
    out = []
    for _ in range(n):
        t = ObjectVisualTool()
        t.add_gaussian(os.path.join(d, "object.ply"), os.path.join(d, "rest.obj"), "Object")
        out.append(t)
    return out


def _fused(obj, table, cam, bg, aux):
    """the single-frame fused path on one gather table: forward_deformed_begin(...).finish()"""
    import math
    from gaussianmesh_amd import rasterizer as Rz
    out = Rz.forward_deformed_begin(bg, obj["tri"], obj["weights"], table, obj["cov"], obj["pos"], obj["shs"], obj["opac"], cam.world_view_transform,
                                    cam.full_proj_transform, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), cam.image_height, cam.image_width,
                                    3, cam.camera_center, aux=aux).finish(image_only=True)
    return (out[1], out[6], out[7]) if aux else out[1]


def _snapshot(tool):
    keys = ("gaussian_deform_pos", "gaussian_deform_cov", "gaussian_deform_rot", "gaussian_deform_cov6", "deform_state")
    return [[getattr(o, k) for k in keys] for o in tool.gaussians_list]


def _frames(d, cams):
    from gaussianmesh_amd import io as gio, scenes
    verts, faces = gio.read_obj(os.path.join(d, "rest.obj"))
    meshes = [scenes.twist_bend_frame(verts, t=t)[0].astype(np.float32) for t in (3, 7, 11, 14, 19, 23, 30)]
    V = lambda i: torch.tensor(meshes[i], device="cuda")
    # 10 frames (not a multiple of 4): tensors, an array, an OBJ path, and frames that name nothing (the current state)
    gio.write_obj(os.path.join(d, "seq_obj.obj"), meshes[6], faces)
    deforms = [{"Object": V(0)}, {"Object": V(1)}, None, {"Object": meshes[2]}, {"Object": V(3)}, {"Object": os.path.join(d, "seq_obj.obj")},
               None, {"Object": V(4)}, {"Object": V(5)}, {"Object": V(1)}]
    return [(cams[i % len(cams)], deforms[i]) for i in range(10)], meshes


@pytest.mark.parametrize("aux", [False, True])
def test_one_object_sequence_equals_the_fused_and_the_generic_paths(tmp_path, aux):
    from gaussianmesh_amd import io as gio, scenes
    from gaussianmesh_amd.deform import mesh_rs_packed, pack_mesh_state
    from gaussianmesh_amd.renderer import render_deformed
    d = str(tmp_path)
    _write_scene(d)
    tool, ref_tool = _tools(d)
    cams = tool.get_camera(d)
    frames, meshes = _frames(d, cams)
    V_now = torch.tensor(scenes.twist_bend_frame(gio.read_obj(os.path.join(d, "rest.obj"))[0], t=9)[0].astype(np.float32), device="cuda")
    tool.gaussians_list[0].deform_vertices(V_now)                       # the current state: rendered by frames that name nothing
    before = _snapshot(tool)
    got = list(tool.render_sequence(frames, frames_per_launch=4, aux=aux))
    torch.cuda.synchronize()
    assert len(got) == 10
    after = _snapshot(tool)
    assert all(a is b for ra, rb in zip(before, after) for a, b in zip(ra, rb)), "render_sequence changed an object attribute"
    o = tool.gaussians_list[0]
    cloud = dict(tri=o.gaussian_triangles, weights=o.coord, cov=o.gaussian_cov, pos=o.gaussian_pos, shs=o.gaussian_feature, opac=o.gaussian_o)
    bg = torch.ones(3, device="cuda")
    for i, (cam, dfm) in enumerate(frames):                              # (every yielded tensor held until now: none was reused)
        if dfm is None:
            V1, R, S = o.deform_state
            table = pack_mesh_state(torch.cat([V1, R.reshape(-1, 9), S.reshape(-1, 9)], dim=1), o.vertex)
            V = V_now
        else:
            v = dfm["Object"]
            V = torch.tensor(gio.read_obj(v)[0], dtype=torch.float32, device="cuda") if isinstance(v, str) else torch.as_tensor(v, device="cuda")
            table = mesh_rs_packed(o.vertex, V, o.faces, o._adjacency)
        exact = _fused(cloud, table, cam, bg, aux)
        outs = got[i] if aux else (got[i],)
        exp = exact if aux else (exact,)
        for g_, e_, name in zip(outs, exp, ("image", "depth", "alpha")):
            assert torch.equal(g_, e_), "frame %d: %s differs from the fused single-frame path" % (i, name)
        ref_tool.gaussians_list[0].deform_vertices(V)
        generic = render_deformed(cam, ref_tool.gaussians_list, return_aux=True)
        assert outs[0].shape == generic[0].shape
        for g_, e_, name in zip(outs, generic, ("image", "depth", "alpha")):
            _gate(g_, e_, "frame %d %s vs deform_vertices + render_deformed" % (i, name))


def test_two_objects_one_animated(tmp_path):
    from gaussianmesh_amd import io as gio, scenes
    from gaussianmesh_amd.deform import mesh_rs, mesh_rs_packed, pack_mesh_state, rest_mesh_state
    from gaussianmesh_amd.edittool import ObjectVisualTool
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    os.makedirs(d1); os.makedirs(d2)
    _write_scene(d1)
    _write_scene(d2, N=2000, seed=5)
    tools = []
    for _ in range(2):
        t = ObjectVisualTool()
        t.add_gaussian(os.path.join(d1, "object.ply"), os.path.join(d1, "rest.obj"), "A")
        t.add_gaussian(os.path.join(d2, "object.ply"), os.path.join(d2, "rest.obj"), "B")
        tools.append(t)
    tool, ref_tool = tools
    verts = gio.read_obj(os.path.join(d1, "rest.obj"))[0]
    meshes = [torch.tensor(scenes.twist_bend_frame(verts, t=t)[0].astype(np.float32), device="cuda") for t in (4, 8, 12, 16, 20)]
    cams = tool.get_camera(d1)
    frames = [(cams[i % 3], {"A": meshes[i]}) for i in range(5)]
    # the combined gather table: the per-object tables concatenated (B at rest, then B in a deformed current state)
    A, B = tool.gaussians_list
    for b_state in ("rest", "deformed"):
        tabs = tool.gather_tables([f[1] for f in frames[:3]])
        for k in range(3):
            ta = mesh_rs_packed(A.vertex, meshes[k], A.faces, A._adjacency)
            st = rest_mesh_state(B.vertex) if B.deform_state is None else \
                torch.cat([B.deform_state[0], B.deform_state[1].reshape(-1, 9), B.deform_state[2].reshape(-1, 9)], dim=1)
            tb = pack_mesh_state(st, B.vertex)
            assert torch.equal(tabs[k], torch.cat([ta, tb], dim=0)), (b_state, k)
        if b_state == "rest":
            VB = torch.tensor(scenes.twist_bend_frame(verts, t=6)[0].astype(np.float32), device="cuda")
            R, S = mesh_rs(B.vertex, VB, B.faces, adjacency=B._adjacency)
            B.deform(VB, R, S)
            ref_tool.gaussians_list[1].deform(VB, R, S)
    got = list(tool.render_sequence(frames, frames_per_launch=4))
    for i, (cam, dfm) in enumerate(frames):
        ref_tool.gaussians_list[0].deform_vertices(dfm["A"])
        _gate(got[i], ref_tool.render_gaussian(cam), "frame %d vs render_gaussian" % i)


def test_resolution_changes_and_the_single_frame_fallback(tmp_path):
    from gaussianmesh_amd import rasterizer as Rz
    from gaussianmesh_amd.deform import mesh_rs_packed
    d = str(tmp_path)
    _write_scene(d)
    tool, = _tools(d, 1)
    cams = tool.get_camera(d)

    def resized(c, W, H):
        c2 = copy.copy(c)
        c2.image_width, c2.image_height = W, H
        return c2
    frames, meshes = _frames(d, cams)
    sizes = [(200, 120), (200, 120), (320, 200), (320, 200), (320, 200), (200, 120), (768, 768), (768, 768), (200, 120), (200, 120)]
    frames = [(resized(c, *s), f) for (c, f), s in zip(frames, sizes)]
    o = tool.gaussians_list[0]
    cloud = dict(tri=o.gaussian_triangles, weights=o.coord, cov=o.gaussian_cov, pos=o.gaussian_pos, shs=o.gaussian_feature, opac=o.gaussian_o)
    Rz.set_default_emission_policy(1)                      # 768 x 768: 2304 list tiles of 16 px - more than the batch takes
    try:
        from gaussianmesh_amd.deform import plan_sequence
        assert ("single", [6]) in plan_sequence(sizes, 3)
        got = list(tool.render_sequence(frames, frames_per_launch=3, aux=True))
        for i, (cam, dfm) in enumerate(frames):
            table = tool.gather_tables([dfm])[0]
            exact = _fused(cloud, table, cam, torch.ones(3, device="cuda"), True)
            assert got[i][0].shape == (3, cam.image_height, cam.image_width)
            for g_, e_ in zip(got[i], exact):
                assert torch.equal(g_, e_), i
    finally:
        Rz.set_default_emission_policy("auto")


def test_frames_per_launch_limits(tmp_path):
    from gaussianmesh_amd import _lib
    d = str(tmp_path)
    _write_scene(d)
    tool, = _tools(d, 1)
    cams = tool.get_camera(d)
    frames, _ = _frames(d, cams)
    ref = list(tool.render_sequence(frames, frames_per_launch=4))
    for K in (1, _lib.GM_BATCH_MAX):
        got = list(tool.render_sequence(frames, frames_per_launch=K))
        assert all(torch.equal(a, b) for a, b in zip(got, ref)), K
    for K in (0, _lib.GM_BATCH_MAX + 1):
        with pytest.raises(ValueError):
            tool.render_sequence(frames, frames_per_launch=K)


def test_scene_tool_sequence_is_its_render_gaussian_per_frame(tmp_path):
    from gaussianmesh_amd import _lib
    from gaussianmesh_amd.edittool import SceneVisualTool
    d = str(tmp_path)
    _write_scene(d)
    tools = []
    for _ in range(2):
        t = SceneVisualTool(os.path.join(d, "background.ply"))
        t.add_gaussian(os.path.join(d, "object.ply"), os.path.join(d, "rest.obj"), "Object")
        tools.append(t)
    tool, ref_tool = tools
    cams = tool.get_camera(d)
    frames, meshes = _frames(d, cams)
    before = _snapshot(tool)
    got = list(tool.render_sequence(frames, frames_per_launch=4))
    after = _snapshot(tool)
    assert all(a is b for ra, rb in zip(before, after) for a, b in zip(ra, rb))
    for i, (cam, dfm) in enumerate(frames):
        obj = ref_tool.gaussians_list[0]
        if dfm is None:                                      # the current state: the rest pose
            obj.gaussian_deform_pos, obj.gaussian_deform_cov = obj.gaussian_pos, obj.gaussian_cov
        else:
            ref_tool.deform_one_gaussian("Object", dfm["Object"]) if isinstance(dfm["Object"], str) else \
                obj.deform_vertices(torch.as_tensor(dfm["Object"], device="cuda"))
        assert torch.equal(got[i], ref_tool.render_gaussian(cam)), i
    with pytest.raises(_lib.GmeshError):
        tool.render_sequence(frames, aux=True)


def test_cli_writes_what_the_api_renders(tmp_path):
    from PIL import Image
    from gaussianmesh_amd import io as gio, scenes
    d = str(tmp_path)
    _write_scene(d)
    verts, faces = gio.read_obj(os.path.join(d, "rest.obj"))
    seq = os.path.join(d, "seq")
    os.makedirs(seq)
    for i in range(1, 12):                                    # 1.obj .. 11.obj: numeric, not lexical, order
        gio.write_obj(os.path.join(seq, "%d.obj" % i), scenes.twist_bend_frame(verts, t=2 * i)[0], faces)
    out = os.path.join(d, "renders")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "gaussianmesh_amd.edit_sequence", "--object_gaussian", os.path.join(d, "object.ply"),
                        "--object_origin_mesh", os.path.join(d, "rest.obj"), "--camera_path", d, "--render_path", out, "--mesh_sequence", seq,
                        "--frames_per_launch", "4", "--save_maps"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    tool, = _tools(d, 1)
    cams = tool.get_camera(d)
    frames = [(cams[(i - 1) % len(cams)], {"Object": os.path.join(seq, "%d.obj" % i)}) for i in range(1, 12)]
    for i, (image, depth, alpha) in enumerate(tool.render_sequence(frames, aux=True)):
        png = np.asarray(Image.open(os.path.join(out, "%05d.png" % i)))
        exp = (np.clip(image.cpu().numpy(), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8).transpose(1, 2, 0)
        assert np.array_equal(png, exp), i
        assert np.array_equal(np.load(os.path.join(out, "%05d_depth.npy" % i)), depth[0].cpu().numpy()), i
        assert np.array_equal(np.load(os.path.join(out, "%05d_alpha.npy" % i)), alpha[0].cpu().numpy()), i
    assert not os.path.exists(os.path.join(out, "%05d.png" % 11))
