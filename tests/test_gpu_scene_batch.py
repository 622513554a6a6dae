"""-m gpu: gm_forward_scene_batch_async (rasterizer.forward_scene_batch) - K frames of a scene (background cloud + mesh-bound objects) from
ONE pass over its rows - against its contract, frame by frame and bit for bit: gm_cov_to_scale_rot + the rasterizer's forward
(NewGaussianRasterizer's scales / rotations / SH route) on the concatenated rows, the deformed objects from mesh_rs + deform.  Then
SceneVisualTool.render_sequence, which now takes that route, against render_gaussian, and the CLI's background mode."""
import copy
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_edittool import _write_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(tmp_path):
    """SceneVisualTool with the background of _write_scene and two objects: A (3000 rows) and B (2000 rows, its own torus)"""
    from gaussianmesh_amd.edittool import SceneVisualTool
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    os.makedirs(d1, exist_ok=True); os.makedirs(d2, exist_ok=True)
    _write_scene(d1)
    _write_scene(d2, N=2000, seed=5)
    t = SceneVisualTool(os.path.join(d1, "background.ply"))
    t.add_gaussian(os.path.join(d1, "object.ply"), os.path.join(d1, "rest.obj"), "A")
    t.add_gaussian(os.path.join(d2, "object.ply"), os.path.join(d2, "rest.obj"), "B")
    return t, d1, d2


def _cam(c):
    return dict(view=c.world_view_transform, proj=c.full_proj_transform, campos=c.camera_center, tanx=math.tan(c.FoVx * 0.5),
                tany=math.tan(c.FoVy * 0.5))


def _mesh(o, t):
    from gaussianmesh_amd import scenes
    return torch.tensor(scenes.twist_bend_frame(o.vertex.cpu().numpy(), t=t)[0].astype(np.float32), device="cuda")


def _layout(tool, name):
    """(background rows, [(object, row slice)]) of a test scene: P = 5800 ("scene", not a multiple of 64); "straddle": 30 background rows,
    20 rows of A, all of B - wave 0 holds background, A and B rows; "no_bg": the objects alone; "bg_only": no object"""
    A, B = tool.gaussians_list
    every = slice(None)
    return {"scene": (800, [(A, every), (B, every)]), "straddle": (30, [(A, slice(0, 20)), (B, every)]),
            "no_bg": (0, [(A, every), (B, every)]), "bg_only": (800, [])}[name]


def _batch_inputs(tool, nbg, objs):
    cat = lambda xs: torch.cat(xs, dim=0).contiguous()
    rows = [nbg]
    for o, sl in objs:
        rows.append(rows[-1] + o.gaussian_pos[sl].shape[0])
    voff = np.cumsum([0] + [o.vertex.shape[0] for o, _ in objs])
    g = dict(rows=rows, voff=voff,
             pos=cat([tool.bg_mean3D[:nbg]] + [o.gaussian_pos[sl] for o, sl in objs]),
             cov=cat([tool.bg_cov3D[:nbg]] + [o.gaussian_cov[sl] for o, sl in objs]),
             shs=cat([tool.bg_shs[:nbg]] + [o.gaussian_feature[sl] for o, sl in objs]),
             opac=cat([tool.bg_opacity[:nbg].reshape(-1)] + [o.gaussian_o[sl].reshape(-1) for o, sl in objs]))
    g["tri"] = cat([o.gaussian_triangles[sl] + int(voff[j]) for j, (o, sl) in enumerate(objs)]).to(torch.int32) if objs else None
    g["w"] = cat([o.coord[sl] for o, sl in objs]) if objs else None
    g["ocov"] = cat([o.gaussian_cov[sl].reshape(-1, 9) for o, sl in objs]) if objs else None
    return g


def _reference(tool, nbg, objs, defs, cam, H, W, bg):
    """The contract: the rows concatenated in render_gaussian's order (deformed objects through mesh_rs + deform), gm_cov_to_scale_rot of
    every row, the rasterizer's forward with scales / rotations / SH rows -> (num_rendered, image, radii)"""
    from gaussianmesh_amd import rasterizer as Rz
    from gaussianmesh_amd.deform import cov_to_scale_rot, deform_tensors, mesh_rs
    pos, cov = [tool.bg_mean3D[:nbg]], [tool.bg_cov3D[:nbg]]
    for j, (o, sl) in enumerate(objs):
        if j in defs:
            R, S = mesh_rs(o.vertex, defs[j], o.faces, adjacency=o._adjacency)
            p, c, _, _ = deform_tensors(o.gaussian_triangles[sl], o.coord[sl], defs[j] - o.vertex, R, S, o.gaussian_cov[sl], o.gaussian_pos[sl])
        else:
            p, c = o.gaussian_pos[sl], o.gaussian_cov[sl]
        pos.append(p); cov.append(c)
    g = _batch_inputs(tool, nbg, objs)
    s, q = cov_to_scale_rot(torch.cat(cov, dim=0))
    out = Rz.rasterize_forward_begin(bg, torch.cat(pos, dim=0), None, g["opac"], s, q, 1, None, cam["view"], cam["proj"], cam["tanx"], cam["tany"],
                                     H, W, g["shs"], 3, cam["campos"], False, False, force_M=16).finish(image_only=True)
    return out[0], out[1].clone(), out[2].clone()


def _tables(objs, defs_list):
    """the combined gather table of each frame (None for a frame that deforms nothing)"""
    from gaussianmesh_amd.deform import mesh_rs_packed, pack_mesh_state, rest_mesh_state
    out = []
    for defs in defs_list:
        if not defs:
            out.append(None)
            continue
        parts = [mesh_rs_packed(o.vertex, defs[j], o.faces, o._adjacency) if j in defs else pack_mesh_state(rest_mesh_state(o.vertex), o.vertex)
                 for j, (o, _) in enumerate(objs)]
        out.append(torch.cat(parts, dim=0).contiguous())
    return out


def _run_batch(tool, nbg, objs, defs_list, cams, H, W, bg, cap):
    from gaussianmesh_amd import rasterizer as Rz
    from gaussianmesh_amd.deform import cov_to_scale_rot
    g = _batch_inputs(tool, nbg, objs)
    s, q = cov_to_scale_rot(g["cov"])                                  # the static rows: every row's resting (scale, rotation)
    masks = [sum(1 << j for j in defs) for defs in defs_list]
    ws = [Rz.RasterWorkspace() for _ in defs_list]
    for w_ in ws:
        w_.capacity = cap
    hs = Rz.forward_scene_batch(bg, g["rows"], masks, g["pos"], s, q, g["shs"], g["opac"], g["tri"], g["w"], g["ocov"], _tables(objs, defs_list),
                                cams, H, W, 3, ws, image_only=True)
    return hs


# which objects frame k deforms: A only, both, none, B only, ...
_PATTERN = [(0,), (0, 1), (), (1,), (0, 1), (0,), (), (0, 1)]


@pytest.mark.parametrize("K,layout", [(1, "scene"), (3, "scene"), (8, "scene"), (8, "straddle"), (3, "no_bg"), (3, "bg_only")])
def test_scene_batch_frames_equal_the_contract(tmp_path, K, layout):
    from gaussianmesh_amd import rasterizer as Rz
    tool, d1, _ = _tool(tmp_path)
    nbg, objs = _layout(tool, layout)
    cams = [_cam(c) for c in tool.get_camera(d1)]
    H, W = 120, 200
    bg = torch.tensor([0.2, 0.5, 0.7], device="cuda")
    defs_list = []
    for k in range(K):
        defs_list.append({j: _mesh(o, 3 + 2 * k + 5 * j) for j, (o, _) in enumerate(objs) if j in _PATTERN[k]})
    frame_cams = [cams[k % len(cams)] for k in range(K)]
    ref = [_reference(tool, nbg, objs, defs, c, H, W, bg) for defs, c in zip(defs_list, frame_cams)]
    assert all(r[0] > 0 for r in ref), [r[0] for r in ref]
    cap = int(max(r[0] for r in ref) * 1.25) + 1024
    hs = _run_batch(tool, nbg, objs, defs_list, frame_cams, H, W, bg, cap)
    policy = Rz.get_default_emission_policy(W, H)
    for k, h in enumerate(hs):
        ok, nr = h.check()
        assert ok and nr == ref[k][0], (k, ok, nr, ref[k][0])
        assert h.workspace.status()[0].tolist() == [nr, 0, policy, 0], k
        assert torch.equal(h.radii, ref[k][2]), "frame %d of %d (%s): radii" % (k, K, layout)
        assert torch.equal(h.color, ref[k][1]), "frame %d of %d (%s): image" % (k, K, layout)


def test_a_scene_frame_refused_for_capacity_is_rendered_again_exactly(tmp_path):
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.renderer import Camera
    tool, _, _ = _tool(tmp_path)
    nbg, objs = _layout(tool, "scene")
    H, W = 120, 200
    bg = torch.tensor([0.9, 0.1, 0.3], device="cuda")
    near, far = (_cam(Camera(scenes.orbit_camera(1, 7, W, H, radius=r), "cuda")) for r in (6.5, 18.0))
    defs_list = [{0: _mesh(objs[0][0], 6), 1: _mesh(objs[1][0], 9)}] * 2
    ref = [_reference(tool, nbg, objs, defs, c, H, W, bg) for defs, c in zip(defs_list, (near, far))]
    counts = [r[0] for r in ref]
    assert counts[0] != counts[1] and min(counts) > 0, counts
    heavy = 0 if counts[0] > counts[1] else 1
    hs = _run_batch(tool, nbg, objs, defs_list, [near, far], H, W, bg, (counts[0] + counts[1]) // 2)
    for k, h in enumerate(hs):
        ok, nr = h.check()
        assert (ok, nr) == (k != heavy, counts[k]), (k, ok, nr, counts)
    light = hs[1 - heavy]
    assert torch.equal(light.color, ref[1 - heavy][1]) and torch.equal(light.radii, ref[1 - heavy][2])
    assert torch.equal(hs[heavy].color, bg.reshape(3, 1, 1).expand(3, H, W))               # refused: the background
    nr, color, radii, *_ = hs[heavy].finish(image_only=True)
    torch.cuda.synchronize()
    assert nr == counts[heavy] and torch.equal(color, ref[heavy][1]) and torch.equal(radii, ref[heavy][2])


def _snapshot(tool):
    keys = ("gaussian_deform_pos", "gaussian_deform_cov", "gaussian_deform_rot", "gaussian_deform_cov6", "deform_state")
    return [[getattr(o, k) for k in keys] for o in tool.gaussians_list]


def test_scene_sequence_takes_the_batch_and_equals_render_gaussian(tmp_path, monkeypatch):
    from gaussianmesh_amd import io as gio, rasterizer as Rz
    from gaussianmesh_amd.deform import mesh_rs
    tools = [_tool(tmp_path / n) for n in ("t", "r")]
    (tool, d1, _), (ref_tool, _, _) = tools
    # B in a deformed current state (rendered so by every frame that does not name it), in both tools
    for t in (tool, ref_tool):
        B = t.gaussians_list[1]
        VB = _mesh(B, 13)
        R, S = mesh_rs(B.vertex, VB, B.faces, adjacency=B._adjacency)
        B.deform(VB, R, S)
    A = tool.gaussians_list[0]
    faces = A.faces.cpu().numpy()
    obj_path = os.path.join(d1, "seq_a.obj")
    gio.write_obj(obj_path, _mesh(A, 21).cpu().numpy(), faces)
    base = tool.get_camera(d1)

    def resized(c, W, H):
        c2 = copy.copy(c)
        c2.image_width, c2.image_height = W, H
        return c2
    sizes = [(200, 120)] * 3 + [(160, 96)] * 2 + [(200, 120)] * 4 + [(160, 96)] * 2
    deforms = [{"A": _mesh(A, 3)}, {"A": obj_path}, None, {"A": _mesh(A, 7), "B": _mesh(A, 30)}, {"B": obj_path}, {"A": _mesh(A, 11).cpu().numpy()},
               None, {"B": _mesh(A, 25)}, {"A": _mesh(A, 17), "B": _mesh(A, 5)}, {"A": obj_path}, None]
    frames = [(resized(base[i % len(base)], *sizes[i]), deforms[i]) for i in range(len(sizes))]
    calls = dict(batch=0, batched_frames=0, render_gaussian=0)
    real_batch = Rz.forward_scene_batch

    def counting_batch(*a, **kw):
        calls["batch"] += 1
        calls["batched_frames"] += len(a[12])                         # the cameras
        return real_batch(*a, **kw)
    monkeypatch.setattr(Rz, "forward_scene_batch", counting_batch)
    real_render = tool.render_gaussian

    def counting_render(*a, **kw):
        calls["render_gaussian"] += 1
        return real_render(*a, **kw)
    monkeypatch.setattr(tool, "render_gaussian", counting_render)
    before = _snapshot(tool)
    got = list(tool.render_sequence(frames, frames_per_launch=4))
    torch.cuda.synchronize()
    assert all(a is b for ra, rb in zip(before, _snapshot(tool)) for a, b in zip(ra, rb)), "render_sequence changed an object attribute"
    # two resolutions: the first frame of each teaches the capacity, the other nine go through the batch
    assert calls["render_gaussian"] == 0 and calls["batched_frames"] == len(frames) - 2 and calls["batch"] >= 3, calls
    rA, rB = ref_tool.gaussians_list
    B_state = (rB.gaussian_deform_pos, rB.gaussian_deform_cov, rB.gaussian_deform_rot, rB.gaussian_deform_cov6, rB.deform_state)
    for i, (cam, dfm) in enumerate(frames):
        dfm = dfm or {}
        rA.gaussian_deform_pos, rA.gaussian_deform_cov = rA.gaussian_pos, rA.gaussian_cov                  # A's current state: the rest pose
        rB.gaussian_deform_pos, rB.gaussian_deform_cov, rB.gaussian_deform_rot, rB.gaussian_deform_cov6, rB.deform_state = B_state
        for name, o in (("A", rA), ("B", rB)):
            if name in dfm:
                v = dfm[name]
                if isinstance(v, str):
                    ref_tool.deform_one_gaussian(name, v)
                else:
                    o.deform_vertices(torch.as_tensor(v, device="cuda"))
        assert got[i].shape == (3, sizes[i][1], sizes[i][0])
        assert torch.equal(got[i], ref_tool.render_gaussian(cam)), i


def test_cli_with_a_background_writes_what_the_api_renders(tmp_path):
    from PIL import Image
    from gaussianmesh_amd import io as gio, scenes
    from gaussianmesh_amd.edittool import SceneVisualTool
    d = str(tmp_path)
    _write_scene(d)
    verts, faces = gio.read_obj(os.path.join(d, "rest.obj"))
    seq = os.path.join(d, "seq")
    os.makedirs(seq)
    for i in range(1, 8):
        gio.write_obj(os.path.join(seq, "%d.obj" % i), scenes.twist_bend_frame(verts, t=3 * i)[0], faces)
    out = os.path.join(d, "renders")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "gaussianmesh_amd.edit_sequence", "--is_exist_bg", "--background_gaussian",
                        os.path.join(d, "background.ply"), "--object_gaussian", os.path.join(d, "object.ply"), "--object_origin_mesh",
                        os.path.join(d, "rest.obj"), "--camera_path", d, "--render_path", out, "--mesh_sequence", seq, "--frames_per_launch", "3"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    tool = SceneVisualTool(os.path.join(d, "background.ply"))
    tool.add_gaussian(os.path.join(d, "object.ply"), os.path.join(d, "rest.obj"), "Object")
    cams = tool.get_camera(d)
    frames = [(cams[(i - 1) % len(cams)], {"Object": os.path.join(seq, "%d.obj" % i)}) for i in range(1, 8)]
    n = 0
    for i, image in enumerate(tool.render_sequence(frames, frames_per_launch=3)):
        png = np.asarray(Image.open(os.path.join(out, "%05d.png" % i)))
        exp = (np.clip(image.cpu().numpy(), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8).transpose(1, 2, 0)
        assert np.array_equal(png, exp), i
        n += 1
    assert n == 7 and not os.path.exists(os.path.join(out, "%05d.png" % 7))
