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


def _batch_inputs(tool, nbg, objs, ntail=0):
    """the scene's rows: background rows [0, nbg), the objects' slices, then ntail more background rows (static rows behind the last
    object: object_rows[n_objects] < P).  Each (object, slice) entry is an object of the batch with its own copy of its mesh's vertices in
    the combined gather table (voff)."""
    cat = lambda xs: torch.cat(xs, dim=0).contiguous()
    rows = [nbg]
    for o, sl in objs:
        rows.append(rows[-1] + o.gaussian_pos[sl].shape[0])
    voff = np.cumsum([0] + [o.vertex.shape[0] for o, _ in objs])
    bgr = lambda t: (t[:nbg], t[nbg:nbg + ntail])
    assert nbg + ntail <= tool.bg_mean3D.shape[0]
    g = dict(rows=rows, voff=voff,
             pos=cat([bgr(tool.bg_mean3D)[0]] + [o.gaussian_pos[sl] for o, sl in objs] + [bgr(tool.bg_mean3D)[1]]),
             cov=cat([bgr(tool.bg_cov3D)[0]] + [o.gaussian_cov[sl] for o, sl in objs] + [bgr(tool.bg_cov3D)[1]]),
             shs=cat([bgr(tool.bg_shs)[0]] + [o.gaussian_feature[sl] for o, sl in objs] + [bgr(tool.bg_shs)[1]]),
             opac=cat([bgr(tool.bg_opacity)[0].reshape(-1)] + [o.gaussian_o[sl].reshape(-1) for o, sl in objs] +
                      [bgr(tool.bg_opacity)[1].reshape(-1)]))
    g["tri"] = cat([o.gaussian_triangles[sl] + int(voff[j]) for j, (o, sl) in enumerate(objs)]).to(torch.int32) if objs else None
    g["w"] = cat([o.coord[sl] for o, sl in objs]) if objs else None
    g["ocov"] = cat([o.gaussian_cov[sl].reshape(-1, 9) for o, sl in objs]) if objs else None
    return g


def _reference(tool, nbg, objs, defs, cam, H, W, bg, ntail=0, policy=None, deg=3):
    """The contract: the rows concatenated in render_gaussian's order (deformed objects through mesh_rs + deform), gm_cov_to_scale_rot of
    every row, the rasterizer's forward with scales / rotations / SH rows -> (num_rendered, image, radii, dict(the frame's rows: pos,
    scales, rots; its binning buffer, laid out for num_rendered instances))"""
    from gaussianmesh_amd import rasterizer as Rz
    from gaussianmesh_amd.deform import cov_to_scale_rot, deform_tensors, mesh_rs
    pos, cov = [tool.bg_mean3D[:nbg]], [tool.bg_cov3D[:nbg]]
    for j, (o, sl) in enumerate(objs):
        if j in defs and o.gaussian_pos[sl].shape[0]:
            R, S = mesh_rs(o.vertex, defs[j], o.faces, adjacency=o._adjacency)
            p, c, _, _ = deform_tensors(o.gaussian_triangles[sl], o.coord[sl], defs[j] - o.vertex, R, S, o.gaussian_cov[sl], o.gaussian_pos[sl])
        else:
            p, c = o.gaussian_pos[sl], o.gaussian_cov[sl]
        pos.append(p); cov.append(c)
    pos.append(tool.bg_mean3D[nbg:nbg + ntail]); cov.append(tool.bg_cov3D[nbg:nbg + ntail])
    g = _batch_inputs(tool, nbg, objs, ntail)
    s, q = cov_to_scale_rot(torch.cat(cov, dim=0))
    pos = torch.cat(pos, dim=0)
    out = Rz.rasterize_forward_begin(bg, pos, None, g["opac"], s, q, 1, None, cam["view"], cam["proj"], cam["tanx"], cam["tany"],
                                     H, W, g["shs"], deg, cam["campos"], False, False, emission_policy=policy, force_M=16).finish(image_only=True)
    return out[0], out[1].clone(), out[2].clone(), dict(pos=pos, scales=s, rots=q, binning=out[4])


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


def _run_batch(tool, nbg, objs, defs_list, cams, H, W, bg, cap, ntail=0, policy=None, deg=3):
    from gaussianmesh_amd import rasterizer as Rz
    from gaussianmesh_amd.deform import cov_to_scale_rot
    g = _batch_inputs(tool, nbg, objs, ntail)
    s, q = cov_to_scale_rot(g["cov"])                                  # the static rows: every row's resting (scale, rotation)
    masks = [sum(1 << j for j in defs) for defs in defs_list]
    ws = [Rz.RasterWorkspace() for _ in defs_list]
    for w_ in ws:
        w_.capacity = cap
    hs = Rz.forward_scene_batch(bg, g["rows"], masks, g["pos"], s, q, g["shs"], g["opac"], g["tri"], g["w"], g["ocov"], _tables(objs, defs_list),
                                cams, H, W, deg, ws, image_only=True, emission_policy=policy)
    return hs


# which objects frame k deforms: A only, both, none, B only, ...
_PATTERN = [(0,), (0, 1), (), (1,), (0, 1), (0,), (), (0, 1)]


@pytest.mark.parametrize("K,layout", [(1, "scene"), (3, "scene"), (8, "scene"), (8, "straddle"), (3, "no_bg"), (3, "bg_only")])
def test_scene_batch_frames_equal_the_contract(tmp_path, K, layout):
    _scene_batch_frames_equal_the_contract(tmp_path, K, layout, 3)


@pytest.mark.parametrize("D", [0, 1, 2, 3])
def test_scene_batch_frames_equal_the_contract_at_every_sh_degree(tmp_path, D):
    """the straddling layout (wave 0 holds background, A and B rows) with the degree a model sends before its SH degree has grown, in the
    kernel call and in the contract"""
    _scene_batch_frames_equal_the_contract(tmp_path, 3, "straddle", D)


def _scene_batch_frames_equal_the_contract(tmp_path, K, layout, deg):
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
    ref = [_reference(tool, nbg, objs, defs, c, H, W, bg, deg=deg) for defs, c in zip(defs_list, frame_cams)]
    assert all(r[0] > 0 for r in ref), [r[0] for r in ref]
    cap = int(max(r[0] for r in ref) * 1.25) + 1024
    hs = _run_batch(tool, nbg, objs, defs_list, frame_cams, H, W, bg, cap, deg=deg)
    policy = Rz.get_default_emission_policy(W, H)
    for k, h in enumerate(hs):
        ok, nr = h.check()
        assert ok and nr == ref[k][0], (k, ok, nr, ref[k][0])
        assert h.workspace.status()[0].tolist() == [nr, 0, policy, 0], k
        assert torch.equal(h.radii, ref[k][2]), "frame %d of %d (%s, degree %d): radii" % (k, K, layout, deg)
        assert torch.equal(h.color, ref[k][1]), "frame %d of %d (%s, degree %d): image" % (k, K, layout, deg)


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


# ---------------------------------------------------------------------------------------------
# The batch at the edges of its ABI: every emission policy at ragged sizes and at the 2048-list-tile limit of a batch, 32 objects, empty
# objects, static rows behind the last object, object boundaries on wave boundaries, deformed rows on both sides of the near plane, full
# batches; each frame bit for bit against the contract above (images, radii, instance count, status words; lists under policy 0).

def _edge_layout(tool, name):
    """(background rows before the objects, [(object, row slice)], background rows after them)
    "split32": A and B cut into 16 slices each - 32 objects (GM_SCENE_OBJECTS_MAX), each with its own copy of its mesh in the table;
    "empty": empty objects first, in the middle and last; "tail": static rows behind the last object (object_rows[n] < P);
    "tail_only": object_rows[0] == 0 and trailing rows; "waves": P = 3110 (not a multiple of 64), object boundaries at rows = 63, 0, 1
    (mod 64)"""
    A, B = tool.gaussians_list
    if name == "split32":
        objs = []
        for o in (A, B):
            cut = np.linspace(0, o.gaussian_pos.shape[0], 17).astype(int)
            objs += [(o, slice(int(a), int(b))) for a, b in zip(cut[:-1], cut[1:])]
        return 100, objs, 0
    return {"empty": (200, [(A, slice(0, 0)), (A, slice(0, 1500)), (B, slice(7, 7)), (A, slice(1500, None)), (B, slice(None)), (B, slice(5, 5))], 0),
            "tail": (300, [(A, slice(None)), (B, slice(0, 1000))], 400),
            "tail_only": (0, [(A, slice(None))], 500),
            "waves": (63, [(A, slice(0, 65)), (B, slice(0, 1)), (A, slice(65, 127)), (B, slice(1, 66)), (A, slice(127, 2944))], 37)}[name]


def _pairs(binning, laid_out_for, nr, W, H, policy):
    """the sorted (key, id) instance list of a frame from its binning buffer (laid out for `laid_out_for` instances)"""
    from gpu_utils import _view
    from gaussianmesh_amd import _lib
    return _view(binning, _lib.lib().gm_binning_field(binning.data_ptr(), laid_out_for, W, H, policy, b"pairs"), 2 * nr, torch.int32)


def _frames_equal_the_contract(tool, nbg, objs, ntail, masks, cams, H, W, bg, policy=None, lists=False, t0=3):
    """frame k deforms object j (its own twist of the object's mesh) when bit j of masks[k] is set; the batch of the K frames against
    the contract frame by frame: instance count, status words, radii, image, with lists=True the instance list.  Returns (ref, handles)."""
    from gaussianmesh_amd import rasterizer as Rz
    defs_list = [{j: _mesh(o, t0 + 2 * k + 5 * (j % 7)) for j, (o, _) in enumerate(objs) if (m >> j) & 1} for k, m in enumerate(masks)]
    ref = [_reference(tool, nbg, objs, defs, c, H, W, bg, ntail, policy) for defs, c in zip(defs_list, cams)]
    assert all(r[0] > 0 for r in ref), [r[0] for r in ref]
    cap = int(max(r[0] for r in ref) * 1.25) + 1024
    hs = _run_batch(tool, nbg, objs, defs_list, cams, H, W, bg, cap, ntail, policy)
    pol = Rz.get_default_emission_policy(W, H) if policy is None else policy
    what = "%dx%d policy %d, %d objects" % (W, H, pol, len(objs))
    for k, h in enumerate(hs):
        ok, nr = h.check()
        assert ok and nr == ref[k][0], (what, k, ok, nr, ref[k][0])
        assert h.workspace.status()[0].tolist() == [nr, 0, pol, 0], (what, k)
        assert torch.equal(h.radii, ref[k][2]), "%s, frame %d (mask %#x): radii" % (what, k, masks[k])
        assert torch.equal(h.color, ref[k][1]), "%s, frame %d (mask %#x): image" % (what, k, masks[k])
        if lists:
            assert np.array_equal(_pairs(h.binning, h.workspace.capacity, nr, W, H, pol), _pairs(ref[k][3]["binning"], nr, nr, W, H, pol)), (
                "%s, frame %d: instance list" % (what, k))
    return ref, hs


def _list_tiles(W, H, policy):
    sh = max(policy - 1, 0)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    return ((gx + (1 << sh) - 1) >> sh) * ((gy + (1 << sh) - 1) >> sh)


# per policy a ragged size with exactly 2048 list tiles (16-px tiles under 0 and 1, 32-px parents under 2, 64-px under 3): the most a
# batch takes (the one-pass tile sort)
_AT_THE_LIMIT = {0: (1017, 509), 1: (2041, 241), 2: (2033, 1009), 3: (4065, 2017)}


@pytest.mark.parametrize("policy", [0, 1, 2, 3])
def test_scene_batch_under_every_emission_policy(tmp_path, policy):
    tool, d1, _ = _tool(tmp_path)
    nbg, objs = _layout(tool, "scene")
    cams = [_cam(c) for c in tool.get_camera(d1)]
    bg = torch.tensor([0.3, 0.1, 0.6], device="cuda")
    assert _list_tiles(*_AT_THE_LIMIT[policy], policy) == 2048
    for W, H in [(161, 97), (333, 211), _AT_THE_LIMIT[policy]]:
        _frames_equal_the_contract(tool, nbg, objs, 0, [0b01, 0b11, 0b00], cams, H, W, bg, policy=policy, lists=policy == 0)


def test_scene_batch_of_32_objects_full_batch(tmp_path):
    """GM_SCENE_OBJECTS_MAX objects and GM_BATCH_MAX frames: only object 31, all 32, none, alternating both ways, the first and the last,
    each half"""
    from gaussianmesh_amd import _lib
    tool, d1, _ = _tool(tmp_path)
    nbg, objs, ntail = _edge_layout(tool, "split32")
    assert len(objs) == _lib.GM_SCENE_OBJECTS_MAX
    masks = [1 << 31, 0xFFFFFFFF, 0, 0x55555555, 0xAAAAAAAA, (1 << 31) | 1, 0xFFFF0000, 0x0000FFFF]
    assert len(masks) == _lib.GM_BATCH_MAX
    cams = [_cam(c) for c in tool.get_camera(d1)]
    _frames_equal_the_contract(tool, nbg, objs, ntail, masks, [cams[k % len(cams)] for k in range(len(masks))], 120, 200,
                               torch.tensor([0.2, 0.5, 0.7], device="cuda"))


@pytest.mark.parametrize("layout", ["empty", "tail", "tail_only", "waves"])
def test_scene_batch_row_layout_edges(tmp_path, layout):
    tool, d1, _ = _tool(tmp_path)
    nbg, objs, ntail = _edge_layout(tool, layout)
    g = _batch_inputs(tool, nbg, objs, ntail)
    P, rows = g["pos"].shape[0], g["rows"]
    if layout == "empty":
        assert rows[0] == rows[1] and rows[2] == rows[3] and rows[-2] == rows[-1] == P
    elif layout in ("tail", "tail_only"):
        assert rows[-1] < P and (rows[0] == 0) == (layout == "tail_only")
    else:
        assert P == 3110 and rows == [63, 128, 129, 191, 256, 3073]                # boundaries at 63, 0, 1, 63, 0, 1 (mod 64)
    n = len(objs)
    full, even = (1 << n) - 1, sum(1 << j for j in range(0, n, 2))
    masks = [full, even, 0, full ^ even, full]
    cams = [_cam(c) for c in tool.get_camera(d1)]
    _frames_equal_the_contract(tool, nbg, objs, ntail, masks, [cams[k % len(cams)] for k in range(len(masks))], 97, 161,
                               torch.tensor([0.6, 0.2, 0.1], device="cuda"), policy=0, lists=True)


def test_scene_batch_deformed_rows_at_the_near_plane(tmp_path):
    """a camera inside the tori's tube: deformed rows on both sides of view-space z = 0.2, where the fused pass skips the Jacobi of a row
    (pre_project culls it) and the contract does not"""
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.renderer import Camera
    tool, _, _ = _tool(tmp_path)
    nbg, objs = _layout(tool, "scene")
    H, W = 120, 200
    cams = [_cam(Camera(scenes.orbit_camera(k, 7, W, H, radius=2.0, height=0.0), "cuda")) for k in (1, 4, 6)]
    masks = [0b01, 0b11, 0b10]
    ref, _ = _frames_equal_the_contract(tool, nbg, objs, 0, masks, cams, H, W, torch.tensor([0.1, 0.1, 0.1], device="cuda"))
    rows = _batch_inputs(tool, nbg, objs)["rows"]
    for k, (r, c) in enumerate(zip(ref, cams)):
        z = r[3]["pos"] @ c["view"][:3, 2] + c["view"][3, 2]                    # view-space depth (the row-vector view matrix)
        moved = torch.zeros_like(z, dtype=torch.bool)
        for j in range(len(objs)):
            if (masks[k] >> j) & 1:
                moved[rows[j]:rows[j + 1]] = True
        near, front = int(((z <= 0.2) & moved).sum()), int(((z > 0.2) & (z < 0.4) & moved).sum())
        assert near >= 50 and front >= 50, (k, near, front)


@pytest.mark.parametrize("policy", [0, 2])
def test_scene_frames_against_the_oracle(tmp_path, oracle, policy):
    """each frame of a scene batch against the CPU oracle directly (not only against the HIP single-frame route): the frame's rows as the
    contract builds them (positions, (scale, rotation) from cov_to_scale_rot) through oracle.forward_full - radii equal, under policy 0
    the instance count and sorted list equal, and the strict forward gate on the image"""
    from helpers import assert_forward_gate
    tool, d1, _ = _tool(tmp_path)
    nbg, objs, ntail = _edge_layout(tool, "waves")
    H, W = 120, 200
    cams = [_cam(c) for c in tool.get_camera(d1)]
    bg = torch.tensor([0.2, 0.5, 0.7], device="cuda")
    n = len(objs)
    masks = [(1 << n) - 1, 0b10101, 0]
    ref, hs = _frames_equal_the_contract(tool, nbg, objs, ntail, masks, cams, H, W, bg, policy=policy)
    g = _batch_inputs(tool, nbg, objs, ntail)
    host = lambda t: t.detach().cpu().numpy()
    for k, (r, h, c) in enumerate(zip(ref, hs, cams)):
        sc = dict(means=host(r[3]["pos"]), opac=host(g["opac"]), shs=host(g["shs"]), scales=host(r[3]["scales"]), rots=host(r[3]["rots"]))
        cam = dict(view=host(c["view"]), proj=host(c["proj"]), campos=host(c["campos"]), W=W, H=H, tanx=c["tanx"], tany=c["tany"])
        fw = oracle.forward_full(sc, cam, host(bg), D=3)
        assert np.array_equal(host(h.radii), fw["geo"]["radii"]), (policy, k)
        if policy == 0:
            nr = h.check()[1]
            assert nr == fw["bins"]["R"], (k, nr, fw["bins"]["R"])
            assert np.array_equal(_pairs(h.binning, h.workspace.capacity, nr, W, H, 0)[1::2].astype(np.uint32), fw["bins"]["point_list"]), k
        assert_forward_gate(fw, host(h.color), W, H, 1e-4, "scene frame %d policy %d" % (k, policy), plain_tol=5e-5)
