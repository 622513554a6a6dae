"""Host side of picking mesh vertices from the screen: gm_ray_mesh's declaration, typing and refusals (before any GPU work), the Python
refusals, camera_rays / screen_offset (plain torch: they run on CPU tensors) against a float64 statement and the projection they
invert, the --pick_sequence reader's refusals, and the float32 brute force of tests/ray_ref.py - the definition the device is held to in
test_gpu_raycast.py - against the same formula in float64."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from gaussianmesh_amd import _lib, scenes
from gaussianmesh_amd.renderer import Camera

import ray_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24


def _declared_args(name, ret="int"):
    text = open(os.path.join(ROOT, "include", "gmesh_hip.h")).read()
    m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, name), text)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name, ret, n", [("gm_ray_mesh", "int", 15), ("gm_ray_mesh_workspace_bytes", "size_t", 2)])
def test_header_declares_and_lib_types_the_entry_points(name, ret, n):
    assert name in _lib.header_symbols()
    assert len(_declared_args(name, ret)) == n
    assert len(_lib.SIGNATURES[name][1]) == n
    assert hasattr(_lib.lib(), name)


def test_ray_mesh_refuses_before_any_gpu_work():
    l = _lib.lib()
    a = 1 << 24                                               # a non-null "pointer": never dereferenced, every call is refused first
    big = 1 << 40
    call = lambda R=10, O=a, D=a, Vm=8, V=a, F=5, T=a, t0=0.0, t1=math.inf, ot=a, of=a, uv=a, ws=a, nbytes=big: \
        l.gm_ray_mesh(R, O, D, Vm, V, F, T, t0, t1, ot, of, uv, ws, nbytes, None)
    for kw in (dict(R=-1), dict(Vm=-1), dict(F=-1)):
        assert call(**kw) == 1 and b"negative" in l.gm_last_error(), kw
    assert call(F=0) == 1 and b"F == 0" in l.gm_last_error()
    assert call(Vm=0) == 1 and b"Vm == 0" in l.gm_last_error()
    for kw in (dict(O=None), dict(D=None), dict(V=None), dict(T=None), dict(ot=None), dict(of=None), dict(ws=None)):
        assert call(**kw) == 1 and b"null" in l.gm_last_error(), kw
    for kw in (dict(t0=-1.0), dict(t0=-1e-30), dict(t0=math.nan), dict(t1=math.nan), dict(t0=math.nan, R=0)):
        assert call(**kw) == 1 and b"t_min" in l.gm_last_error(), kw
    assert call(R=(1 << 31) - 1, F=(1 << 31) - 1) == 1 and b"too large" in l.gm_last_error()      # more workgroups than one grid holds
    need = l.gm_ray_mesh_workspace_bytes(10, 5)
    assert need > 0
    assert call(nbytes=need - 1) == 3 and b"workspace" in l.gm_last_error()
    assert l.gm_ray_mesh(0, None, None, 0, None, 0, None, 0.0, math.inf, None, None, None, None, 0, None) == 0      # R == 0: nothing launched


def test_workspace_bytes_are_monotonic_in_both_sizes():
    l = _lib.lib()
    sizes = [0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 100000, 1000000, 2073600, 6000000, (1 << 31) - 1]
    for fixed in (0, 1, 15000, 1600000, (1 << 31) - 1):
        in_r = [l.gm_ray_mesh_workspace_bytes(n, fixed) for n in sizes]
        in_f = [l.gm_ray_mesh_workspace_bytes(fixed, f) for f in sizes]
        assert in_r == sorted(in_r) and in_f == sorted(in_f), fixed
    assert l.gm_ray_mesh_workspace_bytes(0, 0) == l.gm_ray_mesh_workspace_bytes(1, 1) > 0
    assert l.gm_ray_mesh_workspace_bytes(1000, 5000) >= 48 * 5000 + 8 * 1000


def test_the_kernel_file_waits_for_nothing_and_allocates_nothing():
    """gm_ray_mesh's "no host synchronisation, no device allocation": its translation unit names no such runtime call"""
    text = open(os.path.join(ROOT, "gaussianmesh_amd", "csrc", "gm_raycast.hip")).read()
    assert "gm_raycast.hip" in open(os.path.join(ROOT, "gaussianmesh_amd", "csrc", "Makefile")).read()
    hits = re.findall(r"hipMemcpy\w*|hipMemset\w*|hip\w*Synchronize|hipMalloc\w*|hipFree\w*|GM_LAUNCH_CHECK", text)
    assert not hits, hits
    assert "#pragma clang fp contract(off)" in text


def _small_mesh():
    verts, faces = scenes.torus_mesh(8, 6)
    return verts.astype(np.float32), faces


def test_python_refusals():
    from gaussianmesh_amd import mesh_pick as mp
    verts, faces = _small_mesh()
    o, d = torch.zeros((4, 3)), torch.ones((4, 3))
    with pytest.raises(_lib.GmeshError, match="no CPU path"):
        mp.ray_mesh_hits(o, d, verts, faces)                                           # CPU tensors: no CPU path
    cam = Camera(scenes.look_at_camera((4, 3, 5), (0, 0, 0), 64, 48), "cpu")
    for fn in (lambda: mp.pick(cam, np.zeros((2, 2)), verts, faces), lambda: mp.visible_vertices(cam, verts, faces)):
        with pytest.raises(_lib.GmeshError, match="no CPU path"):
            fn()
    with pytest.raises(ValueError, match=r"\[R,3\]"):
        mp.ray_mesh_hits(torch.zeros((4, 2)), d, verts, faces)
    with pytest.raises(ValueError, match=r"\[R,3\]"):
        mp.ray_mesh_hits(o, d.numpy(), verts, faces)
    with pytest.raises(ValueError, match="one direction per origin"):
        mp.ray_mesh_hits(o, d[:3], verts, faces)
    with pytest.raises(ValueError, match=r"\[Vm,3\]"):
        mp.ray_mesh_hits(o, d, verts[:, :2], faces)
    with pytest.raises(ValueError, match=r"\[F,3\]"):
        mp.ray_mesh_hits(o, d, verts, faces[:, :2])
    for bad in (len(verts), -1):
        f = faces.copy(); f[3, 1] = bad
        with pytest.raises(ValueError, match="face index outside"):
            mp.ray_mesh_hits(o, d, verts, f)
    with pytest.raises(ValueError, match="integer"):
        mp.ray_mesh_hits(o, d, verts, faces.astype(np.float32))
    with pytest.raises(ValueError, match="empty"):
        mp.ray_mesh_hits(o, d, verts, faces[:0])
    for kw in (dict(t_min=-1.0), dict(t_min=math.nan), dict(t_max=math.nan)):
        with pytest.raises(ValueError, match="t_min"):
            mp.ray_mesh_hits(o, d, verts, faces, **kw)
    with pytest.raises(ValueError, match=r"\[P,2\]"):
        mp.camera_rays(cam, np.zeros((3, 3)))
    with pytest.raises(ValueError, match="one pixel offset per point"):
        mp.screen_offset(cam, torch.zeros((3, 3)), torch.zeros((2, 2)))


def test_edit_surface_refusals():
    """the screen-space methods of the tensor-in object: no faces / no handles are refused before anything needs a device"""
    from gaussianmesh_amd.deform import SingleObjectDeform
    from gaussianmesh_amd import edittool
    N, Vm = 5, 4
    o = SingleObjectDeform(torch.zeros((N, 3)), torch.eye(3).expand(N, 3, 3), torch.ones((N, 1)), torch.zeros((N, 16, 3)),
                           torch.zeros((N, 3), dtype=torch.int32), torch.full((N, 3), 1.0 / 3), torch.rand((Vm, 3)))
    cam = Camera(scenes.look_at_camera((4, 3, 5), (0, 0, 0), 64, 48), "cpu")
    with pytest.raises(ValueError, match="has no faces"):
        o.pick(cam, np.zeros((1, 2)))
    with pytest.raises(ValueError, match="has no faces"):
        o.select_visible(cam)
    with pytest.raises(ValueError, match="set_handles"):
        o.drag_pixels(cam, np.zeros((1, 2)))
    for cls in (edittool.SingleObjectDeform, ):
        assert all(hasattr(cls, m) for m in ("pick", "select_visible", "drag_pixels"))
    assert hasattr(edittool.ObjectVisualTool, "pick_one_gaussian") and hasattr(edittool.SceneVisualTool, "pick_one_gaussian")
    with pytest.raises(ValueError, match="no object named"):
        edittool.ObjectVisualTool(device="cpu").pick_one_gaussian("nobody", cam, np.zeros((1, 2)))


# ---- camera_rays / screen_offset: the float64 statement and the projection they invert ----
def _pix(ndc, S):
    return ((ndc + 1.0) * S - 1.0) * 0.5                       # ndc2pix, csrc/gm_pre_body.h


def _project(cam, points):
    """pixels and view depth of world points [P,3] through full_proj_transform (stored transposed: rows multiply from the left), float64"""
    P = np.asarray(cam["proj"], np.float64)
    h = np.concatenate([np.asarray(points, np.float64), np.ones((len(points), 1))], 1) @ P
    return np.stack([_pix(h[:, 0] / h[:, 3], cam["W"]), _pix(h[:, 1] / h[:, 3], cam["H"])], 1), h[:, 3]


def _pixels(W, H):
    rng = np.random.default_rng(5)
    whole = np.stack(np.meshgrid(np.arange(W), np.arange(H), indexing="xy"), -1).reshape(-1, 2).astype(np.float64)
    return np.concatenate([whole, rng.uniform(-0.5, [W - 0.5, H - 0.5], size=(200, 2)), [[-0.5, -0.5], [W - 0.5, H - 0.5]]], 0)


@pytest.mark.parametrize("as_dict", [False, True])
def test_camera_rays_against_float64_and_round_trip(as_dict):
    """Float32 evaluation of ((2x+1)/W - 1) tan, a 3-term product with the rotation: at most 8 roundings of values <= 1 in size on top of
    each other -> |d32 - d64| <= 8 eps per component.  Round trip: o + t d through full_proj_transform (float32 entries, relative error
    eps each) and ndc2pix returns to its pixel; a direction error of 8 eps is 8 eps W / (2 tan(FoVx/2)) (1 + |ndc|) < 2e-4 px at W = 64,
    60 degrees, and the bound asserted is 1e-4 px (measured: below 5e-6)."""
    from gaussianmesh_amd.mesh_pick import camera_rays
    cd = scenes.look_at_camera((4, 3, 5), (0, 0, 0), 64, 48)
    cam = cd if as_dict else Camera(cd, "cpu")
    pix = _pixels(64, 48)
    o, d = camera_rays(cam, pix)
    assert o.dtype == d.dtype == torch.float32 and o.shape == d.shape == (len(pix), 3)
    assert np.array_equal(o.numpy(), np.broadcast_to(cd["campos"], o.shape))
    view = np.asarray(cd["view"], np.float64)
    dv = np.stack([((2 * pix[:, 0] + 1) / 64 - 1) * cd["tanx"], ((2 * pix[:, 1] + 1) / 48 - 1) * cd["tany"], np.ones(len(pix))], 1)
    d64 = dv @ view[:3, :3].T
    assert np.abs(d.numpy() - d64).max() <= 8 * EPS
    for t in (0.5, 3.0, 40.0):
        back, depth = _project(cd, o.numpy().astype(np.float64) + t * d.numpy().astype(np.float64))
        assert np.abs(back - pix).max() <= 1e-4, (t, np.abs(back - pix).max())
        assert np.abs(depth - t).max() <= 1e-5 * t                 # directions are not normalised: t is the view depth


def test_screen_offset_against_float64_and_the_projection():
    """the move is parallel to the image plane (view depth unchanged), shifts the projected pixel by the offset, is the float64
    statement within float32 rounding of values of the points' size (16 eps (|p| + |move|)), and a zero offset returns the point itself"""
    from gaussianmesh_amd.mesh_pick import screen_offset
    cd = scenes.look_at_camera((4, 3, 5), (0, 0, 0), 64, 48)
    cam = Camera(cd, "cpu")
    rng = np.random.default_rng(8)
    pts = rng.uniform(-2.5, 2.5, size=(300, 3)).astype(np.float32)
    off = rng.uniform(-20, 20, size=(300, 2)).astype(np.float32)
    got = screen_offset(cam, torch.tensor(pts), torch.tensor(off)).numpy()
    view = np.asarray(cd["view"], np.float64)
    pv = pts.astype(np.float64) @ view[:3, :3] + view[3, :3]
    z = pv[:, 2]
    pv[:, 0] += off[:, 0] * 2 * cd["tanx"] / 64 * z
    pv[:, 1] += off[:, 1] * 2 * cd["tany"] / 48 * z
    exp = (pv - view[3, :3]) @ view[:3, :3].T
    size = np.abs(pts).max() + np.abs(exp - pts).max()
    assert np.abs(got - exp).max() <= 16 * EPS * size
    (p0, z0), (p1, z1) = _project(cd, pts), _project(cd, got)
    assert np.abs(z1 - z0).max() <= 1e-5 * np.abs(z0).max()
    assert np.abs((p1 - p0) - off).max() <= 1e-3
    assert np.array_equal(screen_offset(cam, torch.tensor(pts), torch.zeros((300, 2))).numpy(), pts)
    assert np.array_equal(screen_offset(cd, pts, off).numpy(), got)                     # host arrays and the dict camera: the same


# ---- the definition against itself in float64 ----
def test_float32_definition_agrees_with_float64_on_the_torus():
    """torus_mesh(24, 16) seen from look_at_camera((4, 3, 5), (0, 0, 0), 64, 48): the float32 brute force and the same formula in float64
    name the same first-hit face on every one of the 3072 pixel rays, and t agrees within 1e-5 (found: 909 hits, 4.5e-6)."""
    from gaussianmesh_amd.mesh_pick import camera_rays
    verts, faces = scenes.torus_mesh(24, 16)
    cam = Camera(scenes.look_at_camera((4, 3, 5), (0, 0, 0), 64, 48), "cpu")
    pix = np.stack(np.meshgrid(np.arange(64), np.arange(48), indexing="xy"), -1).reshape(-1, 2)
    o, d = (x.numpy() for x in camera_rays(cam, pix))
    t32, f32_, uv32 = rr.ray_mesh_ref(o, d, verts.astype(np.float32), faces)
    t64, f64_, uv64 = rr.ray_mesh_ref(o, d, verts.astype(np.float32), faces, dtype=np.float64)
    assert t32.dtype == np.float32 and uv32.dtype == np.float32 and t64.dtype == np.float64
    hit = f64_ >= 0
    print("hits %d of %d, max |t32 - t64| = %.3g" % (hit.sum(), len(hit), np.abs(t32[hit] - t64[hit]).max()))
    assert np.array_equal(f32_, f64_)
    assert 800 <= hit.sum() <= 1000                                                   # the torus fills about a third of the frame
    assert np.abs(t32[hit] - t64[hit]).max() <= 1e-5
    assert np.isinf(t32[~hit]).all() and np.isnan(uv32[~hit]).all() and np.abs(uv32[hit] - uv64[hit]).max() <= 1e-4


def test_reference_rules_on_hand_made_cases():
    """ties to the lowest index, -0 reported as +0, det = 0 and a zero direction miss, the bounds cut hits off, both sides hit"""
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1]], np.float32)
    F = np.array([[3, 4, 5], [0, 1, 2], [0, 1, 2], [0, 2, 1]], np.int32)               # the plane z = 1, then z = 0 three times (one flipped)
    O = np.array([[0.25, 0.25, -1], [0.25, 0.25, 0], [0.25, 0.25, 2], [0.25, 0.25, -1], [0.25, 0.25, 0.5], [0.25, 0.25, -1], [0, 0, -1]], np.float32)
    D = np.array([[0, 0, 1], [0, 0, -1], [0, 0, -1], [1, 0, 0], [1, 1, 0], [0, 0, 0], [0, 0, 1]], np.float32)
    t, f, uv = rr.ray_mesh_ref(O, D, V, F)
    assert f.tolist() == [1, 1, 0, -1, -1, -1, 1]
    assert t[:3].tolist() == [1.0, 0.0, 1.0] and not np.signbit(t[1]) and np.isinf(t[3:6]).all()
    assert np.array_equal(uv[0], [0.25, 0.25]) and np.isnan(uv[3:6]).all()
    assert rr.ray_mesh_ref(O[:1], D[:1], V, F, t_min=1.5)[1].tolist() == [0]            # the first hit cut off: the second wins
    assert rr.ray_mesh_ref(O[:1], D[:1], V, F, t_max=0.5)[1].tolist() == [-1]
    assert rr.ray_mesh_ref(O[:1], D[:1], V, F, t_min=1.0, t_max=1.0)[1].tolist() == [1]  # the bounds are inclusive


# ---- --pick_sequence ----
def test_pick_sequence_reader(tmp_path):
    from gaussianmesh_amd.edit_sequence import main, read_pick_sequence
    path = str(tmp_path / "picks.json")

    def refused(doc, word, raw=None):
        with open(path, "w") as fh:
            fh.write(raw if raw is not None else json.dumps(doc))
        with pytest.raises(SystemExit, match=word):
            read_pick_sequence(path)
    good = dict(camera_id=1, handles=[[10, 20], [30.5, 8]], anchors=[[5, 5]], offsets=[[[1, 0], [0, 1]], [[2, 0], [0, 2]], [[3, 0], [0, 3]]])
    refused(None, "JSON", raw="{not json")
    refused([1, 2], "JSON object")
    for cam in (None, -1, 1.5, "0", True):
        refused(dict(good, camera_id=cam), "camera_id")
    refused({k: v for k, v in good.items() if k != "camera_id"}, "camera_id")
    for h in ([], [[1, 2, 3]], [1, 2], "ab", [[1, None]], None):
        refused(dict(good, handles=h), '"handles"')
    refused(dict(good, anchors=[[1]]), '"anchors"')
    for o in (None, [], [[[1, 0]]], [[[1, 0], [0, 1], [2, 2]]], [[[1, 0, 0], [0, 1, 0]]], [[1, 0], [0, 1]], [[[1, 0], [0, float("inf")]]]):
        refused(dict(good, offsets=o), '"offsets"')
    with pytest.raises(SystemExit, match="cannot read"):
        read_pick_sequence(str(tmp_path / "missing.json"))
    with open(path, "w") as fh:
        json.dump(good, fh)
    cam, handles, anchors, offsets = read_pick_sequence(path)
    assert cam == 1 and handles.shape == (2, 2) and anchors.shape == (1, 2) and offsets.shape == (3, 2, 2) and offsets.dtype == np.float32
    del good["anchors"]
    with open(path, "w") as fh:
        json.dump(good, fh)
    assert read_pick_sequence(path)[2].shape == (0, 2)
    # the three sources exclude each other, and a bad file ends the run before anything is loaded
    common = ["--object_gaussian", "x.ply", "--object_origin_mesh", "x.obj", "--camera_path", str(tmp_path), "--render_path", str(tmp_path / "out")]
    with pytest.raises(SystemExit):
        main(common + ["--pick_sequence", path, "--handle_sequence", "h.npz"])
    with pytest.raises(SystemExit):
        main(common + ["--pick_sequence", path, "--mesh_sequence", str(tmp_path)])
    with open(path, "w") as fh:
        json.dump(dict(good, camera_id=None), fh)
    with pytest.raises(SystemExit, match="camera_id"):
        main(common + ["--pick_sequence", path])
