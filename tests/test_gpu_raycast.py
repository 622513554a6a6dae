"""-m gpu: gm_ray_mesh (mesh_pick.ray_mesh_hits) against its definition - the float32 brute force of tests/ray_ref.py, bit for bit in t,
face and (u, v) - at every size where a face chunk, a partial wave or the merge can go wrong and on inputs made to hurt; then the glue
above it: pick, visible_vertices, SingleObjectDeform.pick / drag_pixels, and the CLI's --pick_sequence against --handle_sequence."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import ray_ref as rr
from test_gpu_arap import _drags, _scene64, _tool

pytestmark = pytest.mark.gpu
f32 = np.float32
CHUNK = 64                      # RC_CHUNK of csrc/gm_raycast.hip: faces per workgroup
R_MAX = 3000


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


def _device_cast(O, D, V, F, **kw):
    from gaussianmesh_amd.mesh_pick import ray_mesh_hits
    t, face, uv = ray_mesh_hits(_dev(O), _dev(D), V, F, **kw)
    torch.cuda.synchronize()
    return t.cpu().numpy(), face.cpu().numpy(), uv.cpu().numpy()


def _same(got, ref, what, rows=None):
    (t, face, uv), (rt, rface, ruv) = ((x if rows is None else x[rows]) for x in got), ((x if rows is None else x[rows]) for x in ref)
    bad = np.nonzero(face != rface)[0]
    assert len(bad) == 0, "%s: %d faces differ, first row %d: device %d (t %r) brute force %d (t %r)" % (
        what, len(bad), bad[0], face[bad[0]], t[bad[0]], rface[bad[0]], rt[bad[0]])
    assert np.array_equal(_bits(t), _bits(rt)), "%s: t bits differ" % what
    hit = rface >= 0
    assert np.array_equal(_bits(uv[hit]), _bits(ruv[hit])), "%s: (u, v) bits differ" % what
    assert np.isnan(uv[~hit]).all() and np.isinf(t[~hit]).all() and not np.signbit(t).any()


@functools.lru_cache(maxsize=None)
def _case(family, F):
    """(V, faces, O, D, brute force) with R_MAX rays, computed once; the smaller ray counts take a prefix of it"""
    rng = np.random.default_rng(1000 + F)
    if family == "grid":
        V, faces = rr.grid(F)
        O, D = rr.grid_rays(V, R_MAX, rng)
    else:
        V, faces = rr.torus(F)
        O, D = rr.torus_rays(V, faces, R_MAX, rng)
    return V, faces, O, D, rr.ray_mesh_ref(O, D, V, faces)


# ---- 1. every size at which a chunk edge, a partial wave or the merge can go wrong ----
@pytest.mark.parametrize("R", [1, 63, 64, 65, 257, R_MAX])
@pytest.mark.parametrize("F", [1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, 5000])
@pytest.mark.parametrize("family", ["grid", "torus"])
def test_sizes_bit_for_bit(family, F, R):
    V, faces, O, D, ref = _case(family, F)
    assert len(faces) == F
    _same(_device_cast(O[:R], D[:R], V, faces), tuple(x[:R] for x in ref), "%s F=%d R=%d" % (family, F, R))


def test_the_hurtful_families_hold_what_they_promise():
    """the grid case really has exact ties, -0 hits, parallel rays and misses; the torus case rays with several crossings"""
    V, faces, O, D, (t, face, uv) = _case("grid", 5000)
    n = 600
    hit, tt, _, _ = rr.ray_face(O[:n, None, :], D[:n, None, :], V[faces[:, 0]][None], V[faces[:, 1]][None], V[faces[:, 2]][None])
    assert ((hit & (tt == t[:n, None])).sum(axis=1) >= 2)[face[:n] >= 0].all()         # every hit is a tie (each face is there twice)
    assert (face >= 0).sum() > 1000 and (face < 0).sum() > 500
    assert (hit & np.signbit(tt)).any() and not np.signbit(t).any()                    # t = -0 occurs among the hits and is reported as +0
    assert (face[(D == 0).all(axis=1)] == -1).all() and (face[D[:, 2] == 0] == -1).all()
    V, faces, O, D, (t, face, uv) = _case("torus", 5000)
    hit = rr.ray_face(O[:500, None, :], D[:500, None, :], V[faces[:, 0]][None], V[faces[:, 1]][None], V[faces[:, 2]][None])[0]
    assert (hit.sum(axis=1) >= 8).any() and (face >= 0).sum() > 2000 and (face < 0).sum() > 100


# ---- 2. inputs made to hurt ----
def test_zero_area_faces_mixed_in():
    rng = np.random.default_rng(7)
    for family, F in (("grid", 1000), ("torus", 1000)):
        V, faces = (rr.grid if family == "grid" else rr.torus)(F)
        faces = rr.with_degenerate_faces(V, faces, rng)
        O, D = rr.grid_rays(V, 1000, rng) if family == "grid" else rr.torus_rays(V, faces, 1000, rng)
        ref = rr.ray_mesh_ref(O, D, V, faces)
        assert (ref[1] >= 0).sum() > 200
        _same(_device_cast(O, D, V, faces), ref, family)
    V, faces = rr.torus(200)
    faces[:, 2] = faces[:, 0]                                                          # no face with area at all: nothing is hit
    O, D = rr.torus_rays(*rr.torus(200), 300, rng)
    t, face, uv = _device_cast(O, D, V, faces)
    assert (face == -1).all() and np.isinf(t).all() and np.isnan(uv).all()


def test_bounds_cut_off_the_first_hit():
    V, faces, O, D, ref = _case("torus", 5000)
    O, D = O[:1000], D[:1000]
    for t_min, t_max in ((0.9, math.inf), (0.0, 0.8), (0.9, 1.3), (1.0, 1.0), (0.0, 0.0)):
        cut = rr.ray_mesh_ref(O, D, V, faces, t_min=t_min, t_max=t_max)
        if t_min < t_max:
            later = (cut[1] >= 0) & (cut[1] != ref[1][:1000])
            assert later.sum() > 20 if t_min else (cut[1] < 0).sum() > (ref[1][:1000] < 0).sum()      # a second hit wins / a hit is lost
        _same(_device_cast(O, D, V, faces, t_min=t_min, t_max=t_max), cut, "t in [%g, %g]" % (t_min, t_max))
    V, faces, O, D, _ = _case("grid", 5000)                                            # origins on the plane: t = +-0 passes t_max = 0
    cut = rr.ray_mesh_ref(O, D, V, faces, t_max=0.0)
    assert (cut[1] >= 0).sum() > 50
    _same(_device_cast(O, D, V, faces, t_max=0.0), cut, "grid, t_max = 0")


def _raw_call(O, D, V, faces, want_uv=True):
    """gm_ray_mesh through ctypes on device buffers: (t, face, uv or None)"""
    from gaussianmesh_amd import _lib
    lib = _lib.lib()
    o, d, v, f = _dev(O), _dev(D), _dev(V), _dev(faces, torch.int32)
    R = o.shape[0]
    t = torch.full((R,), -7.0, device="cuda"); face = torch.full((R,), -7, dtype=torch.int32, device="cuda")
    uv = torch.full((R, 2), -7.0, device="cuda")
    nbytes = lib.gm_ray_mesh_workspace_bytes(R, f.shape[0])
    ws = torch.empty((nbytes + 64,), dtype=torch.uint8, device="cuda")
    _lib.check(lib.gm_ray_mesh(R, o.data_ptr(), d.data_ptr(), v.shape[0], v.data_ptr(), f.shape[0], f.data_ptr(), 0.0, math.inf, t.data_ptr(),
                               face.data_ptr(), uv.data_ptr() if want_uv else None, ws.data_ptr() + 4, nbytes,          # (an odd workspace address)
                               torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return t.cpu().numpy(), face.cpu().numpy().astype(np.int64), uv.cpu().numpy()


def test_same_bits_twice_and_without_uv():
    V, faces, O, D, ref = _case("torus", 5000)
    one, two = _raw_call(O, D, V, faces), _raw_call(O, D, V, faces)
    _same(one, ref, "through ctypes")
    assert all(np.array_equal(a.view(np.uint32) if a.dtype == f32 else a, b.view(np.uint32) if b.dtype == f32 else b) for a, b in zip(one, two))
    t, face, uv = _raw_call(O, D, V, faces, want_uv=False)
    assert np.array_equal(_bits(t), _bits(one[0])) and np.array_equal(face, one[1]) and (uv == -7.0).all()      # out_uv = NULL: nothing written there


def test_a_face_index_out_of_range_does_not_fault():
    """one face with indices outside [0, Vm): forced into range on the device (no fault); the rays that such a face could claim are
    not compared, every other ray is"""
    V, faces, O, D, _ = _case("grid", 2 * CHUNK + 1)
    bad = faces.copy()
    bad[77] = (-3, len(V) + 5, 7)                                                      # forced to (0, Vm - 1, 7): a face with area
    forced = bad.copy(); forced[77] = np.clip(bad[77], 0, len(V) - 1)
    ref = rr.ray_mesh_ref(O, D, V, forced)
    hit77 = rr.ray_face(O, D, V[forced[77, 0]][None], V[forced[77, 1]][None], V[forced[77, 2]][None])[0]
    got = _raw_call(O, D, V, bad)
    assert hit77.sum() > 10 and (~hit77).sum() > R_MAX // 2
    _same(got, ref, "face 77 out of range", rows=~hit77)


# ---- 3. pick / visible_vertices on the torus ----
def _torus_camera():
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.renderer import Camera
    cd = scenes.look_at_camera((4, 3, 5), (0, 0, 0), 64, 48)
    verts, faces = scenes.torus_mesh(24, 16)
    return cd, Camera(cd, "cuda"), verts.astype(f32), faces


def test_pick_on_the_torus():
    from gaussianmesh_amd.mesh_pick import camera_rays, pick
    cd, cam, verts, faces = _torus_camera()
    pix = np.stack(np.meshgrid(np.arange(64), np.arange(48), indexing="xy"), -1).reshape(-1, 2).astype(f32)
    out = {k: v.cpu().numpy() for k, v in pick(cam, pix, verts, faces).items()}
    o, d = (x.cpu().numpy() for x in camera_rays(cam, pix))
    t, face, uv = rr.ray_mesh_ref(o, d, verts, faces)                                  # the device's own rays through the brute force
    assert np.array_equal(out["face"], face) and np.array_equal(_bits(out["depth"]), _bits(t))
    hit = face >= 0
    assert 800 <= hit.sum() <= 1000
    assert (out["vertex"][~hit] == -1).all() and np.isnan(out["point"][~hit]).all() and np.isinf(out["depth"][~hit]).all()
    tri = faces[face[hit]].astype(np.int64)
    w = np.stack([f32(1) - uv[hit, 0] - uv[hit, 1], uv[hit, 0], uv[hit, 1]], 1)
    assert np.array_equal(out["vertex"][hit], tri[np.arange(len(tri)), np.argmax(w, axis=1)])      # a corner of the face: the heaviest, the first of equals
    a, b, c = (verts[tri[:, k]] for k in range(3))
    assert np.array_equal(_bits(out["point"][hit]), _bits((a + (b - a) * uv[hit, :1]) + (c - a) * uv[hit, 1:]))
    # the hit point returns to its pixel through full_proj_transform and ndc2pix (float64 on the host)
    h = np.concatenate([out["point"][hit].astype(np.float64), np.ones((hit.sum(), 1))], 1) @ np.asarray(cd["proj"], np.float64)
    back = np.stack([((h[:, 0] / h[:, 3] + 1) * 64 - 1) * 0.5, ((h[:, 1] / h[:, 3] + 1) * 48 - 1) * 0.5], 1)
    err = np.abs(back - pix[hit]).max()
    print("pick: %d hits, reprojection error %.3g px" % (hit.sum(), err))
    assert err <= 1e-3
    assert np.abs(h[:, 3] - out["depth"][hit]).max() <= 1e-4                           # depth is the view depth


def _visible_rule64(cd, verts, faces, rect=None):
    """visible_vertices' definition evaluated in float64 on the host: (mask, the smallest distance in pixels of a vertex from the
    rectangle's edges)"""
    o = np.asarray(cd["campos"], np.float64)
    V = verts.astype(np.float64)
    t, face, _ = rr.ray_mesh_ref(np.broadcast_to(o, V.shape), V - o, V, faces, dtype=np.float64)
    own = (faces[np.maximum(face, 0)] == np.arange(len(V))[:, None]).any(axis=1)
    vis = (face < 0) | own | (t >= 1.0 - 2.0 ** -10)
    margin = np.inf
    if rect is not None:
        view = np.asarray(cd["view"], np.float64)
        pv = V @ view[:3, :3] + view[3, :3]
        px = ((pv[:, 0] / (pv[:, 2] * cd["tanx"]) + 1) * cd["W"] - 1) * 0.5
        py = ((pv[:, 1] / (pv[:, 2] * cd["tany"]) + 1) * cd["H"] - 1) * 0.5
        x0, y0, x1, y1 = rect
        vis &= (pv[:, 2] > 0) & (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)
        margin = min(np.abs(px - x0).min(), np.abs(px - x1).min(), np.abs(py - y0).min(), np.abs(py - y1).min())
    return vis, (face < 0).sum(), margin


def test_visible_vertices_on_the_torus():
    from gaussianmesh_amd.mesh_pick import visible_vertices
    cd, cam, verts, faces = _torus_camera()
    exp, slipped, _ = _visible_rule64(cd, verts, faces)
    got = visible_vertices(cam, verts, faces)
    assert got.dtype == torch.bool and got.shape == (384,)
    print("visible: %d of 384 (float64 rule %d), %d rays hit nothing" % (int(got.sum()), exp.sum(), slipped))
    assert np.array_equal(got.cpu().numpy(), exp)
    assert 150 <= exp.sum() <= 230                                                     # about half of the torus faces the eye
    for rect in ((20.3, 10.3, 44.7, 30.7), (-5.0, -5.0, 100.0, 100.0), (1.3, 1.3, 9.7, 8.7)):
        exp_r, _, margin = _visible_rule64(cd, verts, faces, rect)
        assert margin > 1e-3                                                           # no vertex so close to an edge that float32 could differ
        assert np.array_equal(visible_vertices(cam, verts, faces, rect=rect).cpu().numpy(), exp_r), rect
    assert np.array_equal(_visible_rule64(cd, verts, faces, (-5.0, -5.0, 100.0, 100.0))[0], exp)


# ---- 4. the edit surface ----
def _all_pixels(n=64):
    return np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="xy"), -1).reshape(-1, 2).astype(f32)


def test_object_pick_follows_the_drag(tmp_path):
    d = str(tmp_path)
    _scene64(d)
    tool = _tool(d)
    o = tool.gaussians_list[0]
    cam = tool.get_camera(d)[1]
    pix = _all_pixels()
    rest = {k: v.cpu().numpy() for k, v in o.pick(cam, pix).items()}
    assert np.array_equal(rest["face"], tool.pick_one_gaussian("Object", cam, pix)["face"].cpu().numpy())
    ids, pos = _drags(o.vertex.cpu().numpy())
    o.set_handles(ids)
    o.drag(pos[2])
    after = {k: v.cpu().numpy() for k, v in o.pick(cam, pix).items()}
    from gaussianmesh_amd.mesh_pick import camera_rays
    rays = [x.cpu().numpy() for x in camera_rays(cam, pix)]
    faces = o.faces.cpu().numpy()
    for got, V in ((rest, o.vertex), (after, o.mesh_vertex_current)):
        t, face, _ = rr.ray_mesh_ref(rays[0], rays[1], V.cpu().numpy(), faces)
        assert np.array_equal(got["face"], face) and np.array_equal(_bits(got["depth"]), _bits(t))
    left = (rest["face"] >= 0) & (after["face"] < 0)                                   # pixels the rest mesh covers and the dragged mesh does not
    entered = (rest["face"] < 0) & (after["face"] >= 0)
    print("pixels left %d, entered %d" % (left.sum(), entered.sum()))
    assert left.sum() >= 5 and entered.sum() >= 5
    vis = o.select_visible(cam)
    from gaussianmesh_amd.mesh_pick import visible_vertices
    assert vis.dtype == torch.int64 and torch.equal(vis, torch.nonzero(visible_vertices(cam, o.mesh_vertex_current, o.faces))[:, 0])
    assert 0 < len(vis) < o.vertex.shape[0]
    inside = o.select_visible(cam, rect=(0, 0, 31.5, 63))
    assert 0 < len(inside) < len(vis) and np.isin(inside.cpu().numpy(), vis.cpu().numpy()).all()


def test_drag_pixels_is_drag_of_screen_offset(tmp_path):
    from gaussianmesh_amd.mesh_pick import screen_offset
    d = str(tmp_path)
    _scene64(d)
    a, b = _tool(d).gaussians_list[0], _tool(d).gaussians_list[0]
    cam = _tool(d).get_camera(d)[1]
    ids, _ = _drags(a.vertex.cpu().numpy())
    rng = np.random.default_rng(4)
    a.set_handles(ids); b.set_handles(ids)
    idx = torch.as_tensor(ids, device="cuda")
    for k in range(2):                                                                 # the second call starts from the first one's mesh
        off = _dev(rng.uniform(-6, 6, size=(len(ids), 2)))
        at = (b.vertex if b.mesh_vertex_current is None else b.mesh_vertex_current)[idx]
        got, exp = a.drag_pixels(cam, off, outer_iterations=2), b.drag(screen_offset(cam, at, off), outer_iterations=2)
        assert all(torch.equal(g, e) for g, e in zip(got, exp)) and torch.equal(a.mesh_vertex_current, b.mesh_vertex_current), k
        assert not torch.equal(a.mesh_vertex_current[idx], at)


def test_pick_drag_render_enqueue_without_a_host_wait(tmp_path):
    """with the face tensor checked once and the pixels on the device, pick -> drag_pixels -> pick -> render only enqueues: torch's
    synchronisation check stays silent"""
    d = str(tmp_path)
    _scene64(d)
    tool = _tool(d)
    o = tool.gaussians_list[0]
    cam = tool.get_camera(d)[1]
    pix = _dev(_all_pixels()[::37])
    ids = np.unique(o.pick(cam, pix)["vertex"].cpu().numpy())                          # the read-back that chooses the handles
    ids = ids[ids >= 0]
    assert len(ids) >= 4
    o.set_handles(ids)
    off = _dev(np.tile([[3.0, -2.0]], (len(ids), 1)))
    o.drag_pixels(cam, off); tool.render_gaussian(cam)                                 # warm: libraries and caches initialise
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        o.drag_pixels(cam, off)
        picked = o.pick(cam, pix)
        image = tool.render_gaussian(cam)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert image.shape == (3, 64, 64) and bool((picked["face"] >= 0).any())


def _run_cli(d, out, source):
    from gaussianmesh_amd.edit_sequence import main
    return main(["--object_gaussian", os.path.join(d, "object.ply"), "--object_origin_mesh", os.path.join(d, "rest.obj"), "--camera_path", d,
                 "--render_path", out, "--save_meshes", "--camera_id", "1"] + source)


def test_cli_pick_sequence_equals_the_handle_sequence(tmp_path):
    from gaussianmesh_amd.mesh_pick import screen_offset
    d = str(tmp_path)
    _scene64(d)
    tool = _tool(d)
    o, cam = tool.gaussians_list[0], tool.get_camera(d)[1]
    pix = _all_pixels()
    vertex = o.pick(cam, pix)["vertex"].cpu().numpy()
    hits = np.nonzero(vertex >= 0)[0]
    chosen = [hits[0], hits[-1], hits[len(hits) // 2], hits[len(hits) // 3]]           # two handles, two anchors
    ids = vertex[chosen]
    assert len(set(ids.tolist())) == 4
    offsets = np.array([[[2.0 * (k + 1), -1.5 * (k + 1)], [-1.0 * (k + 1), 2.5 * (k + 1)]] for k in range(3)], f32)
    doc = dict(camera_id=1, handles=pix[chosen[:2]].tolist(), anchors=pix[chosen[2:]].tolist(), offsets=offsets.tolist())
    picks = os.path.join(d, "picks.json")
    with open(picks, "w") as fh:
        json.dump(doc, fh)
    assert _run_cli(d, os.path.join(d, "by_pick"), ["--pick_sequence", picks]) == 3
    rest = o.vertex[torch.as_tensor(ids, device="cuda")]
    positions = np.stack([torch.cat([screen_offset(cam, rest[:2], _dev(offsets[k])), rest[2:]], 0).cpu().numpy() for k in range(3)])
    np.savez(os.path.join(d, "handles.npz"), handles=ids, positions=positions)
    assert _run_cli(d, os.path.join(d, "by_handle"), ["--handle_sequence", os.path.join(d, "handles.npz")]) == 3
    names = sorted(os.listdir(os.path.join(d, "by_pick")))
    assert names == ["%05d.%s" % (k, e) for k in range(3) for e in ("obj", "png")] == sorted(os.listdir(os.path.join(d, "by_handle")))
    for n in names:
        assert open(os.path.join(d, "by_pick", n), "rb").read() == open(os.path.join(d, "by_handle", n), "rb").read(), n
    from gaussianmesh_amd import io as gio
    moved = gio.read_obj(os.path.join(d, "by_pick", "00002.obj"))[0]
    assert np.array_equal(moved[ids], positions[2].astype(np.float64)) and np.abs(moved - o.vertex.cpu().numpy()).max() > 0.05
    # a pick that misses the mesh, two picks of one vertex, a camera that is not there: the run ends and says which
    for change, word in ((dict(handles=[pix[chosen[0]].tolist(), [0.0, 0.0]]), "handle 1 at pixel .* misses the mesh"),
                         (dict(anchors=[pix[chosen[0]].tolist()], ), "handle 0 and anchor 0 pick the same vertex"),
                         (dict(camera_id=9), "camera_id 9")):
        with open(picks, "w") as fh:
            json.dump(dict(doc, **change), fh)
        with pytest.raises(SystemExit, match=word):
            _run_cli(d, os.path.join(d, "refused"), ["--pick_sequence", picks])
