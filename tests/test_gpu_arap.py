"""-m gpu: gm_arap_solve (arap.ArapSolver) against the float64 reference of tests/arap_ref.py on the cases of tests/arap_cases.py, its
fixed points, inexact solves, determinism, aliasing and pinned vertices, and the edit surface on top of it (SingleObjectDeform.drag,
ObjectVisualTool.drag_one_gaussian, render_sequence over solver outputs, edit_sequence --handle_sequence --save_meshes)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import arap_cases as ac
from test_gpu_edittool import _write_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_solvers = {}


def _solver(name):
    from gaussianmesh_amd.arap import ArapSolver
    if name not in _solvers:
        c = ac.case(name)
        _solvers[name] = ArapSolver(c["V0"], c["faces"], c["handles"])
    return _solvers[name]


def _dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


# ---- 1. against the reference ----
@pytest.mark.parametrize("outer", [1, 2, 10])
@pytest.mark.parametrize("name", ac.NAMES)
def test_against_the_reference(name, outer):
    """max |V_hip - V_ref| <= 1e-6: coordinates are below 4, so the float32 rounding of the output is at most 1.2e-7, and PCG converged
    to 1e-10 stays within about 1e-9 of the exact global step the reference takes (test_arap_host: at most 4.3e-10).
    Both energies of every outer iteration within 1e-6 relative of the reference's.  The energies are far from zero on every case (the
    smallest is the one-handle case's 2.5e-5 after ten iterations, where the mesh is still settling towards a translation)."""
    c = ac.case(name)
    want, want_stats = ac.reference_run(name)
    V, stats = _solver(name).solve(c["targets"], outer_iterations=outer, cg_iterations=400, cg_tolerance=1e-10, want_stats=True)
    V, stats = V.cpu().numpy().astype(np.float64), stats.cpu().numpy()
    assert V.shape == want[0].shape and stats.shape == (outer, 8)
    err = float(np.abs(V - want[outer - 1]).max())
    print("%s outer %d: max |V_hip - V_ref| = %.3g, CG steps at most %d, residual at most %.3g" % (name, outer, err, int(stats[:, 2:5].max()), stats[:, 5:8].max()))
    assert err <= 1e-6
    assert np.array_equal(V[c["handles"]], c["targets"].astype(np.float64))          # the handles sit exactly on their targets
    assert (stats[:, 5:8] <= 1e-10).all() and (stats[:, 2:5] <= 400).all() and (stats[:, 2:5] == np.round(stats[:, 2:5])).all()
    e_rel = np.abs(stats[:, :2] - want_stats[:outer, :2]) / want_stats[:outer, :2]
    print("   energies:", stats[:, :2].reshape(-1), "largest relative deviation %.3g" % e_rel.max())
    assert (want_stats[:outer, :2] > 0).all() and (e_rel <= 1e-6).all()


# ---- 2. fixed points ----
def test_fixed_points():
    c = ac.case("torus_b")
    s = _solver("torus_b")
    V0 = c["V0"].astype(np.float64)
    V = s.solve(c["V0"][c["handles"]])                                               # handles at rest, rest-pose init
    assert float((V.cpu().numpy() - V0).__abs__().max()) <= 1e-6
    Q, t = ac.rotation((1, 2, -0.5), 0.9), np.array([0.3, -2.0, 5.0])
    rigid = (V0 @ Q.T + t).astype(np.float32)
    V = s.solve(rigid[c["handles"]], init=_dev(rigid))
    err = float(np.abs(V.cpu().numpy().astype(np.float64) - rigid).max())
    print("rigid image: %.3g" % err)
    assert err <= 1e-6
    one = ac.case("one_handle")
    moved = (one["V0"].astype(np.float64) + t).astype(np.float32)
    V = _solver("one_handle").solve(moved[one["handles"]], init=_dev(moved))
    err = float(np.abs(V.cpu().numpy().astype(np.float64) - moved).max())
    print("one handle, translated: %.3g" % err)
    assert err <= 1e-6


# ---- 3. inexact solves ----
@pytest.mark.parametrize("cg", [1, 3])
@pytest.mark.parametrize("name", ["torus_b", "flat_patch"])
def test_inexact_solves_never_raise_the_energy(name, cg):
    c = ac.case(name)
    V, stats = _solver(name).solve(c["targets"], outer_iterations=10, cg_iterations=cg, cg_tolerance=0.0, want_stats=True)
    stats = stats.cpu().numpy()
    chain = stats[:, :2].reshape(-1)                                                 # local, global, local, ...
    print(name, cg, chain)
    assert np.isfinite(chain).all() and torch.isfinite(V).all()
    assert (stats[:, 2:5] == cg).all()
    assert (np.diff(chain) <= 1e-9 * chain[0]).all()
    if cg == 3:
        assert chain[-1] < chain[0]


# ---- 4. determinism and aliasing ----
def test_determinism_aliasing_and_zero_iterations():
    c, s = ac.case("torus_c"), _solver("torus_c")
    tg = _dev(c["targets"])
    a = s.solve(tg).clone()
    b = s.solve(tg)
    assert torch.equal(a, b)
    st1 = s.solve(tg, want_stats=True)[1].clone()
    assert torch.equal(st1, s.solve(tg, want_stats=True)[1])
    init = _dev(ac.reference_run("torus_c")[0][0].astype(np.float32))                # some deformed start
    plain = s.solve(tg, init=init, outer_iterations=2)
    assert plain.data_ptr() != init.data_ptr()
    apart = torch.empty_like(init)
    assert s.solve(tg, init=init, outer_iterations=2, out=apart) is apart and torch.equal(apart, plain)   # V_out apart from V_init
    alias = init.clone()
    assert s.solve(tg, init=alias, outer_iterations=2, out=alias) is alias and torch.equal(alias, plain)  # V_out == V_init
    zero = s.solve(tg, init=init, outer_iterations=0)
    want = init.clone()
    want[_dev(c["handles"], torch.int64)] = tg
    assert torch.equal(zero, want)
    apart.zero_()
    s.solve(tg, init=init, outer_iterations=0, out=apart)
    assert torch.equal(apart, want)


# ---- 5. pinned vertices ----
def test_pinned_vertices_keep_their_place():
    from gaussianmesh_amd.arap import ArapSolver
    V0, faces = ac.pinned_mesh()
    tor = ac.case("torus_a")
    s = ArapSolver(V0, faces, tor["handles"])
    assert list(s.pinned) == [96, 97]
    init = V0.copy()
    init[96] = [1.25, -3.5, 0.75]
    init[97] = [-0.5, 2.0, 3.0]
    V = s.solve(tor["targets"], init=_dev(init), outer_iterations=3, cg_iterations=400, cg_tolerance=1e-10).cpu().numpy()
    assert np.array_equal(V[96:98], init[96:98])
    assert np.isfinite(V).all()
    ref = ac.reference_run("torus_a")[0][2]                                          # the torus itself deforms as without the extras
    assert np.abs(V[:96] - ref).max() <= 1e-6


# ---- 6. the edit surface ----
def _scene64(d):
    """_write_scene's object, mesh and files with three 64 x 64 cameras"""
    from gaussianmesh_amd import io as gio, scenes
    _write_scene(d)
    cams = []
    for k in range(3):
        c = scenes.orbit_camera(k, 7, 64, 64, radius=6.5)
        view = c["view"].reshape(4, 4).T.astype(np.float64)
        cams.append(gio.camera_to_json(k, view[:3, :3].T, view[:3, 3], 64, 64, c["fovx"], c["fovy"], "img_%d" % k))
    with open(os.path.join(d, "cameras.json"), "w") as f:
        json.dump(cams, f)


def _tool(d):
    from gaussianmesh_amd.edittool import ObjectVisualTool
    t = ObjectVisualTool()
    t.add_gaussian(os.path.join(d, "object.ply"), os.path.join(d, "rest.obj"), "Object")
    return t


def _drags(verts, T=3):
    """handles as on the test tori and T targets for them: the moved ring rotated and lifted a little more each frame"""
    V0 = np.asarray(verts, np.float32)
    ang = np.arctan2(V0[:, 2].astype(np.float64), V0[:, 0].astype(np.float64))
    still, moved = np.nonzero(np.abs(ang) < 0.25)[0], np.nonzero(np.abs(np.abs(ang) - math.pi) < 0.25)[0]
    pos = [np.concatenate([V0[still].astype(np.float64), V0[moved].astype(np.float64) @ ac.rotation((0, 0, 1), 0.2 * (k + 1)).T + [0, 0.25 * (k + 1), 0]], 0)
           for k in range(T)]
    return np.concatenate([still, moved]), np.asarray(pos, np.float32)


def test_drag_is_solve_then_deform_vertices(tmp_path):
    from gaussianmesh_amd.arap import ArapSolver
    d = str(tmp_path)
    _scene64(d)
    tool, other = _tool(d), _tool(d)
    o, p = tool.gaussians_list[0], other.gaussians_list[0]
    ids, pos = _drags(o.vertex.cpu().numpy())
    assert o.mesh_vertex_current is None
    assert isinstance(o.set_handles(ids), ArapSolver)
    got = o.drag(pos[0])
    solver = ArapSolver(p.vertex, p.faces, ids)
    V1 = solver.solve(pos[0])
    exp = p.deform_vertices(V1)
    assert len(got) == len(exp) == 3 and all(torch.equal(g, e) for g, e in zip(got, exp))
    assert torch.equal(o.mesh_vertex_current, V1)
    o.drag(pos[1], outer_iterations=2)                                               # warm start: from the first drag's mesh
    V2 = solver.solve(pos[1], init=V1, outer_iterations=2)
    assert torch.equal(o.mesh_vertex_current, V2)
    assert not torch.equal(V2, solver.solve(pos[1], outer_iterations=2))
    with pytest.raises(ValueError, match="set_handles"):
        p.drag(pos[0])
    # the tool: drag_one_gaussian + render_gaussian against deform_vertices + render_gaussian on the same vertices
    cam = tool.get_camera(d)[1]
    third, fourth = _tool(d), _tool(d)
    third.drag_one_gaussian("Object", ids, pos[0])
    fourth.gaussians_list[0].deform_vertices(V1)
    assert torch.equal(third.render_gaussian(cam), fourth.render_gaussian(cam))
    kept = third.gaussians_list[0].arap
    third.drag_one_gaussian("Object", ids, pos[1], outer_iterations=2)              # the same handles: the solver is kept, the drag warm-starts
    assert third.gaussians_list[0].arap is kept and torch.equal(third.gaussians_list[0].mesh_vertex_current, V2)


def test_tensor_in_object_drags_like_the_file_based_one(tmp_path):
    """deform.SingleObjectDeform built from tensors alone: set_handles(faces=...) supplies the mesh, drag and deform_vertices are the
    class's own"""
    from gaussianmesh_amd.deform import SingleObjectDeform as TensorObject
    d = str(tmp_path)
    _scene64(d)
    f = _tool(d).gaussians_list[0]
    t = TensorObject(f.gaussian_pos, f.gaussian_cov, f.gaussian_o, f.gaussian_feature, f.gaussian_triangles, f.coord, f.vertex, name="T")
    ids, pos = _drags(f.vertex.cpu().numpy())
    with pytest.raises(ValueError, match="no faces"):
        t.set_handles(ids)
    with pytest.raises(ValueError, match="no faces"):
        t.deform_vertices(f.vertex)
    t.set_handles(ids, faces=f.faces.cpu().numpy())
    f.set_handles(ids)
    for k in range(2):                                                               # the second drag warm-starts in both
        got, exp = t.drag(pos[k]), f.drag(pos[k])
        assert all(torch.equal(g, e) for g, e in zip(got, exp)) and torch.equal(t.mesh_vertex_current, f.mesh_vertex_current)


def test_render_sequence_over_solver_outputs(tmp_path):
    from gaussianmesh_amd import rasterizer as Rz
    from gaussianmesh_amd.deform import mesh_rs_packed
    d = str(tmp_path)
    _scene64(d)
    tool = _tool(d)
    o = tool.gaussians_list[0]
    ids, pos = _drags(o.vertex.cpu().numpy())
    solver = o.set_handles(ids)
    meshes, cur = [], None
    for k in range(3):
        cur = solver.solve(pos[k], init=cur)
        meshes.append(cur)
    cams = tool.get_camera(d)
    got = list(tool.render_sequence([(cams[k], {"Object": meshes[k]}) for k in range(3)], frames_per_launch=4))
    assert len(got) == 3
    bg = torch.ones(3, device="cuda")
    for k in range(3):
        cam = cams[k]
        table = mesh_rs_packed(o.vertex, meshes[k], o.faces, o._adjacency)
        exp = Rz.forward_deformed_begin(bg, o.gaussian_triangles, o.coord, table, o.gaussian_cov, o.gaussian_pos, o.gaussian_feature, o.gaussian_o,
                                        cam.world_view_transform, cam.full_proj_transform, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5),
                                        cam.image_height, cam.image_width, 3, cam.camera_center).finish(image_only=True)[1]
        assert got[k].shape == (3, 64, 64) and torch.equal(got[k], exp), k
        assert float((got[k] - 1.0).abs().max()) > 0.1                               # the object is in the picture


def test_cli_handle_sequence_writes_images_and_meshes(tmp_path):
    from gaussianmesh_amd import io as gio
    from gaussianmesh_amd.arap import ArapSolver
    d = str(tmp_path)
    _scene64(d)
    verts, faces = gio.read_obj(os.path.join(d, "rest.obj"))
    ids, pos = _drags(verts)
    np.savez(os.path.join(d, "handles.npz"), handles=ids, positions=pos)
    out = os.path.join(d, "renders")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "gaussianmesh_amd.edit_sequence", "--object_gaussian", os.path.join(d, "object.ply"),
                        "--object_origin_mesh", os.path.join(d, "rest.obj"), "--camera_path", d, "--render_path", out,
                        "--handle_sequence", os.path.join(d, "handles.npz"), "--save_meshes"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    solver = ArapSolver(verts.astype(np.float32), faces, ids)
    cur = None
    for k in range(3):
        cur = solver.solve(pos[k], init=cur)
        assert os.path.exists(os.path.join(out, "%05d.png" % k))
        v, f = gio.read_obj(os.path.join(out, "%05d.obj" % k))
        assert np.array_equal(f, faces) and np.array_equal(v, cur.cpu().numpy().astype(np.float64)), k
    assert sorted(os.listdir(out)) == ["%05d.%s" % (k, e) for k in range(3) for e in ("obj", "png")]
