"""-m gpu: the whole-chip ARAP global step (gm_arap_solve_grid, ArapSolver.solve(global_step="grid")) held to what test_gpu_arap.py
holds the column step to, with that file's tolerances: the float64 reference on the cases of arap_cases.py (1, 3 and 5 workgroups, a
last one of 49 rows) and on the workgroup-edge cases of arap_grid_cases.py, fixed points, inexact solves, determinism, aliasing, pinned
vertices; then grid against column on the device at 30 and 258 workgroups, and the edit surface (drag, edit_sequence --arap_global_step)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import arap_cases as ac
import arap_grid_cases as gc
from test_gpu_arap import _drags, _scene64, _tool

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_solvers = {}


def _case(name):
    return gc.case(name) if name in gc.NAMES else ac.case(name)


def _solver(name):
    from gaussianmesh_amd.arap import ArapSolver
    if name not in _solvers:
        c = _case(name)
        _solvers[name] = ArapSolver(c["V0"], c["faces"], c["handles"])
    return _solvers[name]


def _dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


def _hold_to_reference(name, outer, want, want_stats, init=None):
    """test_gpu_arap.test_against_the_reference's assertions, on the grid path"""
    c = _case(name)
    V, stats = _solver(name).solve(c["targets"], init=init, outer_iterations=outer, cg_iterations=400, cg_tolerance=1e-10, want_stats=True,
                                   global_step="grid")
    V, stats = V.cpu().numpy().astype(np.float64), stats.cpu().numpy()
    assert V.shape == want[0].shape and stats.shape == (outer, 8)
    err = float(np.abs(V - want[outer - 1]).max())
    print("%s outer %d: max |V_grid - V_ref| = %.3g, CG steps at most %d, residual at most %.3g" % (name, outer, err, int(stats[:, 2:5].max()), stats[:, 5:8].max()))
    assert err <= 1e-6
    assert np.array_equal(V[c["handles"]], c["targets"].astype(np.float64))          # the handles sit exactly on their targets
    assert (stats[:, 5:8] <= 1e-10).all() and (stats[:, 2:5] <= 400).all() and (stats[:, 2:5] == np.round(stats[:, 2:5])).all()
    e_rel = np.abs(stats[:, :2] - want_stats[:outer, :2]) / want_stats[:outer, :2]
    print("   energies:", stats[:, :2].reshape(-1), "largest relative deviation %.3g" % e_rel.max())
    assert (want_stats[:outer, :2] > 0).all() and (e_rel <= 1e-6).all()
    return V


# ---- 1. against the reference: 96, 600, 1073, 108, 41 and 1073 rows ----
@pytest.mark.parametrize("outer", [1, 2, 10])
@pytest.mark.parametrize("name", ac.NAMES)
def test_against_the_reference(name, outer):
    """max |V_grid - V_ref| <= 1e-6 (float32 rounding of the output 1.2e-7, PCG at 1e-10 within about 1e-9 of the exact global step),
    every column converged, both energies of every outer iteration within 1e-6 relative"""
    _hold_to_reference(name, outer, *ac.reference_run(name))


# ---- 2. workgroup edges: exactly one full workgroup; one more row, pinned ----
@pytest.mark.parametrize("outer", [1, 2, 10])
@pytest.mark.parametrize("name", gc.NAMES)
def test_workgroup_edges_against_the_reference(name, outer):
    c = gc.case(name)
    assert len(c["V0"]) == (256 if name == "one_block" else 257)
    V = _hold_to_reference(name, outer, *gc.reference_run(name), init=_dev(c["init"]))
    if name == "one_block_plus_pinned":
        assert list(_solver(name).pinned) == [256]
        assert np.array_equal(V[256], np.asarray(gc.EXTRA_START, np.float32).astype(np.float64))   # kept exactly


# ---- 3. fixed points ----
def test_fixed_points():
    c = ac.case("torus_b")
    s = _solver("torus_b")
    V0 = c["V0"].astype(np.float64)
    V = s.solve(c["V0"][c["handles"]], global_step="grid")                           # handles at rest, rest-pose init
    assert float(np.abs(V.cpu().numpy() - V0).max()) <= 1e-6
    Q, t = ac.rotation((1, 2, -0.5), 0.9), np.array([0.3, -2.0, 5.0])
    rigid = (V0 @ Q.T + t).astype(np.float32)
    V = s.solve(rigid[c["handles"]], init=_dev(rigid), global_step="grid")
    err = float(np.abs(V.cpu().numpy().astype(np.float64) - rigid).max())
    print("rigid image: %.3g" % err)
    assert err <= 1e-6
    one = ac.case("one_handle")
    moved = (one["V0"].astype(np.float64) + t).astype(np.float32)
    V = _solver("one_handle").solve(moved[one["handles"]], init=_dev(moved), global_step="grid")
    err = float(np.abs(V.cpu().numpy().astype(np.float64) - moved).max())
    print("one handle, translated: %.3g" % err)
    assert err <= 1e-6


# ---- 4. inexact solves ----
@pytest.mark.parametrize("cg", [1, 3])
@pytest.mark.parametrize("name", ["torus_b", "flat_patch"])
def test_inexact_solves_never_raise_the_energy(name, cg):
    c = ac.case(name)
    V, stats = _solver(name).solve(c["targets"], outer_iterations=10, cg_iterations=cg, cg_tolerance=0.0, want_stats=True, global_step="grid")
    stats = stats.cpu().numpy()
    chain = stats[:, :2].reshape(-1)                                                 # local, global, local, ...
    print(name, cg, chain)
    assert np.isfinite(chain).all() and torch.isfinite(V).all()
    assert (stats[:, 2:5] == cg).all()
    assert (np.diff(chain) <= 1e-9 * chain[0]).all()
    if cg == 3:
        assert chain[-1] < chain[0]


# ---- 5. determinism, aliasing, zero iterations, the two paths side by side ----
def test_determinism_aliasing_and_zero_iterations():
    c, s = ac.case("torus_c"), _solver("torus_c")
    tg = _dev(c["targets"])
    g = dict(global_step="grid")
    a = s.solve(tg, **g).clone()
    assert torch.equal(a, s.solve(tg, **g))
    v1, st1 = s.solve(tg, want_stats=True, **g)
    v1, st1 = v1.clone(), st1.clone()
    v2, st2 = s.solve(tg, want_stats=True, **g)
    assert torch.equal(st1, st2) and torch.equal(v1, v2)
    assert torch.equal(v1, a)                                                        # asking for the statistics moves no bit of the mesh
    init = _dev(ac.reference_run("torus_c")[0][0].astype(np.float32))                # some deformed start
    plain = s.solve(tg, init=init, outer_iterations=2, **g)
    assert plain.data_ptr() != init.data_ptr()
    apart = torch.empty_like(init)
    assert s.solve(tg, init=init, outer_iterations=2, out=apart, **g) is apart and torch.equal(apart, plain)   # V_out apart from V_init
    alias = init.clone()
    assert s.solve(tg, init=alias, outer_iterations=2, out=alias, **g) is alias and torch.equal(alias, plain)  # V_out == V_init
    zero = s.solve(tg, init=init, outer_iterations=0, **g)
    want = init.clone()
    want[_dev(c["handles"], torch.int64)] = tg
    assert torch.equal(zero, want)
    apart.zero_()
    s.solve(tg, init=init, outer_iterations=0, out=apart, **g)
    assert torch.equal(apart, want)
    assert s.solve(tg, outer_iterations=0, want_stats=True, **g)[1].shape == (0, 8)


def test_alternating_paths_on_one_solver_leave_each_other_alone():
    """the two workspaces are separate: column, grid, column, grid on one solver object give each path the bits it gives alone"""
    from gaussianmesh_amd.arap import ArapSolver
    c = ac.case("torus_c")
    tg = _dev(c["targets"])
    alone = {}
    for path in ("column", "grid"):
        fresh = ArapSolver(c["V0"], c["faces"], c["handles"])
        alone[path] = [t.clone() for t in fresh.solve(tg, want_stats=True, global_step=path)]
        if path == "column":
            assert fresh._grid_ws is None                                            # made by the first grid solve only
            assert torch.equal(alone[path][0], fresh.solve(tg))                      # the default is the column path
    s = ArapSolver(c["V0"], c["faces"], c["handles"])
    for path in ("column", "grid", "column", "grid"):
        V, st = s.solve(tg, want_stats=True, global_step=path)
        assert torch.equal(V, alone[path][0]) and torch.equal(st, alone[path][1]), path
    assert s._grid_ws is not None and s._grid_ws.data_ptr() != s._ws.data_ptr()
    kept = s._grid_ws
    s.solve(tg, global_step="grid")
    assert s._grid_ws is kept


# ---- 6. pinned vertices ----
def test_pinned_vertices_keep_their_place():
    from gaussianmesh_amd.arap import ArapSolver
    V0, faces = ac.pinned_mesh()
    tor = ac.case("torus_a")
    s = ArapSolver(V0, faces, tor["handles"])
    assert list(s.pinned) == [96, 97]
    init = V0.copy()
    init[96] = [1.25, -3.5, 0.75]
    init[97] = [-0.5, 2.0, 3.0]
    V = s.solve(tor["targets"], init=_dev(init), outer_iterations=3, cg_iterations=400, cg_tolerance=1e-10, global_step="grid").cpu().numpy()
    assert np.array_equal(V[96:98], init[96:98])
    assert np.isfinite(V).all()
    ref = ac.reference_run("torus_a")[0][2]                                          # the torus itself deforms as without the extras
    assert np.abs(V[:96] - ref).max() <= 1e-6


# ---- 7. grid against column at size ----
@pytest.mark.parametrize("nu, nv, options", [(100, 75, {}), (300, 220, dict(outer_iterations=1, cg_iterations=8))])
def test_grid_against_column_at_size(nu, nv, options):
    """7 500 rows (30 workgroups) at the defaults, and 66 000 rows: 258 workgroups, more slots than a workgroup has threads.
    max |V_grid - V_column| <= 1e-6 and energies within 1e-6 relative.  The bound is derived: both paths run the same recurrences in
    float64 with the sums in another order, which in a numpy restatement on these inputs moved the result by 2e-14 to 3e-14 after all
    steps; what remains is the float32 rounding of the output, one ulp of which is 2.4e-7 for coordinates below 4.  Step counts of the
    two paths need not be equal."""
    from gaussianmesh_amd.arap import ArapSolver
    V0, faces, handles, targets = ac._torus(nu, nv)
    assert len(V0) == nu * nv and np.abs(targets).max() < 4.0
    s = ArapSolver(V0, faces, handles)
    tg = _dev(targets)
    Vc, sc = s.solve(tg, want_stats=True, global_step="column", **options)
    Vg, sg = s.solve(tg, want_stats=True, global_step="grid", **options)
    sc, sg = sc.cpu().numpy(), sg.cpu().numpy()
    err = float((Vg - Vc).abs().max())
    e_rel = np.abs(sg[:, :2] - sc[:, :2]) / sc[:, :2]
    print("%d rows: max |V_grid - V_column| = %.3g, energies relative %.3g, steps column %s grid %s" % (
        len(V0), err, e_rel.max(), sc[:, 2:5].astype(int).tolist(), sg[:, 2:5].astype(int).tolist()))
    assert torch.isfinite(Vg).all() and float(Vg.abs().max()) < 4.0
    assert err <= 1e-6
    assert (sc[:, :2] > 0).all() and (e_rel <= 1e-6).all()
    assert torch.equal(Vg.index_select(0, _dev(handles, torch.int64)), tg)


# ---- 8. the edit surface ----
def test_drag_with_the_grid_step_is_solve_then_deform_vertices(tmp_path):
    from gaussianmesh_amd.arap import ArapSolver
    d = str(tmp_path)
    _scene64(d)
    o, p = _tool(d).gaussians_list[0], _tool(d).gaussians_list[0]
    ids, pos = _drags(o.vertex.cpu().numpy())
    o.set_handles(ids)
    solver = ArapSolver(p.vertex, p.faces, ids)
    current = None
    for k in range(2):                                                               # the second drag warm-starts from the first one's mesh
        got = o.drag(pos[k], global_step="grid")
        current = solver.solve(pos[k], init=current, global_step="grid")
        exp = p.deform_vertices(current)
        assert len(got) == len(exp) == 3 and all(torch.equal(g, e) for g, e in zip(got, exp))
        assert torch.equal(o.mesh_vertex_current, current)
    with pytest.raises(ValueError, match="global_step"):
        o.drag(pos[0], global_step="bogus")


def test_cli_arap_global_step_grid_writes_the_column_runs_meshes(tmp_path):
    """--arap_global_step grid --save_meshes: the meshes of the grid path bit for bit (the option reaches the solver), and within 1e-6 of
    the column run's (which test_gpu_arap.test_cli_handle_sequence_writes_images_and_meshes shows to be this process's column solves)"""
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
                        "--handle_sequence", os.path.join(d, "handles.npz"), "--save_meshes", "--arap_global_step", "grid"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    solver = ArapSolver(verts.astype(np.float32), faces, ids)
    grid = column = None
    for k in range(3):
        grid = solver.solve(pos[k], init=grid, global_step="grid")
        column = solver.solve(pos[k], init=column, global_step="column")
        v, f = gio.read_obj(os.path.join(out, "%05d.obj" % k))
        assert np.array_equal(f, faces) and np.array_equal(v, grid.cpu().numpy().astype(np.float64)), k
        err = float(np.abs(v - column.cpu().numpy().astype(np.float64)).max())
        print("frame %d: max |grid - column| = %.3g" % (k, err))
        assert err <= 1e-6
