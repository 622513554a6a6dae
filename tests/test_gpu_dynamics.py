"""-m gpu: gm_mesh_dynamics (dynamics.MeshDynamics) against the float64 reference of tests/dynamics_ref.py on the cases and materials
of tests/dynamics_cases.py, its batches, repeatability on poisoned memory, its constraints, the properties that tie it to the rest of the
package (rest stays at rest, a free body, the quasi-static limit, the release of a handle), refusals, and the edit surface on top of it
(SingleObjectDeform.simulate, ObjectVisualTool.simulate_one_gaussian, render_sequence over the simulated meshes, edit_sequence
--dynamics)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import arap_cases as ac
import dynamics_cases as dc
from poison import differing, run_under_fills, same_bits
from test_gpu_arap import _drags, _scene64, _tool

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIGHT = dict(cg_iterations=dc.TIGHT[0], cg_tolerance=dc.TIGHT[1])
STIFFEST = dc.MATERIALS.index((50.0, dc.GRAVITY, 0.02))


def _dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


def _dyn(name, material, pinned=None, handles=None, **kw):
    """a fresh MeshDynamics of the case at its starting state, with the reference's own masses"""
    from gaussianmesh_amd.dynamics import MeshDynamics
    c = dc.case(name)
    k, g, d = dc.MATERIALS[material] if isinstance(material, int) else material
    opts = dict(TIGHT, mass=c["mass"], stiffness=k, gravity=g, damping=d, dt=dc.DT, iterations=dc.ITERATIONS)
    opts.update(kw)
    m = MeshDynamics(c["V0"], c["faces"], pinned=c["pinned"] if pinned is None else pinned, handles=c["handles"] if handles is None else handles, **opts)
    m.reset(velocities=_dev(c["v0"]))
    return m


def _targets(name, steps=dc.STEPS):
    """the case's handle targets on the device, held at the last ones beyond its 16 steps; None without handles"""
    t = dc.case(name)["targets"]
    if t is None:
        return None
    if steps > len(t):
        t = np.concatenate([t, np.broadcast_to(t[-1], (steps - len(t),) + t.shape[1:])], 0)
    return _dev(t[:steps])


# ---- 1. against the reference ----
@pytest.mark.parametrize("name, material", dc.ALL, ids=["%s-%d" % c for c in dc.ALL])
def test_against_the_reference(name, material):
    """16 steps at (400, 1e-10): max |X_out - X_ref| <= 1e-6 (coordinates stay below 4: gm_arap_solve's own bound), max |v_out - v_ref|
    <= 1e-6 / dt (one position bound over a step).  On the CPU, PCG against exact solves gave at most 2.4e-7 and 6.5e-6."""
    want_x, want_v = dc.reference_run(name, material)
    m = _dyn(name, material)
    X, stats = m.run(dc.STEPS, _targets(name), want_stats=True)
    X, v, stats = X.cpu().numpy().astype(np.float64), m.velocities.cpu().numpy().astype(np.float64), stats.cpu().numpy()
    assert X.shape == want_x.shape and v.shape == want_v.shape and stats.shape == (dc.STEPS, 6)
    ex, ev = float(np.abs(X - want_x).max()), float(np.abs(v - want_v).max())
    print("%s material %d: max |X_hip - X_ref| %.3g, max |v_hip - v_ref| %.3g, CG steps at most %d, residual at most %.3g"
          % (name, material, ex, ev, int(stats[:, :3].max()), stats[:, 3:].max()))
    assert np.isfinite(X).all() and np.isfinite(v).all()
    assert ex <= 1e-6 and ev <= 1e-6 / dc.DT
    assert (stats[:, 3:] <= 1e-10).all() and (stats[:, :3] <= 400).all() and (stats[:, :3] == np.round(stats[:, :3])).all()
    assert same_bits(m.positions, _dev(X[-1]))


def test_area_masses_are_the_references():
    from gaussianmesh_amd.dynamics import MeshDynamics
    c = dc.case("torus_a")
    m = MeshDynamics(c["V0"], c["faces"], handles=c["handles"], density=1.0)
    assert np.allclose(m.mass, c["mass"], rtol=1e-13, atol=0.0)


# ---- 2. batches ----
@pytest.mark.parametrize("name, material", [("torus_c", STIFFEST), ("pinned", 1), ("free_torus", 6), ("fan", 4)])
def test_a_run_is_its_steps_one_by_one(name, material):
    """run(16) equals sixteen step() calls bit for bit, positions, velocities and stats"""
    t = _targets(name)
    a, b = _dyn(name, material), _dyn(name, material)
    X, stats = a.run(dc.STEPS, t, want_stats=True)
    single = torch.stack([b.step(None if t is None else t[k]) for k in range(dc.STEPS)], 0)
    assert same_bits(X, single) and same_bits(a.velocities, b.velocities) and same_bits(a.positions, b.positions)
    c = _dyn(name, material)
    one = torch.cat([c.run(1, None if t is None else t[k:k + 1], want_stats=True)[1] for k in range(dc.STEPS)], 0)
    assert same_bits(stats, one)
    assert not same_bits(X[7], X[8])


def test_a_run_across_a_chunk_boundary():
    from gaussianmesh_amd import _lib
    n = _lib.GM_MESH_DYNAMICS_STEPS_MAX + 3
    t = _targets("torus_a", n)
    a, b = _dyn("torus_a", STIFFEST), _dyn("torus_a", STIFFEST)
    X = a.run(n, t)
    single = torch.stack([b.step(t[k]) for k in range(n)], 0)
    assert X.shape == (n, 96, 3) and same_bits(X, single) and same_bits(a.velocities, b.velocities)
    c = _dyn("torus_a", STIFFEST)                                     # and in two calls of other lengths
    assert same_bits(torch.cat([c.run(5, t[:5]), c.run(n - 5, t[5:])], 0), X)


# ---- 3. repeatability ----
@pytest.mark.parametrize("name, material", [("torus_c", STIFFEST), ("pinned", 3), ("free_torus", 2), ("flat_patch", 5)])
def test_same_bits_from_call_to_call_and_on_poisoned_memory(name, material):
    """two runs give the same bits; so do runs whose every allocation (X_out, the workspace of a fresh object) was filled with 0x00, 0xFF
    and 0x5A beforehand, and no guard band around any of them is touched"""
    t = _targets(name)

    def route():
        m = _dyn(name, material)
        X, stats = m.run(dc.STEPS, t, want_stats=True)
        return X, stats, m.velocities, m.positions
    first = route()
    assert same_bits(first, route())
    runs = run_under_fills(route)
    assert all(r[0].handed_out >= 2 for r in runs)
    assert differing(runs) == [] and same_bits(runs[0][1], first)


# ---- 4. constraints ----
def test_handle_rows_are_their_targets_and_held_rows_stay():
    """handle rows of X_out[t] equal handle_targets[t] bit for bit; pinned rows and rows whose weights sum to 0 equal x_in bit for bit and
    have zero velocity - from a start that is not the rest pose, with velocity in every row"""
    c = dc.case("pinned")
    pins = np.setdiff1d(np.arange(96), c["handles"])[[2, 30, 31]]
    rng = np.random.default_rng(11)
    x_in = (c["V0"] + rng.uniform(-0.02, 0.02, c["V0"].shape)).astype(np.float32)
    v_in = rng.uniform(-0.5, 0.5, c["V0"].shape).astype(np.float32)
    m = _dyn("pinned", STIFFEST, pinned=pins)
    m.reset(positions=_dev(x_in), velocities=_dev(v_in))
    n = 6                                                              # inside the ramp: the handles are moving
    t = _targets("pinned", n)
    X = m.run(n, t)
    assert same_bits(X[:, _dev(c["handles"], torch.int64)], t)
    held = np.concatenate([pins, [96, 97]])
    assert np.array_equal(X.cpu().numpy()[:, held], np.broadcast_to(x_in[held], (n, len(held), 3)))
    v = m.velocities.cpu().numpy()
    assert (v[held] == 0.0).all()
    h = c["handles"]
    want = (c["targets"][n - 1].astype(np.float64) - c["targets"][n - 2].astype(np.float64)) / dc.DT          # a handle carries its own velocity
    assert np.array_equal(v[h], want.astype(np.float32)) and float(np.abs(want).max()) > 0.1
    free = np.setdiff1d(np.arange(98), np.concatenate([held, h]))
    assert float(np.abs(X.cpu().numpy()[-1, free] - x_in[free]).max()) > 1e-3


# ---- 5. rest stays at rest ----
@pytest.mark.parametrize("name", ["torus_a", "torus_c", "flat_patch", "one_handle", "pinned", "free_torus"])
@pytest.mark.parametrize("tol", [1e-10, 1e-6])
def test_rest_stays_at_rest(name, tol):
    """the rest pose with v = 0 and no gravity, under the case's handles (at their rest positions), a few pins, or nothing: X_out is x_in
    bit for bit and v_out is zero - the residual of the unchanged state is of order 1e-14 |b|, so CG takes no step.  (`fan` is below: its
    free rows lie in the plane z = 0 under a held apex, so the z column's restricted right-hand side is 0 up to rounding and the
    relative rule has nothing to be relative to.)"""
    c = dc.case(name)
    for pinned in ((), (1, 2, 30)):
        m = _dyn(name, (50.0, (0.0, 0.0, 0.0), 0.02), pinned=[p for p in pinned if p not in c["handles"]], cg_tolerance=tol)
        m.reset()
        t = None if c["targets"] is None else _dev(np.broadcast_to(c["V0"][c["handles"]], (4, len(c["handles"]), 3)))
        X, stats = m.run(4, t, want_stats=True)
        assert same_bits(X, _dev(np.broadcast_to(c["V0"], (4,) + c["V0"].shape)))
        print("%s pins %s: |r| / |b| of the unchanged state at most %.3g" % (name, pinned, float(stats[:, 3:].max())))
        assert bool((m.velocities == 0).all()) and bool((stats[:, :3] == 0).all())


def test_rest_stays_at_rest_to_rounding_where_a_column_has_no_right_hand_side():
    """fan: the rim is free, lies in z = 0 and hangs on the held apex, whose share -w z_apex of L x cancels the rotations' term: b of the z
    column is 0 in exact arithmetic and of order 1e-17 as computed, like r, so |r| <= tol |b| does not stop CG and it removes the
    rounding of the local step's rotations (I + O(1e-16)): the state moves by less than 1e-15 and v stays below 1e-13, x and y bit for
    bit in place"""
    c = dc.case("fan")
    m = _dyn("fan", (50.0, (0.0, 0.0, 0.0), 0.02))
    m.reset()
    X = m.run(4, _dev(np.broadcast_to(c["V0"][c["handles"]], (4, len(c["handles"]), 3)))).cpu().numpy()
    assert np.array_equal(X[:, :, :2], np.broadcast_to(c["V0"][:, :2], (4, 41, 2)))
    assert float(np.abs(X.astype(np.float64) - c["V0"]).max()) <= 1e-15 and float(m.velocities.abs().max()) <= 1e-13


# ---- 6. a free body ----
def test_a_free_body_moves_uniformly_and_falls_as_implicit_euler():
    """torus_a, nothing held, damping 0, uniform velocity u: after n = 8 steps every vertex is at x_0 + n h u within 1e-6 n, and with
    gravity on implicit Euler's closed form v_n = u + n h a, x_n = x_{n-1} + h v_n within the same bound: the translated state solves
    every step exactly, so this checks the mass term and the prediction and nothing else"""
    def run(grav, v, n):
        m = _dyn("free_torus", (10.0, grav, 0.0), cg_iterations=64, cg_tolerance=1e-6)
        m.reset(velocities=_dev(v))
        return m.run(n).cpu().numpy()
    errs = dc.free_body_error(run)
    print("free body: error per step %.3g (no gravity), %.3g (gravity)" % tuple(errs))
    assert max(errs) <= 1e-6


# ---- 7. the quasi-static limit ----
@pytest.mark.parametrize("name", ["torus_a", "flat_patch"])
def test_settles_to_the_quasi_static_solution(name):
    """handles at their targets from step 0, stiffness 50, damping 0.1, no gravity, 240 steps: within 1e-5 of
    arap_ref.Reference.solve(start, 400)'s last iterate (the reference dynamics reached 1.6e-7 and 5.4e-8), max |v| below 1e-4 - the
    fixed point of ArapSolver"""
    a = ac.case(name)
    static = ac.reference(name).solve(ac.start(a), 400)[0][-1]
    m = _dyn(name, (50.0, (0.0, 0.0, 0.0), 0.1))
    X = m.run(240, _dev(np.broadcast_to(a["targets"], (240,) + a["targets"].shape)))
    err, vmax = float(np.abs(X[-1].cpu().numpy().astype(np.float64) - static).max()), float(m.velocities.abs().max())
    print("%s: %.3g from the quasi-static solution, max |v| %.3g" % (name, err, vmax))
    assert err <= 1e-5 and vmax < 1e-4


# ---- 8. release ----
@pytest.mark.parametrize("material", [0, STIFFEST])
def test_a_released_handle_keeps_its_momentum(material):
    """one_handle dragged for 8 steps, then set_constraints(pinned=(), handles=()) and 8 more: against the reference driven the same way,
    within the bounds of the first test"""
    c = dc.case("one_handle")
    ref = dc.reference("one_handle", material)
    x1, v1, _ = ref.run(c["V0"], c["v0"], 8, c["targets"][:8])
    ref.set_constraints((), ())
    x2, v2, _ = ref.run(x1[-1], v1, 8)
    m = _dyn("one_handle", material)
    X1 = m.run(8, _targets("one_handle", 8))
    m.set_constraints(pinned=(), handles=())
    X2 = m.run(8)
    X = torch.cat([X1, X2], 0).cpu().numpy().astype(np.float64)
    ex = float(np.abs(X - np.concatenate([x1, x2], 0)).max())
    ev = float(np.abs(m.velocities.cpu().numpy().astype(np.float64) - v2).max())
    print("release, material %d: positions %.3g, velocities %.3g" % (material, ex, ev))
    assert ex <= 1e-6 and ev <= 1e-6 / dc.DT
    h = int(c["handles"][0])
    assert float(np.abs(X[8, h] - X[7, h]).max()) > 1e-3                                 # it flies on


# ---- 9. refusals ----
def test_python_refusals_launch_nothing():
    m = _dyn("torus_a", 0)
    t = _targets("torus_a", 2)
    before = (m.positions, m.velocities)
    out = torch.full((2, 96, 3), 5.0, device="cuda")
    for call in (lambda: m.run(0, t[:0], out=out), lambda: m.run(2, out=out), lambda: m.run(2, t[:, :3], out=out), lambda: m.run(3, t, out=out),
                 lambda: m.run(2, t, out=out[:, :50]), lambda: m.run(2, t, out=out.double()), lambda: m.run(2, t, out=out.cpu()),
                 lambda: m.set_constraints(handles=[3, 3]), lambda: m.reset(positions=out)):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and same_bits(before, (m.positions, m.velocities))


def test_c_refusals_launch_nothing_and_the_workspace_is_kept():
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    m = _dyn("torus_a", 0)
    assert m._ws is None
    t = _targets("torus_a", 4)
    m.run(1, t[:1])
    ws = m._ws
    assert ws.numel() == l.gm_mesh_dynamics_workspace_bytes(96)
    m.run(3, t[1:])
    assert m._ws is ws                                                 # kept: its size does not depend on the number of steps
    # straight through ctypes, on real device memory: every refusal leaves poisoned outputs untouched
    T, H = 2, len(m.handles)
    x, v = m.positions, m.velocities
    out = torch.full((T, 96, 3), 5.0, device="cuda")
    vout = torch.full((96, 3), 6.0, device="cuda")
    stats = torch.full((T, 6), -3.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(T=T, Vm=96, H=H, dt=dc.DT, k=10.0, damp=0.0, its=3, cg=16, tol=1e-6, nbytes=None, **kw):
        a = dict(off=m._off, cols=m._cols, w=m._w, V0=m.rest, mass=m._mass, held=m._held, ids=m._handle_ids, targets=t, x=x, v=v, out=out, vout=vout,
                 stats=stats, ws=ws)
        a.update(kw)
        q = {n: (p.data_ptr() if torch.is_tensor(p) else p) for n, p in a.items()}
        return l.gm_mesh_dynamics(T, Vm, q["off"], q["cols"], q["w"], q["V0"], q["mass"], q["held"], H, q["ids"], q["targets"], q["x"], q["v"], dt, k, damp,
                                  0.0, 0.0, 0.0, its, cg, tol, q["out"], q["vout"], q["stats"], q["ws"], ws.numel() if nbytes is None else nbytes,
                                  ctypes.c_void_p(stream))
    for kw, rc in ((dict(T=0), 1), (dict(T=65), 1), (dict(Vm=0), 1), (dict(H=-1), 1), (dict(H=97), 1), (dict(dt=0.0), 1), (dict(k=0.0), 1),
                   (dict(damp=1.0), 1), (dict(its=0), 1), (dict(cg=0), 1), (dict(tol=-1.0), 1), (dict(x=None), 1), (dict(mass=None), 1),
                   (dict(ids=None), 1), (dict(out=None), 1), (dict(vout=None), 1), (dict(ws=None), 1), (dict(out=x), 1), (dict(out=m.rest), 1),
                   (dict(vout=x), 1), (dict(stats=out), 1), (dict(ws=out), 1), (dict(out=t), 1),
                   (dict(nbytes=l.gm_mesh_dynamics_workspace_bytes(96) - 1), 3), (dict(nbytes=0), 3)):
        assert call(**kw) == rc and b"gm_mesh_dynamics" in l.gm_last_error(), (kw, l.gm_last_error())
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((vout == 6.0).all()) and bool((stats == -3.0).all())
    assert call() == 0                                                 # and the same call, unrefused, writes all three
    torch.cuda.synchronize()
    n = _dyn("torus_a", (10.0, (0.0, 0.0, 0.0), 0.0), cg_iterations=16, cg_tolerance=1e-6)
    n.reset(positions=x, velocities=v)
    want, want_stats = n.run(2, t[:2], want_stats=True)
    assert same_bits(out, want) and same_bits(stats, want_stats) and same_bits(vout, n.velocities)


# ---- 10. the edit surface ----
def test_simulate_is_run_and_leaves_the_object_at_the_last_frame(tmp_path):
    from gaussianmesh_amd.dynamics import MeshDynamics
    d = str(tmp_path)
    _scene64(d)
    tool, other = _tool(d), _tool(d)
    o, q = tool.gaussians_list[0], other.gaussians_list[0]
    ids, pos = _drags(o.vertex.cpu().numpy(), T=5)
    pos = _dev(pos)
    o.set_handles(ids)
    m = MeshDynamics(o.vertex, o.faces, handles=ids, stiffness=20.0)
    got = o.simulate(3, pos[:3], stiffness=20.0)
    want = m.run(3, pos[:3])
    assert got.shape == (3, o.vertex.shape[0], 3) and same_bits(got, want)
    assert torch.equal(o.mesh_vertex_current, want[-1])
    exp = q.deform_vertices(want[-1])
    assert all(torch.equal(g, e) for g, e in zip(o.deform_vertices(o.mesh_vertex_current), exp))
    kept = o._operators["dynamics"]
    again = o.simulate(2, pos[3:], stiffness=20.0)                     # from the current mesh with the velocity the first call left
    assert o._operators["dynamics"] is kept and same_bits(again, m.run(2, pos[3:]))
    m.reset(positions=again[-1])
    cold = o.simulate(2, pos[3:], keep_velocity=False, stiffness=20.0)
    assert same_bits(cold, m.run(2, pos[3:])) and not same_bits(cold, again)
    pins = np.setdiff1d(np.arange(o.vertex.shape[0]), ids)[:2]
    pinned = o.simulate(1, pos[4:], pinned=pins, stiffness=20.0)
    assert o._operators["dynamics"] is not kept and bool((pinned[0, _dev(pins, torch.int64)] == cold[-1, _dev(pins, torch.int64)]).all())
    # the tool's wrapper, and a free body: no handles chosen, gravity on
    third = _tool(d)
    fall = third.simulate_one_gaussian("Object", 4, gravity=dc.GRAVITY)
    assert third.simulate_one_gaussian("Nobody", 4) is None
    assert same_bits(fall, MeshDynamics(o.vertex, o.faces, gravity=dc.GRAVITY).run(4))
    assert torch.equal(third.gaussians_list[0].mesh_vertex_current, fall[-1])
    assert float((fall[-1] - o.vertex)[:, 1].max()) < -1e-2                              # it fell
    with pytest.raises(ValueError, match="handle_targets"):
        o.simulate(2)


def test_render_sequence_over_the_simulated_meshes(tmp_path):
    d = str(tmp_path)
    _scene64(d)
    tool = _tool(d)
    o = tool.gaussians_list[0]
    ids, pos = _drags(o.vertex.cpu().numpy(), T=5)
    o.set_handles(ids)
    meshes = o.simulate(5, _dev(pos))
    cams = tool.get_camera(d)
    got = list(tool.render_sequence([(cams[k % 3], {"Object": meshes[k]}) for k in range(5)], frames_per_launch=4))
    assert len(got) == 5
    for k in range(5):
        assert got[k].shape == (3, 64, 64) and bool(torch.isfinite(got[k]).all())
        assert float((got[k] - 1.0).abs().max()) > 0.1                                   # the object is in the picture


def _cli(d, out, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "gaussianmesh_amd.edit_sequence", "--object_gaussian", os.path.join(d, "object.ply"),
                        "--object_origin_mesh", os.path.join(d, "rest.obj"), "--camera_path", d, "--render_path", out,
                        "--handle_sequence", os.path.join(d, "handles.npz"), "--save_meshes"] + list(extra), cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]


def test_cli_dynamics_writes_the_frames_and_the_default_is_unchanged(tmp_path):
    """--dynamics --settle 4 writes T + 4 frames, the meshes MeshDynamics gives; without the new flags the files are byte for byte what
    the routes the CLI has always taken give (ArapSolver.solve_sequence one frame at a time, render_sequence, save_image, write_obj)"""
    from gaussianmesh_amd import io as gio
    from gaussianmesh_amd.arap import ArapSolver
    from gaussianmesh_amd.dynamics import MeshDynamics
    d = str(tmp_path)
    _scene64(d)
    verts, faces = gio.read_obj(os.path.join(d, "rest.obj"))
    ids, pos = _drags(verts)
    np.savez(os.path.join(d, "handles.npz"), handles=ids, positions=pos)
    sim, plain, byhand = os.path.join(d, "sim"), os.path.join(d, "plain"), os.path.join(d, "byhand")
    _cli(d, sim, "--dynamics", "--settle", "4", "--stiffness", "20", "--gravity", "0", "-9.8", "0")
    T = len(pos)
    assert sorted(os.listdir(sim)) == ["%05d.%s" % (k, e) for k in range(T + 4) for e in ("obj", "png")]
    targets = np.concatenate([pos, np.broadcast_to(pos[-1], (4,) + pos.shape[1:])], 0)
    want = MeshDynamics(verts.astype(np.float32), faces, handles=ids, stiffness=20.0, gravity=dc.GRAVITY).run(T + 4, _dev(targets)).cpu().numpy()
    for k in range(T + 4):
        v, f = gio.read_obj(os.path.join(sim, "%05d.obj" % k))
        assert np.array_equal(f, faces) and np.array_equal(v, want[k].astype(np.float64)), k
    _cli(d, plain)
    tool = _tool(d)
    cams = tool.get_camera(d)
    meshes = list(ArapSolver(verts.astype(np.float32), faces, ids).solve_sequence(pos, batch=1))
    os.makedirs(byhand)
    with torch.no_grad():
        for k, img in enumerate(tool.render_sequence([(cams[k % len(cams)], {"Object": m}) for k, m in enumerate(meshes)], frames_per_launch=4)):
            gio.save_image(img, os.path.join(byhand, "%05d.png" % k))
            gio.write_obj(os.path.join(byhand, "%05d.obj" % k), meshes[k].cpu().numpy(), tool.gaussians_list[-1].faces.cpu().numpy())
    names = sorted(os.listdir(plain))
    assert names == sorted(os.listdir(byhand)) == ["%05d.%s" % (k, e) for k in range(T) for e in ("obj", "png")]
    for n in names:
        assert open(os.path.join(plain, n), "rb").read() == open(os.path.join(byhand, n), "rb").read(), n
