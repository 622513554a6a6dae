"""-m gpu: gm_mesh_dynamics_fields (dynamics.MeshDynamics(fields=[SdfGrid, ...]), run(field_poses=)) against the float64 reference of
tests/dynamics_moving_field_ref.py on the cases and materials of tests/dynamics_moving_field_cases.py: positions, velocities and the
active set; identity poses against gm_mesh_dynamics_field, bit for bit; fields nothing reaches against the fieldless entries, bit for
bit; a plane grid under a constant pose against the equal half-space; run(66) against 66 steps; poisoned memory; refusals; and the edit
surface on top of it (SceneVisualTool.object_fields with dynamics.rigid_poses, edit_sequence --obstacle_motion)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dynamics_cases as dc
import dynamics_contact_cases as cc
import dynamics_contact_ref as cr
import dynamics_field_cases as fc
import dynamics_moving_field_cases as mc
import dynamics_moving_field_ref as mr
import mesh_sdf_ref
from poison import differing, run_under_fills, same_bits
from test_dynamics_field_ref_host import DYADIC, FLOOR
from test_gpu_arap import _drags, _scene64
from test_gpu_dynamics import ROOT, _cli
from test_gpu_edittool import _write_scene

pytestmark = pytest.mark.gpu
TIGHT = dict(cg_iterations=mc.TIGHT[0], cg_tolerance=mc.TIGHT[1])
SOFT, STIFF = mc.MATERIALS


def _dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


def _colliders(ref_colliders):
    return [("sphere" if k == cr.SPHERE else "half_space", tuple(float(x) for x in row), mu) for k, row, mu in ref_colliders]


def _grid_of(f):
    from gaussianmesh_amd.dynamics import SdfGrid
    return SdfGrid(f["values"], f["origin"], f["voxel"])


@pytest.fixture(scope="module")
def grids():
    """the SdfGrids of a case (of dynamics_moving_field_cases: a list; of dynamics_field_cases: one), prepared once and shared"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = [_grid_of(f) for f in mc.case(name)["fields"]] if name in mc.NAMES else _grid_of(fc.case(name)["field"])
        return made[name]
    return get


def _material(material):
    k, g, d = dc.MATERIALS[material] if isinstance(material, int) else material
    return dict(TIGHT, stiffness=k, gravity=g, damping=d, dt=mc.DT, iterations=mc.ITERATIONS, contact_stiffness=mc.KC)


def _dyn(name, material, fields, **kw):
    """a fresh MeshDynamics of a moving-field case at its starting state, with the reference's own masses, the case's colliders, `fields`
    at the case's pose0"""
    from gaussianmesh_amd.dynamics import MeshDynamics
    c = mc.case(name)
    opts = dict(_material(material), mass=c["mass"], colliders=_colliders(c["colliders"]), fields=fields, field_frictions=[f["friction"] for f in c["fields"]])
    opts.update(kw)
    m = MeshDynamics(c["V0"], c["faces"], pinned=c["pinned"], handles=c["handles"], **opts)
    m.reset(velocities=_dev(c["v0"]), field_poses=c["pose0"] if m.NF else None)
    return m


def _static(name, material, **kw):
    """a fresh MeshDynamics of a dynamics_field_cases case without its field: kw says what stands in its place"""
    from gaussianmesh_amd.dynamics import MeshDynamics
    c = fc.case(name)
    opts = dict(_material(material), mass=c["mass"], colliders=_colliders(c["colliders"]))
    opts.update(kw)
    m = MeshDynamics(c["V0"], c["faces"], pinned=c["pinned"], handles=c["handles"], **opts)
    m.reset(velocities=_dev(c["v0"]))
    return m


def _rows(c, steps=mc.STEPS):
    return None if c["collider_rows"] is None else _dev(c["collider_rows"][:steps])


# ---- 1. against the reference ----
@pytest.mark.parametrize("name, material", mc.ALL, ids=["%s-%d" % c for c in mc.ALL])
def test_against_the_reference(name, material, grids):
    """16 steps at (400, 1e-10): max |X_out - X_ref| <= 1e-6 and max |v_out - v_ref| <= 1e-6 / dt, section AA's bounds: on the CPU the
    reference's PCG against its exact solves gave E_x <= 2.4e-7 and E_v <= 4.7e-6 on these cases, at or below a quarter of them
    (test_dynamics_moving_field_ref_host.py asserts it).  contact_out equals the reference's active set on every row but those within
    1e-5 of a surface, of a second candidate or of where a field stops being known, with values up to 1 + K + F - 1.  The poses go in as
    a host array (checked) for the soft material and as a device tensor (taken as it is) for the stiff one."""
    want_x, want_v, want_c, compare = mc.reference_run(name, material)
    c = mc.case(name)
    m = _dyn(name, material, grids(name))
    poses = c["field_poses"] if material == SOFT else _dev(c["field_poses"], torch.float64)
    X, contact, stats = m.run(mc.STEPS, collider_rows=_rows(c), field_poses=poses, want_contacts=True, want_stats=True)
    X, v, stats = X.cpu().numpy().astype(np.float64), m.velocities.cpu().numpy().astype(np.float64), stats.cpu().numpy()
    contact = contact.cpu().numpy()
    assert X.shape == want_x.shape and v.shape == want_v.shape and stats.shape == (mc.STEPS, 6) and contact.shape == want_c.shape
    ex, ev = float(np.abs(X - want_x).max()), float(np.abs(v - want_v).max())
    wrong = int((contact != want_c)[compare].sum())
    print("%s material %d: max |X_hip - X_ref| %.3g, max |v_hip - v_ref| %.3g, CG steps at most %d, residual at most %.3g, %d rows x steps in "
          "contact, %d compared rows differ, %d of the rows left out differ"
          % (name, material, ex, ev, int(stats[:, :3].max()), stats[:, 3:].max(), int((contact > 0).sum()), wrong, int((contact != want_c)[~compare].sum())))
    assert np.isfinite(X).all() and np.isfinite(v).all()
    assert ex <= 1e-6 and ev <= 1e-6 / mc.DT
    assert wrong == 0 and contact.dtype == np.int32 and int(contact.max()) == int(want_c.max()) <= m.K + m.NF
    assert (stats[:, 3:] <= 1e-10).all() and (stats[:, :3] <= 400).all()
    assert same_bits(m.positions, _dev(X[-1])) and same_bits(m.field_poses, _dev(c["field_poses"][-1], torch.float64))


# ---- 2. identity poses against the static entry ----
@pytest.mark.parametrize("name, material", [("tilt_rough", SOFT), ("bump", STIFF), ("field_pusher", STIFF), ("field_sixteen", SOFT), ("sheet1056", STIFF),
                                            ("unknown_block", SOFT)])
def test_identity_poses_give_the_bits_of_the_static_entry(name, material, grids):
    """fields=[g] at the identity - poses not given, and given as identities - is field=g through gm_mesh_dynamics_field: positions,
    velocities, contacts and stats bit for bit, without analytic colliders and with one (moving) and sixteen"""
    c = fc.case(name)
    g, mu = grids(name), c["field"]["friction"]
    rows = _rows(c)
    want = _static(name, material, field=g, field_friction=mu)
    W = want.run(fc.STEPS, collider_rows=rows, want_contacts=True, want_stats=True)
    for poses in (None, np.tile(mr.IDENTITY, (fc.STEPS, 1, 1, 1)), _dev(np.tile(mr.IDENTITY, (fc.STEPS, 1, 1, 1)), torch.float64)):
        m = _static(name, material, fields=[g], field_frictions=[mu])
        got = m.run(fc.STEPS, collider_rows=rows, field_poses=poses, want_contacts=True, want_stats=True)
        assert same_bits(got, W) and same_bits(m.velocities, want.velocities) and same_bits(m.positions, want.positions)
    assert bool((W[1] == 1 + want.K).any())


# ---- 3. fields nothing reaches ----
@pytest.mark.parametrize("material", mc.MATERIALS)
def test_fields_nothing_reaches_give_the_bits_of_the_fieldless_run(material):
    """a floor grid far below, a grid of NaNs, and the floor grid itself posed 100 away (and moving there): kappa = 0 in every row, and the
    result is bit for bit that of the object without fields - through gm_mesh_dynamics with no colliders, through
    gm_mesh_dynamics_contact with the corner's two; all three at once too"""
    from gaussianmesh_amd.dynamics import SdfGrid
    dims, origin, voxel = fc.TORUS_GRID
    far = SdfGrid(fc.plane_values(dims, origin, voxel, (0.0, 1.0, 0.0), -2.3), origin, voxel)
    unknown = SdfGrid(np.full((dims[2], dims[1], dims[0]), np.nan, np.float32), origin, voxel)
    floor = SdfGrid(fc.plane_values(dims, origin, voxel, (0.0, 1.0, 0.0), fc.GROUND), origin, voxel)
    away = mc.translations((0.5, 0.0, 0.0))[:, None] + np.concatenate([np.zeros((3, 3)), [[100.0], [0.0], [0.0]]], axis=1)
    still = np.tile(mr.IDENTITY, (mc.STEPS, 1, 1, 1))
    spin = np.array([mc.pose(mc.rotation((0.0, 1.0, 0.0), 0.02 * (k + 1))) for k in range(mc.STEPS)])[:, None]
    corner = cc.case("corner")["colliders"]
    for colliders in ((), corner):
        plain = _static("field_sixteen", material, colliders=_colliders(colliders))
        P, pc, ps = plain.run(mc.STEPS, want_contacts=True, want_stats=True)
        for fields, poses in (([far], spin), ([unknown], still), ([floor], away), ([far, unknown, floor], np.concatenate([spin, still, away], axis=1))):
            m = _static("field_sixteen", material, colliders=_colliders(colliders), fields=fields, field_frictions=[0.3] * len(fields))
            X, contact, stats = m.run(mc.STEPS, field_poses=poses, want_contacts=True, want_stats=True)
            assert same_bits(X, P) and same_bits(m.velocities, plain.velocities) and same_bits(contact, pc) and same_bits(stats, ps)
        assert bool((pc > 0).any()) == bool(colliders) and int(pc.max()) <= len(colliders)
    reached = _static("field_sixteen", material, colliders=(), fields=[floor], field_frictions=[0.3])
    assert bool((reached.run(mc.STEPS, want_contacts=True)[1] == 1).any())         # (the floor grid, where it was sampled, is reached)


# ---- 4. a constant pose that is not the identity ----
@pytest.mark.parametrize("material", mc.MATERIALS)
def test_a_posed_plane_grid_against_the_equal_half_space(material):
    """the dyadic floor grid (every sample exact in float32: the grid IS the plane y = -0.875) turned by 0.3 about the y axis and moved by
    (0.3, 0.125, -0.2), in every step: the half-space y < -0.75 with the same friction.  The pose keeps the normal (0, 1, 0) and the
    offset exact, so the two differ by roundings of 1e-16 and by nothing else: positions within 1e-6, velocities within 1e-6 / dt, the
    contacts equal wherever the analytic phi is not within 1e-5 of 0.  The pose is constant, so the anchor is xs itself, as for the
    half-space; x and z do go through R^T (X - t) into the grid's cells."""
    from gaussianmesh_amd.dynamics import MeshDynamics, SdfGrid, floor
    dims, origin, voxel = DYADIC
    grid = SdfGrid(fc.plane_values(dims, origin, voxel, (0.0, 1.0, 0.0), FLOOR), origin, voxel)
    P = mc.pose(mc.rotation((0.0, 1.0, 0.0), 0.3), t=(0.3, 0.125, -0.2))
    assert P[0, 1] == 0.0 and P[2, 1] == 0.0 and P[1, 1] == 1.0
    c = fc.case("tilt_rough")
    a = _static("tilt_rough", material, fields=[grid], field_frictions=[0.5])
    a.reset(velocities=_dev(c["v0"]), field_poses=P[None])
    b = _static("tilt_rough", material, colliders=[floor(FLOOR + 0.125, friction=0.5)])
    Xa, ca = a.run(fc.STEPS, want_contacts=True)                       # None: every field stays where it is
    Xb, cb = b.run(fc.STEPS, want_contacts=True)
    ex, ev = float((Xa.double() - Xb.double()).abs().max()), float((a.velocities.double() - b.velocities.double()).abs().max())
    near = (Xb[:, :, 1].double() - (FLOOR + 0.125)).abs() < fc.NEAR
    print("posed plane grid against the half-space, material %d: positions %.3g, velocities %.3g, %d contacts" % (material, ex, ev, int((cb > 0).sum())))
    assert ex <= 1e-6 and ev <= 1e-6 / fc.DT and bool((ca[~near] == cb[~near]).all()) and int((cb > 0).sum()) > 100 and int(ca.max()) == 1
    again = _static("tilt_rough", material, fields=[grid], field_frictions=[0.5])
    again.reset(velocities=_dev(c["v0"]), field_poses=_dev(P[None], torch.float64))
    assert same_bits(again.run(fc.STEPS, field_poses=np.tile(P, (fc.STEPS, 1, 1, 1))), Xa) and same_bits(again.field_poses, a.field_poses)


# ---- 5. step by step ----
def test_a_run_of_66_is_66_steps(grids):
    """the 25-vertex sheet, damped, on the rough plate that translates AND turns in every step: run(66), 66 calls of step() and two runs
    of other lengths give the same bits, contacts and stats included, on both sides of the 64-step chain boundary, and leave the same
    poses behind"""
    from gaussianmesh_amd import _lib
    n = _lib.GM_MESH_DYNAMICS_STEPS_MAX + 2
    poses = np.array([mc.pose(mc.rotation((0.0, 1.0, 0.0), 0.004 * (k + 1)), t=(0.005 * (k + 1), 0.0005 * (k + 1), -0.002 * (k + 1))) for k in range(n)])[:, None]
    damped = (10.0, dc.GRAVITY, 0.2)
    a, b, c = (_dyn("pause", damped, grids("pause")) for _ in range(3))
    X, contact, stats = a.run(n, field_poses=poses, want_contacts=True, want_stats=True)
    single = torch.stack([b.step(field_poses=poses[k]) for k in range(n)], 0)
    assert X.shape == (n, 25, 3) and same_bits(X, single) and same_bits(a.velocities, b.velocities) and same_bits(a.field_poses, b.field_poses)
    first = c.run(7, field_poses=_dev(poses[:7], torch.float64), want_contacts=True, want_stats=True)
    second = c.run(n - 7, field_poses=poses[7:], want_contacts=True, want_stats=True)
    for k in range(3):
        assert same_bits(torch.cat([first[k], second[k]], 0), (X, contact, stats)[k])
    assert bool((contact[60:64] == 1).any()) and bool((contact[64:] == 1).any()) and not same_bits(X[64], X[65])
    moved = _dyn("pause", damped, grids("pause"))                        # and the poses matter: the plate standing still gives other bits
    assert not same_bits(moved.run(n), X)


# ---- 6. poisoned memory ----
@pytest.mark.parametrize("name, material", [("four_sixteen", STIFF), ("tilt_spin", SOFT), ("slide_rough", STIFF), ("half_leaves", SOFT)])
def test_same_bits_from_call_to_call_and_on_poisoned_memory(name, material):
    """two runs give the same bits; so do runs whose every allocation (X_out, contact_out, stats, the pose table, the workspace of a fresh
    object, and the grids themselves, prepared anew) was filled with 0x00, 0xFF and 0x5A beforehand, and no guard band is touched"""
    c = mc.case(name)
    rows = _rows(c)

    def route():
        m = _dyn(name, material, [_grid_of(f) for f in c["fields"]])
        X, contact, stats = m.run(mc.STEPS, collider_rows=rows, field_poses=c["field_poses"], want_contacts=True, want_stats=True)
        return X, contact, stats, m.velocities, m.positions, m.field_poses
    first = route()
    assert same_bits(first, route())
    runs = run_under_fills(route)
    assert all(p.handed_out >= 4 for p, _ in runs)
    assert differing(runs) == [] and same_bits(runs[0][1], first)


# ---- 7. refusals ----
def test_python_refusals_launch_nothing(grids):
    from gaussianmesh_amd.dynamics import MeshDynamics
    c = mc.case("pause")
    g = grids("pause")[0]
    for kw in (dict(fields=g), dict(fields=[g.grid]), dict(fields=[g] * 5), dict(fields=[g], field=g), dict(fields=[g], field_frictions=[-1.0]),
               dict(fields=[g], field_frictions=[float("nan")]), dict(fields=[g], field_frictions=[0.1, 0.2]), dict(fields=[g], field_frictions=0.1),
               dict(fields=[g], device="cpu")):
        with pytest.raises(ValueError):
            MeshDynamics(c["V0"], c["faces"], **kw)
    m = _dyn("pause", SOFT, [g])
    before = (m.positions, m.velocities, m.field_poses)
    out = torch.full((2, 25, 3), 5.0, device="cuda")
    eye = np.tile(mr.IDENTITY, (2, 1, 1, 1))
    sheared, mirrored, big, nan = eye.copy(), eye.copy(), eye.copy(), eye.copy()
    sheared[1, 0, 0, 1] = 1e-3
    mirrored[0, 0, 2, 2] = -1.0
    big[1, 0, :, :3] *= 1.0 + 1e-5
    nan[0, 0, 1, 3] = np.nan
    for poses in (eye[:1], eye[:, 0], np.tile(mr.IDENTITY, (2, 2, 1, 1)), eye[..., :3], sheared, mirrored, big, nan, torch.as_tensor(sheared)):
        with pytest.raises(ValueError):
            m.run(2, field_poses=poses, out=out)
    for call in (lambda: m.step(field_poses=eye[0, 0]), lambda: m.step(field_poses=sheared[1]), lambda: m.reset(field_poses=sheared[1]),
                 lambda: m.reset(field_poses=eye)):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and same_bits(before, (m.positions, m.velocities, m.field_poses))
    m.run(2, field_poses=_dev(sheared, torch.float64), out=out)          # a device tensor is taken as it is
    assert bool(torch.isfinite(out).all()) and not bool((out == 5.0).all())


def test_c_refusals_launch_nothing(grids):
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    gs = grids("two")
    m = _dyn("two", SOFT, gs, cg_iterations=16, cg_tolerance=1e-6)
    T, Vm = 2, 96
    x, v = m.positions, m.velocities
    poses = _dev(np.concatenate([mc.case("two")["pose0"][None], mc.case("two")["field_poses"][:T]], 0), torch.float64)
    out = torch.full((T, Vm, 3), 5.0, device="cuda")
    vout = torch.full((Vm, 3), 6.0, device="cuda")
    stats = torch.full((T, 6), -3.0, dtype=torch.float64, device="cuda")
    con = torch.full((T, Vm), 9, dtype=torch.int32, device="cuda")
    ws = torch.empty((l.gm_mesh_dynamics_contact_workspace_bytes(Vm),), dtype=torch.uint8, device="cuda")
    q = lambda p: p.data_ptr() if torch.is_tensor(p) else p

    def call(F=2, nbytes=None, change=None, **kw):
        a = dict(poses=poses, contact=con, out=out, vout=vout, stats=stats, ws=ws)
        a.update(kw)
        table = (_lib.DynamicsField * 4)(*[_lib.DynamicsField(g.nx, g.ny, g.nz, (ctypes.c_float * 3)(*g.origin.tolist()), g.voxel, g.grid.data_ptr(), mu)
                                            for g, mu in zip(gs, m.field_frictions)])
        if change:
            change(table)
        gr = m.gravity
        return l.gm_mesh_dynamics_fields(T, Vm, q(m._off), q(m._cols), q(m._w), q(m.rest), q(m._mass), q(m._held), 0, None, None, q(x), q(v), m.dt, m.stiffness,
                                         m.damping, gr[0], gr[1], gr[2], m.iterations, 16, 1e-6, 0, None, None, None, mc.KC, F, table, q(a["poses"]), q(a["out"]),
                                         q(a["vout"]), q(a["contact"]), q(a["stats"]), q(a["ws"]), a["ws"].numel() if nbytes is None else nbytes,
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def setter(f, field, value):
        def change(table):
            setattr(table[f], field, value)
        return change
    nan = float("nan")
    for kw, rc in ((dict(F=5), 1), (dict(F=-1), 1), (dict(poses=None), 1), (dict(change=setter(1, "nx", 1)), 1), (dict(change=setter(0, "voxel", 0.0)), 1),
                   (dict(change=setter(1, "voxel", nan)), 1), (dict(change=setter(1, "grid", None)), 1), (dict(change=setter(1, "grid", gs[1].grid.data_ptr() + 4)), 1),
                   (dict(change=setter(0, "friction", -0.5)), 1), (dict(change=setter(1, "friction", nan)), 1), (dict(out=gs[1].grid), 1), (dict(contact=gs[0].grid), 1),
                   (dict(ws=gs[1].grid), 1), (dict(stats=poses), 1), (dict(vout=poses), 1), (dict(change=setter(1, "grid", out.data_ptr())), 1),
                   (dict(nbytes=l.gm_mesh_dynamics_contact_workspace_bytes(Vm) - 1), 3), (dict(nbytes=l.gm_mesh_dynamics_workspace_bytes(Vm)), 3)):
        assert call(**kw) == rc and b"gm_mesh_dynamics_fields" in l.gm_last_error(), (kw, l.gm_last_error())
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((vout == 6.0).all()) and bool((stats == -3.0).all()) and bool((con == 9).all())
    assert call() == 0                                                 # and the same call, unrefused, writes all four
    torch.cuda.synchronize()
    want = m.run(T, field_poses=poses[1:], want_contacts=True, want_stats=True)
    assert same_bits((out, con, stats), want) and same_bits(vout, m.velocities)
    assert call(contact=None, stats=None) == 0                         # both optional
    assert call(F=0, poses=None) == 0                                  # F == 0: gm_mesh_dynamics_contact's launches, here gm_mesh_dynamics' own
    torch.cuda.synchronize()
    k0 = _dyn("two", SOFT, [], field_frictions=[], cg_iterations=16, cg_tolerance=1e-6)
    assert same_bits((out, con), k0.run(T, want_contacts=True)) and int(con.max()) == 0


# ---- 8. the edit surface ----
def test_object_fields_and_rigid_poses_let_one_object_push_another(tmp_path):
    """two copies of test_gpu_edittool's object: A is moved rigidly - from 2.0 below, up by 1.4 and turning about y, so that its top ends 0.8 above where B's underside rests - while B is simulated
    against object_fields(["A"]) posed by rigid_poses of A's frames.  simulate(fields=, field_poses=) is MeshDynamics.run bit for bit and
    reuses its operator; B's contact rows are not empty, no vertex of B ends deeper inside A than a voxel, and so B's lowest vertex has
    risen by more than 0.8 less a voxel"""
    from gaussianmesh_amd import mesh_sdf
    from gaussianmesh_amd.dynamics import MeshDynamics, SdfGrid, rigid_poses
    from gaussianmesh_amd.edittool import SceneVisualTool
    d = str(tmp_path)
    _write_scene(d)
    tool = SceneVisualTool(os.path.join(d, "background.ply"))
    for name in ("A", "B"):
        tool.add_gaussian(os.path.join(d, "object.ply"), os.path.join(d, "rest.obj"), name)
    A, B = tool.gaussians_list
    T = 12
    rest = A.vertex.cpu().numpy().astype(np.float64)
    want = np.array([mc.pose(mc.rotation((0.0, 1.0, 0.0), 0.03 * (k + 1)), t=(0.0, -2.0 + 1.4 * (k + 1) / T, 0.0)) for k in range(T)])
    frames = np.array([rest @ P[:, :3].T + P[:, 3] for P in want]).astype(np.float32)
    poses = rigid_poses(A.vertex, frames)
    assert float(np.abs(poses - want).max()) <= 1e-5                   # (the frames are float32)
    fields = tool.object_fields(["A"], resolution=32)
    assert len(fields) == 1 and isinstance(fields[0], SdfGrid) and max(fields[0].nx, fields[0].ny, fields[0].nz) == 32
    assert same_bits(fields[0].grid, SdfGrid.from_mesh(A.vertex, A.faces, resolution=32).grid)       # sampled at the REST mesh
    got = B.simulate(T, stiffness=50.0, damping=0.2, fields=fields, field_frictions=[0.3], field_poses=poses[:, None])
    m = MeshDynamics(B.vertex, B.faces, stiffness=50.0, damping=0.2, fields=fields, field_frictions=[0.3])
    X, contact = m.run(T, field_poses=poses[:, None], want_contacts=True)
    assert same_bits(got, X) and torch.equal(B.mesh_vertex_current, X[-1])
    assert int((contact == 1).sum()) > 10 and not bool(contact[0].any())
    lift = float(X[-1][:, 1].min() - B.vertex[:, 1].min())
    deepest = float(mesh_sdf.signed_distances(X[-1].contiguous(), frames[-1], A.faces.cpu().numpy()).min())
    print("A pushes B: B's lowest vertex rose by %.3f, deepest vertex %.4f inside A, voxel %.4f, %d contact rows" % (lift, -deepest, fields[0].voxel, int((contact > 0).sum())))
    assert lift > 0.8 - fields[0].voxel and deepest >= -fields[0].voxel and float((X[-1][:, 1] - B.vertex[:, 1]).mean()) > 0.0
    kept = B._operators["dynamics"]
    again = tool.simulate_one_gaussian("B", 2, stiffness=50.0, damping=0.2, fields=fields, field_frictions=[0.3], field_poses=poses[-2:, None])
    assert B._operators["dynamics"] is kept and again.shape == (2, B.vertex.shape[0], 3)
    A.deform_vertices(_dev(frames[-1]))                                 # A itself is shown where its last frame puts it, as any mesh sequence is
    for bad in ([], ["Nobody"], ["A"] * 5):
        with pytest.raises(ValueError):
            tool.object_fields(bad)


def _cli_raw(d, out, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "gaussianmesh_amd.edit_sequence", "--object_gaussian", os.path.join(d, "object.ply"),
                           "--object_origin_mesh", os.path.join(d, "rest.obj"), "--camera_path", d, "--render_path", out,
                           "--handle_sequence", os.path.join(d, "handles.npz"), "--save_meshes"] + list(extra), cwd=ROOT, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)


def test_cli_obstacle_motion_moves_the_obstacle(tmp_path):
    """--dynamics --obstacle_mesh BOX.obj --obstacle_motion M.json over four frames of the 64-pixel scene, the box rising by 0.1 per frame:
    the frames are written, differ from those over the box standing still, and the free vertices end higher; a file with another number
    of frames is refused"""
    from gaussianmesh_amd import io as gio
    d = str(tmp_path)
    _scene64(d)
    verts, faces = gio.read_obj(os.path.join(d, "rest.obj"))
    ids, pos = _drags(verts, T=4)
    np.savez(os.path.join(d, "handles.npz"), handles=ids, positions=pos)
    low = float(verts[:, 1].min())
    bv, bf = mesh_sdf_ref.cube((-3.5, low - 1.0, -3.5), (3.5, low + 0.1, 3.5))
    gio.write_obj(os.path.join(d, "box.obj"), bv, bf)
    rising = [mc.pose(t=(0.0, 0.1 * (k + 1), 0.0)).tolist() for k in range(4)]
    with open(os.path.join(d, "motion.json"), "w") as fh:
        json.dump(rising, fh)
    with open(os.path.join(d, "short.json"), "w") as fh:
        json.dump(rising[:3], fh)
    still, moving = os.path.join(d, "still"), os.path.join(d, "moving")
    common = ("--dynamics", "--gravity", "0", "-9.8", "0", "--obstacle_mesh", os.path.join(d, "box.obj"), "--obstacle_resolution", "32", "--obstacle_margin",
              "0.25", "--friction", "0.3")
    _cli(d, still, *common)
    _cli(d, moving, *common, "--obstacle_motion", os.path.join(d, "motion.json"))
    names = ["%05d.%s" % (k, e) for k in range(4) for e in ("obj", "png")]
    assert sorted(os.listdir(still)) == names and sorted(os.listdir(moving)) == names
    last_still, last_moving = (np.asarray(gio.read_obj(os.path.join(f, "00003.obj"))[0]) for f in (still, moving))
    free = np.setdiff1d(np.arange(len(verts)), ids)
    voxel = 7.0 * 1.5 / 32
    assert np.isfinite(last_moving).all() and last_moving[free, 1].min() > low + 0.5 - voxel and last_moving[free, 1].min() > last_still[free, 1].min() + 0.2
    r = _cli_raw(d, os.path.join(d, "refused"), *common, "--obstacle_motion", os.path.join(d, "short.json"))
    assert r.returncode != 0 and "3 matrices, but the simulation has 4 frames" in r.stdout, r.stdout[-2000:]
