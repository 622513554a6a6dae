"""The float64 reference of contact with moving fields (tests/dynamics_moving_field_ref.py) against things it does not define: its
parent FieldDynamics under identity poses, invariance under a change of frame, a plate that carries or slides under a sheet, the scalar
recursion of section AB under a rising plate; its own PCG against its exact solves on every case of tests/dynamics_moving_field_cases.py
and the cap on the rows that the active-set comparison of test_gpu_dynamics_moving_field.py leaves out; dynamics.rigid_pose; then
gm_mesh_dynamics_fields' refusals that need no device, MeshDynamics(fields=)'s own, and the command line's.  No device."""
import ctypes as C
import json

import numpy as np
import pytest

import dynamics_cases as dc
import dynamics_contact_cases as cc
import dynamics_contact_ref as cr
import dynamics_field_cases as fc
import dynamics_moving_field_cases as mc
import dynamics_moving_field_ref as mr
from gaussianmesh_amd import _lib, edit_sequence

SOFT, STIFF = mc.MATERIALS


# ---- the reference against what it does not define ----
@pytest.mark.parametrize("name", ["tilt_rough", "field_pusher", "unknown_block"])
def test_identity_poses_are_the_static_field_exactly(name):
    """one field at the identity in every step: positions, velocities, contacts, phi*, gaps and the fringe are FieldDynamics' arrays"""
    c = fc.case(name)
    want = fc.reference(name, SOFT)
    wX, wv, _ = want.run(c["V0"], c["v0"], fc.STEPS, c["targets"], collider_rows=c["collider_rows"])
    f = c["field"]
    k, g, d = dc.MATERIALS[SOFT]
    r = mr.MovingFieldDynamics(c["V0"], c["faces"], c["mass"], pinned=c["pinned"], handles=c["handles"], dt=fc.DT, stiffness=k, damping=d, gravity=g,
                               iterations=fc.ITERATIONS, colliders=c["colliders"], contact_stiffness=fc.KC,
                               fields=[(fc.prepared(name), f["origin"], f["voxel"])], field_frictions=[f["friction"]])
    for poses in (None, np.tile(mr.IDENTITY, (fc.STEPS, 1, 1, 1))):
        r.poses = mr.IDENTITY[None].copy()
        X, v, _ = r.run(c["V0"], c["v0"], fc.STEPS, c["targets"], collider_rows=c["collider_rows"], field_poses=poses)
        assert np.array_equal(X, wX) and np.array_equal(v, wv) and np.array_equal(r.contact, want.contact) and np.array_equal(r.fringe, want.fringe)
        assert np.array_equal(r.phi_star, want.phi_star) and np.array_equal(r.gap, want.gap) and (r.contact > 0).sum() > 50


def _turned(c, Q):
    """a case's colliders and collider rows turned by the rotation Q (normals and centres; offsets and radii stay)"""
    def turn(rows):
        rows = np.array(rows, np.float32, copy=True)
        rows[..., :3] = (rows[..., :3].astype(np.float64) @ Q.T).astype(np.float32)
        return rows
    colliders = tuple((k, turn(row), mu) for k, row, mu in c["colliders"])
    return colliders, None if c["collider_rows"] is None else turn(c["collider_rows"])


@pytest.mark.parametrize("name", ["tilt_spin", "two", "four_sixteen", "slide_rough"])
def test_frame_invariance(name):
    """mesh, state, gravity, colliders and poses all turned by one rigid motion Q: the result is the turned result within 1e-9.  The
    state is rounded to float32 at every step boundary, and that rounding is not invariant under a general motion (a turned coordinate
    rounds elsewhere, by 1e-7); so Q is the rotation by 120 degrees about (1, 1, 1), which permutes the axes: every float32 number stays
    one, and what is left is the order of float64 roundings in R^T (X - t), R nl and the carried anchor - the products Q R are general
    rotation matrices, and the grids keep their own frames."""
    Q = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    assert np.linalg.det(Q) == 1.0
    c = mc.case(name)
    X, v, contact, _ = mc.reference_run(name, STIFF)
    k, g, d = dc.MATERIALS[STIFF]
    colliders, rows = _turned(c, Q)
    r = mr.MovingFieldDynamics(c["V0"] @ Q.T.astype(np.float32), c["faces"], c["mass"], pinned=c["pinned"], handles=c["handles"], dt=mc.DT, stiffness=k,
                               damping=d, gravity=tuple(Q @ np.asarray(g)), iterations=mc.ITERATIONS, colliders=colliders, contact_stiffness=mc.KC,
                               fields=mc.prepared(name), field_frictions=[f["friction"] for f in c["fields"]])
    turn = lambda P: np.concatenate([Q @ P[..., :3], Q @ P[..., 3:]], axis=-1)
    r.poses = turn(c["pose0"])
    tX, tv, _ = r.run(c["V0"] @ Q.T.astype(np.float32), c["v0"] @ Q.T.astype(np.float32), mc.STEPS, collider_rows=rows, field_poses=turn(c["field_poses"]))
    ex = float(np.abs(tX.astype(np.float64) - X.astype(np.float64) @ Q.T).max())
    ev = float(np.abs(tv.astype(np.float64) - v.astype(np.float64) @ Q.T).max())
    print("%s turned: positions %.3g, velocities %.3g" % (name, ex, ev))
    assert ex <= 1e-9 and ev <= 1e-9 and (contact > 0).sum() > 100


def _plate_run(friction, velocity, steps, v0=(0.4, -0.5, 0.2), material=(10.0, dc.GRAVITY, 0.0)):
    """the 25-vertex sheet 0.1 above dynamics_field_cases' plate grid, which moves at `velocity`: (reference, positions, last velocities)"""
    V0, faces = cc.sheet(5, 5, height=0.1)
    k, g, d = material
    plate = (fc.sg.prepare(fc.plane_values(*fc.SHEET_GRID, (0.0, 1.0, 0.0), 0.0), fc.SHEET_GRID[2]), np.asarray(fc.SHEET_GRID[1], np.float32), fc.SHEET_GRID[2])
    r = mr.MovingFieldDynamics(V0, faces, cr.dr.vertex_masses(V0, faces), dt=mc.DT, stiffness=k, damping=d, gravity=g, iterations=mc.ITERATIONS,
                               contact_stiffness=mc.KC, fields=[plate], field_frictions=[friction])
    X, v, _ = r.run(V0, np.tile(np.asarray(v0, np.float32), (len(V0), 1)), steps, field_poses=mc.translations(velocity, steps)[:, None])
    return r, X.astype(np.float64), v.astype(np.float64)


def test_a_rough_plate_carries_the_sheet_and_a_smooth_one_does_not():
    """the plate translates at (0.3, 0, 0) under a sheet that arrives with (0.4, ., 0.2).  Friction 0.5: Coulomb's limit mu |phi| kc h^2
    is worth mu |g| = 4.9 per second of tangential velocity, so the relative velocity (0.1, 0.2) is gone within three steps of the
    landing; from then on the row is held to the carried anchor with the weight kc h^2 = 11.1 against its inertia, so what is left of the
    relative velocity shrinks by 12.1 per step: after 20 steps the sheet's tangential velocity is the plate's to 1e-6 (float32 keeps 3e-8
    of 0.3).  Friction 0: the tangential velocity stays the sheet's own, to the float32 rounding of the state (1e-6 over 20 steps)."""
    r, X, v = _plate_run(0.5, (mc.PLATE_SPEED, 0.0, 0.0), 20)
    assert (r.contact[-8:] == 1).all()
    assert float(np.abs(v[:, 0] - mc.PLATE_SPEED).max()) <= 1e-6 and float(np.abs(v[:, 2]).max()) <= 1e-6
    r, X, v = _plate_run(0.0, (mc.PLATE_SPEED, 0.0, 0.0), 20)
    assert (r.contact[-8:] == 1).all()
    assert float(np.abs(v[:, 0] - np.float32(0.4)).max()) <= 1e-6 and float(np.abs(v[:, 2] - np.float32(0.2)).max()) <= 1e-6


@pytest.mark.parametrize("damping", [0.0, 0.02])
def test_a_rising_plate_reproduces_the_scalar_recursion(damping):
    """section AB's recursion with the plate's height of each step: Y <- (Y + h v + h^2 a + kc h^2 H_t) / (1 + kc h^2) while the
    prediction is below H_t = 0.3 (t + 1) h, the prediction itself above; to 1e-7, as test_dynamics_contact_ref_host.py holds the static
    floor to (float32 rounding of heights below 0.2 at the step boundaries)"""
    steps = 24
    r, X, _ = _plate_run(0.0, (0.0, mc.PLATE_SPEED, 0.0), steps, v0=(0.0, -0.5, 0.0), material=(10.0, dc.GRAVITY, damping))
    Y, v, want = float(np.float32(0.1)), float(np.float32(-0.5)), []
    h, kh = mc.DT, mc.KC * mc.DT * mc.DT
    for t in range(steps):
        H = mc.PLATE_SPEED * (t + 1) * h
        y = Y + h * v + h * h * dc.GRAVITY[1]
        new = (y + kh * H) / (1.0 + kh) if y < H else y
        v = float(np.float32((1.0 - damping) * (new - Y) / h))
        Y = float(np.float32(new))
        want.append(Y)
    want = np.array(want)
    assert float(np.abs(X[:, :, 1] - want[:, None]).max()) <= 1e-7
    assert (r.contact[0] == 0).all() and (r.contact[-1] == 1).all() and want[-1] > 0.1       # it was caught, and lifted above where it began


def test_a_carried_anchor_is_where_the_obstacle_took_it():
    before = mc.pose(mc.rotation((0.3, 1.0, -0.2), 0.4), t=(0.5, -0.2, 0.1))
    now = mc.pose(mc.rotation((1.0, 0.2, 0.1), -0.7), t=(-0.3, 0.4, 0.9))
    p = np.random.default_rng(3).normal(size=(10, 3))
    local = np.linalg.solve(before[:, :3], (p - before[:, 3]).T).T
    assert np.allclose(mr.carry(before, now, p), local @ now[:, :3].T + now[:, 3], atol=1e-14)
    assert np.allclose(mr.carry(before, before, p), p, atol=1e-15)


# ---- the cases ----
@pytest.mark.parametrize("name, material", mc.ALL, ids=["%s-%d" % c for c in mc.ALL])
def test_pcg_against_exact_and_the_rows_left_out(name, material):
    """the reference's PCG at TIGHT against its exact solves: E_x and E_v lie at or below a quarter of section AA's bounds (1e-6 and
    1e-6 / dt), so those bounds are the device's here too - the rule of test_dynamics_field_ref_host.py; measured: E_x at most 2.4e-7
    (one float32 rounding of a coordinate between 2 and 4 that falls the other way), E_v at most 4.7e-6.  And the rows the device's
    active-set comparison leaves out (|phi*| or the gap to a second candidate below 1e-5, or within 1e-5 of where a field stops being
    known) are at most 2 % of rows x steps; measured: at most 0.07 %."""
    X, v, contact, compare = mc.reference_run(name, material)
    Xp, vp = mc.reference_run_pcg(name, material)
    ex, ev = float(np.abs(X.astype(np.float64) - Xp).max()), float(np.abs(v.astype(np.float64) - vp).max())
    left = 1.0 - float(compare.mean())
    print("%s material %d: E_x %.3g, E_v %.3g, left out %.3g %%, active rows x steps %d" % (name, material, ex, ev, 100.0 * left, int((contact > 0).sum())))
    assert ex <= 0.25e-6 and ev <= 0.25e-6 / mc.DT
    assert left <= 0.02
    c = mc.case(name)
    assert np.isfinite(X).all() and int(contact.max()) <= len(c["colliders"]) + len(c["fields"]) and (contact > 0).sum() >= 100


def test_the_cases_exercise_what_they_are_for():
    K = 16
    assert set(np.unique(mc.reference_run("two", SOFT)[2])) == {0, 1, 2}
    assert set(np.unique(mc.reference_run("four_sixteen", SOFT)[2])) == {0, 12, 1 + K, 1 + K + 3}           # the wall, the first and the last field
    c = mc.case("two")                                                 # the two contact regions meet: a row changes from one field to the other
    contact = mc.reference_run("two", SOFT)[2]
    assert ((contact[:-1] == 1) & (contact[1:] == 2)).any()
    for name in ("slide_smooth", "slide_rough", "rise", "pause"):
        c = mc.case(name)
        assert len(c["V0"]) == (1056 if name == "slide_rough" else 25) and c["field_poses"].shape == (mc.STEPS, 1, 3, 4)
    p = mc.case("pause")["field_poses"][:, 0]
    same = [np.array_equal(p[k], p[k - 1]) for k in range(1, mc.STEPS)]
    assert same[6:9] == [True] * 3 and sum(same) == 3 and p[-1, 0, 3] > p[9, 0, 3]           # it stands in steps 7 .. 9 and moves on
    R = mc.case("tilt_spin")["field_poses"][-1, 0, :, :3]
    assert np.abs(R - np.eye(3)).min() > 1e-5 and abs(np.linalg.det(R) - 1.0) < 1e-14          # all nine entries matter
    # half_leaves: rows below the floor that the grid has left are not in contact, rows it still covers are
    X, _, contact, _ = mc.reference_run("half_leaves", SOFT)
    r = mc.reference("half_leaves", SOFT)
    r.now = mc.case("half_leaves")["field_poses"][-1]
    P = X[-1].astype(np.float64)
    probes = [np.isnan(fc.sg.sample(*mc.prepared("half_leaves")[0], r.local(0, P + d))[0]) for d in 0.1 * np.concatenate([np.zeros((1, 3)), np.eye(3), -np.eye(3)])]
    unknown, known = np.all(probes, axis=0), ~np.any(probes, axis=0)
    low = P[:, 1] < mc.GROUND - 1e-3
    assert (low & unknown).sum() >= 4 and not contact[-1][unknown].any() and contact[-1][low & known].all() and (low & known).sum() >= 4
    assert unknown.sum() >= 40 and known.sum() >= 20                   # about half of the 96 rows on either side


# ---- rigid_pose ----
def test_rigid_pose_recovers_exact_motions_and_refuses_a_shear():
    from gaussianmesh_amd.dynamics import rigid_pose, rigid_poses
    V = dc.case("free_torus")["V0"].astype(np.float64)
    poses = [mc.pose(), mc.pose(mc.rotation((0.3, 1.0, -0.2), 0.4), t=(0.5, -0.2, 0.1)), mc.pose(mc.rotation((1.0, 0.2, 0.1), 3.0), t=(-3.0, 0.4, 9.0)),
             mc.pose(mc.rotation((0.0, 0.0, 1.0), np.pi))]
    moved = np.array([V @ P[:, :3].T + P[:, 3] for P in poses])
    for P, m in zip(poses, moved):
        got = rigid_pose(V, m, tolerance=1e-12)
        assert got.shape == (3, 4) and got.dtype == np.float64 and float(np.abs(got - P).max()) <= 1e-12
    assert float(np.abs(rigid_poses(V, moved, tolerance=1e-12) - np.array(poses)).max()) <= 1e-12
    flat = V * np.array([1.0, 0.0, 1.0])                               # a planar mesh has a rotation too (no reflection)
    assert abs(np.linalg.det(rigid_pose(flat, flat @ poses[1][:, :3].T, tolerance=1e-12)[:, :3]) - 1.0) <= 1e-12
    shear = np.array([[1.0, 0.05, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    for bad in (V @ shear.T, V * 1.01, V * np.array([1.0, 1.0, -1.0])):
        with pytest.raises(ValueError, match="rigid"):
            rigid_pose(V, bad)
    with pytest.raises(ValueError, match="frame 1"):
        rigid_poses(V, np.array([moved[1], V @ shear.T]))
    assert rigid_pose(V, V @ shear.T, tolerance=1.0).shape == (3, 4)   # the tolerance is the caller's
    for a, b in ((V[:2], V[:2]), (V, V[:-1]), (V.reshape(-1), V.reshape(-1)), (V, np.full_like(V, np.nan))):
        with pytest.raises(ValueError):
            rigid_pose(a, b)
    with pytest.raises(ValueError):
        rigid_poses(V, V)


# ---- gm_mesh_dynamics_fields' refusals ----
def test_mesh_dynamics_fields_refuses_before_any_gpu_work():
    l = _lib.lib()
    Vm, T, H, K, F = 100, 4, 3, 2, 3
    a = 1 << 30                                                        # non-null "pointers", 4 MiB apart: never dereferenced
    names = ("off", "cols", "w", "V0", "mass", "held", "ids", "targets", "x", "v", "out", "vout", "stats", "ws", "kinds", "rows", "mus", "contact", "poses",
             "grid0", "grid1", "grid2", "grid3")
    P = {k: a + (i << 22) for i, k in enumerate(names)}
    need = l.gm_mesh_dynamics_contact_workspace_bytes(Vm)

    def call(T=T, Vm=Vm, H=H, dt=1 / 30, k=10.0, damp=0.02, its=3, cg=8, tol=1e-6, K=K, kc=1e4, F=F, n=(8, 9, 10), origin=(0.0, 0.0, 0.0), voxel=0.1, mu=0.3,
             nbytes=need, bad=1, table=True, **kw):
        """field `bad` takes n, origin, voxel, mu and the grid given as grid=; the others are plain"""
        p = dict(P, **kw)
        rows = []
        for f in range(min(max(F, 0), 4)):                              # (the table holds four at the most, whatever F says)
            mine = f == bad
            rows.append(_lib.DynamicsField(*(n if mine else (8, 9, 10)), (C.c_float * 3)(*(origin if mine else (0.0, 0.0, 0.0))), voxel if mine else 0.1,
                                           p.get("grid", p["grid%d" % f]) if mine else p["grid%d" % f], mu if mine else 0.3))
        fields = (_lib.DynamicsField * max(len(rows), 1))(*rows) if table else None
        return l.gm_mesh_dynamics_fields(T, Vm, p["off"], p["cols"], p["w"], p["V0"], p["mass"], p["held"], H, p["ids"], p["targets"], p["x"], p["v"], dt, k,
                                         damp, 0.0, -9.8, 0.0, its, cg, tol, K, p["kinds"], p["rows"], p["mus"], kc, F, fields, p["poses"], p["out"], p["vout"],
                                         p["contact"], p["stats"], p["ws"], nbytes, None)

    def refused(what, rc=1, **kw):
        assert call(**kw) == rc and b"gm_mesh_dynamics_fields" in l.gm_last_error() and what in l.gm_last_error(), (kw, l.gm_last_error())
    nan, inf = float("nan"), float("inf")
    # everything gm_mesh_dynamics_contact refuses
    for kw, what in ((dict(T=0), b"T ="), (dict(T=65), b"T ="), (dict(Vm=0), b"Vm"), (dict(H=-1), b"H ="), (dict(dt=0.0), b"dt"), (dict(k=nan), b"stiffness"),
                     (dict(damp=1.0), b"damping"), (dict(its=0), b"iterations"), (dict(cg=0), b"cg_iterations"), (dict(tol=-1.0), b"cg_tolerance"),
                     (dict(K=17), b"K ="), (dict(K=-1), b"K ="), (dict(kc=0.0), b"contact_stiffness"), (dict(kc=nan), b"contact_stiffness"),
                     (dict(kinds=None), b"null"), (dict(rows=None), b"null"), (dict(mus=None), b"null"), (dict(x=None), b"null"), (dict(out=None), b"null"),
                     (dict(ws=None), b"null")):
        refused(what, **kw)
    # the table
    assert _lib.GM_MESH_FIELDS_MAX == 4
    refused(b"F =", F=5)
    refused(b"F =", F=-1)
    refused(b"null", table=False)
    refused(b"field_poses", poses=None)
    # one grid of the table, first, middle and last
    for bad in (0, 1, 2):
        for n in ((1, 9, 10), (8, 1, 10), (8, 9, 1), (0, 9, 10)):
            refused(b"at least 2", n=n, bad=bad)
        refused(b"2^28", n=(1 << 10, 1 << 10, (1 << 8) + 1), bad=bad)
        for voxel in (0.0, -0.1, nan, inf):
            refused(b"voxel", voxel=voxel, bad=bad)
        for org in ((nan, 0.0, 0.0), (0.0, inf, 0.0), (0.0, 0.0, -inf)):
            refused(b"origin", origin=org, bad=bad)
        refused(b"null", grid=None, bad=bad)
        refused(b"aligned", grid=P["grid%d" % bad] + 4, bad=bad)
        for mu in (-0.1, nan, -inf):
            refused(b"friction", mu=mu, bad=bad)
        for out in ("out", "vout", "stats", "ws", "contact"):
            refused(b"overlaps", bad=bad, **{out: P["grid%d" % bad] + 16})
        refused(b"overlaps", grid=P["ws"] + 16 * 8, bad=bad)
        refused(b"overlaps", grid=P["out"] - 16 * 719, bad=bad)        # the grid's last sample meets X_out
    for out in ("out", "vout", "stats", "ws", "contact"):               # the poses: 96 (T + 1) F bytes
        refused(b"overlaps", **{out: P["poses"] + 96 * (T + 1) * F - 8})
    refused(b"workspace", rc=3, nbytes=need - 1, **{"out": P["poses"] + 96 * (T + 1) * F})     # just behind them is fine
    # what may be: F == 0 with no table and no poses, K == 0 without collider arrays, no contact_out, no stats, grids that alias inputs
    refused(b"workspace", rc=3, F=0, table=False, poses=None, nbytes=need - 1)
    refused(b"workspace", rc=3, K=0, kinds=None, rows=None, mus=None, nbytes=need - 1)
    refused(b"workspace", rc=3, contact=None, stats=None, nbytes=need - 1)
    refused(b"workspace", rc=3, nbytes=l.gm_mesh_dynamics_workspace_bytes(Vm))
    refused(b"workspace", rc=3, mu=inf, grid=P["V0"] + 16, nbytes=0)
    refused(b"workspace", rc=3, F=4, grid=P["grid0"], bad=3, nbytes=0)  # two fields may share one grid


def test_mesh_dynamics_refuses_fields_on_the_host():
    from gaussianmesh_amd.dynamics import MeshDynamics
    c = cc.case("sheet5")
    for kw in (dict(fields="grid"), dict(fields=[np.zeros((3, 3, 3, 4), np.float32)]), dict(fields=[None]), dict(field_frictions=[0.1]),
               dict(fields=[], field_frictions=0.3), dict(fields=[], field_frictions=[0.1])):
        with pytest.raises(ValueError):
            MeshDynamics(c["V0"], c["faces"], device="cpu", **kw)
    m = MeshDynamics(c["V0"], c["faces"], device="cpu", fields=[], field_frictions=[])
    assert m.NF == 0 and m.fields == () and m.field is None
    with pytest.raises(ValueError, match="no fields"):
        m.run(2, field_poses=np.tile(mr.IDENTITY, (2, 1, 1, 1)))
    with pytest.raises(ValueError, match="no fields"):
        m.reset(field_poses=mr.IDENTITY[None])


# ---- the command line ----
BASE = ["--object_gaussian", "o.ply", "--object_origin_mesh", "m.obj", "--camera_path", ".", "--render_path", "out", "--handle_sequence", "h.npz"]


def _motion(tmp_path, doc):
    path = str(tmp_path / "motion.json")
    with open(path, "w") as fh:
        json.dump(doc, fh)
    return path


def test_cli_obstacle_motion_refusals_come_before_any_device_work(tmp_path, monkeypatch):
    import builtins
    good = [mc.pose(mc.rotation((0.0, 1.0, 0.0), 0.1 * k), t=(0.1 * k, 0.0, 0.0)).tolist() for k in range(3)]
    four = [np.vstack([np.array(p), [0.0, 0.0, 0.0, 1.0]]).tolist() for p in good]
    assert np.array_equal(edit_sequence.read_obstacle_motion(_motion(tmp_path, good)), np.array(good))
    assert np.array_equal(edit_sequence.read_obstacle_motion(_motion(tmp_path, four)), np.array(good))
    obj = str(tmp_path / "obstacle.obj")
    with open(obj, "w") as fh:
        fh.write("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    sheared, mirrored, scaled, nonfinite, bottom = (json.loads(json.dumps(good)) for _ in range(5))
    sheared[1][0][1] += 0.01
    mirrored[2] = (np.array(good[2]) * np.array([[1.0], [1.0], [-1.0]])).tolist()
    scaled[0] = (np.array(good[0]) * 1.001).tolist()
    nonfinite[1][0][3] = float("inf")
    bottom = json.loads(json.dumps(four))
    bottom[1][3] = [0.0, 0.0, 0.0, 2.0]
    real = builtins.__import__

    def no_torch(name, *a, **kw):
        assert name != "torch" and not name.endswith("edittool"), name
        return real(name, *a, **kw)
    monkeypatch.setattr(builtins, "__import__", no_torch)
    cases = [(["--dynamics", "--obstacle_motion", _motion(tmp_path, good)], "--obstacle_motion moves the solid of --obstacle_mesh and needs it"),
             (["--obstacle_motion", "m.json"], "--obstacle_motion moves the solid of --obstacle_mesh and needs it"),
             (["--dynamics", "--obstacle_mesh", obj, "--obstacle_motion", str(tmp_path / "none.json")], "cannot read it as JSON")]
    for doc, what in ((sheared, "frame 1"), (mirrored, "frame 2"), (scaled, "frame 0"), (nonfinite, "frame 1"), (bottom, "0 0 0 1"), ([], "at least one"),
                      ({"poses": good}, "3x4 or 4x4"), ([[1.0, 2.0, 3.0]], "3x4 or 4x4")):
        path = str(tmp_path / ("bad%d.json" % len(cases)))
        with open(path, "w") as fh:
            json.dump(doc, fh)
        cases.append((["--dynamics", "--obstacle_mesh", obj, "--obstacle_motion", path], what))
    for extra, what in cases:
        with pytest.raises(SystemExit) as e:
            edit_sequence.main(BASE + extra)
        assert what in str(e.value) and "edit_sequence:" in str(e.value), (extra, str(e.value))
    # what was refused before stays refused, in the same words
    with pytest.raises(SystemExit) as e:
        edit_sequence.main(BASE + ["--dynamics", "--background_gaussian", "bg.ply", "--background_contact", "--obstacle_mesh", obj, "--obstacle_motion",
                                   _motion(tmp_path, good)])
    assert "--obstacle_mesh with --background_contact: a simulation takes one volume" in str(e.value)
