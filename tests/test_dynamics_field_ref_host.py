"""The float64 reference of field contact (tests/dynamics_field_ref.py) against dynamics_contact_ref.ContactDynamics where a grid holds
a plane, its own PCG against its exact solves on every case of tests/dynamics_field_cases.py, the cap on the rows that the active-set
comparison of test_gpu_dynamics_field.py leaves out; then gm_mesh_dynamics_field's refusals that need no device, MeshDynamics(field=)'s
own, and the command line's.  No device."""
import ctypes as C

import numpy as np
import pytest

import dynamics_cases as dc
import dynamics_contact_cases as cc
import dynamics_contact_ref as cr
import dynamics_field_cases as fc
import sdf_grid_ref as sg
from gaussianmesh_amd import _lib, edit_sequence

# a grid whose samples lie at multiples of 1/8 and a floor at -0.875: every sample value is exact in float32, so the grid IS the plane
DYADIC = ((30, 20, 30), (-3.75, -2.5, -3.75), 0.25)
FLOOR = -0.875


def dyadic_floor():
    dims, origin, voxel = DYADIC
    return sg.prepare(fc.plane_values(dims, origin, voxel, (0.0, 1.0, 0.0), FLOOR), voxel), np.asarray(origin, np.float32), voxel


@pytest.mark.parametrize("material", fc.MATERIALS)
@pytest.mark.parametrize("friction", [0.0, 0.5])
def test_a_plane_grid_is_the_equal_half_space(material, friction):
    """the free torus on the dyadic floor grid against ContactDynamics with floor(-0.875): positions and velocities within 1e-9 (the
    interpolated phi differs from n . x - d by roundings of 1e-16), the active sets equal after mapping 1 + K -> 1"""
    c = fc.case("tilt_smooth")
    r = fc.reference("tilt_smooth", material, field=dyadic_floor(), field_friction=friction)
    X, v, _ = r.run(c["V0"], c["v0"], fc.STEPS)
    want = cc.reference("drop_smooth", material, colliders=(cr.floor(FLOOR, friction=friction),))
    wX, wv, _ = want.run(c["V0"], c["v0"], fc.STEPS)
    assert float(np.abs(X.astype(np.float64) - wX).max()) <= 1e-9 and float(np.abs(v.astype(np.float64) - wv).max()) <= 1e-9
    near = np.abs(want.phi_star) < fc.NEAR
    assert np.array_equal(r.contact[~near], want.contact[~near]) and set(np.unique(r.contact)) == {0, 1} and (r.contact > 0).sum() > 100
    assert not r.fringe.any()


def test_the_field_is_candidate_K_ties_go_to_the_analytic_collider_and_nan_is_never_chosen():
    grid = dyadic_floor()
    X = dc.case("free_torus")["V0"].astype(np.float64)
    X[:, 1] -= 0.5
    tie = fc.reference("tilt_smooth", fc.MATERIALS[0], field=grid, colliders=(cr.floor(FLOOR),))
    _, _, which, best, gap = tie.contact_terms(X, X, tie.rows)
    below = X[:, 1] < FLOOR
    assert below.sum() > 10 and (which[below] == 1).all() and (which[~below] == 0).all() and np.allclose(gap[below], 0.0, atol=1e-15)
    lower = fc.reference("tilt_smooth", fc.MATERIALS[0], field=grid, colliders=(cr.floor(FLOOR - 0.01),), field_friction=0.4)
    which2 = lower.contact_terms(X, X, lower.rows)[2]
    assert (which2[below] == 2).all()                                  # the field's phi is the smaller one: 1 + K
    empty = (np.full_like(grid[0], np.nan), grid[1], grid[2])
    nothing = fc.reference("tilt_smooth", fc.MATERIALS[0], field=empty)
    kappa, c, which3, best3, _ = nothing.contact_terms(X, X, nothing.rows)
    assert not which3.any() and not kappa.any() and np.isinf(best3).all()
    kappa, c, which4, _, _ = lower.contact_terms(X, X - np.array([0.3, 0.0, 0.0]), lower.rows)      # the field's friction caps the pull back
    depth = FLOOR - X[below, 1]
    assert np.allclose(c[below][:, 1], FLOOR, atol=1e-12) and np.allclose(X[below, 0] - c[below][:, 0], np.minimum(0.3, lower.field_friction * depth), atol=1e-12)


@pytest.mark.parametrize("name, material", fc.ALL, ids=["%s-%d" % c for c in fc.ALL])
def test_pcg_against_exact_and_the_rows_left_out(name, material):
    """the reference's PCG at TIGHT against its exact solves: E_x and E_v lie at or below a quarter of section AA's bounds (1e-6 and
    1e-6 / dt), so those bounds are the device's here too; measured: E_x at most 2.4e-7 (one float32 rounding of a coordinate between 2
    and 4 that falls the other way), E_v at most 6.5e-6.  And the rows the device's active-set comparison leaves out (|phi*| or the gap to
    a second candidate below 1e-5, or within 1e-5 of where the field stops being known) are at most 2 % of rows x steps; measured: at
    most 0.07 %."""
    X, v, contact, compare = fc.reference_run(name, material)
    Xp, vp = fc.reference_run_pcg(name, material)
    ex, ev = float(np.abs(X.astype(np.float64) - Xp).max()), float(np.abs(v.astype(np.float64) - vp).max())
    left = 1.0 - float(compare.mean())
    print("%s material %d: E_x %.3g, E_v %.3g, left out %.3g %%, active rows x steps %d" % (name, material, ex, ev, 100.0 * left, int((contact > 0).sum())))
    assert ex <= 0.25e-6 and ev <= 0.25e-6 / fc.DT
    assert left <= 0.02
    c = fc.case(name)
    K = len(c["colliders"])
    assert (contact == 1 + K).sum() >= 16 and np.isfinite(X).all() and int(contact.max()) <= 1 + K


def test_pcg_against_exact_on_the_fused_floor():
    """the end-to-end case of test_gpu_dynamics_field.py - the stiff damped torus dropped from rest onto a floor fused from two top views
    (here by tsdf_ref.integrate_ref) - gets the same measurement: E_x, E_v at or below a quarter of the bounds (measured 3e-8 and 6e-8),
    the rows left out at most 2 %; and the volume is what the test needs: phi = y - floor in the band, unknown behind it"""
    tsdf, weight, origin, voxel, trunc = fc.fused_floor_volume()
    c = dc.case("free_torus")
    zero = np.zeros_like(c["V0"])
    r = fc.fused_floor_reference(tsdf, weight, origin, voxel, trunc)
    X, v, _ = r.run(c["V0"], zero, fc.STEPS)
    Xp, vp, _ = fc.fused_floor_reference(tsdf, weight, origin, voxel, trunc).run(c["V0"], zero, fc.STEPS, pcg=fc.TIGHT)
    ex, ev = float(np.abs(X.astype(np.float64) - Xp).max()), float(np.abs(v.astype(np.float64) - vp).max())
    left = float(((np.abs(r.phi_star) < fc.NEAR) | r.fringe).mean())
    print("fused floor: E_x %.3g, E_v %.3g, left out %.3g %%, active rows x steps %d" % (ex, ev, 100.0 * left, int((r.contact > 0).sum())))
    assert ex <= 0.25e-6 and ev <= 0.25e-6 / fc.DT and left <= 0.02 and (r.contact[-1] == 1).sum() >= 8
    assert (weight == 2).sum() > 32 * 32 * 4 and (weight == 0).sum() > 32 * 32 * 4
    phi, n = r.field_sample(np.array([[0.3, fc.GROUND + 0.1, -0.2], [0.3, fc.GROUND - 0.2, -0.2], [0.3, fc.GROUND - 1.2, -0.2]]))
    assert abs(phi[0] - 0.1) <= 1e-6 and abs(phi[1] + 0.2) <= 1e-6 and np.isnan(phi[2]) and np.allclose(n[:2], [0.0, 1.0, 0.0], atol=1e-6)


def test_the_cases_exercise_what_they_are_for():
    soft = fc.MATERIALS[0]
    g = fc.prepared("tilt_rough")
    assert (np.abs(g[..., 1:]).min(axis=(0, 1, 2)) > 0.05).all()       # all three gradient channels
    g = fc.prepared("bump")
    assert len(np.unique(np.round(g[..., 2], 3))) > 10                 # the crease: the y gradient is not one number
    for name in ("sheet25", "sheet1056"):
        c = fc.case(name)
        assert c["field"]["friction"] > 0.0 and abs(float(c["v0"][0, 0])) > 0.1 and len(c["V0"]) == (25 if name == "sheet25" else 1056)
    for name in ("half_outside", "unknown_block"):        # rows that are below the floor and not in contact, beside rows that are
        X, _, contact, _ = fc.reference_run(name, soft)
        r = fc.reference(name, soft)
        P = X[-1].astype(np.float64)                                   # (contact is that of the last ITERATE: rows 0.1 clear of the border)
        probes = [np.isnan(r.field_sample(P + d)[0]) for d in 0.1 * np.concatenate([np.zeros((1, 3)), np.eye(3), -np.eye(3)])]
        unknown, known = np.all(probes, axis=0), ~np.any(probes, axis=0)
        low = P[:, 1] < fc.GROUND - 1e-3
        assert (low & unknown).sum() >= 4 and not contact[-1][unknown].any() and contact[-1][low & known].all() and (low & known).sum() >= 4
    assert set(np.unique(fc.reference_run("field_pusher", soft)[2])) == {0, 1, 2}
    assert set(np.unique(fc.reference_run("field_sixteen", soft)[2])) == {0, 12, 17}
    assert np.isnan(fc.prepared("unknown_block")[..., 0]).sum() == 6 * 16 * 4 and fc.prepared("half_outside").shape == (24, 16, 14, 4)


# ---- gm_mesh_dynamics_field's refusals ----
def test_mesh_dynamics_field_refuses_before_any_gpu_work():
    l = _lib.lib()
    Vm, T, H, K = 100, 4, 3, 2
    a = 1 << 30                                                        # non-null "pointers", 4 MiB apart: never dereferenced
    names = ("off", "cols", "w", "V0", "mass", "held", "ids", "targets", "x", "v", "out", "vout", "stats", "ws", "kinds", "rows", "mus", "contact", "grid")
    P = {k: a + (i << 22) for i, k in enumerate(names)}
    need = l.gm_mesh_dynamics_contact_workspace_bytes(Vm)
    org = (C.c_float * 3)(0.0, 0.0, 0.0)

    def call(T=T, Vm=Vm, H=H, dt=1 / 30, k=10.0, damp=0.02, its=3, cg=8, tol=1e-6, K=K, kc=1e4, n=(8, 9, 10), origin=org, voxel=0.1, mu=0.3, nbytes=need, **kw):
        p = dict(P, **kw)
        return l.gm_mesh_dynamics_field(T, Vm, p["off"], p["cols"], p["w"], p["V0"], p["mass"], p["held"], H, p["ids"], p["targets"], p["x"], p["v"], dt, k,
                                        damp, 0.0, -9.8, 0.0, its, cg, tol, K, p["kinds"], p["rows"], p["mus"], kc, n[0], n[1], n[2], origin, voxel, p["grid"],
                                        mu, p["out"], p["vout"], p["contact"], p["stats"], p["ws"], nbytes, None)

    def refused(what, rc=1, **kw):
        assert call(**kw) == rc and b"gm_mesh_dynamics_field" in l.gm_last_error() and what in l.gm_last_error(), (kw, l.gm_last_error())
    nan, inf = float("nan"), float("inf")
    # everything gm_mesh_dynamics_contact refuses
    for kw, what in ((dict(T=0), b"T ="), (dict(T=65), b"T ="), (dict(Vm=0), b"Vm"), (dict(H=-1), b"H ="), (dict(dt=0.0), b"dt"), (dict(k=nan), b"stiffness"),
                     (dict(damp=1.0), b"damping"), (dict(its=0), b"iterations"), (dict(cg=0), b"cg_iterations"), (dict(tol=-1.0), b"cg_tolerance"),
                     (dict(K=17), b"K ="), (dict(K=-1), b"K ="), (dict(kc=0.0), b"contact_stiffness"), (dict(kc=nan), b"contact_stiffness"),
                     (dict(kinds=None), b"null"), (dict(rows=None), b"null"), (dict(mus=None), b"null"), (dict(x=None), b"null"), (dict(out=None), b"null"),
                     (dict(ws=None), b"null")):
        refused(what, **kw)
    # the grid
    for n in ((1, 9, 10), (8, 1, 10), (8, 9, 1), (0, 9, 10)):
        refused(b"at least 2", n=n)
    refused(b"2^28", n=(1 << 10, 1 << 10, (1 << 8) + 1))
    for voxel in (0.0, -0.1, nan, inf):
        refused(b"voxel", voxel=voxel)
    for bad in ((nan, 0.0, 0.0), (0.0, inf, 0.0), (0.0, 0.0, -inf)):
        refused(b"origin", origin=(C.c_float * 3)(*bad))
    refused(b"null", origin=None)
    refused(b"null", grid=None)                                        # refused, not routed to gm_mesh_dynamics_contact
    refused(b"aligned", grid=P["grid"] + 4)
    for mu in (-0.1, nan, -inf):
        refused(b"field_friction", mu=mu)
    for out in ("out", "vout", "stats", "ws", "contact"):
        refused(b"overlaps", **{out: P["grid"] + 16})
    refused(b"overlaps", grid=P["ws"] + 16 * 8)
    refused(b"overlaps", grid=P["out"] - 16 * 719)                     # the grid's last sample meets X_out
    # what may be: K == 0 without collider arrays, no contact_out, no stats - these reach the workspace check
    refused(b"workspace", rc=3, K=0, kinds=None, rows=None, mus=None, nbytes=need - 1)
    refused(b"workspace", rc=3, contact=None, stats=None, nbytes=need - 1)
    refused(b"workspace", rc=3, nbytes=l.gm_mesh_dynamics_workspace_bytes(Vm))                    # the contact entry's workspace, for every K
    refused(b"workspace", rc=3, mu=inf, grid=P["V0"] + 16, nbytes=0)                               # the grid is an input: it may alias one


def test_mesh_dynamics_refuses_a_field_that_is_none_on_the_host():
    from gaussianmesh_amd.dynamics import MeshDynamics
    c = cc.case("sheet5")
    for kw in (dict(field="grid"), dict(field=np.zeros((3, 3, 3, 4), np.float32)), dict(field_friction=-0.1), dict(field_friction=float("nan")),
               dict(field_friction=float("inf")), dict(field_friction="0.3"), dict(field_friction=True)):
        with pytest.raises(ValueError):
            MeshDynamics(c["V0"], c["faces"], device="cpu", **kw)
    m = MeshDynamics(c["V0"], c["faces"], device="cpu", field=None, field_friction=0.25)
    assert m.field is None and m.field_friction == 0.25


BASE = ["--object_gaussian", "o.ply", "--object_origin_mesh", "m.obj", "--camera_path", ".", "--render_path", "out", "--handle_sequence", "h.npz"]


@pytest.mark.parametrize("extra, what", [
    (["--background_gaussian", "bg.ply", "--background_contact"], "--background_contact sets what the simulated mesh collides with and needs --dynamics"),
    (["--dynamics", "--background_contact"], "--background_contact collides with the background cloud and needs --background_gaussian"),
    (["--dynamics", "--background_contact", "64"], "needs --background_gaussian"),
    (["--dynamics", "--background_gaussian", "bg.ply", "--background_contact", "1"], "--background_contact 1"),
    (["--dynamics", "--background_gaussian", "bg.ply", "--contact_margin", "0.2"], "--contact_margin grows the volume of --background_contact and needs it"),
    (["--dynamics", "--background_gaussian", "bg.ply", "--background_contact", "--contact_margin", "-1"], "--contact_margin -1"),
    (["--dynamics", "--background_gaussian", "bg.ply", "--background_contact", "--contact_margin", "nan"], "--contact_margin nan"),
    (["--dynamics", "--friction", "0.3"], "--friction is the friction of"),
    (["--dynamics", "--contact_stiffness", "100"], "--contact_stiffness needs something to collide with"),
])
def test_cli_flag_refusals_come_before_any_device_work(extra, what, monkeypatch):
    import builtins
    real = builtins.__import__

    def no_torch(name, *a, **kw):
        assert name != "torch" and not name.endswith("edittool"), name
        return real(name, *a, **kw)
    monkeypatch.setattr(builtins, "__import__", no_torch)
    with pytest.raises(SystemExit) as e:
        edit_sequence.main(BASE + extra)
    assert what in str(e.value) and "edit_sequence:" in str(e.value)


@pytest.mark.parametrize("extra", [["--friction", "0.3"], ["--contact_stiffness", "2e4"], ["--contact_margin", "0.25", "--floor", "-1", "--gravity", "0", "-9.8", "0"]])
def test_cli_accepts_friction_and_stiffness_with_the_background_alone(extra):
    """with --background_contact as the only thing to collide with, --friction and --contact_stiffness pass the flag checks: the run
    ends at the first file it cannot read, not at a refusal"""
    with pytest.raises((SystemExit, OSError)) as e:
        edit_sequence.main(BASE + ["--dynamics", "--background_gaussian", "no_such_bg.ply", "--background_contact", "32"] + extra)
    assert "edit_sequence: --" not in str(e.value)
