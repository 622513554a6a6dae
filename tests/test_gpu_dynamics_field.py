"""-m gpu: gm_mesh_dynamics_field (dynamics.MeshDynamics(field=SdfGrid)) against the float64 reference of tests/dynamics_field_ref.py on
the cases and materials of tests/dynamics_field_cases.py: positions, velocities and the active set; a plane grid against the equal
half-space; fields nothing reaches against the old entries, bit for bit; batches and repeatability on poisoned memory; what the field
leaves alone; the tie rule; a real TsdfVolume end to end; refusals; and the edit surface on top of it (SingleObjectDeform.simulate,
SceneVisualTool.background_field, edit_sequence --background_contact)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dynamics_cases as dc
import dynamics_contact_cases as cc
import dynamics_contact_ref as cr
import dynamics_field_cases as fc
import sdf_grid_ref as sg
from poison import differing, run_under_fills, same_bits
from test_dynamics_field_ref_host import DYADIC, FLOOR
from test_gpu_arap import _drags, _scene64
from test_gpu_dynamics import _cli

pytestmark = pytest.mark.gpu
TIGHT = dict(cg_iterations=fc.TIGHT[0], cg_tolerance=fc.TIGHT[1])
SOFT, STIFF = fc.MATERIALS


def _dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


def _colliders(ref_colliders):
    return [("sphere" if k == cr.SPHERE else "half_space", tuple(float(x) for x in row), mu) for k, row, mu in ref_colliders]


@pytest.fixture(scope="module")
def grids():
    """one SdfGrid per case, prepared on the device once and shared (a grid is static)"""
    from gaussianmesh_amd.dynamics import SdfGrid
    made = {}

    def get(name):
        if name not in made:
            f = fc.case(name)["field"]
            made[name] = SdfGrid(f["values"], f["origin"], f["voxel"])
        return made[name]
    return get


def _grid_of(values, origin, voxel):
    from gaussianmesh_amd.dynamics import SdfGrid
    return SdfGrid(values, origin, voxel)


def _dyadic_floor():
    dims, origin, voxel = DYADIC
    return _grid_of(fc.plane_values(dims, origin, voxel, (0.0, 1.0, 0.0), FLOOR), origin, voxel)


def _dyn(name, material, field, colliders=None, pinned=None, handles=None, **kw):
    """a fresh MeshDynamics of the case at its starting state, with the reference's own masses, the case's colliders and `field`"""
    from gaussianmesh_amd.dynamics import MeshDynamics
    c = fc.case(name)
    k, g, d = dc.MATERIALS[material] if isinstance(material, int) else material
    opts = dict(TIGHT, mass=c["mass"], stiffness=k, gravity=g, damping=d, dt=fc.DT, iterations=fc.ITERATIONS, contact_stiffness=fc.KC,
                colliders=_colliders(c["colliders"] if colliders is None else colliders), field=field, field_friction=c["field"]["friction"])
    opts.update(kw)
    m = MeshDynamics(c["V0"], c["faces"], pinned=c["pinned"] if pinned is None else pinned, handles=c["handles"] if handles is None else handles, **opts)
    m.reset(velocities=_dev(c["v0"]))
    return m


def _rows(name, steps=fc.STEPS):
    r = fc.case(name)["collider_rows"]
    return None if r is None else _dev(r[:steps])


# ---- 1. against the reference ----
@pytest.mark.parametrize("name, material", fc.ALL, ids=["%s-%d" % c for c in fc.ALL])
def test_against_the_reference(name, material, grids):
    """16 steps at (400, 1e-10): max |X_out - X_ref| <= 1e-6 and max |v_out - v_ref| <= 1e-6 / dt, section AA's bounds: on the CPU the
    reference's PCG against its exact solves gave E_x <= 2.4e-7 and E_v <= 6.5e-6 on these cases, at or below a quarter of them
    (test_dynamics_field_ref_host.py asserts it).  contact_out equals the reference's active set on every row but those within 1e-5 of
    a surface, of a second candidate or of where the field stops being known (at most 0.07 % of rows x steps; the CPU test caps them at
    2 %)."""
    want_x, want_v, want_c, compare = fc.reference_run(name, material)
    m = _dyn(name, material, grids(name))
    X, contact, stats = m.run(fc.STEPS, collider_rows=_rows(name), want_contacts=True, want_stats=True)
    X, v, stats = X.cpu().numpy().astype(np.float64), m.velocities.cpu().numpy().astype(np.float64), stats.cpu().numpy()
    contact = contact.cpu().numpy()
    assert X.shape == want_x.shape and v.shape == want_v.shape and stats.shape == (fc.STEPS, 6) and contact.shape == want_c.shape
    ex, ev = float(np.abs(X - want_x).max()), float(np.abs(v - want_v).max())
    wrong = int((contact != want_c)[compare].sum())
    print("%s material %d: max |X_hip - X_ref| %.3g, max |v_hip - v_ref| %.3g, CG steps at most %d, residual at most %.3g, %d rows x steps in "
          "contact, %d compared rows differ, %d of the rows left out differ"
          % (name, material, ex, ev, int(stats[:, :3].max()), stats[:, 3:].max(), int((contact > 0).sum()), wrong, int((contact != want_c)[~compare].sum())))
    assert np.isfinite(X).all() and np.isfinite(v).all()
    assert ex <= 1e-6 and ev <= 1e-6 / fc.DT
    assert wrong == 0 and contact.dtype == np.int32 and int(contact.max()) == 1 + m.K
    assert (stats[:, 3:] <= 1e-10).all() and (stats[:, :3] <= 400).all() and (stats[:, :3] == np.round(stats[:, :3])).all()
    assert same_bits(m.positions, _dev(X[-1]))


@pytest.mark.parametrize("material", fc.MATERIALS)
def test_a_plane_grid_against_the_equal_half_space(material):
    """a grid whose samples are exact in float32 IS the plane: against gm_mesh_dynamics_contact with floor(-0.875) the positions agree
    within 1e-6 and 1e-6 / dt, and the contacts are equal (1 + K = 1 for both) wherever the analytic phi is not within 1e-5 of 0"""
    from gaussianmesh_amd.dynamics import MeshDynamics, floor
    c = fc.case("tilt_rough")
    a = _dyn("tilt_rough", material, _dyadic_floor())
    k, g, d = dc.MATERIALS[material]
    b = MeshDynamics(c["V0"], c["faces"], mass=c["mass"], stiffness=k, gravity=g, damping=d, dt=fc.DT, iterations=fc.ITERATIONS, contact_stiffness=fc.KC,
                     colliders=[floor(FLOOR, friction=0.5)], **TIGHT)
    b.reset(velocities=_dev(c["v0"]))
    Xa, ca = a.run(fc.STEPS, want_contacts=True)
    Xb, cb = b.run(fc.STEPS, want_contacts=True)
    ex, ev = float((Xa.double() - Xb.double()).abs().max()), float((a.velocities.double() - b.velocities.double()).abs().max())
    near = (Xb[:, :, 1].double() - FLOOR).abs() < fc.NEAR
    print("plane grid against the half-space, material %d: positions %.3g, velocities %.3g, %d contacts" % (material, ex, ev, int((cb > 0).sum())))
    assert ex <= 1e-6 and ev <= 1e-6 / fc.DT and bool((ca[~near] == cb[~near]).all()) and int((cb > 0).sum()) > 100 and int(ca.max()) == 1


# ---- 2. a field nothing reaches, and no field ----
@pytest.mark.parametrize("material", fc.MATERIALS)
def test_a_field_nothing_reaches_gives_the_bits_of_the_old_entries(material):
    """a floor grid far below, and a grid all of whose samples are NaN: kappa = 0 in every row, and the result is bit for bit that of the
    same object without a field - through gm_mesh_dynamics with no colliders, through gm_mesh_dynamics_contact with the corner's two"""
    dims, origin, voxel = fc.TORUS_GRID
    far = _grid_of(fc.plane_values(dims, origin, voxel, (0.0, 1.0, 0.0), -2.3), origin, voxel)
    unknown = _grid_of(np.full((dims[2], dims[1], dims[0]), np.nan, np.float32), origin, voxel)
    corner = cc.case("corner")["colliders"]
    for colliders in ((), corner):
        plain = _dyn("field_sixteen", material, None, colliders=colliders)
        P, pc, ps = plain.run(fc.STEPS, want_contacts=True, want_stats=True)
        for field in (far, unknown):
            m = _dyn("field_sixteen", material, field, colliders=colliders)
            X, contact, stats = m.run(fc.STEPS, want_contacts=True, want_stats=True)
            assert same_bits(X, P) and same_bits(m.velocities, plain.velocities) and same_bits(contact, pc) and same_bits(stats, ps)
        assert bool((pc > 0).any()) == bool(colliders) and int(pc.max()) <= len(colliders)


def test_field_none_calls_the_old_entries():
    """field=None: the object, its workspace and its bits are those of a MeshDynamics built without the argument"""
    from gaussianmesh_amd import _lib
    from gaussianmesh_amd.dynamics import MeshDynamics
    l = _lib.lib()
    c = fc.case("field_sixteen")
    for colliders, size in (((), l.gm_mesh_dynamics_workspace_bytes(96)), (cc.case("corner")["colliders"], l.gm_mesh_dynamics_contact_workspace_bytes(96))):
        a = _dyn("field_sixteen", STIFF, None, colliders=colliders)
        b = MeshDynamics(c["V0"], c["faces"], mass=c["mass"], stiffness=50.0, gravity=dc.GRAVITY, damping=0.02, dt=fc.DT, iterations=fc.ITERATIONS,
                         contact_stiffness=fc.KC, colliders=_colliders(colliders), **TIGHT)
        b.reset(velocities=_dev(c["v0"]))
        assert same_bits(a.run(fc.STEPS, want_contacts=True, want_stats=True), b.run(fc.STEPS, want_contacts=True, want_stats=True))
        assert same_bits(a.velocities, b.velocities) and a._ws.numel() == b._ws.numel() == size and a.field is None


# ---- 3. batches and repeatability ----
@pytest.mark.parametrize("name, material", [("field_pusher", STIFF), ("bump", SOFT), ("unknown_block", STIFF)])
def test_a_run_is_its_steps_one_by_one(name, material, grids):
    r = _rows(name)
    a, b, c = (_dyn(name, material, grids(name)) for _ in range(3))
    X, contact, stats = a.run(fc.STEPS, collider_rows=r, want_contacts=True, want_stats=True)
    single = torch.stack([b.step(collider_rows=None if r is None else r[k]) for k in range(fc.STEPS)], 0)
    assert same_bits(X, single) and same_bits(a.velocities, b.velocities) and same_bits(a.positions, b.positions)
    ones = [c.run(1, collider_rows=None if r is None else r[k:k + 1], want_contacts=True, want_stats=True) for k in range(fc.STEPS)]
    assert same_bits(contact, torch.cat([o[1] for o in ones], 0)) and same_bits(stats, torch.cat([o[2] for o in ones], 0))
    assert bool((contact == 1 + a.K).any()) and not same_bits(X[7], X[8])


def test_a_run_across_the_chunk_boundary(grids):
    """65 steps of the 25-vertex sheet, damped: one run, 65 single steps and two runs of other lengths give the same bits, contacts
    included, and the sheet lies on the field on both sides of step 64"""
    from gaussianmesh_amd import _lib
    n = _lib.GM_MESH_DYNAMICS_STEPS_MAX + 1
    damped = (10.0, dc.GRAVITY, 0.2)
    a, b, c = (_dyn("sheet25", damped, grids("sheet25")) for _ in range(3))
    X, contact = a.run(n, want_contacts=True)
    single = torch.stack([b.step() for _ in range(n)], 0)
    assert X.shape == (n, 25, 3) and same_bits(X, single) and same_bits(a.velocities, b.velocities)
    first = c.run(7, want_contacts=True)
    second = c.run(n - 7, want_contacts=True)
    assert same_bits(torch.cat([first[0], second[0]], 0), X) and same_bits(torch.cat([first[1], second[1]], 0), contact)
    assert bool((contact[60:64] == 1).any()) and bool((contact[64:] == 1).any())


@pytest.mark.parametrize("name, material", [("field_sixteen", STIFF), ("tilt_rough", SOFT), ("sheet1056", STIFF), ("half_outside", SOFT)])
def test_same_bits_from_call_to_call_and_on_poisoned_memory(name, material, grids):
    """two runs give the same bits; so do runs whose every allocation (X_out, contact_out, stats, the workspace of a fresh object, and the
    grid itself, prepared anew) was filled with 0x00, 0xFF and 0x5A beforehand, and no guard band around any of them is touched"""
    r = _rows(name)
    f = fc.case(name)["field"]

    def route():
        m = _dyn(name, material, _grid_of(f["values"], f["origin"], f["voxel"]))
        X, contact, stats = m.run(fc.STEPS, collider_rows=r, want_contacts=True, want_stats=True)
        return X, contact, stats, m.velocities, m.positions
    first = route()
    assert same_bits(first, route())
    runs = run_under_fills(route)
    assert all(p.handed_out >= 4 for p, _ in runs)
    assert differing(runs) == [] and same_bits(runs[0][1], first)


# ---- 4. what the field leaves alone ----
@pytest.mark.parametrize("name", ["half_outside", "unknown_block"])
def test_rows_outside_the_grid_and_over_unknown_samples_are_never_in_contact(name, grids):
    """the rows whose position samples to NaN - and still does 0.1 away along every axis - report 0 in every step although they fall
    below the floor, while their neighbours over known samples are in contact"""
    m = _dyn(name, SOFT, grids(name))
    X, contact = m.run(fc.STEPS, want_contacts=True)
    g = grids(name)
    shifts = 0.1 * torch.cat([torch.zeros((1, 3)), torch.eye(3), -torch.eye(3)]).to("cuda")
    probes = torch.stack([torch.isnan(g.sample((X + d).reshape(-1, 3))[0]).reshape(fc.STEPS, -1) for d in shifts], 0)
    unknown, known = probes.all(dim=0), ~probes.any(dim=0)
    low = X[:, :, 1] < fc.GROUND - 1e-3
    assert int((low & unknown).sum()) >= 16 and not bool(contact[unknown].any())
    assert int((low & known)[-1].sum()) >= 4 and bool((contact[-1][(low & known)[-1]] == 1).all())


def test_handle_and_pinned_rows_inside_the_field_are_untouched(grids):
    """the torus started 0.4 inside the floor grid with six rows scripted and three pinned: handle rows of X_out[t] are their targets bit
    for bit, pinned rows stay, and contact_out is 0 in all of them while free rows beside them are in contact"""
    c = fc.case("field_pusher")
    low = np.argsort(c["V0"][:, 1])
    handles, pins = low[:6].astype(np.int64), low[6:9].astype(np.int64)
    x_in = c["V0"].copy()
    x_in[:, 1] -= 0.4
    targets = np.tile(x_in[handles], (fc.STEPS, 1, 1))
    targets[:, :, 0] += (0.01 * np.arange(1, fc.STEPS + 1, dtype=np.float32))[:, None]
    m = _dyn("field_pusher", STIFF, grids("field_pusher"), colliders=(), pinned=pins, handles=handles)
    m.reset(positions=_dev(x_in))
    t = _dev(targets)
    X, contact = m.run(fc.STEPS, t, want_contacts=True)
    assert same_bits(X[:, _dev(handles, torch.int64)], t)
    assert np.array_equal(X.cpu().numpy()[:, pins], np.broadcast_to(x_in[pins], (fc.STEPS, 3, 3)))
    contact = contact.cpu().numpy()
    held = np.concatenate([handles, pins])
    assert not contact[:, held].any() and (contact == 1).sum() > 50
    assert (x_in[held, 1] < fc.GROUND - 0.05).all()


def test_a_tie_goes_to_the_analytic_collider():
    """the dyadic floor grid and the equal half-space at K = 1: every contact is reported as collider 1, never 2, and the meshes are the
    half-space's alone bit for bit.  Why the tie is exact: the half-space's phi is fma(0, z, fma(1, y, 0 x)) - d = round(y - d).  In the
    grid, y - origin_y is exact for a row in contact (both near -1, Sterbenz), so are the division by 0.25, the - 0.5 and f; the x and z
    interpolations add f * 0; and fma(f_y, q1 - q0 = 0.25, q0) rounds the exact y - d once: round(y - d) again.  A row deeper than the
    grid's first sample (y < -1) is outside the grid, so only the half-space sees it."""
    from gaussianmesh_amd.dynamics import SdfGrid, floor
    dims, origin, voxel = (30, 8, 30), (-3.75, -1.125, -3.75), 0.25
    grid = SdfGrid(fc.plane_values(dims, origin, voxel, (0.0, 1.0, 0.0), FLOOR), origin, voxel)
    flat = [cr.floor(FLOOR, friction=0.5)]
    both = _dyn("tilt_rough", SOFT, grid, colliders=flat)
    alone = _dyn("tilt_rough", SOFT, None, colliders=flat)
    X2, c2 = both.run(fc.STEPS, want_contacts=True)
    X1, c1 = alone.run(fc.STEPS, want_contacts=True)
    assert int((c1 > 0).sum()) > 100 and int(c2.max()) == 1 and same_bits(c1, c2) and same_bits(X1, X2)
    lower = _dyn("tilt_rough", SOFT, grid, colliders=[cr.floor(FLOOR - 0.125, friction=0.5)])
    assert int(lower.run(fc.STEPS, want_contacts=True)[1].max()) == 2   # and where the field's phi is the smaller one it is 1 + K


# ---- 5. a real TsdfVolume ----
def test_end_to_end_from_a_fused_volume():
    """a floor at y = -0.9 seen straight down from two heights, as the analytic depth / alpha maps such views have (a plane square to the
    view axis has one depth), fused into a 32^3 TsdfVolume; SdfGrid.from_tsdf of it; tsdf and weight read back for the reference.  The
    stiff torus dropped from rest agrees with the reference within the bounds above (the reference's own PCG figures for this case:
    test_dynamics_field_ref_host.py), and its lowest row ends within one voxel of the floor (a zero crossing is located no better than
    a cell; it lies |g| / kc deep besides)."""
    from gaussianmesh_amd.dynamics import MeshDynamics, SdfGrid
    from gaussianmesh_amd.proxy_mesh import TsdfVolume
    voxel, lo = fc.FUSED_VOXEL, np.asarray(fc.FUSED_LO)
    vol = TsdfVolume(lo, lo + fc.FUSED_N * voxel, voxel_size=voxel)
    assert (vol.nx, vol.ny, vol.nz) == (32, 32, 32)
    cams, depth, alpha = fc.fused_floor_views()
    vol.integrate(cams, _dev(depth), _dev(alpha))
    grid = SdfGrid.from_tsdf(vol)
    tsdf, weight = vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy()
    ref_grid = sg.prepare(tsdf, vol.voxel, weight, 1.0, vol.trunc)
    assert np.array_equal(grid.grid.cpu().numpy().view(np.uint32), ref_grid.view(np.uint32))
    assert (weight == 2).sum() > 32 * 32 * 4 and (weight == 0).sum() > 32 * 32 * 4       # the band both views saw, and what lies behind the floor
    c = dc.case("free_torus")
    k, g, d = 50.0, dc.GRAVITY, 0.2
    m = MeshDynamics(c["V0"], c["faces"], mass=c["mass"], stiffness=k, gravity=g, damping=d, dt=fc.DT, iterations=fc.ITERATIONS, contact_stiffness=fc.KC,
                     field=grid, field_friction=0.3, **TIGHT)
    X, contact = m.run(fc.STEPS, want_contacts=True)
    r = fc.fused_floor_reference(tsdf, weight, vol.origin, vol.voxel, vol.trunc, (k, g, d), 0.3)
    wX, wv, _ = r.run(c["V0"], np.zeros_like(c["V0"]), fc.STEPS)
    ex = float(np.abs(X.cpu().numpy().astype(np.float64) - wX).max())
    ev = float(np.abs(m.velocities.cpu().numpy().astype(np.float64) - wv).max())
    compare = ~((np.abs(r.phi_star) < fc.NEAR) | r.fringe)
    lowest = float(X[-1][:, 1].min())
    print("fused floor: positions %.3g, velocities %.3g, %d contacts, lowest row %.4f (floor %.1f, voxel %.2f)" % (ex, ev, int((contact > 0).sum()), lowest, fc.GROUND, voxel))
    assert ex <= 1e-6 and ev <= 1e-6 / fc.DT and np.array_equal(contact.cpu().numpy()[compare], r.contact[compare])
    assert int((contact[-1] == 1).sum()) >= 8 and abs(lowest - fc.GROUND) <= voxel


# ---- 6. refusals ----
def test_python_refusals_launch_nothing(grids):
    from gaussianmesh_amd.dynamics import MeshDynamics
    c = fc.case("sheet25")
    g = grids("sheet25")
    for kw in (dict(field="grid"), dict(field=g.grid), dict(field=g, field_friction=-1.0), dict(field=g, field_friction=float("nan")),
               dict(field=g, device="cpu")):
        with pytest.raises(ValueError):
            MeshDynamics(c["V0"], c["faces"], **kw)
    m = _dyn("sheet25", SOFT, g)
    before = (m.positions, m.velocities)
    out = torch.full((2, 25, 3), 5.0, device="cuda")
    for call in (lambda: m.run(0, out=out), lambda: m.run(2, collider_rows=np.zeros((2, 1, 4), np.float32), out=out), lambda: g.sample(torch.zeros((4, 2))),
                 lambda: g.sample(torch.zeros((4,)))):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and same_bits(before, (m.positions, m.velocities))


def test_c_refusals_launch_nothing(grids):
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    g = grids("field_pusher")
    m = _dyn("field_pusher", SOFT, g)
    T = 2
    x, v = m.positions, m.velocities
    rows = m._rows[None].expand(T, 1, 4).contiguous()
    out = torch.full((T, 96, 3), 5.0, device="cuda")
    vout = torch.full((96, 3), 6.0, device="cuda")
    stats = torch.full((T, 6), -3.0, dtype=torch.float64, device="cuda")
    con = torch.full((T, 96), 9, dtype=torch.int32, device="cuda")
    ws = torch.empty((l.gm_mesh_dynamics_contact_workspace_bytes(96),), dtype=torch.uint8, device="cuda")
    q = lambda p: p.data_ptr() if torch.is_tensor(p) else p

    def call(T=T, n=(g.nx, g.ny, g.nz), origin=g._origin_c, voxel=g.voxel, mu=0.3, nbytes=None, **kw):
        a = dict(K=1, kinds=m._kinds, rows=rows, mus=m._mus, grid=g.grid, contact=con, out=out, vout=vout, stats=stats, ws=ws, x=x, v=v)
        a.update(kw)
        gr = m.gravity
        return l.gm_mesh_dynamics_field(T, 96, q(m._off), q(m._cols), q(m._w), q(m.rest), q(m._mass), q(m._held), 0, None, None, q(a["x"]), q(a["v"]), m.dt,
                                        m.stiffness, m.damping, gr[0], gr[1], gr[2], m.iterations, 16, 1e-6, a["K"], q(a["kinds"]), q(a["rows"]), q(a["mus"]),
                                        fc.KC, n[0], n[1], n[2], origin, voxel, q(a["grid"]), mu, q(a["out"]), q(a["vout"]), q(a["contact"]), q(a["stats"]),
                                        q(a["ws"]), a["ws"].numel() if nbytes is None else nbytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    nan = float("nan")
    for kw, rc in ((dict(n=(1, g.ny, g.nz)), 1), (dict(n=(g.nx, g.ny, 1 << 30)), 1), (dict(voxel=0.0), 1), (dict(voxel=nan), 1), (dict(origin=None), 1),
                   (dict(origin=(ctypes.c_float * 3)(0.0, nan, 0.0)), 1), (dict(grid=None), 1), (dict(mu=-0.5), 1), (dict(mu=nan), 1), (dict(K=17), 1),
                   (dict(T=65), 1), (dict(out=g.grid), 1), (dict(contact=g.grid), 1), (dict(ws=g.grid), 1), (dict(stats=g.grid), 1), (dict(vout=g.grid), 1),
                   (dict(grid=out), 1), (dict(nbytes=l.gm_mesh_dynamics_contact_workspace_bytes(96) - 1), 3),
                   (dict(nbytes=l.gm_mesh_dynamics_workspace_bytes(96)), 3), (dict(K=0, kinds=None, rows=None, mus=None, nbytes=0), 3)):
        assert call(**kw) == rc and b"gm_mesh_dynamics_field" in l.gm_last_error(), (kw, l.gm_last_error())
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((vout == 6.0).all()) and bool((stats == -3.0).all()) and bool((con == 9).all())
    assert call() == 0                                                 # and the same call, unrefused, writes all four
    torch.cuda.synchronize()
    n = _dyn("field_pusher", SOFT, g, cg_iterations=16, cg_tolerance=1e-6, field_friction=0.3)
    want = n.run(T, want_contacts=True, want_stats=True)
    assert same_bits((out, con, stats), want) and same_bits(vout, n.velocities)
    assert call(contact=None, stats=None) == 0                         # both optional
    assert call(K=0, kinds=None, rows=None, mus=None) == 0             # and K may be 0
    torch.cuda.synchronize()
    k0 = _dyn("field_pusher", SOFT, g, colliders=(), cg_iterations=16, cg_tolerance=1e-6, field_friction=0.3)
    assert same_bits((out, con), k0.run(T, want_contacts=True)) and int(con.max()) <= 1


# ---- 7. the edit surface ----
def _background(d, height):
    """a background cloud for the 64-pixel scene: a slab of flat opaque Gaussians at y = height, written as a plain Gaussian PLY"""
    from gaussianmesh_amd import io as gio
    i, j = np.meshgrid(np.arange(48), np.arange(48), indexing="ij")
    xyz = np.stack([(i - 23.5) * 0.25, np.full(i.shape, height), (j - 23.5) * 0.25], -1).reshape(-1, 3).astype(np.float32)
    N = len(xyz)
    rot = np.zeros((N, 4), np.float32)
    rot[:, 0] = 1.0
    scaling = np.log(np.tile(np.array([0.2, 0.02, 0.2], np.float32), (N, 1)))
    path = os.path.join(d, "bg.ply")
    gio.save_plain_gaussians(path, dict(xyz=xyz, features_dc=np.full((N, 1, 3), 0.5, np.float32), features_rest=np.zeros((N, 15, 3), np.float32),
                                        opacity=np.full((N, 1), 6.0, np.float32), scaling=scaling, rotation=rot))
    return path


def test_simulate_with_a_field_is_run_and_reuses_the_operator(tmp_path):
    from gaussianmesh_amd import io as gio
    from gaussianmesh_amd.dynamics import MeshDynamics, SdfGrid
    from gaussianmesh_amd.edittool import SceneVisualTool
    d = str(tmp_path)
    _scene64(d)
    verts = np.asarray(gio.read_obj(os.path.join(d, "rest.obj"))[0])
    low = float(verts[:, 1].min())
    tool = SceneVisualTool(_background(d, low - 0.3))
    tool.add_gaussian(os.path.join(d, "object.ply"), os.path.join(d, "rest.obj"), "Object")
    o = tool.gaussians_list[0]
    dims, voxel = (24, 16, 24), 0.3
    origin = (-3.71, low - 0.05 - 4.13 * voxel, -3.67)
    grid = SdfGrid(fc.plane_values(dims, origin, voxel, (0.0, 1.0, 0.0), low - 0.05), origin, voxel)
    got = o.simulate(6, gravity=dc.GRAVITY, field=grid, field_friction=0.3)
    m = MeshDynamics(o.vertex, o.faces, gravity=dc.GRAVITY, field=grid, field_friction=0.3)
    want, contact = m.run(6, want_contacts=True)
    assert same_bits(got, want) and torch.equal(o.mesh_vertex_current, want[-1]) and bool((contact[-1] == 1).any())
    kept = o._operators["dynamics"]
    again = tool.simulate_one_gaussian("Object", 2, gravity=list(dc.GRAVITY), field=grid, field_friction=0.3)
    assert o._operators["dynamics"] is kept and same_bits(again, m.run(2))
    other = SdfGrid(fc.plane_values(dims, origin, voxel, (0.0, 1.0, 0.0), low - 0.05), origin, voxel)      # an equal grid, another object
    o.simulate(1, gravity=dc.GRAVITY, field=other, field_friction=0.3)
    assert o._operators["dynamics"] is not kept and o._operators["dynamics"].field is other
    # the background cloud itself: fused from the scene's cameras, the slab is found where it is
    cams = tool.get_camera(d)
    field = tool.background_field(cams, resolution=32, margin=0.5)
    assert isinstance(field, SdfGrid) and max(field.nx, field.ny, field.nz) == 32 and tool.background_volume.views == len(cams)
    known = ~torch.isnan(field.grid[..., 0])
    assert int(known.sum()) > 100 and int((known & (field.grid[..., 0] < 0)).sum()) > 10 and int((known & (field.grid[..., 0] > 0)).sum()) > 10
    with pytest.raises(ValueError):
        SceneVisualTool(os.path.join(d, "bg.ply")).background_field(cams)


def test_cli_background_contact_writes_its_frames(tmp_path):
    """--dynamics --background_gaussian BG --background_contact 32 --friction --contact_stiffness, with and without --floor, writes the
    frames of the handle sequence"""
    from gaussianmesh_amd import io as gio
    d = str(tmp_path)
    _scene64(d)
    verts, faces = gio.read_obj(os.path.join(d, "rest.obj"))
    ids, pos = _drags(verts)
    np.savez(os.path.join(d, "handles.npz"), handles=ids, positions=pos)
    bg = _background(d, float(verts[:, 1].min()) - 0.2)
    out = os.path.join(d, "sim")
    _cli(d, out, "--dynamics", "--settle", "2", "--gravity", "0", "-9.8", "0", "--background_gaussian", bg, "--background_contact", "32", "--contact_margin",
         "0.4", "--friction", "0.4", "--contact_stiffness", "20000")
    T = len(pos) + 2
    assert sorted(os.listdir(out)) == ["%05d.%s" % (k, e) for k in range(T) for e in ("obj", "png")]
    for k in range(T):
        v, f = gio.read_obj(os.path.join(out, "%05d.obj" % k))
        assert np.array_equal(f, faces) and np.isfinite(v).all()
    both = os.path.join(d, "both")
    _cli(d, both, "--dynamics", "--gravity", "0", "-9.8", "0", "--background_gaussian", bg, "--background_contact", "--floor", repr(float(verts[:, 1].min()) - 0.5))
    assert sorted(os.listdir(both)) == ["%05d.%s" % (k, e) for k in range(len(pos)) for e in ("obj", "png")]
