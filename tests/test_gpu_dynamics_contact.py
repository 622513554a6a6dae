"""-m gpu: gm_mesh_dynamics_contact (dynamics.MeshDynamics(colliders=...)) against the float64 reference of tests/dynamics_contact_ref.py on
the cases and materials of tests/dynamics_contact_cases.py: positions, velocities and the active set; its batches and repeatability on
poisoned memory; K == 0 against gm_mesh_dynamics; closed forms; what contact leaves alone; refusals; and the edit surface on top of it
(SingleObjectDeform.simulate, edit_sequence --dynamics --floor)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import dynamics_cases as dc
import dynamics_contact_cases as cc
import dynamics_contact_ref as cr
from poison import differing, run_under_fills, same_bits
from test_gpu_arap import _drags, _scene64, _tool
from test_gpu_dynamics import _cli

pytestmark = pytest.mark.gpu
TIGHT = dict(cg_iterations=cc.TIGHT[0], cg_tolerance=cc.TIGHT[1])
SOFT, STIFF = cc.MATERIALS
UNIT = abs(dc.GRAVITY[1]) / cc.KC                                      # the rest depth |g| / kc


def _dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


def _colliders(ref_colliders):
    """the reference's (kind, row, friction) as MeshDynamics takes them"""
    return [("sphere" if k == cr.SPHERE else "half_space", tuple(float(x) for x in row), mu) for k, row, mu in ref_colliders]


def _dyn(name, material, colliders=None, pinned=None, **kw):
    """a fresh MeshDynamics of the case at its starting state, with the reference's own masses and the case's colliders"""
    from gaussianmesh_amd.dynamics import MeshDynamics
    c = cc.case(name)
    k, g, d = dc.MATERIALS[material] if isinstance(material, int) else material
    opts = dict(TIGHT, mass=c["mass"], stiffness=k, gravity=g, damping=d, dt=cc.DT, iterations=cc.ITERATIONS, contact_stiffness=cc.KC,
                colliders=_colliders(c["colliders"] if colliders is None else colliders))
    opts.update(kw)
    m = MeshDynamics(c["V0"], c["faces"], pinned=c["pinned"] if pinned is None else pinned, handles=c["handles"], **opts)
    m.reset(velocities=_dev(c["v0"]))
    return m


def _inputs(name, steps=cc.STEPS):
    """(handle targets, collider rows) of the case on the device, None where it has none; beyond its 16 steps the handles stay"""
    c = cc.case(name)
    t, r = c["targets"], c["collider_rows"]
    idx = np.arange(steps)
    if t is not None:
        t = _dev(t[np.minimum(idx, len(t) - 1)])
    if r is not None:
        r = _dev(r[:steps])
    return t, r


# ---- 1. against the reference ----
@pytest.mark.parametrize("name, material", cc.ALL, ids=["%s-%d" % c for c in cc.ALL])
def test_against_the_reference(name, material):
    """16 steps at (400, 1e-10): max |X_out - X_ref| <= 1e-6 and max |v_out - v_ref| <= 1e-6 / dt, section AA's bounds: on the CPU the
    reference's PCG against its exact solves gave E_x <= 2.4e-7 and E_v <= 3.8e-6 on these cases, at or below a quarter of them
    (test_dynamics_contact_ref_host.py asserts it).  contact_out equals the reference's active set on every row but those within 1e-5 of a
    surface or of a second collider there (at most 0.07 % of rows x steps; the CPU test caps them at 2 %)."""
    want_x, want_v, want_c, compare = cc.reference_run(name, material)
    m = _dyn(name, material)
    t, r = _inputs(name)
    X, contact, stats = m.run(cc.STEPS, t, collider_rows=r, want_contacts=True, want_stats=True)
    X, v, stats = X.cpu().numpy().astype(np.float64), m.velocities.cpu().numpy().astype(np.float64), stats.cpu().numpy()
    contact = contact.cpu().numpy()
    assert X.shape == want_x.shape and v.shape == want_v.shape and stats.shape == (cc.STEPS, 6) and contact.shape == want_c.shape
    ex, ev = float(np.abs(X - want_x).max()), float(np.abs(v - want_v).max())
    wrong = int((contact != want_c)[compare].sum())
    print("%s material %d: max |X_hip - X_ref| %.3g, max |v_hip - v_ref| %.3g, CG steps at most %d, residual at most %.3g, %d rows x steps in "
          "contact, %d compared rows differ, %d of the rows left out differ"
          % (name, material, ex, ev, int(stats[:, :3].max()), stats[:, 3:].max(), int((contact > 0).sum()), wrong, int((contact != want_c)[~compare].sum())))
    assert np.isfinite(X).all() and np.isfinite(v).all()
    assert ex <= 1e-6 and ev <= 1e-6 / cc.DT
    assert wrong == 0 and contact.dtype == np.int32
    assert (stats[:, 3:] <= 1e-10).all() and (stats[:, :3] <= 400).all() and (stats[:, :3] == np.round(stats[:, :3])).all()
    assert same_bits(m.positions, _dev(X[-1]))


# ---- 2. batches ----
@pytest.mark.parametrize("name, material", [("pusher", STIFF), ("corner", SOFT), ("drag", STIFF)])
def test_a_run_is_its_steps_one_by_one(name, material):
    """run(16) equals sixteen step() calls bit for bit - positions, velocities, contacts and stats - with a collider that moves"""
    t, r = _inputs(name)
    a, b, c = _dyn(name, material), _dyn(name, material), _dyn(name, material)
    X, contact, stats = a.run(cc.STEPS, t, collider_rows=r, want_contacts=True, want_stats=True)
    single = torch.stack([b.step(None if t is None else t[k], None if r is None else r[k]) for k in range(cc.STEPS)], 0)
    assert same_bits(X, single) and same_bits(a.velocities, b.velocities) and same_bits(a.positions, b.positions)
    ones = [c.run(1, None if t is None else t[k:k + 1], collider_rows=None if r is None else r[k:k + 1], want_contacts=True, want_stats=True)
            for k in range(cc.STEPS)]
    assert same_bits(contact, torch.cat([o[1] for o in ones], 0)) and same_bits(stats, torch.cat([o[2] for o in ones], 0))
    assert bool((contact > 0).any()) and not same_bits(X[7], X[8])


def test_a_run_across_a_chunk_boundary_with_a_moving_collider():
    """67 steps of the torus under weak gravity on a ball that bobs under its tube (the reference has it in contact from step 56 to the
    end): one run, 67 single steps, and two runs of other lengths give the same bits, contacts included"""
    from gaussianmesh_amd import _lib
    n = _lib.GM_MESH_DYNAMICS_STEPS_MAX + 3
    rows = np.tile(cc.case("pusher")["collider_rows"][:1], (n, 1, 1))
    rows[:, 0, 1] = (-1.3 + 0.2 * np.sin(2.0 * np.pi * np.arange(n) / 16.0)).astype(np.float32)
    r = _dev(rows)
    weak = (50.0, (0.0, -2.0, 0.0), 0.02)
    a, b, c = (_dyn("pusher", weak) for _ in range(3))
    for m in (a, b, c):
        m.reset()                                                      # from rest
    X, contact = a.run(n, collider_rows=r, want_contacts=True)
    single = torch.stack([b.step(collider_rows=r[k]) for k in range(n)], 0)
    assert X.shape == (n, 96, 3) and same_bits(X, single) and same_bits(a.velocities, b.velocities)
    first = c.run(5, collider_rows=r[:5], want_contacts=True)          # and in two calls of other lengths
    second = c.run(n - 5, collider_rows=r[5:], want_contacts=True)
    assert same_bits(torch.cat([first[0], second[0]], 0), X) and same_bits(torch.cat([first[1], second[1]], 0), contact)
    assert bool((contact[60:64] > 0).any()) and bool((contact[64:] > 0).any())            # in contact on both sides of the boundary
    d = _dyn("corner", SOFT)                                           # static colliders: their rows are repeated in every chunk
    e = _dyn("corner", SOFT)
    assert same_bits(d.run(n), torch.stack([e.step() for _ in range(n)], 0))


# ---- 3. repeatability ----
@pytest.mark.parametrize("name, material", [("sixteen", STIFF), ("pusher", SOFT), ("drag", SOFT), ("sheet1056", STIFF)])
def test_same_bits_from_call_to_call_and_on_poisoned_memory(name, material):
    """two runs give the same bits; so do runs whose every allocation (X_out, contact_out, the workspace of a fresh object) was filled
    with 0x00, 0xFF and 0x5A beforehand, and no guard band around any of them is touched"""
    t, r = _inputs(name)

    def route():
        m = _dyn(name, material)
        X, contact, stats = m.run(cc.STEPS, t, collider_rows=r, want_contacts=True, want_stats=True)
        return X, contact, stats, m.velocities, m.positions
    first = route()
    assert same_bits(first, route())
    runs = run_under_fills(route)
    assert all(p.handed_out >= 3 for p, _ in runs)
    assert differing(runs) == [] and same_bits(runs[0][1], first)


# ---- 4. no colliders, and colliders out of reach ----
def _c_call(l, entry, m, T, t, x, v, out, vout, stats, ws, K=None, kinds=None, rows=None, mus=None, kc=cc.KC, contact=None, nbytes=None, cg=16, tol=1e-6):
    """gm_mesh_dynamics (K is None) or gm_mesh_dynamics_contact through ctypes on m's device arrays"""
    q = lambda p: p.data_ptr() if torch.is_tensor(p) else p
    g = m.gravity
    head = (T, m.Vm, q(m._off), q(m._cols), q(m._w), q(m.rest), q(m._mass), q(m._held), len(m.handles), q(m._handle_ids), q(t), q(x), q(v), m.dt,
            m.stiffness, m.damping, g[0], g[1], g[2], m.iterations, cg, tol)
    tail = (q(ws), ws.numel() if nbytes is None else nbytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if K is None:
        return l.gm_mesh_dynamics(*head, q(out), q(vout), q(stats), *tail)
    return getattr(l, entry)(*head, K, q(kinds), q(rows), q(mus), kc, q(out), q(vout), q(contact), q(stats), *tail)


@pytest.mark.parametrize("name", ["drag", "drop_smooth"])
def test_no_colliders_through_the_contact_entry_is_gm_mesh_dynamics(name):
    """K == 0: the launches of gm_mesh_dynamics, so its bits - X_out, v_out, stats - and contact_out all 0; MeshDynamics without
    colliders does not even take this entry"""
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    m = _dyn(name, STIFF, colliders=())
    assert m.K == 0
    T = 5
    t, _ = _inputs(name, T)
    x, v = m.positions, m.velocities
    ws = torch.empty((l.gm_mesh_dynamics_contact_workspace_bytes(m.Vm),), dtype=torch.uint8, device="cuda")
    assert ws.numel() > l.gm_mesh_dynamics_workspace_bytes(m.Vm) > 0 and l.gm_mesh_dynamics_contact_workspace_bytes(0) == 0
    got = [torch.full((T, m.Vm, 3), 5.0, device="cuda"), torch.full((m.Vm, 3), 6.0, device="cuda"), torch.full((T, 6), -3.0, dtype=torch.float64, device="cuda")]
    want = [torch.full_like(a, 7.0) for a in got]
    contact = torch.full((T, m.Vm), 9, dtype=torch.int32, device="cuda")
    assert _c_call(l, "gm_mesh_dynamics_contact", m, T, t, x, v, got[0], got[1], got[2], ws, K=0, contact=contact) == 0
    assert _c_call(l, None, m, T, t, x, v, want[0], want[1], want[2], ws) == 0
    torch.cuda.synchronize()
    assert same_bits(got, want) and bool((contact == 0).all())
    _, c2 = m.run(T, t, want_contacts=True)                            # and the class, which goes through gm_mesh_dynamics
    assert m._ws.numel() == l.gm_mesh_dynamics_workspace_bytes(m.Vm) and bool((c2 == 0).all()) and c2.dtype == torch.int32


@pytest.mark.parametrize("material", cc.MATERIALS)
def test_colliders_nothing_reaches(material):
    """free_torus with a floor, a wall and a ball far away: within the bounds of the first test of the reference WITHOUT colliders, no
    contact reported; and, printed, whether the result is bit for bit the run without colliders (it was: with kappa = 0 the diagonal,
    the shift and the right-hand side are the same numbers, and both global kernels are one source)"""
    far = (cr.floor(-50.0, friction=0.5), cr.half_space((1.0, 0.0, 0.0), offset=-40.0), cr.sphere((30.0, 0.0, 0.0), 2.0))
    want_x, want_v = dc.reference_run("free_torus", material)
    m, plain = _dyn("drop_smooth", material, colliders=far), _dyn("drop_smooth", material, colliders=())
    X, contact = m.run(cc.STEPS, want_contacts=True)
    P = plain.run(cc.STEPS)
    ex = float(np.abs(X.cpu().numpy().astype(np.float64) - want_x).max())
    ev = float(np.abs(m.velocities.cpu().numpy().astype(np.float64) - want_v).max())
    print("out of reach, material %d: positions %.3g, velocities %.3g; bit-equal to the run without colliders: %s"
          % (material, ex, ev, same_bits(X, P) and same_bits(m.velocities, plain.velocities)))
    assert ex <= 1e-6 and ev <= 1e-6 / cc.DT and not bool(contact.any())


# ---- 5. closed forms ----
def _sheet_run(material, friction, v0, steps, height, **kw):
    from gaussianmesh_amd.dynamics import MeshDynamics, floor
    V0, faces = cc.sheet(5, 5, height=height)
    k, g, d = material
    m = MeshDynamics(V0, faces, stiffness=k, gravity=g, damping=d, dt=cc.DT, iterations=cc.ITERATIONS, colliders=[floor(0.0, friction=friction)],
                     contact_stiffness=cc.KC, **dict(TIGHT, **kw))
    m.reset(velocities=_dev(np.tile(np.asarray(v0, np.float32), (len(V0), 1))))
    X, contact = m.run(steps, want_contacts=True)
    return X.cpu().numpy().astype(np.float64), contact.cpu().numpy(), V0.astype(np.float64)


@pytest.mark.parametrize("damping", [0.0, 0.02])
def test_a_flat_sheet_follows_the_scalar_recursion(damping):
    """a flat sheet dropped flat onto a frictionless floor: every vertex's height follows Y <- (Y + h v + h^2 a) / (1 + kc h^2) below the
    floor and the free prediction above it, to 1e-7 (the reference's own bound in test_dynamics_contact_ref_host.py), nothing moves
    sideways, and contact_out is all or nothing in every step"""
    X, contact, V0 = _sheet_run((10.0, dc.GRAVITY, damping), 0.0, (0.0, -0.5, 0.0), 24, 0.1)
    want = cc.sheet_recursion(0.1, -0.5, 24, damping=damping)
    err = float(np.abs(X[:, :, 1] - want[:, None]).max())
    print("sheet recursion, damping %g: %.3g" % (damping, err))
    assert err <= 1e-7 and float(np.abs(X[:, :, [0, 2]] - V0[None][:, :, [0, 2]]).max()) <= 1e-7
    assert ((contact == 0).all(1) | (contact == 1).all(1)).all() and (contact[0] == 0).all() and (contact == 1).any()


def test_a_damped_sheet_comes_to_rest_at_a_over_kc():
    X, contact, _ = _sheet_run((10.0, dc.GRAVITY, 0.2), 0.0, (0.0, 0.0, 0.0), 200, 0.01)
    assert float(np.abs(X[-1, :, 1] - dc.GRAVITY[1] / cc.KC).max()) <= 1e-7 and float(np.abs(X[-1] - X[-2]).max()) <= 1e-8
    assert (contact[-1] == 1).all()


def test_without_friction_a_tangential_velocity_is_untouched():
    """at the resting depth with friction 0 and a uniform tangential velocity u, x and z advance by h u a step within 1e-6 n (the free
    body's bound) while the floor holds the height; with friction 0.5 the same sheet is held back"""
    u = np.array([0.3, 0.0, 0.5], np.float32)
    X, contact, V0 = _sheet_run((10.0, dc.GRAVITY, 0.0), 0.0, u, 8, dc.GRAVITY[1] / cc.KC, cg_iterations=64, cg_tolerance=1e-6)
    n = np.arange(1, 9)[:, None, None]
    want = V0[None][:, :, [0, 2]] + n * cc.DT * u.astype(np.float64)[[0, 2]]
    err = float((np.abs(X[:, :, [0, 2]] - want) / n).max())
    print("friction 0: tangential error per step %.3g" % err)
    assert err <= 1e-6 and float(np.abs(X[:, :, 1] - dc.GRAVITY[1] / cc.KC).max()) <= 1e-6 and (contact == 1).all()
    R, _, _ = _sheet_run((10.0, dc.GRAVITY, 0.0), 0.5, u, 8, dc.GRAVITY[1] / cc.KC)
    assert float(np.abs(R[-1][:, [0, 2]] - V0[:, [0, 2]]).max()) < 0.5 * float(np.abs(X[-1][:, [0, 2]] - V0[:, [0, 2]]).max())


# ---- 6. other properties ----
def test_a_settled_body_rests_within_a_few_rest_depths():
    """the stiff torus set down 0.01 above the rough floor, damping 0.2, 60 steps: no vertex is ever deeper than 10 |g| / kc below the
    floor.  The torus stands on a quarter of its vertices, which carry the rest: the reference run of this case has its deepest vertex
    8.5 |g| / kc down at the worst step and 7.9 at the last, hence 10."""
    c = cc.case("drop_rough")
    x0 = c["V0"].copy()
    x0[:, 1] -= 0.19
    m = _dyn("drop_rough", (50.0, dc.GRAVITY, 0.2))
    m.reset(positions=_dev(x0))
    X, contact = m.run(60, want_contacts=True)
    depth = (-0.9 - X[:, :, 1].min(dim=1).values.cpu().numpy().astype(np.float64)) / UNIT
    print("settled torus: deepest vertex %.3g |g| / kc at the worst step, %.3g at the last; max |v| %.3g" % (depth.max(), depth[-1], float(m.velocities.abs().max())))
    assert depth.max() <= 10.0 and 1.0 <= depth[-1] <= 10.0
    assert int((contact[-1] > 0).sum()) >= 12 and float(m.velocities.abs().max()) < 0.05


def test_handle_and_held_rows_are_untouched_by_contact():
    """drag, with three more rows pinned, from a start pushed below the floor: handle rows of X_out[t] are handle_targets[t] bit for bit,
    pinned rows stay where they were, and contact_out is 0 in all of them although they lie below the floor while free rows beside
    them are in contact"""
    c = cc.case("drag")
    pins = np.setdiff1d(np.arange(96), c["handles"])[[2, 30, 31]]
    x_in = c["V0"].copy()
    x_in[:, 1] -= 0.3                                                  # the ring's lower half starts inside the floor at -0.75
    m = _dyn("drag", STIFF, pinned=pins)
    m.reset(positions=_dev(x_in), velocities=_dev(c["v0"]))
    t, _ = _inputs("drag")
    t = t.clone()
    t[:, :, 1] -= 0.3
    X, contact = m.run(cc.STEPS, t, want_contacts=True)
    held = np.concatenate([pins, c["handles"]])
    assert same_bits(X[:, _dev(c["handles"], torch.int64)], t)
    assert np.array_equal(X.cpu().numpy()[:, pins], np.broadcast_to(x_in[pins], (cc.STEPS, 3, 3)))
    contact = contact.cpu().numpy()
    assert not contact[:, held].any() and (contact > 0).sum() > 100
    below = X.cpu().numpy()[:, :, 1] < -0.75 - 1e-3
    assert below[:, held].any() and bool((m.velocities[_dev(pins, torch.int64)] == 0).all())


def test_ties_go_to_the_lowest_index_and_an_unknown_kind_is_never_chosen():
    """two identical floors: every contact is reported as collider 1, never 2, and the meshes are the single floor's bit for bit; through
    the C entry a collider of kind 7 in front changes nothing but the indices"""
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    one = _dyn("drop_rough", SOFT)
    two = _dyn("drop_rough", SOFT, colliders=cc.case("drop_rough")["colliders"] * 2)
    X1, c1 = one.run(cc.STEPS, want_contacts=True)
    X2, c2 = two.run(cc.STEPS, want_contacts=True)
    assert same_bits(X1, X2) and same_bits(c1, c2) and int(c1.max()) == 1
    m = _dyn("drop_rough", SOFT)
    kinds, rows = _dev([7, 0], torch.int32), torch.cat([m._rows, m._rows], 0)[None].expand(cc.STEPS, 2, 4).contiguous()
    mus = _dev([0.0, 0.5], torch.float64)
    out, vout, con = torch.empty_like(X1), torch.empty((96, 3), device="cuda"), torch.empty((cc.STEPS, 96), dtype=torch.int32, device="cuda")
    ws = torch.empty((l.gm_mesh_dynamics_contact_workspace_bytes(96),), dtype=torch.uint8, device="cuda")
    assert _c_call(l, "gm_mesh_dynamics_contact", m, cc.STEPS, None, m.positions, m.velocities, out, vout, None, ws, K=2, kinds=kinds, rows=rows, mus=mus,
                   contact=con, cg=cc.TIGHT[0], tol=cc.TIGHT[1]) == 0
    torch.cuda.synchronize()
    assert same_bits(out, X1) and same_bits(con, c1 * 2) and same_bits(vout, one.velocities)


# ---- 7. refusals ----
def test_python_refusals_launch_nothing():
    from gaussianmesh_amd.dynamics import MeshDynamics, floor, half_space, sphere
    c = cc.case("corner")
    for make in (lambda: half_space((0.0, 0.0, 0.0)), lambda: half_space((0.0, float("nan"), 1.0)), lambda: half_space((0.0, float("inf"), 1.0)),
                 lambda: sphere((0.0, 0.0, 0.0), 0.0), lambda: sphere((0.0, 0.0, 0.0), -1.0), lambda: sphere((0.0, 0.0, 0.0), float("nan")),
                 lambda: floor(friction=-0.1), lambda: sphere((0.0, 0.0, 0.0), 1.0, friction=float("nan")), lambda: half_space((0, 1, 0), offset=1.0, point=(0, 0, 0))):
        with pytest.raises(ValueError):
            make()
    build = lambda **kw: MeshDynamics(c["V0"], c["faces"], **kw)
    for kw in (dict(colliders=[floor()] * 17), dict(colliders=[floor()], contact_stiffness=0.0), dict(colliders=[floor()], contact_stiffness=float("nan")),
               dict(colliders=[floor()], contact_stiffness=float("inf")), dict(colliders=[("half_space", (0.0, 0.0, 0.0, 1.0), 0.0)]),
               dict(colliders=[("sphere", (0.0, 0.0, 0.0, 0.0), 0.0)]), dict(colliders=[("sphere", (0.0, 0.0, 0.0, 1.0), -1.0)]),
               dict(colliders=[("cone", (0.0, 0.0, 0.0, 1.0), 0.0)]), dict(colliders=[dict(kind="sphere", center=[0, 0, 0], radius=-2.0)]),
               dict(colliders=floor())):
        with pytest.raises(ValueError):
            build(**kw)
    assert build(colliders=[floor()] * 16).K == 16 and build(colliders=[["sphere", [0, 0, 0, 1], 0.5], dict(kind="half_space", normal=[0, 2, 0], point=[0, -1, 0])]).K == 2
    m = _dyn("corner", SOFT)
    before = (m.positions, m.velocities)
    out = torch.full((2, 96, 3), 5.0, device="cuda")
    rows = np.tile(m.collider_rows, (2, 1, 1))
    nan, long, flat = rows.copy(), rows.copy(), rows.copy()
    nan[1, 0, 3], long[0, 1, 0], flat[1, 0, :3] = np.nan, 1.5, 0.0
    for call in (lambda: m.run(2, collider_rows=rows[:1], out=out), lambda: m.run(2, collider_rows=rows[:, :1], out=out), lambda: m.run(2, collider_rows=nan, out=out),
                 lambda: m.run(2, collider_rows=long, out=out), lambda: m.run(2, collider_rows=flat, out=out), lambda: m.step(collider_rows=rows),
                 lambda: _dyn("corner", SOFT, colliders=()).run(2, collider_rows=rows, out=out)):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and same_bits(before, (m.positions, m.velocities))


def test_c_refusals_launch_nothing():
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    m = _dyn("corner", SOFT)
    T = 2
    x, v = m.positions, m.velocities
    rows = m._rows[None].expand(T, 2, 4).contiguous()
    out = torch.full((T, 96, 3), 5.0, device="cuda")
    vout = torch.full((96, 3), 6.0, device="cuda")
    stats = torch.full((T, 6), -3.0, dtype=torch.float64, device="cuda")
    con = torch.full((T, 96), 9, dtype=torch.int32, device="cuda")
    ws = torch.empty((l.gm_mesh_dynamics_contact_workspace_bytes(96),), dtype=torch.uint8, device="cuda")

    def call(T=T, **kw):
        a = dict(K=2, kinds=m._kinds, rows=rows, mus=m._mus, contact=con, out=out, vout=vout, stats=stats, ws=ws, x=x, v=v)
        a.update(kw)
        x_, v_, out_, vout_, stats_, ws_ = (a.pop(n) for n in ("x", "v", "out", "vout", "stats", "ws"))
        return _c_call(l, "gm_mesh_dynamics_contact", m, T, None, x_, v_, out_, vout_, stats_, ws_, **a)
    for kw, rc in ((dict(K=17), 1), (dict(K=-1), 1), (dict(kc=0.0), 1), (dict(kc=-1.0), 1), (dict(kc=float("nan")), 1), (dict(kc=float("inf")), 1),
                   (dict(kinds=None), 1), (dict(rows=None), 1), (dict(mus=None), 1), (dict(T=0), 1), (dict(T=65), 1), (dict(x=None), 1), (dict(out=None), 1),
                   (dict(contact=out), 1), (dict(contact=x), 1), (dict(contact=stats), 1), (dict(contact=ws), 1), (dict(out=rows), 1), (dict(ws=m._kinds), 1),
                   (dict(stats=m._mus), 1), (dict(contact=rows), 1), (dict(vout=x), 1),
                   (dict(nbytes=l.gm_mesh_dynamics_contact_workspace_bytes(96) - 1), 3), (dict(nbytes=l.gm_mesh_dynamics_workspace_bytes(96)), 3), (dict(nbytes=0), 3),
                   (dict(K=0, nbytes=l.gm_mesh_dynamics_workspace_bytes(96)), 3)):
        assert call(**kw) == rc and b"gm_mesh_dynamics_contact" in l.gm_last_error(), (kw, l.gm_last_error())
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((vout == 6.0).all()) and bool((stats == -3.0).all()) and bool((con == 9).all())
    assert call() == 0                                                 # and the same call, unrefused, writes all four
    torch.cuda.synchronize()
    n = _dyn("corner", SOFT, cg_iterations=16, cg_tolerance=1e-6)
    want = n.run(T, want_contacts=True, want_stats=True)
    assert same_bits((out, con, stats), want) and same_bits(vout, n.velocities)
    assert call(contact=None, stats=None) == 0                         # both optional


# ---- 8. the edit surface ----
def test_simulate_with_colliders_is_run_and_reuses_the_operator(tmp_path):
    from gaussianmesh_amd.dynamics import MeshDynamics, floor, sphere
    d = str(tmp_path)
    _scene64(d)
    tool = _tool(d)
    o = tool.gaussians_list[0]
    low = float(o.vertex[:, 1].min())
    ground = floor(low - 0.05, friction=0.3)
    got = o.simulate(6, gravity=dc.GRAVITY, colliders=[ground])
    m = MeshDynamics(o.vertex, o.faces, gravity=dc.GRAVITY, colliders=[ground])
    want, contact = m.run(6, want_contacts=True)
    assert same_bits(got, want) and torch.equal(o.mesh_vertex_current, want[-1]) and bool((contact[-1] > 0).any())
    kept = o._operators["dynamics"]
    again = o.simulate(2, gravity=list(dc.GRAVITY), colliders=[[ground[0], list(ground[1]), ground[2]]])          # equal options, as lists
    assert o._operators["dynamics"] is kept and same_bits(again, m.run(2))
    assert float(again[-1][:, 1].min()) > low - 0.05 - 20 * UNIT       # it stands on the floor
    ball = sphere((0.0, low - 2.0, 0.0), 0.5)
    rows = np.tile(MeshDynamics(o.vertex, o.faces, colliders=[ground, ball]).collider_rows, (3, 1, 1))
    rows[:, 1, 1] += np.arange(3, dtype=np.float32)
    moved = tool.simulate_one_gaussian("Object", 3, gravity=dc.GRAVITY, colliders=[ground, ball], collider_rows=rows)
    assert o._operators["dynamics"] is not kept and moved.shape == (3, o.vertex.shape[0], 3) and bool(torch.isfinite(moved).all())
    free = o.simulate(2, gravity=dc.GRAVITY, keep_velocity=False)      # and without colliders the old route, from the same state
    m2 = MeshDynamics(o.vertex, o.faces, gravity=dc.GRAVITY)
    m2.reset(positions=moved[-1])
    assert same_bits(free, m2.run(2)) and o._operators["dynamics"].K == 0


def test_cli_floor_writes_its_frames(tmp_path):
    """--dynamics --floor H --friction MU --contact_stiffness KC writes the meshes MeshDynamics gives with that half-space opposite to
    gravity; --colliders with a moving ball runs; (that the command line without the new flags gives the bytes it always gave is
    test_gpu_dynamics.py's test_cli_dynamics_writes_the_frames_and_the_default_is_unchanged, which stays as it is)"""
    from gaussianmesh_amd import io as gio
    from gaussianmesh_amd.dynamics import MeshDynamics, half_space
    d = str(tmp_path)
    _scene64(d)
    verts, faces = gio.read_obj(os.path.join(d, "rest.obj"))
    ids, pos = _drags(verts)
    np.savez(os.path.join(d, "handles.npz"), handles=ids, positions=pos)
    H = float(verts[:, 1].min()) - 0.02
    sim = os.path.join(d, "sim")
    _cli(d, sim, "--dynamics", "--settle", "3", "--gravity", "0", "-9.8", "0", "--floor", repr(H), "--friction", "0.4", "--contact_stiffness", "20000")
    T = len(pos) + 3
    assert sorted(os.listdir(sim)) == ["%05d.%s" % (k, e) for k in range(T) for e in ("obj", "png")]
    targets = np.concatenate([pos, np.broadcast_to(pos[-1], (3,) + pos.shape[1:])], 0)
    m = MeshDynamics(verts.astype(np.float32), faces, handles=ids, gravity=dc.GRAVITY, contact_stiffness=20000.0,
                     colliders=[half_space((0.0, 9.8, 0.0), offset=H, friction=0.4)])
    want, contact = m.run(T, _dev(targets), want_contacts=True)
    assert bool((contact > 0).any())
    for k in range(T):
        v, f = gio.read_obj(os.path.join(sim, "%05d.obj" % k))
        assert np.array_equal(f, faces) and np.array_equal(v, want[k].cpu().numpy().astype(np.float64)), k
    with open(os.path.join(d, "colliders.json"), "w") as fh:
        json.dump([{"kind": "sphere", "radius": 0.4, "centers": [[0.0, H - 1.0 + 0.5 * k, 0.0] for k in range(3)]},
                   {"kind": "half_space", "normal": [0, 1, 0], "offset": H, "friction": 0.2}], fh)
    ball = os.path.join(d, "ball")
    _cli(d, ball, "--dynamics", "--gravity", "0", "-9.8", "0", "--colliders", os.path.join(d, "colliders.json"))
    assert sorted(os.listdir(ball)) == ["%05d.%s" % (k, e) for k in range(len(pos)) for e in ("obj", "png")]
