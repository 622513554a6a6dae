"""The float64 reference of mesh contact (tests/dynamics_contact_ref.py) against closed forms, against its parent where nothing is in
reach, its own PCG against its exact solves on every case of tests/dynamics_contact_cases.py, and the cap on the rows that the
active-set comparison of test_gpu_dynamics_contact.py leaves out.  No device."""
import numpy as np
import pytest

import dynamics_cases as dc
import dynamics_contact_cases as cc
import dynamics_contact_ref as cr
import dynamics_ref as dr


def _sheet(material, colliders, v0, steps, height=0.0, nu=5, nv=5, kc=cc.KC):
    """a flat nu x nv sheet at `height` with the uniform velocity v0 over `colliders`: (reference, positions [steps,Vm,3] float64, V0)"""
    V0, faces = cc.sheet(nu, nv, height=height)
    k, g, d = material
    r = cr.ContactDynamics(V0, faces, dr.vertex_masses(V0, faces), dt=cc.DT, stiffness=k, damping=d, gravity=g, iterations=cc.ITERATIONS,
                           colliders=colliders, contact_stiffness=kc)
    X, _, _ = r.run(V0, np.tile(np.asarray(v0, np.float32), (len(V0), 1)), steps)
    return r, X.astype(np.float64), V0.astype(np.float64)


@pytest.mark.parametrize("damping", [0.0, 0.02])
def test_a_flat_sheet_follows_the_scalar_recursion(damping):
    """dropped flat onto a frictionless floor the sheet translates rigidly (the elastic term vanishes), so every vertex's height follows
    Y <- (Y + h v + h^2 a) / (1 + kc h^2) below the floor and the free prediction above it: to 1e-7 (float32 rounding of heights below
    0.2 at the step boundaries is 1.5e-8; the recursion rounds the same way, so what is left is where a rounding falls differently)"""
    r, X, V0 = _sheet((10.0, dc.GRAVITY, damping), (cr.floor(0.0),), (0.0, -0.5, 0.0), 24, height=0.1)
    want = cc.sheet_recursion(0.1, -0.5, 24, damping=damping)
    assert float(np.abs(X[:, :, 1] - want[:, None]).max()) <= 1e-7
    assert float(np.abs(X[:, :, [0, 2]] - V0[None][:, :, [0, 2]]).max()) <= 1e-7           # and nothing moves sideways
    assert want.min() < 0.0 < want[0] and (r.contact.sum(1) > 0).any() and (r.contact[0] == 0).all()


def test_a_damped_sheet_comes_to_rest_at_a_over_kc():
    """damping 0.2, 200 steps: the height settles at gravity / kc = -9.8e-4 (to float32's rounding of the state), the fixed point of the
    recursion: Y kc h^2 = h^2 a"""
    _, X, _ = _sheet((10.0, dc.GRAVITY, 0.2), (cr.floor(0.0),), (0.0, 0.0, 0.0), 200, height=0.01)
    assert float(np.abs(X[-1, :, 1] - dc.GRAVITY[1] / cc.KC).max()) <= 1e-7
    assert float(np.abs(X[-1] - X[-2]).max()) <= 1e-8


def test_without_friction_a_tangential_velocity_is_untouched():
    """resting depth, friction 0, uniform tangential velocity u: x and z advance by h u every step, as a free body's (free_body_error's
    form), while the floor holds the height"""
    u = np.array([0.3, 0.0, 0.5], np.float32)
    _, X, V0 = _sheet((10.0, dc.GRAVITY, 0.0), (cr.floor(0.0),), u, 8, height=dc.GRAVITY[1] / cc.KC)
    n = np.arange(1, 9)[:, None, None]
    want = V0[None][:, :, [0, 2]] + n * cc.DT * u.astype(np.float64)[[0, 2]]
    assert float((np.abs(X[:, :, [0, 2]] - want) / n).max()) <= 1e-6
    assert float(np.abs(X[:, :, 1] - dc.GRAVITY[1] / cc.KC).max()) <= 1e-6


def test_an_incline_holds_above_the_friction_angle_and_slides_below_it():
    """a sheet lying on a plane tilted by 20 degrees (tan = 0.364), at its resting depth: with mu = 0.6 the anchor at the step's start
    holds it, and the tangential creep of a step stays below 2 |a_t| / kc (the anchor is the last step's position, so gravity's
    tangential part moves it by about |a_t| / kc a step); with mu = 0.2 it accelerates: every step is longer than the one before, and
    step n is n h^2 (|a_t| - mu |a_n|) long, Coulomb's law under implicit Euler, within 2 % (the cap is reached in every step)"""
    th = np.radians(20.0)
    n = np.array([np.sin(th), np.cos(th), 0.0])
    tdir = np.array([np.cos(th), -np.sin(th), 0.0])                    # downhill
    a_t = abs(float(np.asarray(dc.GRAVITY) @ tdir))
    V0, faces = cc.sheet(5, 5)
    Rm = np.array([tdir, n, [0.0, 0.0, 1.0]]).T                        # the sheet's plane y = 0 onto the incline, 9.8 cos / kc deep
    start = (V0.astype(np.float64) @ Rm.T + n * (dc.GRAVITY[1] * np.cos(th) / cc.KC)).astype(np.float32)
    steps = {}
    for mu in (0.6, 0.2):
        r = cr.ContactDynamics(V0, faces, dr.vertex_masses(V0, faces), dt=cc.DT, stiffness=10.0, damping=0.0, gravity=dc.GRAVITY,
                               iterations=cc.ITERATIONS, colliders=(cr.half_space(n, offset=0.0, friction=mu),), contact_stiffness=cc.KC)
        X, _, _ = r.run(start, np.zeros_like(start), 16)
        path = np.concatenate([start[None], X], 0).astype(np.float64)
        steps[mu] = np.abs((path[1:] - path[:-1]) @ tdir).max(axis=1)
        assert (r.contact > 0).all()
    assert steps[0.6].max() <= 2.0 * a_t / cc.KC
    a_n = abs(float(np.asarray(dc.GRAVITY) @ n))
    assert (np.diff(steps[0.2]) > 0.0).all()
    assert np.allclose(steps[0.2], np.arange(1, 17) * cc.DT ** 2 * (a_t - 0.2 * a_n), rtol=0.02, atol=0.0)


@pytest.mark.parametrize("material", cc.MATERIALS)
def test_with_no_collider_in_reach_the_run_is_the_parents(material):
    """free_torus with a floor, a wall and a ball it never meets in 16 steps: Dynamics.run's arrays exactly, and no contact reported"""
    c = dc.case("free_torus")
    far = (cr.floor(-50.0, friction=0.5), cr.half_space((1.0, 0.0, 0.0), offset=-40.0), cr.sphere((30.0, 0.0, 0.0), 2.0))
    r = cc.reference("drop_smooth", material, colliders=far)
    X, v, s = r.run(c["V0"], c["v0"], cc.STEPS)
    wx, wv, ws = dc.reference("free_torus", material).run(c["V0"], c["v0"], cc.STEPS)
    assert np.array_equal(X, wx) and np.array_equal(v, wv) and np.array_equal(s, ws)
    assert not r.contact.any() and np.isfinite(r.phi_star).all() and float(r.phi_star.min()) > 10.0
    none = cc.reference("drop_smooth", material, colliders=())
    assert np.array_equal(none.run(c["V0"], c["v0"], cc.STEPS)[0], wx)


def test_the_smallest_phi_wins_ties_go_to_the_lowest_index_and_nan_is_never_chosen():
    r = cc.reference("corner", cc.MATERIALS[0], colliders=(cr.floor(-0.5), cr.floor(-0.5), cr.floor(-0.4),
                                                           (cr.HALF_SPACE, np.array([np.nan, 1.0, 0.0, 0.0], np.float32), 0.0), (7, np.zeros(4, np.float32), 0.0)))
    X = dc.case("free_torus")["V0"].astype(np.float64)
    kappa, c, which, best, gap = r.contact_terms(X, X, r.rows)
    below = X[:, 1] < -0.4
    assert below.any() and (~below).any()
    assert (which[below] == 3).all() and (which[~below] == 0).all()    # the highest floor has the smallest phi
    assert np.array_equal(best, X[:, 1] + np.float64(np.float32(0.4)))
    assert np.allclose(c[below][:, 1], np.float64(np.float32(-0.4))) and np.array_equal(c[below][:, [0, 2]], X[below][:, [0, 2]])
    r2 = cc.reference("corner", cc.MATERIALS[0], colliders=(cr.floor(-0.5), cr.floor(-0.5)))
    which2 = r2.contact_terms(X, X, r2.rows)[2]
    assert set(np.unique(which2)) == {0, 1}                            # the tie: never 2
    assert np.array_equal(kappa[below], r.mu[below] * (cc.KC * cc.DT * cc.DT))


@pytest.mark.parametrize("name, material", cc.ALL, ids=["%s-%d" % c for c in cc.ALL])
def test_pcg_against_exact_and_the_rows_left_out(name, material):
    """the reference's PCG at TIGHT against its exact solves: E_x and E_v, the largest position and velocity differences, lie at or below
    a quarter of section AA's bounds (1e-6 and 1e-6 / dt), so those bounds are the device's too; measured: E_x at most 2.4e-7 (one
    float32 rounding of a coordinate between 2 and 4 that falls the other way), E_v at most 3.8e-6.  And the rows that the device's
    active-set comparison leaves out (|phi*| or the gap to the second collider below 1e-5) are at most 2 % of rows x steps; measured: at
    most 0.07 %."""
    X, v, contact, compare = cc.reference_run(name, material)
    Xp, vp = cc.reference_run_pcg(name, material)
    ex, ev = float(np.abs(X.astype(np.float64) - Xp).max()), float(np.abs(v.astype(np.float64) - vp).max())
    left = 1.0 - float(compare.mean())
    print("%s material %d: E_x %.3g, E_v %.3g, left out %.3g %%, active rows x steps %d" % (name, material, ex, ev, 100.0 * left, int((contact > 0).sum())))
    assert ex <= 0.25e-6 and ev <= 0.25e-6 / cc.DT
    assert left <= 0.02
    assert (contact > 0).sum() >= 16 and np.isfinite(X).all()
    c = cc.case(name)
    assert contact.shape == (cc.STEPS, len(c["V0"])) and not contact[:, c["handles"]].any()
    assert int(contact.max()) <= len(c["colliders"])


def test_the_cases_exercise_what_they_are_for():
    """corner and sixteen reach both the floor and the wall, sixteen only through colliders 6 and 12 of its 16; the pusher moves; the big
    sheet has more than 1024 rows; drag's handles are never in contact although they go below its floor"""
    assert set(np.unique(cc.reference_run("corner", cc.MATERIALS[0])[2])) == {0, 1, 2}
    assert set(np.unique(cc.reference_run("sixteen", cc.MATERIALS[0])[2])) == {0, 6, 12}
    assert np.array_equal(cc.reference_run("sixteen", cc.MATERIALS[1])[0], cc.reference_run("corner", cc.MATERIALS[1])[0])
    rows = cc.case("pusher")["collider_rows"]
    assert rows.shape == (cc.STEPS, 1, 4) and rows[-1, 0, 1] - rows[0, 0, 1] > 2.5
    assert len(cc.case("sheet1056")["V0"]) == 1056 and len(cc.case("sheet5")["V0"]) == 25
    d = cc.case("drag")
    assert float(d["targets"][-1][:, 1].min()) < -1.0 and not cc.reference_run("drag", cc.MATERIALS[0])[2][:, d["handles"]].any()
