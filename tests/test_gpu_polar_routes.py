"""-m gpu: arap_rotation (csrc/gm_arap_shared.h) per row on every route of its eigen-route polar decomposition, through its three callers:
the pose energy and gradient (arap.ArapEnergy: arap_pose_local_kernel, arap_energy_grad_kernel), the local step of the three solvers
(arap.ArapSolver: arap_local_kernel), and the face keys of pose_interp.PoseInterpolator (pi_polar); and the row loops of the two pose
kernels at every ring size around ARAP_POSE_BATCH = 8.  Mesh, classes and bars: tests/polar_route_cases.py.

WHAT IS HELD TO WHAT.  Against arap_energy_ref / arap_ref.Reference, whose rotations come from an SVD:
  gradient  |g - g_ref| <= 1e-9 max(1, max|g_ref|) per element (the bar of test_gpu_arap_energy.py) on every row whose own class and
            all of whose neighbours' classes are `well` or `identity`; every other row finite.  0 exactly on a translated component.
  energy    E_dev - E_ref = 2 sum_i deficit_i, so  -64 eps sum_i s0_i <= E_dev - E_ref <= 2 sum_i bar_i  with bar_i by class:
            64 eps s0 (well), 8 sqrt(eps) s0 (window, gap0), 0 (identity).
On window rows R_i is NOT compared: it differs from the SVD's rotation by a turn about the strongest direction (O(1) for s1 / s0 below
1e-8) that costs the energy at most 2 bar_i.  The float64 restatement of the device's arithmetic against the SVD
(test_polar_routes_host.py, 994 rows): worst |Q^T Q - I| 2.2e-15 and |det Q - 1| 2.4e-15; worst deficit / s0 1.5e-15 on well rows
(bar 1.4e-14), 1.6e-9 on window rows (bar 1.2e-7, at s1 / s0 = 6.3e-9), below 0 on gap0 rows; worst |Q - R_svd| 3.6e-14 on well rows
(at gap 0.02) and 0.9 on window rows.
What a real fault costs: a transposed rotation, a lost flip or two mis-sorted columns lose O(gap s0) >= 1e-2 s0 on a well row, 1e12
well bars; an edge added twice or dropped at a ring size moves a gradient row by O(1).
Each test prints its worst ratio to its bar (NOTEBOOK.md "Polar routes").
THE UNMOVED SHORTCUT.  A row whose pose edges equal its rest edges takes R_i = I itself.  Where a whole component is translated that
is observable exactly (g = 0, and the energy of the translated components alone is 0); for an unmoved row next to moved rows ("one_moved":
four such rows) R_i = I against I + O(1e-16) moves g by 1e-16 and is only observable through the reference's bar, which holds those rows
with R_i = I.
POSE INTERPOLATOR.  The face matrices D(V) D(V0)^-1 carry the deformed face's UNIT normal, so a needle key gives faces with singular
values (1, 1, tiny): `well`; a line or point key gives rank <= 1: identity.  The branch of the rotation logarithm below 1e-6 rad
moves a vertex by less than 1e-6 of an edge, which float32 vertices do not show: it is not tested here.  Near a half turn the definition
leaves the side open: pairs with a face at 3.1 rad or more are held to finiteness only (none of the present keys reaches it).
A "line" key is not reproduced at its end of the interval BY DEFINITION: its faces have rank 1, R = I, and the stretch keeps only the
symmetric part of the (unsymmetric) face matrix; the reference misses it by 0.5, and the device is held to the reference there."""
import functools

import numpy as np
import pytest
import torch

import arap_energy_ref as er
import arap_ref
import poison
import polar_route_cases as pc
import pose_interp_ref

pytestmark = pytest.mark.gpu

TIGHT = dict(cg_iterations=400, cg_tolerance=1e-12)


def _dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


@functools.lru_cache(maxsize=None)
def energy_of(which):
    """(mesh, ArapEnergy, E_ref, g_ref); shared, do not modify"""
    from gaussianmesh_amd.arap import ArapEnergy
    m = pc.mesh(which)
    E_ref, g_ref = er.value_and_grad(m.ref, m.V1.astype(np.float64))
    return m, ArapEnergy(m.V0, m.faces, device="cuda:0"), E_ref, g_ref


def energy_window(m):
    """(lowest, highest) E_dev - E_ref the classes of the mesh allow"""
    t = m.table
    return -64 * pc.EPS * float(t["s"][:, 0].sum()), 2.0 * float(t["bar"].sum())


def check_energy_value(m, E, E_ref, label):
    lo, hi = energy_window(m)
    diff = E - E_ref
    print("%s: E %.6g, E - E_ref = %.3g in [%.3g, %.3g]: ratio to its bar %.3g" % (label, E_ref, diff, lo, hi, diff / hi if diff > 0 else diff / lo))
    assert np.isfinite(E) and lo <= diff <= hi, label


def check_energy(which, rows=None):
    """value_and_grad on the mesh against the reference; returns (E, g).  rows: the rows whose ok flag must be set (their comparison may
    not be lost to a neighbour's class)"""
    m, energy, E_ref, g_ref = energy_of(which)
    t = m.table
    E, g = energy.value_and_grad(_dev(m.V1))
    E, g = float(E.cpu()), g.cpu().numpy()
    assert g.shape == g_ref.shape and np.isfinite(g).all()
    ok = t["ok"]
    if rows is not None:
        assert ok[rows].all()
    g_bar = 1e-9 * max(1.0, float(np.abs(g_ref[ok]).max()) if ok.any() else 0.0)
    g_err = float(np.abs(g - g_ref)[ok].max()) if ok.any() else 0.0
    loose = float(np.abs(g - g_ref)[~ok].max()) if (~ok).any() else 0.0
    print("%s (Vm %d, %d rows compared): max|g_ref| %.3g, |g - ref| / bar = %.3g (on the %d other rows |g - ref| up to %.3g)" % (
        which, m.Vm, ok.sum(), np.abs(g_ref).max(), g_err / g_bar, (~ok).sum(), loose))
    assert g_err <= g_bar, which
    check_energy_value(m, E, E_ref, str(which))
    still = np.concatenate([m.rows_of(c) for c in m.comps if c["map"] in ("rest", "translation")] + [np.nonzero(m.comp == -1)[0]])
    assert not g[still.astype(np.int64)].any()                          # translated components and unreferenced vertices: 0 exactly
    return E, g


# ---- a. the pose energy and its gradient ----
@pytest.mark.parametrize("which", pc.GROUPS)
def test_energy_and_gradient_on_every_route(which):
    """the whole table, its `well` and its `window` components apart (a needle's loose energy bar cannot hide a well row), and at 256
    and 257 rows with a window fan ending at / lying across the edge between two workgroups"""
    m = pc.mesh(which)
    rows = None
    if which == "well":
        rows = np.arange(m.Vm)
    check_energy(which, rows)
    if which == "all":
        moved = [c for c in m.comps if c["map"] == "one_moved"][0]
        assert m.table["ok"][m.rows_of(moved)].all()                    # the unmoved rows next to moved ones are compared


def test_translated_components_alone_have_no_energy_at_all():
    from gaussianmesh_amd.arap import ArapEnergy
    m = pc.Mesh([s for s in pc.full_spec() if s[1] in ("rest", "translation")])
    assert m.Vm > 20 and not np.array_equal(m.V0, m.V1)
    E, g = ArapEnergy(m.V0, m.faces, device="cuda:0").value_and_grad(_dev(m.V1))
    assert float(E.cpu()) == 0.0 and not g.cpu().numpy().any()


@pytest.mark.parametrize("which", ("all", "p257"))
def test_same_bits_on_every_call_and_fill(which):
    m, energy, _, _ = energy_of(which)
    V1 = _dev(m.V1)
    route = lambda: energy.value_and_grad(V1)
    first = route()
    assert poison.same_bits(first, route())
    if which == "p257":
        runs = poison.run_under_fills(route)                            # a damaged band around E or grad raises GuardViolation
        assert all(p.handed_out == 2 for p, _ in runs)
        assert poison.differing(runs) == [] and poison.same_bits(runs[0][1], first)


# ---- c. ring sizes ----
@pytest.mark.parametrize("n", pc.RING_SIZES)
def test_the_apex_row_at_every_ring_size(n):
    """each fan alone, its apex row of n edges, with a generic, a reflected and a window pose: both pose kernels read ARAP_POSE_BATCH = 8
    edges at a time and re-read the last edge past the row's end; an edge added twice or dropped moves g and E by O(1)"""
    for name in pc.RING_MAPS:
        m = pc.mesh(("fan%d" % n, name))
        assert m.table["valence"][0] == n
        check_energy(("fan%d" % n, name), rows=None if name == pc.needle(20) else np.array([0]))


# ---- b. the local step of the three solvers ----
@functools.lru_cache(maxsize=None)
def solver_of(which, held):
    from gaussianmesh_amd.arap import ArapSolver
    m = pc.mesh(which)
    return ArapSolver(m.V0, m.faces, np.arange(m.Vm) if held == "all" else m.handles())


def local_energies(which):
    """E after arap_local_kernel with every vertex held at the route pose: {variant: E}"""
    m, s = pc.mesh(which), solver_of(which, "all")
    out = {}
    for step in ("column", "grid"):
        V, stats = s.solve(_dev(m.V1), outer_iterations=1, cg_iterations=1, want_stats=True, global_step=step)
        assert torch.equal(V.cpu(), torch.tensor(m.V1))                 # nothing is free: nothing moves
        out[step] = float(stats[0, 0].cpu())
        assert float(stats[0, 1].cpu()) == out[step]
        poses = _dev(np.stack([m.V0, m.V1, (1.5 * m.V1.astype(np.float64)).astype(np.float32)], 0))
        Vb, sb = s.solve_batch(poses, outer_iterations=1, cg_iterations=1, want_stats=True, global_step=step)
        assert sb.shape == (3, 1, 8) and torch.equal(Vb, poses)
        out["batch, " + step] = float(sb[1, 0, 0].cpu())
        assert float(sb[0, 0, 0].cpu()) <= 64 * pc.EPS * float(m.table["s"][:, 0].sum())      # item 0 is the rest pose
    return out


def test_local_step_energy_on_the_well_rows():
    """E after the local step, all vertices held, equals ArapEnergy's E within 1e-12 relative on the well components, in all variants"""
    m, energy, E_ref, _ = energy_of("well")
    E_pose = float(energy.value_and_grad(_dev(m.V1), want_grad=False)[0].cpu())
    assert E_pose > 1.0
    for variant, E in local_energies("well").items():
        print("well, %s: E_local %.15g, E_pose %.15g, relative difference / 1e-12 = %.3g" % (variant, E, E_pose, abs(E - E_pose) / E_pose / 1e-12))
        assert abs(E - E_pose) <= 1e-12 * E_pose, variant
        check_energy_value(m, E, E_ref, "well, " + variant)


def test_local_step_energy_on_every_route():
    m, _, E_ref, _ = energy_of("all")
    for variant, E in local_energies("all").items():
        check_energy_value(m, E, E_ref, "all, " + variant)


def free_solves(which):
    """one outer iteration from the route pose with two vertices of every component held: {variant: (V float64, stats [8])}"""
    m, s = pc.mesh(which), solver_of(which, "two")
    h = m.handles()
    out = {}
    for step in ("column", "grid"):
        V, stats = s.solve(_dev(m.V1[h]), init=_dev(m.V1), outer_iterations=1, want_stats=True, global_step=step, **TIGHT)
        out[step] = (V.cpu().numpy().astype(np.float64), stats[0].cpu().numpy())
        poses = np.stack([m.V0, m.V1, (1.5 * m.V1.astype(np.float64)).astype(np.float32)], 0)
        Vb, sb = s.solve_batch(_dev(poses[:, h]), init=_dev(poses), outer_iterations=1, want_stats=True, global_step=step, **TIGHT)
        assert torch.equal(Vb[1], V) and torch.equal(sb[1, 0], stats[0])        # an item's bits do not depend on its batch
        out["batch, " + step] = (Vb[1].cpu().numpy().astype(np.float64), sb[1, 0].cpu().numpy())
    return out


def test_one_iteration_with_free_rows_on_the_well_rows():
    """max |V_hip - V_ref| <= 1e-6, the bar of test_gpu_arap.py::test_against_the_reference: pose coordinates are below 4 (the pose carries
    no offset), so the float32 rounding of the output is at most 2.4e-7, and PCG to 1e-12 stays within 1e-9 of the exact global step"""
    m = pc.mesh("well")
    ref = arap_ref.Reference(m.V0, m.faces, m.handles())
    want, want_stats = ref.solve(m.V1, 1)
    assert ref.free.sum() > m.Vm // 2
    for variant, (V, stats) in free_solves("well").items():
        err = float(np.abs(V - want[0]).max())
        print("well, %s: max |V_hip - V_ref| / 1e-6 = %.3g; CG steps at most %d, residual at most %.3g" % (variant, err / 1e-6, stats[2:5].max(), stats[5:8].max()))
        assert err <= 1e-6, variant
        assert np.array_equal(V[m.handles()], m.V1[m.handles()].astype(np.float64))
        assert stats[1] <= stats[0] * (1 + 1e-12)
        assert abs(stats[0] - want_stats[0, 0]) <= 1e-9 * want_stats[0, 0] and abs(stats[1] - want_stats[0, 1]) <= 1e-6 * want_stats[0, 1]


def test_one_iteration_with_free_rows_on_every_route():
    """the global step behind rotations that are only energy-optimal: finite positions, and it does not raise the energy"""
    m, _, E_ref, _ = energy_of("all")
    for variant, (V, stats) in free_solves("all").items():
        print("all, %s: E local %.15g -> global %.15g; CG steps at most %d, residual at most %.3g" % (variant, stats[0], stats[1], stats[2:5].max(), stats[5:8].max()))
        assert np.isfinite(V).all() and np.isfinite(stats).all()
        assert stats[1] <= stats[0] * (1 + 1e-12), variant
        check_energy_value(m, stats[0], E_ref, "all, free rows, " + variant)


# ---- d. the pose interpolator's face keys ----
@functools.lru_cache(maxsize=None)
def interp_of(mode):
    from gaussianmesh_amd.pose_interp import PoseInterpolator
    m = pc.interp_key("rest")
    anchors = None if mode == "centroid" else pc.interp_anchors()
    return PoseInterpolator(m.V0, m.faces, anchors=anchors), pose_interp_ref.Reference(m.V0, m.faces, anchors)


@pytest.mark.parametrize("mode", ("centroid", "anchors"))
def test_pose_interpolator_between_degenerate_keys(mode):
    """every ordered pair of the keys rest, needle k = 10, needle k = 30, line, point and a generic map on two tetrahedra and two fans,
    at t in {0, 1/4, 1/2, 1}: max |V_hip - V_ref| <= 1e-6 (the bar of test_gpu_pose_interp.py: coordinates below 4) where every face's
    rotation between the keys stays below 3.1 rad, finite output elsewhere; t = 0 and t = 1 give the keys wherever the definition does"""
    p, ref = interp_of(mode)
    worst, compared = 0.0, 0
    for a, b in pc.INTERP_PAIRS:
        A, B = pc.interp_key(a).V1, pc.interp_key(b).V1
        V, stats = p.between(_dev(A), _dev(B), pc.INTERP_TS, want_stats=True, cg_iterations=2000, cg_tolerance=1e-10)
        V, stats = V.cpu().numpy().astype(np.float64), stats.cpu().numpy()
        assert V.shape == (len(pc.INTERP_TS), len(A), 3) and np.isfinite(V).all() and not np.isnan(stats).any(), (a, b)
        if not float(ref.relative_angles(A, B).max()) < 3.1:
            continue
        want = ref.between(A, B, pc.INTERP_TS)
        err = float(np.abs(V - want).max())
        worst, compared = max(worst, err), compared + 1
        assert err <= 1e-6, (a, b, err)
        for key, name, k in ((A, a, 0), (B, b, -1)):
            if name == "line":                                          # by definition not reproduced: see the module's docstring
                assert float(np.abs(want[k] - key).max()) > 0.1
            else:
                assert float(np.abs(V[k] - key).max()) <= 1e-6, (a, b, name)
    print("pose interpolator, %s: %d of %d pairs compared, worst |V_hip - V_ref| / 1e-6 = %.3g" % (mode, compared, len(pc.INTERP_PAIRS), worst / 1e-6))
    assert compared >= 20
