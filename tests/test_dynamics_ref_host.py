"""Host side of the mesh dynamics (gm_mesh_dynamics, dynamics.MeshDynamics, edit_sequence --dynamics): the float64 reference of
tests/dynamics_ref.py is established before the device is held to it - its PCG variant against its exact global step, the stationarity
of an exact step, the free-body and settle properties - then vertex_masses, the constructors' refusals without a device, the declaration
and typing of the two entry points, the C refusals that need no device (made on pointers that are never dereferenced) and the CLI's flag
refusals."""
import os
import re

import numpy as np
import pytest

import arap_cases as ac
import dynamics_cases as dc
import dynamics_ref as dr
from gaussianmesh_amd import _lib, edit_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ("torus_a", "flat_patch", "fan", "pinned", "free_torus")
STIFFEST = dc.MATERIALS.index((50.0, dc.GRAVITY, 0.0))
# every material on the small meshes; the two meshes of 1073 vertices at the stiffest material with gravity, where PCG needs the most steps
PCG_CASES = [(n, m) for n in SMALL for m in range(len(dc.MATERIALS))] + [("torus_c", STIFFEST), ("one_handle", STIFFEST)]


def test_the_cases_are_the_ones_named():
    assert dc.STEPS == 16 and dc.RAMP == 8 and dc.ITERATIONS == 3 and dc.DT == 1.0 / 30.0
    assert sorted(set(k for k, _, _ in dc.MATERIALS)) == [1.0, 50.0] and sorted(set(d for _, _, d in dc.MATERIALS)) == [0.0, 0.02]
    assert set(g for _, g, _ in dc.MATERIALS) == {(0.0, 0.0, 0.0), (0.0, -9.8, 0.0)} and len(dc.MATERIALS) == 8
    assert [dc.case(n)["V0"].shape[0] for n in dc.NAMES] == [96, 1073, 108, 41, 1073, 98, 96]
    for n in ("torus_a", "torus_c", "flat_patch", "fan", "one_handle"):
        c, a = dc.case(n), ac.case(n)
        assert np.array_equal(c["targets"][7], a["targets"]) and np.array_equal(c["targets"][15], a["targets"])
        assert np.array_equal(c["targets"][3], (0.5 * a["V0"][a["handles"]].astype(np.float64) + 0.5 * a["targets"].astype(np.float64)).astype(np.float32))
    p = dc.reference("pinned", 0)
    assert p.ref.pinned.nonzero()[0].tolist() == [96, 97] and p.held[[96, 97]].all()
    f = dc.reference("free_torus", 0)
    assert not f.held.any() and float(np.abs(dc.case("free_torus")["v0"]).max()) > 1.0


@pytest.mark.parametrize("name, material", PCG_CASES, ids=["%s-%d" % c for c in PCG_CASES])
def test_reference_pcg_matches_the_exact_global_step(name, material):
    """16 steps with PCG at (400, 1e-10) against exact solves: positions within 1e-6 (the prototype measured at most 2.4e-7), the last
    velocities within 1e-6 / dt; the residuals reach the tolerance within the cap"""
    c = dc.case(name)
    want_x, want_v = dc.reference_run(name, material)
    X, v, stats = dc.reference(name, material).run(c["V0"], c["v0"], dc.STEPS, c["targets"], pcg=dc.TIGHT)
    ex, ev = float(np.abs(X.astype(np.float64) - want_x).max()), float(np.abs(v.astype(np.float64) - want_v).max())
    print("%s material %d: positions %.3g, velocities %.3g, CG steps at most %d" % (name, material, ex, ev, int(stats[:, :3].max())))
    assert float(np.abs(want_x).max()) < 4.0
    assert ex <= 1e-6 and ev <= 1e-6 / dc.DT
    assert (stats[:, 3:] <= 1e-10).all() and (stats[:, :3] <= 400).all()


@pytest.mark.parametrize("name", SMALL)
def test_an_exact_step_is_stationary_for_its_own_rotations(name):
    """the gradient of sum_i mass_i / (2 h^2) |X_i - y_i|^2 + (k / 2) E_arap(X, R) vanishes on the free rows at the exact global step's X
    for the R it was solved with - by the closed form, and by central differences of the objective itself (a quadratic: exact up to
    rounding)"""
    c = dc.case(name)
    for material in (0, STIFFEST):
        d = dc.reference(name, material)
        d.iterations = 1
        t = None if c["targets"] is None else c["targets"][4]
        X, y, R, _ = d.solve_step(c["V0"], c["v0"] + np.float32(0.1), t)
        g = d.objective_gradient(X, y, R)
        size = float(np.abs(2.0 * d.k * d.mu[:, None] * y).max()) + 2.0 * d.k * float(np.abs(d.ref.L).sum(axis=1).max()) * 4.0
        assert float(np.abs(g[d.free]).max()) <= 1e-12 * size
        if d.held.any() and name != "pinned":
            assert float(np.abs(g[d.handles]).max()) > 1e-6                            # the handles are not at rest: a force acts on them
        rng = np.random.default_rng(2)
        rows = rng.choice(np.nonzero(d.free)[0], 6, replace=False)
        for i in rows:
            for a in range(3):
                e = np.zeros_like(X)
                e[i, a] = 1e-3
                fd = (d.objective(X + e, y, R) - d.objective(X - e, y, R)) / 2e-3
                assert abs(fd - g[i, a]) <= 1e-9 * max(1.0, d.objective(X, y, R)) / 1e-3


def test_reference_free_body_moves_uniformly_and_falls_as_implicit_euler():
    """nothing held, damping 0, uniform velocity: every vertex is at x_0 + n h u (with gravity: on implicit Euler's parabola) within
    1e-6 n - the translated state solves every step exactly, so this is the mass term and the prediction alone"""
    def run(grav, v, n):
        d = dc.reference("free_torus", (10.0, grav, 0.0))
        return d.run(dc.case("free_torus")["V0"], v, n)[0]
    errs = dc.free_body_error(run)
    print("free body: error per step %.3g (no gravity), %.3g (gravity)" % tuple(errs))
    assert max(errs) <= 1e-6


@pytest.mark.parametrize("name", ["torus_a", "flat_patch"])
def test_reference_settles_to_the_quasi_static_solution(name):
    """handles at their targets from step 0, stiffness 50, damping 0.1, no gravity, 240 steps: within 1e-5 of the ARAP fixed point
    (arap_ref.Reference.solve(start, 400)'s last iterate; the prototype reached 1.6e-7 and 5.4e-8), max |v| below 1e-4"""
    c, a = dc.case(name), ac.case(name)
    static = ac.reference(name).solve(ac.start(a), 400)[0][-1]
    d = dc.reference(name, (50.0, (0.0, 0.0, 0.0), 0.1))
    X, v, _ = d.run(c["V0"], c["v0"], 240, np.broadcast_to(a["targets"], (240,) + a["targets"].shape))
    err, vmax = float(np.abs(X[-1].astype(np.float64) - static).max()), float(np.abs(v).max())
    print("%s: %.3g from the quasi-static solution, max |v| %.3g" % (name, err, vmax))
    assert err <= 1e-5 and vmax < 1e-4


def test_vertex_masses_sum_to_density_times_area():
    from gaussianmesh_amd.dynamics import vertex_masses
    for name in ("torus_a", "flat_patch", "fan", "pinned"):
        c = dc.case(name)
        V = c["V0"].astype(np.float64)
        f = c["faces"].astype(np.int64)
        area = 0.5 * np.linalg.norm(np.cross(V[f[:, 1]] - V[f[:, 0]], V[f[:, 2]] - V[f[:, 0]]), axis=1).sum()
        m = vertex_masses(c["V0"], c["faces"], density=2.5)
        assert m.dtype == np.float64 and m.shape == (len(V),) and abs(m.sum() - 2.5 * area) <= 1e-12 * area
        assert np.allclose(m, 2.5 * dr.vertex_masses(c["V0"], c["faces"]), rtol=1e-13, atol=0.0)
    assert abs(vertex_masses(dc.case("flat_patch")["V0"], dc.case("flat_patch")["faces"]).sum() - 4.0) <= 1e-6    # a 2 x 2 square
    m = vertex_masses(dc.case("pinned")["V0"], dc.case("pinned")["faces"])
    assert m[96] == 0.0 and m[97] == 0.0 and (m[:96] > 0).all()
    for kw in (dict(density=0.0), dict(density=float("nan")), dict(density=-1.0)):
        with pytest.raises(ValueError, match="density"):
            vertex_masses(c["V0"], c["faces"], **kw)
    with pytest.raises(ValueError, match="face index"):
        vertex_masses(c["V0"], c["faces"] + 1000)


def test_python_refusals_without_a_device():
    from gaussianmesh_amd.dynamics import MeshDynamics
    c = dc.case("pinned")
    V0, faces = c["V0"], c["faces"]
    d = MeshDynamics(V0, faces, pinned=[3], handles=[7, 9], device="cpu")
    assert d.Vm == 98 and sorted(np.nonzero(d.held)[0].tolist()) == [3, 7, 9, 96, 97] and d.handles.tolist() == [7, 9] and d.pinned.tolist() == [3]
    assert np.array_equal(d.mass, dr.vertex_masses(V0, faces)) or np.allclose(d.mass, dr.vertex_masses(V0, faces), rtol=1e-13)
    assert not MeshDynamics(V0[:96], faces[:-1], device="cpu").held.any()                # a free body is a valid input
    for bad in (V0[:, :2], V0[:0], V0.reshape(-1)):
        with pytest.raises(ValueError, match="rest_vertices"):
            MeshDynamics(bad, faces, device="cpu")
    with pytest.raises(ValueError, match="face index"):
        MeshDynamics(V0, faces + 100, device="cpu")
    for kw, what in ((dict(handles=[5, 5]), "twice"), (dict(handles=[98]), "outside"), (dict(pinned=[-1]), "outside"), (dict(handles=[0.5]), "integer"),
                     (dict(pinned=[4, 6], handles=[6]), "both a handle and pinned"), (dict(mass="volume"), "mass"), (dict(mass=np.ones(97)), "mass"),
                     (dict(mass=np.zeros(98)), "mass"), (dict(mass=-np.ones(98)), "mass"), (dict(mass=np.full(98, np.nan)), "mass"),
                     (dict(density=0.0), "density"), (dict(dt=0.0), "dt"), (dict(dt=float("inf")), "dt"), (dict(stiffness=-1.0), "stiffness"),
                     (dict(stiffness=float("nan")), "stiffness"), (dict(damping=1.0), "damping"), (dict(damping=-0.1), "damping"),
                     (dict(gravity=(0, 1)), "gravity"), (dict(gravity=(0, float("nan"), 0)), "gravity"), (dict(iterations=0), "iterations"),
                     (dict(iterations=2.5), "iterations"), (dict(cg_iterations=0), "cg_iterations"), (dict(cg_tolerance=-1e-3), "cg_tolerance"),
                     (dict(cg_tolerance=float("nan")), "cg_tolerance")):
        with pytest.raises(ValueError, match=what):
            MeshDynamics(V0, faces, device="cpu", **kw)
    ok = np.ones(98)
    ok[96:] = 0.0                                                      # zero mass where no edge is: those rows are never unknowns
    MeshDynamics(V0, faces, mass=ok, device="cpu")
    with pytest.raises(ValueError, match="both a handle and pinned"):
        d.set_constraints(pinned=[7], handles=[7])
    assert d.handles.tolist() == [7, 9]                                # a refused change changes nothing
    d.set_constraints()
    assert sorted(np.nonzero(d.held)[0].tolist()) == [96, 97] and len(d.handles) == 0
    # run's refusals come before the device is asked for
    for call, what in ((lambda: d.run(0), "steps"), (lambda: d.run(2.0), "steps"), (lambda: d.run(2, np.zeros((2, 1, 3))), "no handles")):
        with pytest.raises(ValueError, match=what):
            call()
    d.set_constraints(handles=[7, 9])
    for call, what in ((lambda: d.run(2), "handle_targets"), (lambda: d.run(2, np.zeros((3, 2, 3))), "handle_targets"),
                       (lambda: d.run(2, np.zeros((2, 3, 3))), "handle_targets"), (lambda: d.step(np.zeros((2, 2, 3))), "handle_targets"),
                       (lambda: d.reset(positions=np.zeros((5, 3))), "positions"), (lambda: d.reset(velocities=np.zeros((98, 2))), "velocities")):
        with pytest.raises(ValueError, match=what):
            call()
    for call in (lambda: d.run(2, np.zeros((2, 2, 3))), lambda: d.step(np.zeros((2, 3))), lambda: d.reset(), lambda: d.positions, lambda: d.velocities):
        with pytest.raises(_lib.GmeshError, match="no CPU path"):
            call()


@pytest.mark.parametrize("name, ret, n", [("gm_mesh_dynamics", "int", 28), ("gm_mesh_dynamics_workspace_bytes", "size_t", 1)])
def test_header_declares_and_lib_types_the_entry_points(name, ret, n):
    text = open(os.path.join(ROOT, "include", "gmesh_hip.h")).read()
    m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, name), text)
    assert m and len(m.group(1).split(",")) == n
    assert name in _lib.header_symbols()
    res, args = _lib.SIGNATURES[name]
    assert len(args) == n and hasattr(_lib.lib(), name)
    if n == 28:                                                        # the typing, argument by argument, against the prototype's own words
        want = []
        for a in m.group(1).split(","):
            a = re.sub(r"/\*.*?\*/", "", a).strip()
            want.append(_lib.vp if "*" in a else {"int": _lib.i32, "double": _lib.f64, "size_t": _lib.sz}[a.split()[0]])
        assert args == want and res is _lib.i32
    assert "#define GM_MESH_DYNAMICS_STEPS_MAX 64" in text and _lib.GM_MESH_DYNAMICS_STEPS_MAX == 64


def test_workspace_bytes():
    """0 for a Vm that would be refused; otherwise O(Vm) and monotonic: 32 doubles and an int per vertex"""
    l = _lib.lib()
    assert l.gm_mesh_dynamics_workspace_bytes(0) == 0 and l.gm_mesh_dynamics_workspace_bytes(-3) == 0
    got = [l.gm_mesh_dynamics_workspace_bytes(Vm) for Vm in (1, 2, 96, 1073, 7500, 100000)]
    assert got == sorted(got) and got[0] > 0
    for Vm, b in zip((96, 1073, 7500, 100000), got[2:]):
        assert 8 * 32 * Vm + 4 * Vm <= b <= 8 * 32 * Vm + 4 * Vm + 13 * 256


def test_mesh_dynamics_refuses_before_any_gpu_work():
    l = _lib.lib()
    Vm, T, H = 100, 4, 3
    a = 1 << 30                                                        # non-null "pointers", 4 MiB apart: never dereferenced
    names = ("off", "cols", "w", "V0", "mass", "held", "ids", "targets", "x", "v", "out", "vout", "stats", "ws")
    P = {k: a + (i << 22) for i, k in enumerate(names)}
    need = l.gm_mesh_dynamics_workspace_bytes(Vm)

    def call(T=T, Vm=Vm, H=H, dt=1 / 30, k=10.0, damp=0.02, g=(0.0, -9.8, 0.0), its=3, cg=8, tol=1e-6, nbytes=need, **kw):
        p = dict(P, **kw)
        return l.gm_mesh_dynamics(T, Vm, p["off"], p["cols"], p["w"], p["V0"], p["mass"], p["held"], H, p["ids"], p["targets"], p["x"], p["v"], dt, k, damp,
                                  g[0], g[1], g[2], its, cg, tol, p["out"], p["vout"], p["stats"], p["ws"], nbytes, None)

    def refused(what, rc=1, **kw):
        assert call(**kw) == rc and b"gm_mesh_dynamics" in l.gm_last_error() and what in l.gm_last_error(), (kw, l.gm_last_error())
    nan, inf = float("nan"), float("inf")
    for t in (0, -1, 65):
        refused(b"T =", T=t)
    for vm in (0, -5):
        refused(b"Vm", Vm=vm)
    for h in (-1, Vm + 1):
        refused(b"H =", H=h)
    for dt in (0.0, -0.1, nan, inf):
        refused(b"dt", dt=dt)
    for k in (0.0, -1.0, nan, inf):
        refused(b"stiffness", k=k)
    for damp in (-0.01, 1.0, 2.0, nan, inf):
        refused(b"damping", damp=damp)
    for g in ((nan, 0.0, 0.0), (0.0, inf, 0.0), (0.0, 0.0, -inf)):
        refused(b"gravity", g=g)
    refused(b"iterations", its=0)
    refused(b"cg_iterations", cg=0)
    for tol in (-1e-3, nan, inf):
        refused(b"cg_tolerance", tol=tol)
    refused(b"stiffness dt^2", dt=1e-200, k=1e-200)                                      # each in range, their product not
    for k in names:
        if k != "stats":
            refused(b"null", **{k: None})
    # what may be NULL: the handle arrays without handles, stats - these reach the workspace check
    refused(b"workspace", rc=3, H=0, ids=None, targets=None, nbytes=need - 1)
    refused(b"workspace", rc=3, stats=None, nbytes=need - 1)
    refused(b"workspace", rc=3, vout=P["v"], nbytes=need - 1)                            # v_out may be v_in
    refused(b"workspace", rc=3, x=P["V0"], nbytes=need - 1)                              # inputs may alias one another
    refused(b"workspace", rc=3, nbytes=0)
    outs = ("out", "vout", "stats", "ws")
    for i, x in enumerate(outs):
        for y in ("V0", "mass", "held", "ids", "targets", "x", "v") + outs[i + 1:]:
            if (x, y) != ("vout", "v"):
                refused(b"overlaps", **{x: P[y] + 4})
    refused(b"overlaps", vout=P["v"] + 4)                                                # v_out == v_in, or apart
    refused(b"overlaps", x=P["out"] + 12 * Vm * (T - 1) + 4)                             # x_in may not lie inside X_out, over its [T] extent
    refused(b"overlaps", out=P["v"] + 4, vout=P["v"])                                    # the in-place velocity still meets nothing else
    refused(b"overlaps", ws=P["stats"] + 48 * (T - 1) + 8)
    refused(b"overlaps", ws=P["targets"] + 12 * H * (T - 1) + 8)
    refused(b"workspace", rc=3, stats=P["out"] + 12 * Vm * T, nbytes=need - 1)


BASE = ["--object_gaussian", "o.ply", "--object_origin_mesh", "m.obj", "--camera_path", ".", "--render_path", "out"]


@pytest.mark.parametrize("extra, what", [
    (["--mesh_sequence", "dir", "--dynamics"], "--mesh_sequence"),
    (["--handle_sequence", "h.npz", "--dynamics", "--arap_batch", "2"], "--arap_batch"),
    (["--handle_sequence", "h.npz", "--dynamics", "--inbetweens", "1"], "--inbetweens"),
    (["--handle_sequence", "h.npz", "--settle", "3"], "--settle needs --dynamics"),
    (["--pick_sequence", "p.json", "--settle", "1"], "--settle needs --dynamics"),
    (["--handle_sequence", "h.npz", "--dynamics", "--settle", "-2"], "--settle -2"),
    (["--handle_sequence", "h.npz", "--stiffness", "20"], "--stiffness sets the simulated material and needs --dynamics"),
    (["--handle_sequence", "h.npz", "--gravity", "0", "-9.8", "0"], "--gravity sets the simulated material and needs --dynamics"),
])
def test_cli_flag_refusals_come_before_any_device_work(extra, what, monkeypatch):
    """SystemExit with a message, raised ahead of every import that would touch the device or read a file (none of the named files
    exists)"""
    import builtins
    real = builtins.__import__

    def no_torch(name, *a, **kw):
        assert name != "torch" and not name.endswith("edittool"), name
        return real(name, *a, **kw)
    monkeypatch.setattr(builtins, "__import__", no_torch)
    with pytest.raises(SystemExit) as e:
        edit_sequence.main(BASE + extra)
    assert what in str(e.value) and "edit_sequence:" in str(e.value)
