"""Shared cases of the mesh-dynamics tests (test_dynamics_ref_host.py, test_gpu_dynamics.py): the ARAP test meshes of arap_cases with
their handles ramped from rest to their targets over 8 steps and held for 8, the mesh with rows whose weights sum to 0, a torus with no
held row at all; the materials; and the float64 reference (dynamics_ref.Dynamics) run once per (case, material) and shared."""
import functools

import numpy as np

import arap_cases as ac
import dynamics_ref as dr

STEPS, RAMP = 16, 8
DT, ITERATIONS = 1.0 / 30.0, 3
GRAVITY = (0.0, -9.8, 0.0)
NAMES = ("torus_a", "torus_c", "flat_patch", "fan", "one_handle", "pinned", "free_torus")
# (stiffness, gravity, damping)
MATERIALS = tuple((k, g, d) for k in (1.0, 50.0) for g in ((0.0, 0.0, 0.0), GRAVITY) for d in (0.0, 0.02))
ALL = tuple((n, m) for n in NAMES for m in range(len(MATERIALS)))
TIGHT = (400, 1e-10)            # cg_iterations, cg_tolerance of the comparison with the reference


def ramp(rest_rows, targets, steps=STEPS, over=RAMP):
    """handle targets [steps,H,3] float32: from rest to `targets` in `over` equal parts, then held"""
    a, b = np.asarray(rest_rows, np.float32).astype(np.float64), np.asarray(targets, np.float32).astype(np.float64)
    s = np.minimum(np.arange(1, steps + 1) / float(over), 1.0)[:, None, None]
    return ((1.0 - s) * a + s * b).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(V0 float32 [Vm,3], faces int32 [F,3], handles int64 [H], targets float32 [STEPS,H,3] or None, pinned int64 [P], v0 float32 [Vm,3])"""
    if name == "pinned":                                               # vertices 96 and 97 have d_i = 0; the torus moves as torus_a does
        V0, faces = ac.pinned_mesh()
        c = ac.case("torus_a")
        handles, goal = c["handles"], c["targets"]
    elif name == "free_torus":
        c = ac.case("torus_a")
        V0, faces, handles, goal = c["V0"], c["faces"], np.zeros(0, np.int64), None
    else:
        c = ac.case(name)
        V0, faces, handles, goal = c["V0"], c["faces"], c["handles"], c["targets"]
    v0 = np.zeros_like(V0)
    if name == "free_torus":                                           # a spin about y, a drift and a shear: nothing holds it
        X = V0.astype(np.float64)
        v0 = (np.cross(np.array([0.0, 0.6, 0.0]), X) + np.array([0.1, 0.2, -0.1]) + 0.15 * X[:, [1, 2, 0]] * np.array([1.0, 0.0, -0.5])).astype(np.float32)
    return dict(name=name, V0=V0, faces=np.asarray(faces, np.int32), handles=np.asarray(handles, np.int64),
                targets=None if goal is None else ramp(V0[handles], goal), goal=goal, pinned=np.zeros(0, np.int64), v0=v0,
                mass=dr.vertex_masses(V0, faces))


def reference(name, material, pinned=None, handles=None):
    """a fresh dynamics_ref.Dynamics of the case with MATERIALS[material] (an index) or a (stiffness, gravity, damping) triple"""
    c = case(name)
    k, g, d = MATERIALS[material] if isinstance(material, int) else material
    return dr.Dynamics(c["V0"], c["faces"], c["mass"], pinned=c["pinned"] if pinned is None else pinned, handles=c["handles"] if handles is None else handles,
                       dt=DT, stiffness=k, damping=d, gravity=g, iterations=ITERATIONS)


@functools.lru_cache(maxsize=None)
def reference_run(name, material):
    """(positions [STEPS,Vm,3] float32, last velocities [Vm,3] float32) with exact global steps; do not modify"""
    c = case(name)
    X, v, _ = reference(name, material).run(c["V0"], c["v0"], STEPS, c["targets"])
    return X, v


def free_body_error(run, n=8):
    """run(gravity, velocities float32 [Vm,3], n) -> positions [n,Vm,3] of free_torus from rest with a uniform velocity, damping 0: the largest
    distance from implicit Euler's closed form divided by the step's number, without gravity and with it"""
    c = case("free_torus")
    x0 = c["V0"].astype(np.float64)
    u = np.array([0.3, -0.2, 0.5])
    out = []
    for grav in ((0.0, 0.0, 0.0), GRAVITY):
        X = run(grav, np.tile(u, (len(x0), 1)).astype(np.float32), n).astype(np.float64)
        u32 = u.astype(np.float32).astype(np.float64)
        want, x, a = [], x0.copy(), np.asarray(grav)
        for k in range(1, n + 1):                                      # implicit Euler's closed form: v_k = u + k h a, x_k = x_{k-1} + h v_k
            x = x + DT * (u32 + k * DT * a)
            want.append(x)
        out.append(max(float(np.abs(X[k] - want[k]).max()) / (k + 1) for k in range(n)))
    return out
