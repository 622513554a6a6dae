"""Shared cases of the mesh-contact tests (test_dynamics_contact_ref_host.py, test_gpu_dynamics_contact.py): meshes of dynamics_cases and
flat sheets, each with its colliders (static, or scripted per step), and the float64 reference (dynamics_contact_ref.ContactDynamics) run
once per (case, material) and shared."""
import functools

import numpy as np

import dynamics_cases as dc
import dynamics_contact_ref as cr

STEPS, DT, ITERATIONS, TIGHT = dc.STEPS, dc.DT, dc.ITERATIONS, dc.TIGHT
KC = 1.0e4                      # contact_stiffness of every case: rest depth |g| / kc about 1e-3
# of dynamics_cases.MATERIALS (stiffness, gravity, damping): with gravity, soft and stiff, damping 0 and 0.02
MATERIALS = (dc.MATERIALS.index((1.0, dc.GRAVITY, 0.0)), dc.MATERIALS.index((50.0, dc.GRAVITY, 0.02)))
NAMES = ("drop_smooth", "drop_rough", "drag", "pusher", "corner", "sheet5", "sheet1056", "sixteen")
ALL = tuple((n, m) for n in NAMES for m in MATERIALS)
NEAR = 1e-5                     # rows this close to a surface, or to a second collider, are left out of the active-set comparison


def sheet(nu, nv, size=1.0, height=0.0):
    """a flat nu x nv grid in the plane y = height, `size` along x: (V0 float32 [nu nv,3], faces int32 [2 (nu-1)(nv-1),3])"""
    step = size / (nu - 1)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    V = np.stack([i * step - 0.5 * size, np.full(i.shape, height), j * step - 0.5 * step * (nv - 1)], -1).reshape(-1, 3).astype(np.float32)
    q = (i[:-1, :-1] * nv + j[:-1, :-1]).reshape(-1)
    faces = np.concatenate([np.stack([q, q + 1, q + nv + 1], 1), np.stack([q, q + nv + 1, q + nv], 1)], 0).astype(np.int32)
    return V, faces


def _sheet_case(name, nu, nv, friction):
    V0, faces = sheet(nu, nv, height=0.1)
    v0 = np.tile(np.array([0.4, -0.5, 0.2], np.float32), (len(V0), 1))
    return dict(name=name, V0=V0, faces=faces, handles=np.zeros(0, np.int64), targets=None, pinned=np.zeros(0, np.int64), v0=v0,
                mass=cr.dr.vertex_masses(V0, faces), colliders=(cr.floor(0.0, friction=friction),), collider_rows=None)


@functools.lru_cache(maxsize=None)
def case(name):
    """dynamics_cases.case's dict plus colliders (a tuple of (kind, row, friction)) and collider_rows (float32 [STEPS,K,4], or None: static)"""
    if name == "sheet5":
        return _sheet_case(name, 5, 5, 0.3)
    if name == "sheet1056":                                            # dyn_global's stride loop runs twice, the local kernel has 5 blocks
        return _sheet_case(name, 33, 32, 0.3)
    c = dict(dc.case("torus_a" if name == "drag" else "free_torus"), name=name, collider_rows=None)
    ground = -0.9                                                      # the torus spans y in [-0.7, 0.7] and is 5.4 across
    if name == "drop_smooth":
        c["colliders"] = (cr.floor(ground, friction=0.0),)
    elif name == "drop_rough":
        c["colliders"] = (cr.floor(ground, friction=0.5),)
    elif name == "drag":                                               # the handles' ramp takes part of the ring down to y = -1.02
        c["colliders"] = (cr.floor(-0.75, friction=0.3),)
    elif name == "pusher":                                             # a ball rising through the tube at x = 2, the torus falling onto it
        c["colliders"] = (cr.sphere((2.0, -2.0, 0.0), 1.0),)
        s = np.arange(1, STEPS + 1) / float(STEPS)
        rows = np.tile(c["colliders"][0][1], (STEPS, 1, 1))
        rows[:, 0, 1] = (-2.0 + 3.0 * s).astype(np.float32)
        c["collider_rows"] = rows
    elif name == "corner":                                             # a floor and a wall; the torus drifts into the wall as it falls
        c["colliders"] = (cr.floor(ground, friction=0.2), cr.half_space((1.0, 0.0, 0.0), offset=-2.9, friction=0.1))
        c["v0"] = (c["v0"] + np.array([-1.5, 0.0, 0.0], np.float32)).astype(np.float32)
    elif name == "sixteen":                                            # the corner among fourteen colliders that lose or are out of reach
        lower = tuple(cr.floor(ground - 0.01 * (j + 1), friction=0.05 * j) for j in range(5))
        far = tuple(cr.sphere((10.0 + j, 0.0, 0.0), 1.0, friction=0.1) for j in range(5))
        walls = tuple(cr.half_space((0.0, 0.0, s), offset=-6.0 - j) for j, s in enumerate((1.0, -1.0, 1.0, -1.0)))
        c["colliders"] = lower + (cr.floor(ground, friction=0.2),) + far + (cr.half_space((1.0, 0.0, 0.0), offset=-2.9, friction=0.1),) + walls
        c["v0"] = (c["v0"] + np.array([-1.5, 0.0, 0.0], np.float32)).astype(np.float32)
        assert len(c["colliders"]) == 16
    else:
        raise KeyError(name)
    return c


def reference(name, material, colliders=None, contact_stiffness=KC, **kw):
    """a fresh ContactDynamics of the case with dynamics_cases.MATERIALS[material] (an index) or a (stiffness, gravity, damping) triple"""
    c = case(name)
    k, g, d = dc.MATERIALS[material] if isinstance(material, int) else material
    opts = dict(pinned=c["pinned"], handles=c["handles"], dt=DT, stiffness=k, damping=d, gravity=g, iterations=ITERATIONS,
                colliders=c["colliders"] if colliders is None else colliders, contact_stiffness=contact_stiffness)
    opts.update(kw)
    return cr.ContactDynamics(c["V0"], c["faces"], c["mass"], **opts)


@functools.lru_cache(maxsize=None)
def reference_run(name, material):
    """(positions [STEPS,Vm,3] float32, last velocities [Vm,3] float32, contact [STEPS,Vm] int, compare [STEPS,Vm] bool: the rows whose
    active set a device is held to) with exact global steps; do not modify"""
    c = case(name)
    r = reference(name, material)
    X, v, _ = r.run(c["V0"], c["v0"], STEPS, c["targets"], collider_rows=c["collider_rows"])
    compare = ~((np.abs(r.phi_star) < NEAR) | (r.gap < NEAR))
    return X, v, r.contact, compare


@functools.lru_cache(maxsize=None)
def reference_run_pcg(name, material):
    """the same run with the reference's own PCG at TIGHT: (positions, last velocities)"""
    c = case(name)
    X, v, _ = reference(name, material).run(c["V0"], c["v0"], STEPS, c["targets"], pcg=TIGHT, collider_rows=c["collider_rows"])
    return X, v


def sheet_recursion(y0, v0, steps, gravity=dc.GRAVITY[1], damping=0.0, kc=KC, height=0.0, dt=DT):
    """the height of a flat sheet over a frictionless floor at `height`, step by step: Y <- (Y + h v + h^2 a + kc h^2 height) / (1 + kc h^2)
    while the prediction is below the floor, the prediction itself above it; float32 rounding at the step boundaries.  [steps] float64"""
    Y, v, out = float(np.float32(y0)), float(np.float32(v0)), []
    for _ in range(steps):
        y = Y + dt * v + dt * dt * gravity
        new = (y + kc * dt * dt * height) / (1.0 + kc * dt * dt) if y < height else y
        new32 = float(np.float32(new))
        v = float(np.float32((1.0 - damping) * (new - Y) / dt))
        Y = new32
        out.append(Y)
    return np.array(out)
