"""Shared cases of the moving-field tests (test_dynamics_moving_field_ref_host.py, test_gpu_dynamics_moving_field.py): the meshes and
grids of dynamics_field_cases / dynamics_contact_cases (the sheets of 25 and 1056 vertices, the free torus) over one to four sampled grids
that move rigidly, some with analytic colliders beside them, and the float64 reference (dynamics_moving_field_ref.MovingFieldDynamics)
run once per (case, material) and shared.  A pose is (R | t) [3,4], world = R local + t."""
import functools

import numpy as np

import dynamics_cases as dc
import dynamics_contact_cases as cc
import dynamics_field_cases as fc
import dynamics_moving_field_ref as mr
import sdf_grid_ref as sg

STEPS, DT, ITERATIONS, TIGHT, KC, NEAR, MATERIALS = fc.STEPS, fc.DT, fc.ITERATIONS, fc.TIGHT, fc.KC, fc.NEAR, fc.MATERIALS
NAMES = ("slide_smooth", "slide_rough", "rise", "tilt_spin", "bump_sweep", "two", "four_sixteen", "half_leaves", "pause")
ALL = tuple((n, m) for n in NAMES for m in MATERIALS)
GROUND = fc.GROUND
PLATE_SPEED = 0.3               # of the translating and the rising plate


def rotation(axis, angle):
    """Rodrigues' rotation matrix about `axis` (normalised here) by `angle`"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    S = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * S + (1.0 - np.cos(angle)) * (S @ S)


def pose(R=None, t=(0.0, 0.0, 0.0), about=None):
    """(R | t) [3,4]; with `about` the rotation turns about that point and t comes on top: x -> R (x - about) + about + t"""
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    t = np.asarray(t, np.float64)
    if about is not None:
        about = np.asarray(about, np.float64)
        t = t + about - R @ about
    return np.concatenate([R, t[:, None]], axis=1)


def translations(velocity, steps=STEPS, dt=DT):
    """poses [steps,3,4] of a body moving at `velocity` from the identity: step k's pose is the one at the step's end, (k + 1) dt velocity"""
    return np.array([pose(t=(k + 1) * dt * np.asarray(velocity, np.float64)) for k in range(steps)])


def _field(values, grid, friction):
    dims, origin, voxel = grid
    return fc._field(values, origin, voxel, friction)


def _sheet(nu, plate_velocity, friction):
    c = dict(cc.case("sheet5" if nu == 5 else "sheet1056"), colliders=(), collider_rows=None)
    c["fields"] = [_field(fc.plane_values(*fc.SHEET_GRID, (0.0, 1.0, 0.0), 0.0), fc.SHEET_GRID, friction)]
    c["field_poses"] = translations(plate_velocity)[:, None]
    return c


def _ball(centre=(2.0, -2.0, 0.0), radius=1.0):
    return fc.sphere_values(*fc.TORUS_GRID, centre, radius)


@functools.lru_cache(maxsize=None)
def case(name):
    """dynamics_contact_cases.case's dict plus fields (a list of dynamics_field_cases' field dicts), field_poses float64 [STEPS,F,3,4] and
    pose0 float64 [F,3,4], the poses before the first step"""
    dims, origin, voxel = fc.TORUS_GRID
    floor = fc.plane_values(dims, origin, voxel, (0.0, 1.0, 0.0), GROUND)
    if name == "slide_smooth":                                         # a plate translating sideways under the 25-vertex sheet, frictionless
        c = _sheet(5, (PLATE_SPEED, 0.0, 0.0), 0.0)
    elif name == "slide_rough":                                        # the same under the 1056-vertex sheet, with friction 0.5
        c = _sheet(33, (PLATE_SPEED, 0.0, 0.0), 0.5)
    elif name == "rise":                                               # a plate rising at constant speed
        c = _sheet(5, (0.0, PLATE_SPEED, 0.0), 0.3)
    elif name == "pause":                                              # the rough plate stands still in steps 7 .. 9, in the middle of its run
        c = _sheet(5, (PLATE_SPEED, 0.0, 0.0), 0.5)
        poses = c["field_poses"].copy()
        poses[7:10] = poses[6]
        poses[10:] = translations((PLATE_SPEED, 0.0, 0.0))[:STEPS - 10, None] + np.concatenate([np.zeros((3, 3)), poses[6, 0, :, 3:]], axis=1)
        c["field_poses"] = poses
    else:
        c = dict(dc.case("free_torus"), colliders=(), collider_rows=None)
        if name == "tilt_spin":                                        # dynamics_field_cases' tilted plate turning about an axis off its centre
            tilt = (0.2, 1.0, 0.1)
            d = float(np.array([0.0, GROUND, 0.0]) @ (np.asarray(tilt) / np.linalg.norm(tilt)))
            c["fields"] = [_field(fc.plane_values(dims, origin, voxel, tilt, d), fc.TORUS_GRID, 0.5)]
            c["field_poses"] = np.array([pose(rotation((0.1, 1.0, 0.05), 0.008 * (k + 1)), about=(1.0, 0.0, 0.5)) for k in range(STEPS)])[:, None]
        elif name == "bump_sweep":                                     # the floor with a bump sweeping under the tube
            c["fields"] = [_field(np.minimum(floor, fc.sphere_values(dims, origin, voxel, (2.0, -1.5, 0.0), 1.0)), fc.TORUS_GRID, 0.2)]
            c["field_poses"] = translations((-0.6, 0.0, 0.15))[:, None]
        elif name == "two":                                            # a static floor and a ball rising through it: their contact regions meet
            c["fields"] = [_field(floor, fc.TORUS_GRID, 0.3), _field(_ball(), fc.TORUS_GRID, 0.1)]
            c["field_poses"] = np.stack([np.tile(mr.IDENTITY, (STEPS, 1, 1)), translations((0.0, 1.2, 0.0))], axis=1)
        elif name == "four_sixteen":                                   # sixteen analytic colliders and four fields: the last field wins too
            s = cc.case("sixteen")
            c["colliders"], c["v0"] = s["colliders"], s["v0"]
            c["fields"] = [_field(fc.plane_values(dims, origin, voxel, (0.0, 1.0, 0.0), GROUND + 0.02), fc.TORUS_GRID, 0.2),
                           _field(fc.plane_values(dims, origin, voxel, (0.0, 1.0, 0.0), GROUND - 0.3), fc.TORUS_GRID, 0.4),
                           _field(np.full((dims[2], dims[1], dims[0]), np.nan, np.float32), fc.TORUS_GRID, 0.4),
                           _field(_ball(), fc.TORUS_GRID, 0.1)]
            c["field_poses"] = np.stack([translations((0.1, 0.0, 0.05)),
                                         np.array([pose(rotation((0.0, 1.0, 0.0), 0.01 * (k + 1))) for k in range(STEPS)]),
                                         translations((0.0, 0.0, 0.5)), translations((0.0, 1.2, 0.0))], axis=1)
        elif name == "half_leaves":                                    # the floor grid posed so that it ends under the torus, and moving on
            c["fields"] = [_field(floor, fc.TORUS_GRID, 0.3)]
            c["pose0"] = pose(t=(-3.1, 0.0, 0.0))[None]
            c["field_poses"] = translations((-0.3, 0.0, 0.0))[:, None] + np.concatenate([np.zeros((3, 3)), c["pose0"][0, :, 3:]], axis=1)
        else:
            raise KeyError(name)
    c["name"] = name
    c.setdefault("pose0", np.tile(mr.IDENTITY, (len(c["fields"]), 1, 1)))
    return c


@functools.lru_cache(maxsize=None)
def prepared(name):
    """the case's grids as sdf_grid_ref.prepare makes them: a tuple of (grid float32 [nz,ny,nx,4], origin, voxel); do not modify"""
    return tuple((sg.prepare(f["values"], f["voxel"]), f["origin"], f["voxel"]) for f in case(name)["fields"])


def reference(name, material, **kw):
    """a fresh MovingFieldDynamics of the case with dynamics_cases.MATERIALS[material] (an index) or a (stiffness, gravity, damping) triple,
    its fields at pose0"""
    c = case(name)
    k, g, d = dc.MATERIALS[material] if isinstance(material, int) else material
    opts = dict(pinned=c["pinned"], handles=c["handles"], dt=DT, stiffness=k, damping=d, gravity=g, iterations=ITERATIONS, colliders=c["colliders"],
                contact_stiffness=KC, fields=prepared(name), field_frictions=[f["friction"] for f in c["fields"]])
    opts.update(kw)
    r = mr.MovingFieldDynamics(c["V0"], c["faces"], c["mass"], **opts)
    r.poses = c["pose0"].copy()
    return r


@functools.lru_cache(maxsize=None)
def reference_run(name, material):
    """(positions [STEPS,Vm,3] float32, last velocities [Vm,3] float32, contact [STEPS,Vm] int, compare [STEPS,Vm] bool: the rows whose
    active set a device is held to - all but those within NEAR of a surface or of a second candidate, or within dynamics_field_ref.PROBE
    of where a field stops being known) with exact global steps; do not modify"""
    c = case(name)
    r = reference(name, material)
    X, v, _ = r.run(c["V0"], c["v0"], STEPS, c["targets"], collider_rows=c["collider_rows"], field_poses=c["field_poses"])
    compare = ~((np.abs(r.phi_star) < NEAR) | (r.gap < NEAR) | r.fringe)
    return X, v, r.contact, compare


@functools.lru_cache(maxsize=None)
def reference_run_pcg(name, material):
    """the same run with the reference's own PCG at TIGHT: (positions, last velocities)"""
    c = case(name)
    X, v, _ = reference(name, material).run(c["V0"], c["v0"], STEPS, c["targets"], pcg=TIGHT, collider_rows=c["collider_rows"], field_poses=c["field_poses"])
    return X, v
