"""Shared cases of the field-contact tests (test_dynamics_field_ref_host.py, test_gpu_dynamics_field.py): the meshes of
dynamics_contact_cases (the free torus, sheets of 25 and 1056 vertices) over sampled signed-distance grids of about 24^3 samples, some with
analytic colliders beside the grid, and the float64 reference (dynamics_field_ref.FieldDynamics) run once per (case, material) and shared.
The grids' origins are uneven numbers on purpose, so that no row starts on a cell face."""
import functools

import numpy as np

import dynamics_cases as dc
import dynamics_contact_cases as cc
import dynamics_contact_ref as cr
import dynamics_field_ref as fr
import sdf_grid_ref as sg

STEPS, DT, ITERATIONS, TIGHT, KC, NEAR, MATERIALS = cc.STEPS, cc.DT, cc.ITERATIONS, cc.TIGHT, cc.KC, cc.NEAR, cc.MATERIALS
NAMES = ("tilt_smooth", "tilt_rough", "bump", "sheet25", "sheet1056", "half_outside", "unknown_block", "field_pusher", "field_sixteen")
ALL = tuple((n, m) for n in NAMES for m in MATERIALS)
GROUND = -0.9                   # the torus spans y in [-0.7, 0.7] and is 5.4 across


def centres(dims, origin, voxel):
    """the sample positions [nz,ny,nx,3] float64 of a grid (dims = (nx, ny, nz); origin and voxel as their float32 values)"""
    o, h = np.asarray(origin, np.float32).astype(np.float64), float(np.float32(voxel))
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([o[0] + (x + 0.5) * h, o[1] + (y + 0.5) * h, o[2] + (z + 0.5) * h], -1)


def plane_values(dims, origin, voxel, normal, offset):
    """n . p - offset at every sample (the normal normalised), float32 [nz,ny,nx]"""
    n = np.asarray(normal, np.float64)
    return (centres(dims, origin, voxel) @ (n / np.linalg.norm(n)) - offset).astype(np.float32)


def sphere_values(dims, origin, voxel, centre, radius):
    return (np.linalg.norm(centres(dims, origin, voxel) - np.asarray(centre, np.float64), axis=-1) - radius).astype(np.float32)


def _field(values, origin, voxel, friction):
    return dict(values=np.ascontiguousarray(values, np.float32), origin=np.asarray(origin, np.float32), voxel=float(np.float32(voxel)), friction=float(friction))


TORUS_GRID = ((24, 16, 24), (-3.71, -2.53, -3.67), 0.3)               # samples x, z in [-3.5, 3.4], y in [-2.4, 2.1]
SHEET_GRID = ((24, 12, 24), (-1.21, -0.53, -1.17), 0.1)               # samples x, z in [-1.1, 1.1], y in [-0.5, 0.6]


def _sheet_case(name, nu, nv):
    c = dict(cc.case("sheet5" if nu == 5 else "sheet1056"), name=name, colliders=(), collider_rows=None)
    c["field"] = _field(plane_values(*SHEET_GRID, (0.0, 1.0, 0.0), 0.0), SHEET_GRID[1], SHEET_GRID[2], 0.3)
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """dynamics_contact_cases.case's dict plus field = dict(values float32 [nz,ny,nx], origin float32 [3], voxel, friction)"""
    if name == "sheet25":                                              # a tangential start velocity (0.4, -0.5, 0.2) and friction 0.3
        return _sheet_case(name, 5, 5)
    if name == "sheet1056":                                            # five 256-row blocks, two turns of the 1024-thread stride
        return _sheet_case(name, 33, 32)
    c = dict(dc.case("free_torus"), name=name, colliders=(), collider_rows=None)
    dims, origin, voxel = TORUS_GRID
    floor = plane_values(dims, origin, voxel, (0.0, 1.0, 0.0), GROUND)
    if name in ("tilt_smooth", "tilt_rough"):                          # a tilted plane: all three gradient channels matter
        tilt = (0.2, 1.0, 0.1)
        d = float(np.array([0.0, GROUND, 0.0]) @ (np.asarray(tilt) / np.linalg.norm(tilt)))
        c["field"] = _field(plane_values(dims, origin, voxel, tilt, d), origin, voxel, 0.0 if name == "tilt_smooth" else 0.5)
    elif name == "bump":                                               # a floor with a bump under the tube at x = 2: the sampled field has a crease
        c["field"] = _field(np.minimum(floor, sphere_values(dims, origin, voxel, (2.0, -1.5, 0.0), 1.0)), origin, voxel, 0.2)
    elif name == "half_outside":                                       # the grid ends at x = 0.34: the half of the torus beyond it meets nothing
        half = (14, 16, 24)
        c["field"] = _field(plane_values(half, origin, voxel, (0.0, 1.0, 0.0), GROUND), origin, voxel, 0.3)
    elif name == "unknown_block":                                      # nothing is known in a column of samples under the tube at x = -2
        v = floor.copy()
        v[9:15, :, 4:8] = np.nan
        c["field"] = _field(v, origin, voxel, 0.3)
    elif name == "field_pusher":                                       # the floor as a field, and dynamics_contact_cases' rising ball
        p = cc.case("pusher")
        c["colliders"], c["collider_rows"] = p["colliders"], p["collider_rows"]
        c["field"] = _field(floor, origin, voxel, 0.3)
    elif name == "field_sixteen":                                      # sixteen analytic colliders, their floor 0.02 under the field's
        s = cc.case("sixteen")
        c["colliders"], c["v0"] = s["colliders"], s["v0"]
        c["field"] = _field(plane_values(dims, origin, voxel, (0.0, 1.0, 0.0), GROUND + 0.02), origin, voxel, 0.2)
    else:
        raise KeyError(name)
    return c


@functools.lru_cache(maxsize=None)
def prepared(name):
    """the case's grid as sdf_grid_ref.prepare makes it (float32 [nz,ny,nx,4]); do not modify"""
    f = case(name)["field"]
    return sg.prepare(f["values"], f["voxel"])


def reference(name, material, field="case", **kw):
    """a fresh FieldDynamics of the case with dynamics_cases.MATERIALS[material] (an index) or a (stiffness, gravity, damping) triple"""
    c = case(name)
    k, g, d = dc.MATERIALS[material] if isinstance(material, int) else material
    f = c["field"]
    opts = dict(pinned=c["pinned"], handles=c["handles"], dt=DT, stiffness=k, damping=d, gravity=g, iterations=ITERATIONS, colliders=c["colliders"],
                contact_stiffness=KC, field=(prepared(name), f["origin"], f["voxel"]) if field == "case" else field, field_friction=f["friction"])
    opts.update(kw)
    return fr.FieldDynamics(c["V0"], c["faces"], c["mass"], **opts)


@functools.lru_cache(maxsize=None)
def reference_run(name, material):
    """(positions [STEPS,Vm,3] float32, last velocities [Vm,3] float32, contact [STEPS,Vm] int, compare [STEPS,Vm] bool: the rows whose
    active set a device is held to - all but those within NEAR of a surface or of a second candidate, or within dynamics_field_ref.PROBE
    of where the field stops being known) with exact global steps; do not modify"""
    c = case(name)
    r = reference(name, material)
    X, v, _ = r.run(c["V0"], c["v0"], STEPS, c["targets"], collider_rows=c["collider_rows"])
    compare = ~((np.abs(r.phi_star) < NEAR) | (r.gap < NEAR) | r.fringe)
    return X, v, r.contact, compare


@functools.lru_cache(maxsize=None)
def reference_run_pcg(name, material):
    """the same run with the reference's own PCG at TIGHT: (positions, last velocities)"""
    c = case(name)
    X, v, _ = reference(name, material).run(c["V0"], c["v0"], STEPS, c["targets"], pcg=TIGHT, collider_rows=c["collider_rows"])
    return X, v


# ---- a floor fused from two top views (the end-to-end test) ----
FUSED_VOXEL, FUSED_LO, FUSED_N = 0.22, (-3.53, -2.61, -3.49), 32


def fused_floor_views(size=64):
    """(cameras, depth float32 [2,size,size], alpha float32 [2,size,size]): the floor y = GROUND seen straight down from y = 5 and y = 8,
    as the maps such views have - a plane square to the view axis has one depth everywhere, and it is opaque"""
    from gaussianmesh_amd import scenes
    heights = (5.0, 8.0)
    cams = [scenes.look_at_camera((0.0, h, 0.0), (0.0, GROUND, 0.0), size, size, fovx_deg=100.0, up=(0.0, 0.0, 1.0)) for h in heights]
    depth = np.stack([np.full((size, size), h - GROUND, np.float32) for h in heights])
    return cams, depth, np.ones_like(depth)


@functools.lru_cache(maxsize=None)
def fused_floor_volume():
    """(tsdf, weight float32 [32,32,32], origin float32 [3], voxel, trunc) of those views by tsdf_ref.integrate_ref, with the voxel and the
    truncation (3 voxels) a proxy_mesh.TsdfVolume of this box has; do not modify"""
    import tsdf_ref as tr
    cams, depth, alpha = fused_floor_views()
    views, tans = tr.camera_rows(cams)
    origin, voxel, trunc = np.asarray(FUSED_LO, np.float32), float(np.float32(FUSED_VOXEL)), float(np.float32(3.0 * FUSED_VOXEL))
    zero = np.zeros((FUSED_N,) * 3, np.float32)
    tsdf, weight = tr.integrate_ref(zero, zero, depth, alpha, views, tans, origin, voxel, trunc)
    return tsdf, weight, origin, voxel, trunc


def fused_floor_reference(tsdf, weight, origin, voxel, trunc, material=(50.0, dc.GRAVITY, 0.2), friction=0.3):
    """a fresh FieldDynamics of the free torus over SdfGrid.from_tsdf's grid of the volume"""
    c = dc.case("free_torus")
    k, g, d = material
    return fr.FieldDynamics(c["V0"], c["faces"], c["mass"], dt=DT, stiffness=k, damping=d, gravity=g, iterations=ITERATIONS, contact_stiffness=KC,
                            field=(sg.prepare(tsdf, voxel, weight, 1.0, trunc), origin, voxel), field_friction=friction)
