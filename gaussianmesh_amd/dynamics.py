"""Secondary motion of a proxy mesh: implicit-Euler steps of an elastic mesh whose potential is the ARAP energy, on the device
(gm_mesh_dynamics, csrc/gm_dynamics.hip).  ArapSolver, PoseInterpolator and PoseFitter give static equilibria; here the mesh has
velocity: a dragged limb follows through, a released handle swings back, an object sags under its weight and settles.  A step is the
local/global iteration of projective dynamics (Bouaziz et al. 2014) with Sorkine & Alexa's vertex-star energy as the constraint set: the
local step is ArapSolver's, the global step's matrix gains the positive diagonal mass_i / (2 stiffness dt^2), so the system is positive
definite with no held row at all - a free body is a valid input, which ArapSolver cannot express.  The result is a [steps,Vm,3] stack of
meshes: what render_sequence, SingleObjectDeform.deform_vertices and edit_sequence --save_meshes take.  Definition, ABI and rules:
INTEGRATION.md section AA.  With colliders (floor / half_space / sphere) the free rows cannot enter them: unilateral contact with
Coulomb-limited friction (gm_mesh_dynamics_contact), INTEGRATION.md section AB.  With field=SdfGrid(...) they cannot enter a sampled
signed-distance volume either - the fused volume of the scene's background cloud, say (gm_mesh_dynamics_field), section AC.  With
fields=[SdfGrid, ...] and run(field_poses=) up to four such volumes move rigidly, each on its own, while the mesh is simulated against
them, with friction in each obstacle's own frame (gm_mesh_dynamics_fields), section AG; rigid_pose / rigid_poses recover those poses
from a rigidly moved mesh."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._op import enqueue, host, need_cuda, on_device
from .mesh_graph import MeshGraph


def vertex_masses(vertices, faces, density=1.0):
    """Lumped masses of a triangle mesh: every vertex gets one third of the area of each face at it, times density; float64 [Vm], on
    the host (the vertices are read as float32, as everywhere).  Their sum is density x the mesh's area; a vertex no face of positive
    area names gets 0."""
    v = np.asarray(host(vertices), np.float32).astype(np.float64)
    f = np.asarray(host(faces)).astype(np.int64).reshape(-1, 3)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError("vertex_masses: vertices must be [Vm,3]; got %s" % (tuple(v.shape),))
    if f.shape[0] and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):
        raise ValueError("vertex_masses: face index outside [0, %d)" % v.shape[0])
    if not np.isfinite(density) or not density > 0.0:
        raise ValueError("vertex_masses: density must be finite and positive; got %r" % (density,))
    area = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    m = np.zeros(v.shape[0], np.float64)
    for c in range(3):
        np.add.at(m, f[:, c], area / 3.0)
    return m * float(density)


HALF_SPACE, SPHERE = 0, 1          # collider_kind of gm_mesh_dynamics_contact


def _number(who, name, val, ok, rule):
    """val as a float: a real number (no bool), finite, with ok(val); else ValueError('<who>: <name> = <val><rule>')"""
    if isinstance(val, bool) or not isinstance(val, (int, float, np.integer, np.floating)) or not np.isfinite(val) or not ok(float(val)):
        raise ValueError("%s: %s = %r%s" % (who, name, val, rule))
    return float(val)


def _friction(who, friction):
    return _number(who, "friction", friction, lambda x: x >= 0.0, "; a finite number >= 0")


def _shaped(a):
    """an array-like as something that has a .shape: a tensor or an array as it is, anything else as a float32 array"""
    return a if hasattr(a, "shape") else np.asarray(a, np.float32)


def half_space(normal, offset=None, point=None, friction=0.0):
    """A collider that fills the half-space n . x < d: ("half_space", (nx, ny, nz, d), friction) with the normal normalised.  Give the
    plane by offset (d itself, for the normalised normal) or by a point on it; neither: through the origin.  ValueError for a zero or
    non-finite normal, a non-finite plane, both offset and point, a negative friction."""
    who = "half_space"
    n = np.asarray(host(normal), np.float64).reshape(-1)
    if n.shape != (3,) or not np.isfinite(n).all() or not float(np.linalg.norm(n)) > 0.0 or not np.isfinite(np.linalg.norm(n)):
        raise ValueError("%s: normal must be three finite numbers, not all zero; got %r" % (who, normal))
    n = n / np.linalg.norm(n)
    if offset is not None and point is not None:
        raise ValueError("%s: give the plane by offset or by point, not both" % who)
    if point is not None:
        q = np.asarray(host(point), np.float64).reshape(-1)
        if q.shape != (3,):
            raise ValueError("%s: point must be three numbers; got %r" % (who, point))
        d = float(n @ q)
    else:
        d = 0.0 if offset is None else float(offset)
    if not np.isfinite(d):
        raise ValueError("%s: the plane must be finite; got offset %r, point %r" % (who, offset, point))
    return ("half_space", (float(n[0]), float(n[1]), float(n[2]), d), _friction(who, friction))


def floor(height=0.0, up=(0.0, 1.0, 0.0), friction=0.0):
    """half_space(up, offset=height): the ground at `height` along `up`"""
    return half_space(up, offset=height, friction=friction)


def sphere(center, radius, friction=0.0):
    """A solid ball: ("sphere", (cx, cy, cz, r), friction).  ValueError for a non-finite centre, a radius that is not finite and
    positive, a negative friction."""
    who = "sphere"
    c = np.asarray(host(center), np.float64).reshape(-1)
    if c.shape != (3,) or not np.isfinite(c).all():
        raise ValueError("%s: center must be three finite numbers; got %r" % (who, center))
    radius = _number(who, "radius", radius, lambda x: x > 0.0, "; finite and positive")
    return ("sphere", (float(c[0]), float(c[1]), float(c[2]), radius), _friction(who, friction))


def _collider(who, c):
    """one collider, given as half_space / floor / sphere make it (a tuple or list (kind, row, friction), nested lists welcome) or as a
    dict(kind=, friction=, and normal= with offset= or point= / center=, radius=), checked again: (kind id, row [4], friction)"""
    if isinstance(c, dict):
        kind = c.get("kind")
        extra = set(c) - {"kind", "friction", "normal", "offset", "point", "center", "radius"}
        if extra:
            raise ValueError("%s: a collider has no %r" % (who, sorted(extra)[0]))
        if kind == "half_space":
            c = half_space(c.get("normal", ()), c.get("offset"), c.get("point"), c.get("friction", 0.0))
        elif kind == "sphere":
            c = sphere(c.get("center", ()), c.get("radius"), c.get("friction", 0.0))
        else:
            raise ValueError('%s: a collider\'s kind is "half_space" or "sphere"; got %r' % (who, kind))
    if not isinstance(c, (tuple, list)) or len(c) != 3 or c[0] not in ("half_space", "sphere"):
        raise ValueError('%s: a collider is ("half_space" | "sphere", (four numbers), friction), as half_space(), floor() and sphere() make it; got %r' % (who, c))
    row = np.asarray(c[1], np.float64).reshape(-1)
    if row.shape != (4,):
        raise ValueError("%s: a collider's row holds four numbers; got %r" % (who, c[1]))
    if c[0] == "half_space":
        _, r, mu = half_space(row[:3], offset=row[3], friction=c[2])
        return HALF_SPACE, r, mu
    _, r, mu = sphere(row[:3], float(row[3]), friction=c[2])
    return SPHERE, r, mu


def collider_table(colliders, who="collider_table"):
    """The colliders of MeshDynamics(colliders=...) as the arrays gm_mesh_dynamics_contact reads: (kinds int32 [K], rows float32 [K,4],
    friction float64 [K]), every collider checked.  rows is what run's collider_rows repeats or replaces per step."""
    if isinstance(colliders, dict) or not isinstance(colliders, (tuple, list)):
        raise ValueError("%s: colliders must be a sequence of half_space() / floor() / sphere(); got %r" % (who, colliders))
    if len(colliders) > _lib.GM_MESH_CONTACT_COLLIDERS_MAX:
        raise ValueError("%s: %d colliders; at most %d" % (who, len(colliders), _lib.GM_MESH_CONTACT_COLLIDERS_MAX))
    parsed = [_collider(who, c) for c in colliders]
    return (np.array([c[0] for c in parsed], np.int32), np.array([c[1] for c in parsed], np.float32).reshape(len(parsed), 4),
            np.array([c[2] for c in parsed], np.float64))


def _check_poses(who, poses):
    """host poses [..., 3, 4] as float64, each (R | t) finite with |R^T R - I| <= 1e-6 and det R > 0; else ValueError"""
    p = np.asarray(poses, np.float64)
    if not np.isfinite(p).all():
        raise ValueError("%s: field_poses must be finite" % who)
    R = p[..., :3]
    if p.size and (float(np.abs(np.swapaxes(R, -1, -2) @ R - np.eye(3)).max()) > 1e-6 or not bool((np.linalg.det(R) > 0.0).all())):
        raise ValueError("%s: every pose of field_poses must be (R | t) with R a rotation: |R^T R - I| <= 1e-6 and det R > 0" % who)
    return p


def rigid_pose(rest_vertices, moved_vertices, tolerance=1e-5):
    """The rigid motion (R | t), float64 [3,4] on the host, that carries rest_vertices [Vm,3] onto moved_vertices [Vm,3]:
    moved = R rest + t, by Kabsch's method in float64 (the rotation of the SVD of the centred covariance, det R = +1).  What
    run(field_poses=) wants of an obstacle whose SdfGrid was sampled at its rest mesh.  ValueError for shapes, fewer than three
    vertices, non-finite vertices, and where the largest distance |R rest_i + t - moved_i| exceeds `tolerance` (in the mesh's own
    units; the default suits float32 vertices of unit size): a mesh that deforms is refused, not approximated."""
    who = "rigid_pose"
    a, b = np.asarray(host(rest_vertices), np.float64), np.asarray(host(moved_vertices), np.float64)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape != b.shape or a.shape[0] < 3:
        raise ValueError("%s: rest_vertices and moved_vertices must both be [Vm,3] with Vm >= 3; got %s and %s" % (who, tuple(a.shape), tuple(b.shape)))
    tolerance = _number(who, "tolerance", tolerance, lambda x: x >= 0.0, "; a finite number >= 0")
    if not np.isfinite(a).all() or not np.isfinite(b).all():
        raise ValueError("%s: the vertices must be finite" % who)
    ca, cb = a.mean(axis=0), b.mean(axis=0)
    U, _, Vt = np.linalg.svd((b - cb).T @ (a - ca))
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U @ Vt) > 0.0 else -1.0])
    R = U @ D @ Vt
    t = cb - R @ ca
    residual = float(np.linalg.norm(a @ R.T + t - b, axis=1).max())
    if not residual <= tolerance:
        raise ValueError("%s: the meshes differ by more than a rigid motion: residual %.3g > tolerance %.3g" % (who, residual, tolerance))
    return np.concatenate([R, t[:, None]], axis=1)


def rigid_poses(rest_vertices, moved_vertices, tolerance=1e-5):
    """rigid_pose for every mesh of a sequence: moved_vertices [T,Vm,3] -> float64 [T,3,4]; ValueError names the first frame refused"""
    m = host(moved_vertices)
    if m.ndim != 3:
        raise ValueError("rigid_poses: moved_vertices must be [T,Vm,3]; got %s" % (tuple(m.shape),))
    out = np.zeros((m.shape[0], 3, 4))
    for k in range(m.shape[0]):
        try:
            out[k] = rigid_pose(rest_vertices, m[k], tolerance)
        except ValueError as e:
            raise ValueError("rigid_poses: frame %d: %s" % (k, e)) from None
    return out


class SdfGrid:
    """A signed-distance volume prepared for contact (gm_sdf_grid_prepare, INTEGRATION.md section AC).  values: any float32 [nz,ny,nx]
    tensor of signed distances, sample (ix, iy, iz) at origin + (i + 0.5) voxel, negative inside the solid, NaN where nothing is known;
    weight (optional, the same shape): samples with weight < min_weight are unknown too; scale multiplies every value (a TSDF stores
    distance / trunc).  .grid is the prepared float32 [nz,ny,nx,4] tensor (phi, gx, gy, gz) - the gradient over every sample's known
    neighbours - with four NaNs on unknown samples; values and weight are not kept.  Only enqueues; nothing waits for the device.
    ValueError for shapes, fewer than 2 or more than 2^28 samples, a non-finite origin, voxel or scale, a voxel <= 0, a weight of
    another shape; GmeshError without a device."""

    def __init__(self, values, origin, voxel, weight=None, min_weight=1, scale=1.0, device="cuda"):
        who = "SdfGrid"
        if not hasattr(values, "shape") or len(values.shape) != 3:
            raise ValueError("%s: values must be [nz,ny,nx]; got %s" % (who, tuple(getattr(values, "shape", ()))))
        nz, ny, nx = (int(n) for n in values.shape)
        if min(nx, ny, nz) < 2 or nx * ny * nz > 1 << 28:
            raise ValueError("%s: a grid of %d x %d x %d samples (every side at least 2, at most 2^28 in all)" % (who, nx, ny, nz))
        if weight is not None and (not hasattr(weight, "shape") or tuple(weight.shape) != (nz, ny, nx)):
            raise ValueError("%s: weight must be [%d,%d,%d] as values are; got %s" % (who, nz, ny, nx, tuple(getattr(weight, "shape", ()))))
        o = np.asarray(host(origin), np.float64).reshape(-1)
        if o.shape != (3,) or not np.isfinite(o.astype(np.float32)).all():
            raise ValueError("%s: origin must be three finite numbers; got %r" % (who, origin))
        for name, val in (("voxel", voxel), ("scale", scale), ("min_weight", min_weight)):
            _number(who, name, val, lambda x: np.isfinite(np.float32(x)), "; a finite number")      # finite as the float32 it is stored as
        if not float(np.float32(voxel)) > 0.0:
            raise ValueError("%s: voxel = %r; positive" % (who, voxel))
        self.device = torch.device(device)
        need_cuda(self.device, who, "a grid")
        self.nx, self.ny, self.nz = nx, ny, nz
        self.origin = o.astype(np.float32)
        self.voxel, self.scale, self.min_weight = float(np.float32(voxel)), float(np.float32(scale)), float(np.float32(min_weight))
        self._origin_c = (ctypes.c_float * 3)(*self.origin.tolist())
        v = on_device(values, torch.float32, self.device)
        w = None if weight is None else on_device(weight, torch.float32, self.device)
        self.device = v.device
        self.grid = torch.empty((nz, ny, nx, 4), dtype=torch.float32, device=self.device)
        enqueue(self.device, "gm_sdf_grid_prepare", nx, ny, nz, v, w, self.min_weight, self.scale, self.voxel, self.grid)

    @classmethod
    def from_tsdf(cls, volume, min_weight=1, use_fill=True):
        """The grid of a proxy_mesh.TsdfVolume: its filled pair (fill_holes) when it has one and use_fill, else tsdf / weight; samples
        fewer than min_weight views observed are unknown; the scale is the volume's truncation distance."""
        filled = use_fill and getattr(volume, "filled_tsdf", None) is not None
        values, weight = (volume.filled_tsdf, volume.filled_weight) if filled else (volume.tsdf, volume.weight)
        return cls(values, volume.origin, volume.voxel, weight=weight, min_weight=min_weight, scale=volume.trunc, device=values.device)

    @classmethod
    def from_mesh(cls, vertices, faces, resolution=128, bounds=None, margin=0.5, device="cuda"):
        """The grid of a triangle mesh as a solid obstacle (mesh_sdf.grid_values: the distance to the closest face, negative where the
        generalized winding number says inside - open and inward-wound meshes welcome; INTEGRATION.md section AD).  bounds = (min, max),
        by default the mesh's box grown on every side by margin times its longest side; `resolution` voxels along the bounds' longest
        side (SceneVisualTool.background_field's rules).  Every sample is known.  Reads the mesh on the host (its box, its face
        indices).  ValueError for what mesh_sdf.grid_values and mesh_sdf.box_lattice refuse; GmeshError without a device."""
        from .mesh_bind import mesh_arrays
        from .mesh_sdf import box_lattice, grid_values
        who = "SdfGrid.from_mesh"
        v, f = mesh_arrays(vertices, faces, who)
        if f.shape[0] == 0 or v.shape[0] == 0:
            raise ValueError("%s: the mesh is empty (%d vertices, %d faces)" % (who, v.shape[0], f.shape[0]))
        v = np.asarray(v, np.float32)
        if not np.isfinite(v).all():
            raise ValueError("%s: the vertices must be finite" % who)
        origin, voxel, shape = box_lattice(who, v.min(axis=0), v.max(axis=0), resolution, bounds, margin)
        need_cuda(torch.device(device), who, "a grid")
        return cls(grid_values(v, f, origin, voxel, shape, device=device), origin, voxel, device=device)

    def sample(self, points):
        """(phi float64 [N], normal float64 [N,3]) of points [N,3] (read as float32), on the device: the distance and unit normal the
        contact step sees (gm_sdf_grid_sample); NaN outside the grid, next to an unknown sample and where the gradient has no direction"""
        who = "SdfGrid.sample"
        if not hasattr(points, "shape") or len(points.shape) != 2 or points.shape[1] != 3:
            raise ValueError("%s: points must be [N,3]; got %s" % (who, tuple(getattr(points, "shape", ()))))
        p = on_device(points, torch.float32, self.device)
        N = int(p.shape[0])
        phi = torch.empty((N,), dtype=torch.float64, device=self.device)
        normal = torch.empty((N, 3), dtype=torch.float64, device=self.device)
        if N:
            enqueue(self.device, "gm_sdf_grid_sample", N, p, self.nx, self.ny, self.nz, self._origin_c, self.voxel, self.grid, phi, normal)
        return phi, normal


class MeshDynamics:
    """The motion of one mesh under scripted handles, pins, gravity and its own elasticity.  Built once: the mesh's MeshGraph (given as
    rest_vertices with faces=None, it is shared), the masses, the masks, and on a device the state (float32 [Vm,3] each) and the workspace.
    rest_vertices [Vm,3], faces [F,3] vertex ids.  pinned: vertex ids held where they are; handles: H distinct vertex ids whose
    positions every step scripts (run's handle_targets); neither: a free body.  Vertices whose weights sum to 0 (unreferenced, or every
    face at them degenerate) are held too.  mass: "area" (vertex_masses(rest_vertices, faces, density)) or [Vm] numbers, positive on
    every vertex that has an edge.  A step minimises sum_i mass_i / (2 dt^2) |X_i - y_i|^2 + (stiffness / 2) E_arap(X) by `iterations`
    local/global iterations from the prediction y = x + dt v + dt^2 gravity, each global step at most cg_iterations CG steps to the
    relative residual cg_tolerance; the new velocity is (1 - damping)(X - x) / dt (held rows: (X - x) / dt, so a dragged handle carries
    its own velocity and a later release keeps its momentum).
    The defaults stiffness = 10 and damping = 0.02 are unmeasured starting values (a torus of unit size swings visibly and comes to rest
    within a few seconds at dt = 1 / 30); cg_iterations = 64 and cg_tolerance = 1e-6 are ArapSolver.solve's.
    ValueError for shapes, ids out of range or given twice, a handle that is also pinned, a mass that is not finite or not positive
    where it counts, and parameters outside their ranges (dt, stiffness > 0, damping in [0, 1), iterations, cg_iterations >= 1,
    cg_tolerance >= 0, all finite).
    colliders: up to GM_MESH_CONTACT_COLLIDERS_MAX (16) of half_space() / floor() / sphere() (or their tuples, lists or dicts): what the
    free rows cannot enter (gm_mesh_dynamics_contact, INTEGRATION.md section AB).  A free row that is inside a collider at an iterate is
    pushed to its surface with the stiffness contact_stiffness x mass_i and held back tangentially, towards where it was at the step's
    start, by at most the collider's friction times the normal push; a body at rest on a floor sinks in by about |gravity| /
    contact_stiffness.  Handle and pinned rows never take part.  Friction is measured in the world frame: give a moving pusher
    friction 0.  The default contact_stiffness = 1e4 is an unmeasured starting value (a unit-size object under |g| = 9.8 rests about 1e-3
    deep).  With no colliders every call goes through gm_mesh_dynamics, exactly as without these two arguments.  ValueError for a zero or
    non-finite normal, a radius <= 0, a negative friction, more than 16 colliders, a contact_stiffness that is not finite and positive.
    field: an SdfGrid on this object's device, or None: one more collider, static, the sampled volume (gm_mesh_dynamics_field,
    INTEGRATION.md section AC) with the friction field_friction.  It is candidate K behind the K analytic colliders: a tie goes to the
    analytic one, want_contacts reports 1 + K, and a row outside the grid, next to an unknown sample or on a zero gradient is not in
    contact with it.  With field=None every call goes where it went without the argument.  ValueError for a field that is no SdfGrid or
    lives on another device, a field_friction that is negative or not finite.
    fields: up to GM_MESH_FIELDS_MAX (4) SdfGrids on this object's device, each an obstacle that MOVES rigidly on its own
    (gm_mesh_dynamics_fields, INTEGRATION.md section AG), with field_frictions (one number each; None: all 0).  Field f is candidate
    K + f, want_contacts reports 1 + K + f, and every field has a pose (R | t), world = R local + t, that run's and step's field_poses
    move; the object keeps each field's last pose (the identity at first, reset(field_poses=) sets it).  Friction acts in the
    obstacle's frame: a row is held back towards the point of the obstacle it touched at the step's start, so a rough plate carries
    what lies on it.  Not together with field=, which keeps its own entry; an empty list is no fields at all.  ValueError for what
    field= refuses of each grid, more than 4, field_frictions of another length, both field= and fields=."""

    def __init__(self, rest_vertices, faces, pinned=(), handles=(), mass="area", density=1.0, stiffness=10.0, damping=0.02, gravity=(0.0, 0.0, 0.0),
                 dt=1.0 / 30.0, iterations=3, cg_iterations=64, cg_tolerance=1e-6, device="cuda", colliders=(), contact_stiffness=1.0e4, field=None,
                 field_friction=0.0, fields=None, field_frictions=None):
        who = "MeshDynamics"
        table = collider_table(colliders, who)
        if field is not None and not isinstance(field, SdfGrid):
            raise ValueError("%s: field must be an SdfGrid or None; got %r" % (who, type(field).__name__))
        field_friction = _friction(who, field_friction)
        kc = _number(who, "contact_stiffness", contact_stiffness, lambda x: x > 0.0, "; finite and positive")
        mesh = self.mesh = MeshGraph.of(rest_vertices, faces, device, who)
        self.device, Vm = mesh.device, mesh.Vm
        if field is not None and (self.device.type != "cuda" or field.device != (self.device if self.device.index is not None
                                                                                 else torch.device("cuda", torch.cuda.current_device()))):
            raise ValueError("%s: the field is on %s, the mesh on %s" % (who, field.device, self.device))
        self.field, self.field_friction = field, field_friction
        if fields is not None and (isinstance(fields, SdfGrid) or not isinstance(fields, (tuple, list))):
            raise ValueError("%s: fields must be a sequence of SdfGrids; got %r" % (who, type(fields).__name__))
        fields = () if fields is None else tuple(fields)
        if fields and field is not None:
            raise ValueError("%s: give field= or fields=, not both" % who)
        if len(fields) > _lib.GM_MESH_FIELDS_MAX:
            raise ValueError("%s: %d fields; at most %d" % (who, len(fields), _lib.GM_MESH_FIELDS_MAX))
        if field_frictions is None:
            field_frictions = (0.0,) * len(fields)
        if not isinstance(field_frictions, (tuple, list, np.ndarray)) or len(field_frictions) != len(fields):
            raise ValueError("%s: field_frictions must hold one number per field (%d); got %r" % (who, len(fields), field_frictions))
        field_frictions = tuple(_friction(who, mu) for mu in field_frictions)
        here = self.device if self.device.index is not None or self.device.type != "cuda" else torch.device("cuda", torch.cuda.current_device())
        for f in fields:
            if not isinstance(f, SdfGrid):
                raise ValueError("%s: fields must hold SdfGrids; got %r" % (who, type(f).__name__))
            if self.device.type != "cuda" or f.device != here:
                raise ValueError("%s: a field is on %s, the mesh on %s" % (who, f.device, self.device))
        self.fields, self.field_frictions, self.NF = fields, field_frictions, len(fields)
        self._table = (_lib.DynamicsField * max(self.NF, 1))(*[
            _lib.DynamicsField(f.nx, f.ny, f.nz, (ctypes.c_float * 3)(*f.origin.tolist()), f.voxel, f.grid.data_ptr(), mu) for f, mu in zip(fields, field_frictions)])
        self._poses = None
        if isinstance(mass, str):
            if mass != "area":
                raise ValueError('%s: mass must be "area" or [Vm] numbers; got %r' % (who, mass))
            m = vertex_masses(mesh.rest_host, mesh.faces_host, density)
        else:
            m = np.asarray(host(mass), np.float64).reshape(-1)
            if m.shape != (Vm,):
                raise ValueError("%s: mass must hold %d numbers; got %d" % (who, Vm, m.size))
        if not np.isfinite(m).all() or bool((m[~mesh.edgeless] <= 0.0).any()) or bool((m < 0.0).any()):
            raise ValueError("%s: every mass must be finite and positive (negative nowhere, zero only at a vertex without an edge)" % who)
        g = np.asarray(host(gravity), np.float64).reshape(-1)
        if g.shape != (3,) or not np.isfinite(g).all():
            raise ValueError("%s: gravity must be three finite numbers; got %r" % (who, gravity))
        for name, val, ok in (("dt", dt, lambda x: x > 0.0), ("stiffness", stiffness, lambda x: x > 0.0), ("damping", damping, lambda x: 0.0 <= x < 1.0),
                              ("cg_tolerance", cg_tolerance, lambda x: x >= 0.0)):
            _number(who, name, val, ok, " (dt and stiffness positive, damping in [0, 1), cg_tolerance not negative, all finite)")
        for name, val in (("iterations", iterations), ("cg_iterations", cg_iterations)):
            if isinstance(val, bool) or not isinstance(val, (int, np.integer)) or val < 1:
                raise ValueError("%s: %s = %r; an integer >= 1" % (who, name, val))
        self.Vm, self.F, self.csr, self.mass = Vm, mesh.F, mesh.csr, m
        self.dt, self.stiffness, self.damping, self.gravity = float(dt), float(stiffness), float(damping), tuple(float(x) for x in g)
        self.iterations, self.cg_iterations, self.cg_tolerance = int(iterations), int(cg_iterations), float(cg_tolerance)
        self.K, self.contact_stiffness = len(table[0]), kc
        self.collider_kinds, self.collider_rows, self.collider_friction = table
        self._x = self._v = self._ws = None
        if self.device.type == "cuda":
            self.rest, self._off, self._cols, self._w = mesh.device_csr
            self._mass = on_device(m, torch.float64, self.device)
            if self.K:
                self._kinds = on_device(self.collider_kinds, torch.int32, self.device)
                self._rows = on_device(self.collider_rows, torch.float32, self.device)
                self._mus = on_device(self.collider_friction, torch.float64, self.device)
        self.set_constraints(pinned, handles)
        if self.device.type == "cuda":
            self.reset()

    def set_constraints(self, pinned=(), handles=()):
        """Replace the pins and the handles; the state (positions, velocities) stays, so dropping a handle RELEASES it with the velocity
        its drag gave it.  ValueError for an id out of range or given twice among the handles, and for a handle that is also pinned."""
        who = "MeshDynamics.set_constraints"
        p = self.mesh.vertex_ids(pinned, who, "pinned", allow_empty=True, distinct=False)
        h = self.mesh.vertex_ids(handles, who, "handle", allow_empty=True)
        both = np.intersect1d(p, h)
        if len(both):
            raise ValueError("%s: vertex %d is both a handle and pinned" % (who, int(both[0])))
        held = self.mesh.edgeless.copy()
        held[p] = True
        held[h] = True
        self.pinned, self.handles, self.held = np.unique(p), h, held
        if self.device.type == "cuda":
            self._held = on_device(held.astype(np.uint8), torch.uint8, self.device)
            self._handle_ids = on_device(h.astype(np.int32), torch.int32, self.device) if len(h) else None

    def _poses_arg(self, who, poses, lead):
        """field_poses of shape lead + [F,3,4] as a float64 tensor on the device: a device tensor as it is, a host array checked"""
        if self.NF == 0:
            raise ValueError("%s: field_poses given, but there are no fields" % who)
        poses = poses if hasattr(poses, "shape") else np.asarray(poses, np.float64)
        if tuple(poses.shape) != tuple(lead) + (self.NF, 3, 4):
            raise ValueError("%s: field_poses must be [%s]; got %s" % (who, ",".join(str(n) for n in tuple(lead) + (self.NF, 3, 4)), tuple(poses.shape)))
        if not (torch.is_tensor(poses) and poses.device.type == "cuda"):
            poses = _check_poses(who, host(poses))
        return poses

    def reset(self, positions=None, velocities=None, field_poses=None):
        """Set the state: positions [Vm,3] (None: the rest pose), velocities [Vm,3] (None: zero), field_poses [F,3,4] (None: every
        field at the identity - where its grid was sampled); all are copied."""
        who = "MeshDynamics.reset"
        if field_poses is not None:
            field_poses = self._poses_arg(who, field_poses, ())
        if positions is not None and (not hasattr(positions, "shape") or tuple(positions.shape) != (self.Vm, 3)):
            raise ValueError("%s: positions must be [%d,3]; got %s" % (who, self.Vm, tuple(getattr(positions, "shape", ()))))
        if velocities is not None and (not hasattr(velocities, "shape") or tuple(velocities.shape) != (self.Vm, 3)):
            raise ValueError("%s: velocities must be [%d,3]; got %s" % (who, self.Vm, tuple(getattr(velocities, "shape", ()))))
        self.mesh.need_device(who)
        self._x = self.rest.clone() if positions is None else self.mesh.rows_f32(positions, who, "positions", copy=True)
        self._v = torch.zeros_like(self.rest) if velocities is None else self.mesh.rows_f32(velocities, who, "velocities", copy=True)
        if self.NF:
            eye = np.tile(np.eye(3, 4), (self.NF, 1, 1)) if field_poses is None else field_poses
            self._poses = on_device(eye, torch.float64, self.rest.device).clone()

    @property
    def field_poses(self):
        """every field's pose at the state's time, float64 [F,3,4] on the device (a copy)"""
        self.mesh.need_device("MeshDynamics.field_poses")
        return None if self._poses is None else self._poses.clone()

    @property
    def positions(self):
        """the state's positions, float32 [Vm,3] on the device (a copy)"""
        self.mesh.need_device("MeshDynamics.positions")
        return self._x.clone()

    @property
    def velocities(self):
        """the state's velocities, float32 [Vm,3] on the device (a copy)"""
        self.mesh.need_device("MeshDynamics.velocities")
        return self._v.clone()

    def step(self, handle_targets=None, collider_rows=None, field_poses=None):
        """One step: the new positions [Vm,3]; handle_targets [H,3] (in the order of `handles`) exactly when there are handles;
        collider_rows [K,4]: where the colliders are in this step (None: where they were built); field_poses [F,3,4]: where the
        fields are during this step (None: where they were).
        run(1, handle_targets[None], collider_rows[None], field_poses=field_poses[None])[0]."""
        def one_step(a, name, n, width):
            if a is None:
                return None
            a = _shaped(a)
            if len(a.shape) != 2:
                raise ValueError("MeshDynamics.step: %s must be [%d,%d]; got %s" % (name, n, width, tuple(a.shape)))
            return a[None]
        collider_rows = one_step(collider_rows, "collider_rows", self.K, 4)
        if field_poses is not None:
            field_poses = field_poses if hasattr(field_poses, "shape") else np.asarray(field_poses, np.float64)
            if len(field_poses.shape) != 3:
                raise ValueError("MeshDynamics.step: field_poses must be [%d,3,4]; got %s" % (self.NF, tuple(field_poses.shape)))
            field_poses = field_poses[None]
        return self.run(1, one_step(handle_targets, "handle_targets", len(self.handles), 3), collider_rows=collider_rows, field_poses=field_poses)[0]

    def run(self, steps, handle_targets=None, out=None, want_stats=False, collider_rows=None, want_contacts=False, field_poses=None):
        """`steps` steps from the state, which they advance: the positions after every step, [steps,Vm,3] float32 on the device.
        handle_targets [steps,H,3]: where the handles are in every step - required exactly when there are handles.  Cut into launch
        chains of at most GM_MESH_DYNAMICS_STEPS_MAX (64) steps; the state is rounded to float32 at every step boundary, so run(n) is
        bit for bit n calls of step().  out: a contiguous float32 [steps,Vm,3] tensor on the device.  With want_stats returns (meshes,
        stats float64 [steps,6]): CG steps used for x / y / z and final |r| / |b| for x / y / z in each step's last iteration.
        collider_rows [steps,K,4] float32: the colliders' rows in every step ((nx, ny, nz, d) with a unit normal / (cx, cy, cz, r)), which
        is how they move; a tensor on the device is taken as it is, a host array is checked (finite, normals of unit length within 1e-4,
        radii positive); None: the rows they were built with, in every step.  want_contacts: also int32 [steps,Vm], 1 + the index of the
        collider every row was in contact with in the step's last iteration, 0 elsewhere; returned after the meshes (and before stats).
        field_poses [steps,F,3,4] float64: every field's pose (R | t) DURING each step, world = R local + t, which is how the obstacles
        move; the pose before the first step is the one the object kept (the last step's of the call before, the identity at first,
        reset's), and the last one given is kept for the next call, so run(n) stays n calls of step().  A tensor on the device is taken
        as it is, a host array is checked (finite, |R^T R - I| <= 1e-6, det R > 0); None: every field stays where it is.
        Stream-ordered; nothing here waits for the device (reading stats does).  ValueError for steps < 1, shapes, handle_targets without
        handles and handles without handle_targets, collider_rows without colliders, field_poses without fields; GmeshError without a
        device."""
        who = "MeshDynamics.run"
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 1:
            raise ValueError("%s: steps = %r; an integer >= 1" % (who, steps))
        T, Vm, H = int(steps), self.Vm, len(self.handles)
        if H == 0 and handle_targets is not None:
            raise ValueError("%s: handle_targets given, but there are no handles" % who)
        if H > 0 and handle_targets is None:
            raise ValueError("%s: there are %d handles; handle_targets [%d,%d,3] says where they are in every step" % (who, H, T, H))
        if handle_targets is not None:
            handle_targets = _shaped(handle_targets)
            if tuple(handle_targets.shape) != (T, H, 3):
                raise ValueError("%s: handle_targets must be [%d,%d,3]; got %s" % (who, T, H, tuple(handle_targets.shape)))
        K, field = self.K, self.field
        if collider_rows is not None:
            if K == 0:
                raise ValueError("%s: collider_rows given, but there are no colliders" % who)
            collider_rows = _shaped(collider_rows)
            if tuple(collider_rows.shape) != (T, K, 4):
                raise ValueError("%s: collider_rows must be [%d,%d,4]; got %s" % (who, T, K, tuple(collider_rows.shape)))
            if not torch.is_tensor(collider_rows):
                r = np.asarray(collider_rows, np.float64)
                flat = self.collider_kinds == HALF_SPACE
                if not np.isfinite(r).all() or bool((np.abs(np.linalg.norm(r[:, flat, :3], axis=2) - 1.0) > 1e-4).any()) or bool((r[:, ~flat, 3] <= 0.0).any()):
                    raise ValueError("%s: collider_rows must be finite, a half-space's normal of unit length, a sphere's radius positive" % who)
        F = self.NF
        if field_poses is not None:
            field_poses = self._poses_arg(who, field_poses, (T,))
        self.mesh.need_device(who)
        dev = self.rest.device
        if F:                                                          # row 0: the poses kept; row t + 1: step t's
            moving = field_poses is not None
            table = torch.cat([self._poses[None], on_device(field_poses, torch.float64, dev) if moving else self._poses[None].expand(T, F, 3, 4)], 0)
        hp = None if handle_targets is None else on_device(handle_targets, torch.float32, dev)
        out = self.mesh.out_f32(out, (T, Vm, 3), who)
        stats = torch.zeros((T, 6), dtype=torch.float64, device=dev) if want_stats else None
        plain = K == 0 and field is None and F == 0                               # exactly the call there was before there were colliders
        contacts = None
        if want_contacts:
            contacts = (torch.zeros if plain else torch.empty)((T, Vm), dtype=torch.int32, device=dev)
        entry = "gm_mesh_dynamics_fields" if F else "gm_mesh_dynamics_field" if field is not None else "gm_mesh_dynamics" if K == 0 else "gm_mesh_dynamics_contact"
        if self._ws is None:
            need = getattr(_lib.lib(), ("gm_mesh_dynamics" if plain else "gm_mesh_dynamics_contact") + "_workspace_bytes")(Vm)
            self._ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        top = _lib.GM_MESH_DYNAMICS_STEPS_MAX
        if K > 0:
            cp = self._rows.unsqueeze(0).expand(min(T, top), K, 4).contiguous() if collider_rows is None else on_device(collider_rows, torch.float32, dev)
        g = self.gravity
        fld = () if field is None else (field.nx, field.ny, field.nz, field._origin_c, field.voxel, field.grid, self.field_friction)
        for s in range(0, T, top):
            e = min(s + top, T)
            part = lambda a: None if a is None else a[s:e]              # this chain's steps of a per-step array
            state = (e - s, Vm, self._off, self._cols, self._w, self.rest, self._mass, self._held, H, self._handle_ids, part(hp),
                     self._x if s == 0 else out[s - 1], self._v, self.dt, self.stiffness, self.damping, g[0], g[1], g[2], self.iterations,
                     self.cg_iterations, self.cg_tolerance)
            if plain:
                col = ()
            elif K == 0:
                col = (0, None, None, None, self.contact_stiffness)
            else:
                col = (K, self._kinds, cp[:e - s] if collider_rows is None else cp[s:e], self._mus, self.contact_stiffness)
            outs = (out[s:e], self._v) + (() if plain else (part(contacts),)) + (part(stats),)
            if F:
                fld = (F, self._table, table[s:e + 1])
            enqueue(dev, entry, *state, *col, *fld, *outs, workspace=self._ws)
        self._x.copy_(out[T - 1])
        if F and moving:
            self._poses.copy_(table[T])
        got = (out,) + ((contacts,) if want_contacts else ()) + ((stats,) if want_stats else ())
        return got if len(got) > 1 else out
