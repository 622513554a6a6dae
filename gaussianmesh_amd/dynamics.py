"""Secondary motion of a proxy mesh: implicit-Euler steps of an elastic mesh whose potential is the ARAP energy, on the device
(gm_mesh_dynamics, csrc/gm_dynamics.hip).  ArapSolver, PoseInterpolator and PoseFitter give static equilibria; here the mesh has
velocity: a dragged limb follows through, a released handle swings back, an object sags under its weight and settles.  A step is the
local/global iteration of projective dynamics (Bouaziz et al. 2014) with Sorkine & Alexa's vertex-star energy as the constraint set: the
local step is ArapSolver's, the global step's matrix gains the positive diagonal mass_i / (2 stiffness dt^2), so the system is positive
definite with no held row at all - a free body is a valid input, which ArapSolver cannot express.  The result is a [steps,Vm,3] stack of
meshes: what render_sequence, SingleObjectDeform.deform_vertices and edit_sequence --save_meshes take.  Definition, ABI and rules:
INTEGRATION.md section AA."""
import numpy as np
import torch

from . import _lib
from ._op import enqueue, host, on_device
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
    cg_tolerance >= 0, all finite)."""

    def __init__(self, rest_vertices, faces, pinned=(), handles=(), mass="area", density=1.0, stiffness=10.0, damping=0.02, gravity=(0.0, 0.0, 0.0),
                 dt=1.0 / 30.0, iterations=3, cg_iterations=64, cg_tolerance=1e-6, device="cuda"):
        who = "MeshDynamics"
        mesh = self.mesh = MeshGraph.of(rest_vertices, faces, device, who)
        self.device, Vm = mesh.device, mesh.Vm
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
            if isinstance(val, bool) or not isinstance(val, (int, float, np.integer, np.floating)) or not np.isfinite(val) or not ok(float(val)):
                raise ValueError("%s: %s = %r (dt and stiffness positive, damping in [0, 1), cg_tolerance not negative, all finite)" % (who, name, val))
        for name, val in (("iterations", iterations), ("cg_iterations", cg_iterations)):
            if isinstance(val, bool) or not isinstance(val, (int, np.integer)) or val < 1:
                raise ValueError("%s: %s = %r; an integer >= 1" % (who, name, val))
        self.Vm, self.F, self.csr, self.mass = Vm, mesh.F, mesh.csr, m
        self.dt, self.stiffness, self.damping, self.gravity = float(dt), float(stiffness), float(damping), tuple(float(x) for x in g)
        self.iterations, self.cg_iterations, self.cg_tolerance = int(iterations), int(cg_iterations), float(cg_tolerance)
        self._x = self._v = self._ws = None
        if self.device.type == "cuda":
            self.rest, self._off, self._cols, self._w = mesh.device_csr
            self._mass = on_device(m, torch.float64, self.device)
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

    def reset(self, positions=None, velocities=None):
        """Set the state: positions [Vm,3] (None: the rest pose), velocities [Vm,3] (None: zero); both are copied."""
        who = "MeshDynamics.reset"
        if positions is not None and (not hasattr(positions, "shape") or tuple(positions.shape) != (self.Vm, 3)):
            raise ValueError("%s: positions must be [%d,3]; got %s" % (who, self.Vm, tuple(getattr(positions, "shape", ()))))
        if velocities is not None and (not hasattr(velocities, "shape") or tuple(velocities.shape) != (self.Vm, 3)):
            raise ValueError("%s: velocities must be [%d,3]; got %s" % (who, self.Vm, tuple(getattr(velocities, "shape", ()))))
        self.mesh.need_device(who)
        self._x = self.rest.clone() if positions is None else self.mesh.rows_f32(positions, who, "positions", copy=True)
        self._v = torch.zeros_like(self.rest) if velocities is None else self.mesh.rows_f32(velocities, who, "velocities", copy=True)

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

    def step(self, handle_targets=None):
        """One step: the new positions [Vm,3]; handle_targets [H,3] (in the order of `handles`) exactly when there are handles.
        run(1, handle_targets[None])[0]."""
        if handle_targets is not None:
            if not hasattr(handle_targets, "shape"):
                handle_targets = np.asarray(handle_targets, np.float32)
            if len(handle_targets.shape) != 2:
                raise ValueError("MeshDynamics.step: handle_targets must be [%d,3]; got %s" % (len(self.handles), tuple(handle_targets.shape)))
            handle_targets = handle_targets[None]
        return self.run(1, handle_targets)[0]

    def run(self, steps, handle_targets=None, out=None, want_stats=False):
        """`steps` steps from the state, which they advance: the positions after every step, [steps,Vm,3] float32 on the device.
        handle_targets [steps,H,3]: where the handles are in every step - required exactly when there are handles.  Cut into launch
        chains of at most GM_MESH_DYNAMICS_STEPS_MAX (64) steps; the state is rounded to float32 at every step boundary, so run(n) is
        bit for bit n calls of step().  out: a contiguous float32 [steps,Vm,3] tensor on the device.  With want_stats returns (meshes,
        stats float64 [steps,6]): CG steps used for x / y / z and final |r| / |b| for x / y / z in each step's last iteration.
        Stream-ordered; nothing here waits for the device (reading stats does).  ValueError for steps < 1, shapes, handle_targets without
        handles and handles without handle_targets; GmeshError without a device."""
        who = "MeshDynamics.run"
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 1:
            raise ValueError("%s: steps = %r; an integer >= 1" % (who, steps))
        T, Vm, H = int(steps), self.Vm, len(self.handles)
        if H == 0 and handle_targets is not None:
            raise ValueError("%s: handle_targets given, but there are no handles" % who)
        if H > 0 and handle_targets is None:
            raise ValueError("%s: there are %d handles; handle_targets [%d,%d,3] says where they are in every step" % (who, H, T, H))
        if handle_targets is not None:
            if not hasattr(handle_targets, "shape"):
                handle_targets = np.asarray(handle_targets, np.float32)
            if tuple(handle_targets.shape) != (T, H, 3):
                raise ValueError("%s: handle_targets must be [%d,%d,3]; got %s" % (who, T, H, tuple(handle_targets.shape)))
        self.mesh.need_device(who)
        dev = self.rest.device
        hp = None
        if handle_targets is not None:
            hp = on_device(handle_targets, torch.float32, dev)
        out = self.mesh.out_f32(out, (T, Vm, 3), who)
        stats = torch.zeros((T, 6), dtype=torch.float64, device=dev) if want_stats else None
        if self._ws is None:
            need = _lib.lib().gm_mesh_dynamics_workspace_bytes(Vm)
            self._ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        top = _lib.GM_MESH_DYNAMICS_STEPS_MAX
        g = self.gravity
        for s in range(0, T, top):
            e = min(s + top, T)
            enqueue(dev, "gm_mesh_dynamics", e - s, Vm, self._off, self._cols, self._w, self.rest, self._mass, self._held, H, self._handle_ids,
                    None if hp is None else hp[s:e], self._x if s == 0 else out[s - 1], self._v, self.dt, self.stiffness, self.damping, g[0], g[1], g[2],
                    self.iterations, self.cg_iterations, self.cg_tolerance, out[s:e], self._v, None if stats is None else stats[s:e],
                    workspace=self._ws)
        self._x.copy_(out[T - 1])
        return (out, stats) if want_stats else out
