"""Deform a proxy mesh from dragged handle vertices: as-rigid-as-possible (Sorkine & Alexa 2007) on the device (gm_arap_solve,
csrc/gm_arap.hip).  The stage the reference leaves to an external binary: "move these vertices there; the rest of the mesh follows as
rigidly as it can".  Its output is what deform.mesh_rs / SingleObjectDeform.deform_vertices / render_sequence take, so a handle drag is
solve -> gm_mesh_rs -> forward on one stream, with no host wait.  Definition, ABI and rules: INTEGRATION.md section Q.
ArapEnergy is the same energy as a function of a pose, with its gradient, and one-ring smoothing of per-vertex rows (gm_arap_energy_grad,
gm_mesh_smooth_rows): what pose_fit.PoseFitter takes as a rigidity term and for its gradient."""
import numpy as np
import torch

from . import _lib
from ._op import enqueue, need_cuda, on_device, workspace
from .mesh_graph import MeshGraph, components, edge_csr  # noqa: F401  (both re-exported: the tests and the other modules import them from here)


def sequence_runs(T, batch):
    """The runs of ArapSolver.solve_sequence: [(start, end)] covering frames 0 .. T - 1 in order, `batch` frames each, the last one
    possibly shorter; [] for T == 0.  Host arithmetic only."""
    T, batch = int(T), int(batch)
    if T < 0 or batch < 1:
        raise ValueError("sequence_runs: T >= 0 and batch >= 1; got T = %d, batch = %d" % (T, batch))
    return [(a, min(a + batch, T)) for a in range(0, T, batch)]


class _ArapEnergyFunction(torch.autograd.Function):
    """E(V1) / scale of an ArapEnergy as a node of the graph: forward keeps the device's gradient, backward scales it"""

    @staticmethod
    def forward(ctx, V1, energy):
        E, grad = energy.value_and_grad(V1)
        ctx.save_for_backward(grad)
        ctx.scale, ctx.dtype = energy.scale, V1.dtype
        return (E / energy.scale).to(V1.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return (grad_out.to(torch.float64) * grad / ctx.scale).to(ctx.dtype), None


class ArapEnergy:
    """The ARAP energy of a pose of one mesh as a function of the pose alone, with its gradient (gm_arap_energy_grad), and one-ring
    smoothing of per-vertex rows over the same edge graph (gm_mesh_smooth_rows): a rigidity term that sees bending, and the Sobolev
    gradient, for an optimiser of the vertices (pose_fit.PoseFitter).  Built once: the mesh's MeshGraph (given as rest_vertices with
    faces=None, it is shared), scale = sum_ij w_ij |p_i - p_j|^2 (E / scale does not depend on the mesh's units) and the workspaces.
        E(x) = sum_i sum_j w_ij |(x_i - x_j) - R_i (p_i - p_j)|^2, R_i the local step's rotation at x;  0 for a rigid motion of the rest pose
    ValueError for a mesh without an edge (scale = 0).  Definition, ABI and rules: INTEGRATION.md section Y."""

    def __init__(self, rest_vertices, faces, device="cuda"):
        g = self.mesh = MeshGraph.of(rest_vertices, faces, device, "ArapEnergy")
        self.device, self.Vm, self.csr = g.device, g.Vm, g.csr
        v = g.rest_host.astype(np.float64)
        e = v[g.rows] - v[g.csr[1]]
        self.scale = float((g.csr[2] * (e * e).sum(axis=1)).sum())
        if not self.scale > 0.0:
            raise ValueError("ArapEnergy: the mesh has no edge of positive length (scale = %g)" % self.scale)
        if self.device.type != "cuda":                                 # the set-up above is host work; every call needs the device
            return
        self.rest, self._off, self._cols, self._w = g.device_csr
        self._ws = workspace(self.device, "gm_arap_energy_workspace_bytes", self.Vm)
        self._smooth_ws = None                                         # made by the first smooth_rows

    def _pose(self, V1, who):
        self.mesh.need_device(who)
        need_cuda(V1, who, "V1")
        return self.mesh.rows_f32(V1, who, "V1")

    def value_and_grad(self, V1, want_grad=True):
        """(E float64 0-dim, dE/dV1 float64 [Vm,3]) of the pose V1 [Vm,3] (read as float32), on the device; want_grad=False: (E, None),
        the same bits of E.  Stream-ordered, nothing here waits for the device; two identical calls give identical bits."""
        v1 = self._pose(V1, "ArapEnergy.value_and_grad")
        E = torch.empty((), dtype=torch.float64, device=v1.device)
        grad = torch.empty((self.Vm, 3), dtype=torch.float64, device=v1.device) if want_grad else None
        enqueue(v1.device, "gm_arap_energy_grad", self.Vm, self._off, self._cols, self._w, self.rest, v1, E, grad, workspace=self._ws)
        return E, grad

    def __call__(self, V1):
        """E(V1) / scale: a 0-dim tensor of V1's dtype, differentiable in V1 once (a second derivative raises)"""
        self._pose(V1, "ArapEnergy")
        return _ArapEnergyFunction.apply(V1, self)

    def smooth_rows(self, rows, lam, sweeps):
        """`sweeps` Jacobi sweeps of (I + lam L) y = rows from y = rows, L the Laplacian of the edge weights: rows [Vm,3] float32 or
        float64 on the device, returned in the same dtype (a new tensor), the arithmetic in float64.  sweeps = 0 or lam = 0 return the
        rows; max |y| never grows and a constant field stays constant.  GmeshError for lam < 0, sweeps < 0 and a CPU tensor."""
        self.mesh.need_device("ArapEnergy.smooth_rows")
        need_cuda(rows, "ArapEnergy.smooth_rows", "rows")
        if rows.shape != (self.Vm, 3) or rows.dtype not in (torch.float32, torch.float64):
            raise ValueError("ArapEnergy.smooth_rows: rows must be float32 or float64 [%d,3]; got %s %s" % (self.Vm, rows.dtype, tuple(rows.shape)))
        dev = self.rest.device
        if self._smooth_ws is None:
            self._smooth_ws = workspace(dev, "gm_mesh_smooth_workspace_bytes", self.Vm)
        g = rows.detach().to(device=dev, dtype=torch.float64).contiguous()
        out = torch.empty((self.Vm, 3), dtype=torch.float64, device=dev)
        enqueue(dev, "gm_mesh_smooth_rows", self.Vm, self._off, self._cols, self._w, g, float(lam), int(sweeps), out, workspace=self._smooth_ws)
        return out.to(rows.dtype)


class ArapSolver:
    """As-rigid-as-possible deformation of one mesh from one set of handle vertices.  Built once: the mesh's MeshGraph (rest_vertices
    may be one, with faces=None: it is shared, not rebuilt), the mask of held rows (the handles, and PINNED vertices: those whose weights
    sum to 0 - unreferenced, or every face at them degenerate - which keep their `init` position), the device workspace.
    rest_vertices [Vm,3], faces [F,3] vertex ids, handles: H distinct vertex ids.  ValueError for a handle id out of range or given
    twice, an empty handle set, and a connected component of the weighted edge graph that has a free vertex but no handle (its
    positions would be undetermined: the linear system is singular)."""

    def __init__(self, rest_vertices, faces, handles, device="cuda"):
        g = self.mesh = MeshGraph.of(rest_vertices, faces, device, "ArapSolver")
        h = g.vertex_ids(handles, "ArapSolver", "handle")
        fixed = g.edgeless.copy()
        fixed[h] = True
        g.require_anchored(fixed, h, "ArapSolver", "handle")
        self.device, self.Vm, self.csr = g.device, g.Vm, g.csr
        self.handles, self.pinned = h, np.nonzero(g.edgeless)[0]
        if self.device.type != "cuda":                                 # the set-up above is host work; solve() needs the device
            return
        self.rest, self._off, self._cols, self._w = g.device_csr
        self._fixed = on_device(fixed.astype(np.uint8), torch.uint8, self.device)
        self._handle_idx = on_device(h, torch.int64, self.device)
        self._ws = workspace(self.device, "gm_arap_workspace_bytes", g.Vm)
        self._grid_ws = None                                           # the whole-chip global step's own workspace: made by its first solve
        self._batch_ws = {}                                            # global_step -> solve_batch's workspace, grown to the largest B seen

    def _begin(self, who, global_step, handle_positions):
        """the refusals every solve begins with, in their order, and the handle positions as float32 on the device"""
        if global_step not in ("column", "grid"):
            raise ValueError('%s: global_step must be "column" or "grid"; got %r' % (who, global_step))
        self.mesh.need_device(who)
        if torch.is_tensor(handle_positions):
            return handle_positions.detach().to(device=self.device, dtype=torch.float32)
        return torch.as_tensor(np.asarray(handle_positions), dtype=torch.float32, device=self.device)

    def _solve(self, who, lead, hp, init, out, outer_iterations, want_stats, launch):
        """What solve (lead = ()) and solve_batch (lead = (B,)) share once hp is checked: init and out are checked, the guess is made
        (out itself where out is init: in place) with the handle rows replaced, launch(guess, out, stats) enqueues, and the result is
        returned as the caller returns it."""
        Vm, dev, shape = self.Vm, self.device, lead + (self.Vm, 3)
        if init is not None:
            if not torch.is_tensor(init):
                init = torch.as_tensor(np.asarray(init), dtype=torch.float32, device=dev)
            if init.shape != (Vm, 3) and init.shape != shape:
                raise ValueError("%s: init must be [%d,3]%s; got %s" % (who, Vm, " or %s" % list(shape) if lead else "", tuple(init.shape)))
        if out is not None:
            self.mesh.out_f32(out, shape, who)
        if out is not None and out is init:
            guess = out                                                # in place
        else:
            start = self.rest if init is None else init.detach().to(device=dev, dtype=torch.float32)
            guess = start.expand(shape).clone(memory_format=torch.contiguous_format)
        guess.index_copy_(len(lead), self._handle_idx, hp)
        if out is None:
            out = guess
        outer = int(outer_iterations)
        stats = torch.zeros(lead + (max(outer, 0), 8), dtype=torch.float64, device=dev) if want_stats else None
        launch(guess, out, stats if outer > 0 else None)
        return (out, stats) if want_stats else out

    def solve(self, handle_positions, init=None, outer_iterations=4, cg_iterations=64, cg_tolerance=1e-6, out=None, want_stats=False,
              global_step="column"):
        """Positions [Vm,3] float32 on the device with the handles at handle_positions [H,3] (in the order of `handles`) and the rest of
        the mesh following as rigidly as it can.  init: the starting positions (None: the rest pose; the previous frame's solution
        warm-starts a drag); its handle rows are replaced by handle_positions (index_copy on the device).  out: where to write; it may
        be `init` itself (then init's handle rows are overwritten too).  With want_stats returns (vertices, stats): stats float64
        [outer_iterations, 8] on the device = E after the local step, E after the global step, CG steps used for x / y / z, final
        |r| / |b| for x / y / z.  Stream-ordered; nothing here waits for the device (reading stats does).  Two identical calls give
        identical bits.
        global_step: "column" (gm_arap_solve: one workgroup per coordinate runs the whole CG, no launch per step) or "grid"
        (gm_arap_solve_grid: rows over the whole chip, two launches per CG step; the same definition, sums in another order, so the
        last bits differ; its workspace is allocated by the first such solve and kept).  ValueError for any other value, before
        anything else is checked.  Which is faster at which size: INTEGRATION.md section Q.
        The defaults (4 outer iterations, at most 64 CG steps each, relative residual 1e-6) began as unmeasured starting values and
        were kept after tools/arap_time.py: 7.3 ms at 7.5 k vertices on an MI355X; from the rest pose the
        64-step cap binds before the tolerance, and four such outer iterations reach a lower energy than four with converged solves."""
        who = "ArapSolver.solve"
        hp = self._begin(who, global_step, handle_positions)
        if hp.shape != (len(self.handles), 3):
            raise ValueError("%s: handle_positions must be [%d,3]; got %s" % (who, len(self.handles), tuple(hp.shape)))

        def launch(guess, out, stats):
            if global_step == "grid":
                if self._grid_ws is None:
                    self._grid_ws = workspace(self.device, "gm_arap_grid_workspace_bytes", self.Vm)
                entry, ws = "gm_arap_solve_grid", self._grid_ws
            else:
                entry, ws = "gm_arap_solve", self._ws
            enqueue(self.device, entry, self.Vm, self._off, self._cols, self._w, self.rest, self._fixed, guess, int(outer_iterations),
                    int(cg_iterations), float(cg_tolerance), out, stats, workspace=ws)
        return self._solve(who, (), hp, init, out, outer_iterations, want_stats, launch)

    def solve_batch(self, handle_positions, init=None, outer_iterations=4, cg_iterations=64, cg_tolerance=1e-6, out=None, want_stats=False,
                    global_step="column"):
        """B solves of this mesh and handle set in ONE launch chain (gm_arap_solve_batch): handle_positions [B,H,3], B in
        1 .. GM_ARAP_BATCH_MAX (64).  Returns [B,Vm,3] float32 on the device, with want_stats also float64 [B,outer_iterations,8]; item
        b is bit for bit solve(handle_positions[b], init=init[b], ...) with the same options - every item stops on its own sums, and
        the chain has the launches of one single solve, whatever B.  init: None (the rest pose), one [Vm,3] start shared by all items,
        or [B,Vm,3]; out: where to write, which may be the [B,Vm,3] init itself.  The workspace of each global step is allocated by the
        first such call and grown to the largest B seen.  Stream-ordered; nothing here waits for the device.
        THE TRADE.  The items of a batch cannot start from one another: where a chain of solve() calls warm-starts frame t from frame
        t - 1, a batch starts all its frames from one mesh (solve_sequence: the last frame of the previous run), so a frame deep in
        a run starts farther from its answer and, at a fixed number of iterations, may end at a higher energy.  What that costs against
        the time saved: tools/arap_time.py --batch, INTEGRATION.md section Q.
        ValueError for a bad global_step first, then for shapes and B; GmeshError on a solver without a device."""
        who = "ArapSolver.solve_batch"
        hp = self._begin(who, global_step, handle_positions)
        if hp.dim() != 3 or hp.shape[1:] != (len(self.handles), 3):
            raise ValueError("%s: handle_positions must be [B,%d,3]; got %s" % (who, len(self.handles), tuple(hp.shape)))
        B = hp.shape[0]
        if not 1 <= B <= _lib.GM_ARAP_BATCH_MAX:
            raise ValueError("%s: B = %d; a batch holds 1 .. %d solves" % (who, B, _lib.GM_ARAP_BATCH_MAX))

        def launch(guess, out, stats):
            step = 1 if global_step == "grid" else 0
            need = _lib.lib().gm_arap_batch_workspace_bytes(self.Vm, B, step)
            ws = self._batch_ws.get(global_step)
            if ws is None or ws.numel() < need:
                ws = self._batch_ws[global_step] = torch.empty((need,), dtype=torch.uint8, device=self.device)
            enqueue(self.device, "gm_arap_solve_batch", B, step, self.Vm, self._off, self._cols, self._w, self.rest, self._fixed, guess,
                    int(outer_iterations), int(cg_iterations), float(cg_tolerance), out, stats, workspace=ws)
        return self._solve(who, (B,), hp, init, out, outer_iterations, want_stats, launch)

    def solve_sequence(self, positions, init=None, batch=4, **solve_options):
        """The meshes [T,Vm,3] of a drag whose frame t has the handles at positions[t] ([T,H,3]), `batch` frames per launch chain
        (sequence_runs; the last run may be shorter).  Every frame of a run starts from the LAST frame of the previous run, the first
        run from init (None: the rest pose).  batch=1 is the chain solve(positions[t], init=frame t - 1) bit for bit (through solve
        itself); a larger batch gives up the warm start inside a run for its launches (solve_batch: THE TRADE).  solve_options: those
        of solve / solve_batch; with want_stats returns (meshes, stats [T,outer_iterations,8]).  Nothing here waits for the device."""
        step = solve_options.get("global_step", "column")
        if step not in ("column", "grid"):
            raise ValueError('ArapSolver.solve_sequence: global_step must be "column" or "grid"; got %r' % (step,))
        self.mesh.need_device("ArapSolver.solve_sequence")
        if "out" in solve_options:
            raise ValueError("ArapSolver.solve_sequence: out is not an option here; the [T,Vm,3] result is allocated")
        if isinstance(batch, bool) or int(batch) != batch or not 1 <= batch <= _lib.GM_ARAP_BATCH_MAX:
            raise ValueError("ArapSolver.solve_sequence: batch = %r; a run holds 1 .. %d frames" % (batch, _lib.GM_ARAP_BATCH_MAX))
        dev, H = self.device, len(self.handles)
        if isinstance(positions, (list, tuple)) and len(positions) and all(torch.is_tensor(p) for p in positions):
            positions = torch.stack([p.detach().to(device=dev, dtype=torch.float32) for p in positions], 0)
        pos = torch.as_tensor(np.asarray(positions), dtype=torch.float32, device=dev) if not torch.is_tensor(positions) else \
            positions.detach().to(device=dev, dtype=torch.float32)
        if pos.dim() != 3 or pos.shape[1:] != (H, 3):
            raise ValueError("ArapSolver.solve_sequence: positions must be [T,%d,3]; got %s" % (H, tuple(pos.shape)))
        T, want_stats = pos.shape[0], bool(solve_options.get("want_stats"))
        meshes = torch.empty((T, self.Vm, 3), dtype=torch.float32, device=dev)
        stats, current = [], init
        for a, b in sequence_runs(T, int(batch)):
            if batch == 1:
                got = self.solve(pos[a], init=current, out=meshes[a], **solve_options)
            else:
                got = self.solve_batch(pos[a:b], init=current, out=meshes[a:b], **solve_options)
            if want_stats:
                stats.append(got[1].reshape(b - a, -1, 8))
            current = meshes[b - 1]
        if want_stats:
            outer = int(solve_options.get("outer_iterations", 4))
            return meshes, (torch.cat(stats, 0) if stats else torch.zeros((0, max(outer, 0), 8), dtype=torch.float64, device=dev))
        return meshes
