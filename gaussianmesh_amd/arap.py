"""Deform a proxy mesh from dragged handle vertices: as-rigid-as-possible (Sorkine & Alexa 2007) on the device (gm_arap_solve,
csrc/gm_arap.hip).  The stage the reference leaves to an external binary: "move these vertices there; the rest of the mesh follows as
rigidly as it can".  Its output is what deform.mesh_rs / SingleObjectDeform.deform_vertices / render_sequence take, so a handle drag is
solve -> gm_mesh_rs -> forward on one stream, with no host wait.  Definition, ABI and rules: INTEGRATION.md section Q.
ArapEnergy is the same energy as a function of a pose, with its gradient, and one-ring smoothing of per-vertex rows (gm_arap_energy_grad,
gm_mesh_smooth_rows): what pose_fit.PoseFitter takes as a rigidity term and for its gradient."""
import numpy as np
import torch

from . import _lib
from ._op import enqueue, host, on_device, workspace


def edge_csr(vertices, faces):
    """The weighted edge graph of a triangle mesh as a symmetric CSR: (row_offsets int32 [Vm+1], cols int32 [nnz], weights float64
    [nnz]), columns ascending within each row, no diagonal.  Weights as mesh_rs_kernel forms them (gm_mesh.hip), in float64 from the
    float32 vertices: every face corner c opposite edge (a, b) adds max(0.5 cot(angle at c), 1e-3) to w_ab, cot = (u . w) / |u x w| with
    u = a - c, w = b - c; a face with |u x w| <= 1e-30 adds nothing (an edge that only such faces hold does not appear).  Every weight
    is positive.  Host, numpy only; once per mesh, like deform.vertex_face_adjacency."""
    v = np.asarray(host(vertices), np.float32).astype(np.float64)
    f = np.asarray(host(faces)).astype(np.int64).reshape(-1, 3)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError("edge_csr: vertices must be [Vm,3]; got %s" % (tuple(v.shape),))
    Vm = v.shape[0]
    if f.shape[0] and (int(f.min()) < 0 or int(f.max()) >= Vm):
        raise ValueError("edge_csr: face index outside [0, %d)" % Vm)
    keys, vals = [], []
    for c in range(3):
        ia, ib, ic = f[:, (c + 1) % 3], f[:, (c + 2) % 3], f[:, c]
        u, w = v[ia] - v[ic], v[ib] - v[ic]
        area2 = np.linalg.norm(np.cross(u, w), axis=1)
        ok = (area2 > 1e-30) & (ia != ib)
        with np.errstate(divide="ignore", invalid="ignore"):
            wt = np.maximum(0.5 * (u * w).sum(axis=1) / area2, 1e-3)
        keys += [ia[ok] * Vm + ib[ok], ib[ok] * Vm + ia[ok]]
        vals += [wt[ok], wt[ok]]
    keys = np.concatenate(keys) if keys else np.zeros(0, np.int64)
    vals = np.concatenate(vals) if vals else np.zeros(0, np.float64)
    uniq, inv = np.unique(keys, return_inverse=True)                   # sorted: rows ascend, columns ascend within a row
    weights = np.bincount(inv.reshape(-1), weights=vals, minlength=len(uniq)).astype(np.float64)
    rows, cols = uniq // Vm, uniq % Vm
    offsets = np.zeros(Vm + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=Vm), out=offsets[1:])
    return offsets.astype(np.int32), cols.astype(np.int32), weights


def components(Vm, rows, cols):
    """Label of the connected component of every vertex (the smallest vertex id in it): min-label propagation with pointer jumping."""
    label = np.arange(Vm, dtype=np.int64)
    while True:
        new = label.copy()
        np.minimum.at(new, rows, label[cols])
        new = new[new]                                                 # a label is a vertex of the same component: jump to its label
        if np.array_equal(new, label):
            return label
        label = new


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
    gradient, for an optimiser of the vertices (pose_fit.PoseFitter).  Built once: the edge CSR (edge_csr), the rest vertices,
    scale = sum_ij w_ij |p_i - p_j|^2 (the size of E's terms: E / scale does not depend on the mesh's units) and the workspaces.
        E(x) = sum_i sum_j w_ij |(x_i - x_j) - R_i (p_i - p_j)|^2, R_i the local step's rotation at x;  0 for a rigid motion of the rest pose
    ValueError for a mesh without an edge (scale = 0).  Definition, ABI and rules: INTEGRATION.md section Y."""

    def __init__(self, rest_vertices, faces, device="cuda"):
        self.device = torch.device(device)
        v = np.ascontiguousarray(np.asarray(host(rest_vertices), np.float32))
        if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] == 0:
            raise ValueError("ArapEnergy: rest_vertices must be [Vm,3] with Vm > 0; got %s" % (tuple(v.shape),))
        off, cols, weights = edge_csr(v, faces)
        rows = np.repeat(np.arange(v.shape[0], dtype=np.int64), np.diff(off.astype(np.int64)))
        e = v.astype(np.float64)[rows] - v.astype(np.float64)[cols]
        self.Vm, self.csr = v.shape[0], (off, cols, weights)
        self.scale = float((weights * (e * e).sum(axis=1)).sum())
        if not self.scale > 0.0:
            raise ValueError("ArapEnergy: the mesh has no edge of positive length (scale = %g)" % self.scale)
        if self.device.type != "cuda":                                 # the set-up above is host work; every call needs the device
            return
        t = lambda a, dt: on_device(a, dt, self.device)
        self.rest = t(v, torch.float32)
        self._off, self._cols, self._w = t(off, torch.int32), t(cols, torch.int32), t(weights, torch.float64)
        self._ws = workspace(self.device, "gm_arap_energy_workspace_bytes", self.Vm)
        self._smooth_ws = None                                         # made by the first smooth_rows

    def _pose(self, V1, who):
        if self.device.type != "cuda" or not torch.is_tensor(V1) or V1.device.type != "cuda":
            raise _lib.GmeshError("%s needs the object and V1 on a HIP (cuda) device; there is no CPU path" % who)
        if V1.shape != (self.Vm, 3) or not V1.dtype.is_floating_point:
            raise ValueError("%s: V1 must be a floating-point [%d,3] tensor; got %s %s" % (who, self.Vm, V1.dtype, tuple(V1.shape)))
        return V1.detach().to(device=self.rest.device, dtype=torch.float32).contiguous()

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
        if self.device.type != "cuda" or not torch.is_tensor(rows) or rows.device.type != "cuda":
            raise _lib.GmeshError("ArapEnergy.smooth_rows needs the object and rows on a HIP (cuda) device; there is no CPU path")
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
    """As-rigid-as-possible deformation of one mesh from one set of handle vertices.  Built once: the edge CSR (edge_csr), the mask of
    held rows (the handles, and PINNED vertices: those whose weights sum to 0 - unreferenced, or every face at them degenerate - which
    keep their `init` position), the device workspace.
    rest_vertices [Vm,3], faces [F,3] vertex ids, handles: H distinct vertex ids.  ValueError for a handle id out of range or given
    twice, an empty handle set, and a connected component of the weighted edge graph that has a free vertex but no handle (its
    positions would be undetermined: the linear system is singular)."""

    def __init__(self, rest_vertices, faces, handles, device="cuda"):
        self.device = torch.device(device)
        v = np.ascontiguousarray(np.asarray(host(rest_vertices), np.float32))
        if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] == 0:
            raise ValueError("ArapSolver: rest_vertices must be [Vm,3] with Vm > 0; got %s" % (tuple(v.shape),))
        Vm = v.shape[0]
        h = np.asarray(host(handles)).reshape(-1)
        if h.size == 0:
            raise ValueError("ArapSolver: the handle set is empty")
        if h.dtype.kind not in "iu":
            raise ValueError("ArapSolver: handles must be integer vertex ids, got %s" % h.dtype)
        h = h.astype(np.int64)
        if int(h.min()) < 0 or int(h.max()) >= Vm:
            raise ValueError("ArapSolver: handle id outside [0, %d) (min %d, max %d)" % (Vm, int(h.min()), int(h.max())))
        if len(np.unique(h)) != len(h):
            raise ValueError("ArapSolver: a handle id is given twice")
        off, cols, weights = edge_csr(v, faces)
        rows = np.repeat(np.arange(Vm, dtype=np.int64), np.diff(off.astype(np.int64)))
        pinned = np.bincount(rows, weights=weights, minlength=Vm) <= 0.0
        fixed = pinned.copy()
        fixed[h] = True
        label = components(Vm, rows, cols.astype(np.int64))
        has_handle = np.zeros(Vm, bool)
        has_handle[label[h]] = True
        loose = np.nonzero(~fixed & ~has_handle[label])[0]
        if len(loose):
            raise ValueError("ArapSolver: vertex %d lies in a connected component without a handle (%d such vertices): the system is singular"
                             % (int(loose[0]), len(loose)))
        self.Vm, self.handles, self.pinned = Vm, h, np.nonzero(pinned)[0]
        self.csr = (off, cols, weights)
        if self.device.type != "cuda":                                 # the set-up above is host work; solve() needs the device
            return
        t = lambda a, dt: on_device(a, dt, self.device)
        self.rest = t(v, torch.float32)
        self._off, self._cols, self._w = t(off, torch.int32), t(cols, torch.int32), t(weights, torch.float64)
        self._fixed = t(fixed.astype(np.uint8), torch.uint8)
        self._handle_idx = t(h, torch.int64)
        self._ws = workspace(self.device, "gm_arap_workspace_bytes", Vm)
        self._grid_ws = None                                           # the whole-chip global step's own workspace: made by its first solve
        self._batch_ws = {}                                            # global_step -> solve_batch's workspace, grown to the largest B seen

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
        if global_step not in ("column", "grid"):
            raise ValueError('ArapSolver.solve: global_step must be "column" or "grid"; got %r' % (global_step,))
        if self.device.type != "cuda":
            raise _lib.GmeshError("ArapSolver.solve needs a HIP (cuda) device; there is no CPU path")
        Vm, dev = self.Vm, self.device
        hp = torch.as_tensor(handle_positions, dtype=torch.float32, device=dev) if not torch.is_tensor(handle_positions) else \
            handle_positions.detach().to(device=dev, dtype=torch.float32)
        if hp.shape != (len(self.handles), 3):
            raise ValueError("ArapSolver.solve: handle_positions must be [%d,3]; got %s" % (len(self.handles), tuple(hp.shape)))
        if init is not None:
            if not torch.is_tensor(init):
                init = torch.as_tensor(np.asarray(init), dtype=torch.float32, device=dev)
            if init.shape != (Vm, 3):
                raise ValueError("ArapSolver.solve: init must be [%d,3]; got %s" % (Vm, tuple(init.shape)))
        if out is not None and (not torch.is_tensor(out) or out.shape != (Vm, 3) or out.dtype is not torch.float32 or not out.is_contiguous()
                                or out.device != self.rest.device):
            raise ValueError("ArapSolver.solve: out must be a contiguous float32 [%d,3] tensor on the solver's device" % Vm)
        if out is not None and out is init:
            guess = out                                                # in place
        else:
            guess = (self.rest if init is None else init.detach().to(device=dev, dtype=torch.float32)).clone(memory_format=torch.contiguous_format)
        guess.index_copy_(0, self._handle_idx, hp)
        if out is None:
            out = guess
        stats = torch.zeros((int(outer_iterations), 8), dtype=torch.float64, device=dev) if want_stats and outer_iterations > 0 else None
        if global_step == "grid":
            if self._grid_ws is None:
                self._grid_ws = workspace(dev, "gm_arap_grid_workspace_bytes", Vm)
            entry, ws = "gm_arap_solve_grid", self._grid_ws
        else:
            entry, ws = "gm_arap_solve", self._ws
        enqueue(dev, entry, Vm, self._off, self._cols, self._w, self.rest, self._fixed, guess, int(outer_iterations), int(cg_iterations),
                float(cg_tolerance), out, stats, workspace=ws)
        if want_stats:
            return out, (stats if stats is not None else torch.zeros((0, 8), dtype=torch.float64, device=dev))
        return out

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
        if global_step not in ("column", "grid"):
            raise ValueError('ArapSolver.solve_batch: global_step must be "column" or "grid"; got %r' % (global_step,))
        if self.device.type != "cuda":
            raise _lib.GmeshError("ArapSolver.solve_batch needs a HIP (cuda) device; there is no CPU path")
        Vm, dev, H = self.Vm, self.device, len(self.handles)
        hp = torch.as_tensor(np.asarray(handle_positions), dtype=torch.float32, device=dev) if not torch.is_tensor(handle_positions) else \
            handle_positions.detach().to(device=dev, dtype=torch.float32)
        if hp.dim() != 3 or hp.shape[1:] != (H, 3):
            raise ValueError("ArapSolver.solve_batch: handle_positions must be [B,%d,3]; got %s" % (H, tuple(hp.shape)))
        B = hp.shape[0]
        if not 1 <= B <= _lib.GM_ARAP_BATCH_MAX:
            raise ValueError("ArapSolver.solve_batch: B = %d; a batch holds 1 .. %d solves" % (B, _lib.GM_ARAP_BATCH_MAX))
        if init is not None:
            if not torch.is_tensor(init):
                init = torch.as_tensor(np.asarray(init), dtype=torch.float32, device=dev)
            if init.shape != (Vm, 3) and init.shape != (B, Vm, 3):
                raise ValueError("ArapSolver.solve_batch: init must be [%d,3] or [%d,%d,3]; got %s" % (Vm, B, Vm, tuple(init.shape)))
        if out is not None and (not torch.is_tensor(out) or out.shape != (B, Vm, 3) or out.dtype is not torch.float32 or not out.is_contiguous()
                                or out.device != self.rest.device):
            raise ValueError("ArapSolver.solve_batch: out must be a contiguous float32 [%d,%d,3] tensor on the solver's device" % (B, Vm))
        if out is not None and out is init:
            guess = out                                                # in place
        else:
            start = self.rest if init is None else init.detach().to(device=dev, dtype=torch.float32)
            guess = start.expand(B, Vm, 3).clone(memory_format=torch.contiguous_format)
        guess.index_copy_(1, self._handle_idx, hp)
        if out is None:
            out = guess
        stats = torch.zeros((B, int(outer_iterations), 8), dtype=torch.float64, device=dev) if want_stats and outer_iterations > 0 else None
        step = 1 if global_step == "grid" else 0
        need = _lib.lib().gm_arap_batch_workspace_bytes(Vm, B, step)
        ws = self._batch_ws.get(global_step)
        if ws is None or ws.numel() < need:
            ws = self._batch_ws[global_step] = torch.empty((need,), dtype=torch.uint8, device=dev)
        enqueue(dev, "gm_arap_solve_batch", B, step, Vm, self._off, self._cols, self._w, self.rest, self._fixed, guess, int(outer_iterations),
                int(cg_iterations), float(cg_tolerance), out, stats, workspace=ws)
        if want_stats:
            return out, (stats if stats is not None else torch.zeros((B, 0, 8), dtype=torch.float64, device=dev))
        return out

    def solve_sequence(self, positions, init=None, batch=4, **solve_options):
        """The meshes [T,Vm,3] of a drag whose frame t has the handles at positions[t] ([T,H,3]), `batch` frames per launch chain
        (sequence_runs; the last run may be shorter).  Every frame of a run starts from the LAST frame of the previous run, the first
        run from init (None: the rest pose).  batch=1 is the chain solve(positions[t], init=frame t - 1) bit for bit (through solve
        itself); a larger batch gives up the warm start inside a run for its launches (solve_batch: THE TRADE).  solve_options: those
        of solve / solve_batch; with want_stats returns (meshes, stats [T,outer_iterations,8]).  Nothing here waits for the device."""
        step = solve_options.get("global_step", "column")
        if step not in ("column", "grid"):
            raise ValueError('ArapSolver.solve_sequence: global_step must be "column" or "grid"; got %r' % (step,))
        if self.device.type != "cuda":
            raise _lib.GmeshError("ArapSolver.solve_sequence needs a HIP (cuda) device; there is no CPU path")
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
