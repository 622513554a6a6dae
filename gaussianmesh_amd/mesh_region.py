"""Grow a pick into a surface region: distances ALONG the proxy mesh (gm_mesh_geodesic, csrc/gm_geodesic.hip) and the glue that turns
picked vertices plus two radii into an ArapSolver handle set - everything within grab_radius of a pick moves with it, everything farther
than free_radius stays put, the band in between bends.

Distances are shortest paths in a weighted graph built from the rest mesh (surface_graph), not a PDE solve: the result is unique, and
the device is held bit for bit to a float32 Dijkstra (tests/geodesic_ref.py).  Definition, ABI and rules: INTEGRATION.md section U."""
import math

import numpy as np
import torch

from . import _lib
from ._op import enqueue, host
from .mesh_graph import vertex_ids


def _norm3(d):
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def _dot3(x, y):
    return (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]


def surface_graph(vertices, faces, unfold=True):
    """The weighted graph whose shortest paths are this package's surface distances, as a symmetric CSR (row_offsets int32 [Vm+1], cols
    int32 [nnz], lengths float32 [nnz]), columns ascending within a row, no diagonal.  Host, numpy only; once per mesh, like
    arap.edge_csr.  V64: the float32 vertices widened to float64; dot(x, y) = (x0 y0 + x1 y1) + x2 y2, |x| = sqrt(dot(x, x)).
      Real edges: every pair (p, q), p != q, of every face's corner cycle, of length float32(|V64[p] - V64[q]|).
      Unfolded edges (unfold=True): an edge (a, b), a < b, shared by exactly two faces whose opposite vertices c (of the face with the
      lower index) and e differ is laid with both triangles into one plane, in float64:
        L = |b - a|, u = (b - a) / L, cx = dot(c - a, u), cy = sqrt(max(|c - a|^2 - cx^2, 0)), (ex, ey) likewise for e;
        skipped if L, cy or ey <= 0;  x* = cx + (ex - cx) cy / (cy + ey);
        if 0 < x* < L (the straight line from c to e crosses the shared edge): a virtual edge (c, e) of length
        float32(hypot(cx - ex, cy + ey)).
      Without them a "disc" on a regular triangulation is a hexagon (worst path / Euclidean 1.41 on a grid with one diagonal per
      cell; 1.08 with them).
      Duplicates, a virtual edge that is also a real one included, keep the smallest length.
    ValueError for bad shapes and for face ids out of range."""
    v = np.asarray(host(vertices))
    f = np.asarray(host(faces))
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError("surface_graph: vertices must be [Vm,3]; got %s" % (tuple(v.shape),))
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("surface_graph: faces must be [F,3]; got %s" % (tuple(f.shape),))
    if f.size and f.dtype.kind not in "iu":
        raise ValueError("surface_graph: faces must hold integer vertex ids, got %s" % f.dtype)
    v = v.astype(np.float32).astype(np.float64)
    f = f.astype(np.int64)
    Vm = v.shape[0]
    if f.shape[0] and (int(f.min()) < 0 or int(f.max()) >= Vm):
        raise ValueError("surface_graph: face index outside [0, %d)" % Vm)
    # one record per face corner k: the edge (p, q) opposite it
    p = np.concatenate([f[:, (k + 1) % 3] for k in range(3)])
    q = np.concatenate([f[:, (k + 2) % 3] for k in range(3)])
    opp = np.concatenate([f[:, k] for k in range(3)])
    fid = np.tile(np.arange(f.shape[0], dtype=np.int64), 3)
    ok = p != q
    p, q, opp, fid = p[ok], q[ok], opp[ok], fid[ok]
    a, b = np.minimum(p, q), np.maximum(p, q)
    ends = [(a, b, _norm3(v[a] - v[b]).astype(np.float32))]
    if unfold and len(a):
        key = a * Vm + b
        order = np.lexsort((fid, key))                                 # by edge, then by face
        key, opp_s = key[order], opp[order]
        first = np.nonzero(np.r_[True, key[1:] != key[:-1]])[0]
        count = np.diff(np.r_[first, len(key)])
        first = first[count == 2]
        ia, ib, ic, ie = key[first] // Vm, key[first] % Vm, opp_s[first], opp_s[first + 1]
        keep = ic != ie
        ia, ib, ic, ie = ia[keep], ib[keep], ic[keep], ie[keep]
        with np.errstate(divide="ignore", invalid="ignore"):
            ab = v[ib] - v[ia]
            L = _norm3(ab)
            u = ab / L[:, None]
            ca, ea = v[ic] - v[ia], v[ie] - v[ia]
            cx, ex = _dot3(ca, u), _dot3(ea, u)
            cy = np.sqrt(np.maximum(_dot3(ca, ca) - cx * cx, 0.0))
            ey = np.sqrt(np.maximum(_dot3(ea, ea) - ex * ex, 0.0))
            xs = cx + (ex - cx) * cy / (cy + ey)
            good = (L > 0) & (cy > 0) & (ey > 0) & (xs > 0) & (xs < L)  # (NaN: False)
            length = np.hypot(cx - ex, cy + ey).astype(np.float32)
        ends.append((ic[good], ie[good], length[good]))
    rows = np.concatenate([np.concatenate([x, y]) for x, y, _ in ends])
    cols = np.concatenate([np.concatenate([y, x]) for x, y, _ in ends])
    lens = np.concatenate([np.concatenate([l, l]) for _, _, l in ends])
    order = np.lexsort((lens, rows * Vm + cols))                       # by entry, the shortest first
    key, lens = (rows * Vm + cols)[order], lens[order]
    first = np.r_[True, key[1:] != key[:-1]] if len(key) else np.zeros(0, bool)
    key, lens = key[first], lens[first]
    offsets = np.zeros(Vm + 1, np.int64)
    np.cumsum(np.bincount(key // Vm, minlength=Vm) if Vm else np.zeros(0, np.int64), out=offsets[1:])
    return offsets.astype(np.int32), (key % max(Vm, 1)).astype(np.int32), lens.astype(np.float32)


def _radius(name, r):
    r = float(r)
    if not r >= 0.0:
        raise ValueError("%s must be >= 0 and not NaN; got %r" % (name, r))
    return r


def check_radii(who, grab_radius, free_radius):
    grab = _radius("%s: grab_radius" % who, grab_radius)
    free = None if free_radius is None else _radius("%s: free_radius" % who, free_radius)
    if free is not None and free < grab:
        raise ValueError("%s: free_radius %g is below grab_radius %g" % (who, free, grab))
    return grab, free


class SurfaceGraph:
    """surface_graph(vertices, faces, unfold) of one mesh, held on the device with the workspace of gm_mesh_geodesic.  The set-up is
    host work (device="cpu" builds the CSR alone, as ArapSolver does); distances() needs a HIP device."""

    def __init__(self, vertices, faces, unfold=True, device="cuda"):
        self._hold(surface_graph(vertices, faces, unfold=unfold), device)

    @classmethod
    def from_csr(cls, row_offsets, cols, lengths, device="cuda"):
        """A SurfaceGraph of any symmetric CSR with lengths >= 0 (int32 [Vm+1], int32 [nnz], float32 [nnz]; taken as given)."""
        g = cls.__new__(cls)
        g._hold((np.asarray(row_offsets, np.int32), np.asarray(cols, np.int32), np.asarray(lengths, np.float32)), device)
        return g

    def _hold(self, csr, device):
        self.device = torch.device(device)
        self.csr = csr
        self.Vm = len(self.csr[0]) - 1
        self._ws = None
        if self.device.type != "cuda":
            return
        off, cols, lens = (torch.as_tensor(np.ascontiguousarray(a), device=self.device) for a in self.csr)
        if cols.numel() == 0:                                          # a mesh without edges: the kernel reads no entry, but wants a pointer
            cols, lens = torch.zeros(1, dtype=torch.int32, device=self.device), torch.zeros(1, dtype=torch.float32, device=self.device)
        self._off, self._cols, self._lens = off, cols, lens
        self._unsettled = torch.zeros(1, dtype=torch.int32, device=self.device)

    def distances(self, source_sets, max_distance=None, sweeps_per_check=64, max_sweeps=None):
        """float32 [B, Vm] on the device: row b holds every vertex's distance along the graph from the nearest vertex of
        source_sets[b] (a list of B lists of vertex ids; an empty set gives a row of +inf), +inf where no path arrives or, with
        max_distance, where the distance exceeds it (the cutoff is inclusive).  Bit for bit a float32 Dijkstra, whatever the schedule.
        The device relaxes in chunks of sweeps_per_check launches (gm_mesh_geodesic with resume) and after each chunk the host reads
        back ONE int32, the number of rows the chunk's last sweep lowered: a 4-byte device-to-host copy and a wait per chunk, the only
        ones here.  max_sweeps: the budget over all chunks, by default Vm (the Jacobi worst case: a path graph); running out of it
        raises GmeshError - unsettled values are never returned.  ValueError for a source id outside [0, Vm) or not an integer, a
        negative or NaN max_distance, more than 65535 sets."""
        if self.device.type != "cuda":
            raise _lib.GmeshError("SurfaceGraph.distances needs a HIP (cuda) device; there is no CPU path")
        Vm, dev = self.Vm, self.device
        cutoff = math.inf if max_distance is None else _radius("SurfaceGraph.distances: max_distance", max_distance)
        cutoff = float(np.float32(cutoff))                             # the kernel compares in float32: max_distance rounded once
        chunk = int(sweeps_per_check)
        budget = max(Vm, 1) if max_sweeps is None else int(max_sweeps)
        if chunk < 1 or budget < 1:
            raise ValueError("SurfaceGraph.distances: sweeps_per_check and max_sweeps must be >= 1; got %r, %r" % (sweeps_per_check, max_sweeps))
        sets = [vertex_ids(s, Vm, "SurfaceGraph.distances", "source set %d" % b, allow_empty=True, distinct=False) for b, s in enumerate(source_sets)]
        B = len(sets)
        if B > 65535:
            raise ValueError("SurfaceGraph.distances: at most 65535 source sets a call; got %d" % B)
        dist = torch.empty((B, Vm), dtype=torch.float32, device=dev)
        if B == 0 or Vm == 0:
            return dist
        offsets = np.zeros(B + 1, np.int64)
        np.cumsum([len(a) for a in sets], out=offsets[1:])
        src = np.concatenate(sets + [np.zeros(1, np.int64)])            # (one spare entry: never an empty array)
        d_off = torch.as_tensor(offsets.astype(np.int32), device=dev)
        d_src = torch.as_tensor(src.astype(np.int32), device=dev)
        nbytes = _lib.lib().gm_mesh_geodesic_workspace_bytes(Vm, B, chunk)
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        used, resume = 0, 0
        while used < budget:
            n = min(chunk, budget - used)
            enqueue(dev, "gm_mesh_geodesic", Vm, self._off, self._cols, self._lens, B, d_off, d_src, cutoff, n, resume, dist, self._unsettled,
                    workspace=self._ws)
            used, resume = used + n, 1
            if int(self._unsettled.item()) == 0:                       # the 4-byte read-back
                self.sweeps_enqueued = used
                return dist
        raise _lib.GmeshError("SurfaceGraph.distances: %d sweeps did not settle the distances (max_sweeps; Vm = %d always suffices)" % (budget, Vm))


def region_handles(d_handles, d_anchors, grab_radius, free_radius=None):
    """From distance rows to an ArapSolver handle set, host numpy: (ids int64 [n], owner int32 [n]).  d_handles [H,Vm]: row i = the
    distances from pick i (SurfaceGraph.distances); d_anchors [A,Vm] or None.
      Moved rows first: {v : d_handles[i][v] <= grab_radius} with owner = i, in pick order, ascending id inside a pick.
      Then held rows, owner = -1, each vertex once: {v : d_anchors[j][v] <= grab_radius} per anchor in order, ascending inside; then,
      with free_radius, every v with min_i d_handles[i][v] > free_radius, ascending - unreachable vertices are +inf, so they are held,
      and a component without a pick no longer trips ArapSolver's singular-system refusal.
    ValueError for two handle regions that overlap (naming both picks and a shared vertex), a handle region that meets an anchor
    region, free_radius < grab_radius, a negative or NaN radius."""
    grab, free = check_radii("region_handles", grab_radius, free_radius)
    dh = np.asarray(host(d_handles), np.float32)
    if dh.ndim != 2 or dh.shape[0] == 0:
        raise ValueError("region_handles: d_handles must be [H,Vm] with H >= 1; got %s" % (tuple(dh.shape),))
    H, Vm = dh.shape
    da = np.zeros((0, Vm), np.float32) if d_anchors is None else np.asarray(host(d_anchors), np.float32).reshape(-1, Vm)
    owner_of = np.full(Vm, -1, np.int64)
    ids, owner = [], []
    for i in range(H):
        reg = np.nonzero(dh[i] <= grab)[0]
        clash = reg[owner_of[reg] >= 0]
        if len(clash):
            raise ValueError("region_handles: the regions of handle %d and handle %d overlap (vertex %d lies within grab_radius %g of both)"
                             % (int(owner_of[clash[0]]), i, int(clash[0]), grab))
        owner_of[reg] = i
        ids.append(reg); owner.append(np.full(len(reg), i, np.int32))
    held = np.zeros(Vm, bool)
    for j in range(da.shape[0]):
        reg = np.nonzero(da[j] <= grab)[0]
        clash = reg[owner_of[reg] >= 0]
        if len(clash):
            raise ValueError("region_handles: the region of handle %d meets the region of anchor %d (vertex %d lies within grab_radius %g of both)"
                             % (int(owner_of[clash[0]]), j, int(clash[0]), grab))
        reg = reg[~held[reg]]
        held[reg] = True
        ids.append(reg); owner.append(np.full(len(reg), -1, np.int32))
    if free is not None:
        reg = np.nonzero((dh.min(axis=0) > free) & ~held)[0]
        ids.append(reg); owner.append(np.full(len(reg), -1, np.int32))
    return np.concatenate(ids).astype(np.int64), np.concatenate(owner).astype(np.int32)
