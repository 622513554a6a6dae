"""Simplify a proxy mesh on the device: rounds of quadric-error edge collapses with subset placement (csrc/gm_simplify.hip).  A collapse
removes one vertex and moves nothing, so the output vertices are rows of the input; what a surface-nets mesh of 10^5 faces needs before
ArapSolver, SurfaceGraph and MeshBoundGaussians.create_from_mesh, which are sized for about 15 k.  The reference sends its users to
MeshLab for this step.  Definition, ABI and rules: INTEGRATION.md section V.

    r = simplify(V, F, target_faces=15000)          # r.vertices, r.faces, r.kept, r.vertex_map, r.stats; all on the device
    handles_coarse = r.vertex_map[handles_dense]    # carry picks / handle sets over
    python -m gaussianmesh_amd.mesh_simplify --mesh in.obj --out out.obj --target_faces 15000

Per round the integer bookkeeping (unique edges and their face counts, the vertex -> face CSR) is torch sort / unique / cumsum on the
device; the arithmetic - quadrics once, then candidates and selection per round - is gm_mesh_quadrics / gm_mesh_collapse_round.  One
read-back per round: how many collapses were selected.
"""
import argparse
import json
import math
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

from ._op import enqueue, need_cuda, workspace


def _number(name, x):
    """x as a Python float: any real scalar (int, float, numpy scalar, 0-d tensor), finite; bool and text are refused"""
    if isinstance(x, (bool, str, bytes)):
        raise ValueError("simplify: %s must be a number; got %r" % (name, x))
    try:
        v = float(x)
    except (TypeError, ValueError):
        raise ValueError("simplify: %s must be a number; got %r" % (name, x)) from None
    if not math.isfinite(v):
        raise ValueError("simplify: %s must be finite; got %r" % (name, x))
    return v


def _count(name, x):
    """x as a non-negative Python int: any integer-valued scalar; bool is refused"""
    v = _number(name, x)
    if v != int(v) or v < 0:
        raise ValueError("simplify: %s must be a non-negative integer; got %r" % (name, x))
    return int(v)


def resolve_target(n_faces, target_faces=None, ratio=None, max_error=None):
    """the face count a call asks for: target_faces, or floor(ratio * faces), or 0 when only max_error stops the run"""
    if target_faces is not None and ratio is not None:
        raise ValueError("simplify: give target_faces or ratio, not both")
    if target_faces is None and ratio is None:
        if max_error is None:
            raise ValueError("simplify: give target_faces, ratio or max_error")
        return 0
    if ratio is not None:
        r = _number("ratio", ratio)
        if not 0.0 < r <= 1.0:
            raise ValueError("simplify: ratio must be in (0, 1]; got %r" % (ratio,))
        return int(math.floor(r * n_faces))
    return _count("target_faces", target_faces)


def _bookkeeping(F, Vm):
    """(edges int32 [E,2] sorted by lo Vm + hi, face count int32 [E], CSR offsets int32 [Vm+1], CSR face ids int32 [3F]) of the live faces
    F int64 [Fl,3]; integers only, on the device"""
    e = torch.cat([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]], 0)
    k, cnt = torch.unique(e.amin(1) * Vm + e.amax(1), sorted=True, return_counts=True)
    edges = torch.stack([k // Vm, k % Vm], 1).to(torch.int32).contiguous()
    vid = F.reshape(-1)
    order = torch.sort(vid, stable=True).indices
    off = torch.zeros(Vm + 1, dtype=torch.int64, device=F.device)
    torch.cumsum(torch.bincount(vid, minlength=Vm), 0, out=off[1:])
    return edges, cnt.to(torch.int32), off.to(torch.int32), (order // 3).to(torch.int32).contiguous()


def quadrics(vertices, faces):
    """gm_mesh_quadrics: float32 [Vm,10], the error quadric of every vertex (upper triangle, row order)"""
    need_cuda(vertices, "quadrics", "vertices")
    need_cuda(faces, "quadrics", "faces")
    V = vertices.detach().to(torch.float32).contiguous()
    F = faces.detach().to(torch.int64).reshape(-1, 3)
    _, _, off, adj = _bookkeeping(F, V.shape[0])
    return _quadrics(V, F.to(torch.int32).contiguous(), off, adj)


def _quadrics(V, F32, off, adj):
    Q = torch.empty((V.shape[0], 10), dtype=torch.float32, device=V.device)
    enqueue(V.device, "gm_mesh_quadrics", V.shape[0], V, F32.shape[0], F32, off, adj, Q)
    return Q


def collapse_round(V, Q, F32, off, adj, edges, uses, min_cos, max_error):
    """gm_mesh_collapse_round: (selected uint8 [E], from int32 [E], to int32 [E], key int64 [E] (the unsigned key's bits), count int32 [1]),
    all on the device; nothing waits"""
    dev = V.device
    E = edges.shape[0]
    selected = torch.empty((E,), dtype=torch.uint8, device=dev)
    frm = torch.empty((E,), dtype=torch.int32, device=dev)
    to = torch.empty((E,), dtype=torch.int32, device=dev)
    key = torch.empty((E,), dtype=torch.int64, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    ws = workspace(dev, "gm_mesh_collapse_round_workspace_bytes", V.shape[0])
    enqueue(dev, "gm_mesh_collapse_round", V.shape[0], V, Q, F32.shape[0], F32, off, adj, E, edges, uses, float(min_cos), float(max_error), selected,
            frm, to, key, count, workspace=ws)
    return selected, frm, to, key, count


def simplify(vertices, faces, target_faces=None, ratio=None, max_error=None, min_cos=0.2, max_rounds=1024):
    """Simplify the mesh (vertices [V,3], faces [F,3], device tensors) to at most target_faces faces (or floor(ratio F); or, with neither,
    until no collapse costs max_error or less).  Returns an object with
      vertices float32 [V',3], faces int32 [F',3]
      kept int64 [V']: the input row of each output vertex, ascending (unreferenced vertices dropped, ids re-numbered in order)
      vertex_map int64 [V]: the output vertex each input vertex ended in (-1: an unreferenced vertex)
      stats: faces_before, faces, rounds, stalled, locked_vertices, max_cost, degenerate_faces, reached (faces <= the target: False
             after a stall or when max_rounds ended the run)
    max_error bounds the quadric cost of every collapse; min_cos the cosine by which a face normal may turn in one collapse.  A run that
    neither stalls nor runs out of rounds ends at target_faces when (F - target_faces) is even, else at target_faces - 1: a collapse
    removes two faces.  Borders and edges with more than two faces are locked and stay at full resolution; `stalled` says that a round
    found nothing to collapse above the target.  A target at or above the face count returns the input mesh with zero rounds.
    Input faces with a repeated corner are dropped first (stats["degenerate_faces"]; ratio still counts them).  Two input faces over the
    same three vertices are kept: their edges have a face count other than 2 or fail the link condition, so nothing there collapses.
    Parameters may be any real scalars (numpy, 0-d tensors); bool is refused."""
    max_error = None if max_error is None else _number("max_error", max_error)
    if max_error is not None and max_error < 0:
        raise ValueError("simplify: max_error must be >= 0; got %r" % (max_error,))
    min_cos = _number("min_cos", min_cos)
    if not 0.0 <= min_cos <= 1.0:
        raise ValueError("simplify: min_cos must be in [0, 1]; got %r" % (min_cos,))
    max_rounds = _count("max_rounds", max_rounds)
    resolve_target(0, target_faces, ratio, max_error)                  # the parameters alone, before anything touches a tensor
    need_cuda(vertices, "simplify", "vertices")
    need_cuda(faces, "simplify", "faces")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("simplify: vertices must be [V,3] and faces [F,3]; got %s, %s" % (tuple(vertices.shape), tuple(faces.shape)))
    dev = vertices.device
    V = vertices.detach().to(torch.float32).contiguous()
    F = faces.detach().to(torch.int64).contiguous()
    Vm, F0 = V.shape[0], F.shape[0]
    target = resolve_target(F0, target_faces, ratio, max_error)
    if F0 and (int(F.min()) < 0 or int(F.max()) >= Vm):
        raise ValueError("simplify: face ids outside [0, %d)" % Vm)
    bound = float("inf") if max_error is None else float(max_error)
    parent = torch.arange(Vm, dtype=torch.int64, device=dev)
    rounds, stalled, locked_vertices = 0, False, 0
    max_cost = torch.zeros((), dtype=torch.float32, device=dev)
    # a face with a repeated corner has no area and no place in the link condition: dropped before the first round, as every round does
    live, Q = F[(F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 2] != F[:, 0])], None
    degenerate = F0 - int(live.shape[0])
    while live.shape[0] > target and rounds < max_rounds:
        edges, uses, off, adj = _bookkeeping(live, Vm)
        F32 = live.to(torch.int32).contiguous()
        if Q is None:
            Q = _quadrics(V, F32, off, adj)
            locked_vertices = int(torch.unique(edges[uses != 2]).numel())
        selected, frm, to, key, count = collapse_round(V, Q, F32, off, adj, edges, uses, min_cos, bound)
        n = int(count.item())                                          # the round's one read-back
        if n == 0:
            stalled = True
            break
        sel = selected.bool()
        if live.shape[0] - 2 * n < target:
            k = (live.shape[0] - target + 1) // 2
            sel &= key <= torch.sort(key[sel]).values[k - 1]           # (a candidate's key is below 2^63: signed order is its order)
        i, j = frm[sel].long(), to[sel].long()
        Q[j] = Q[i] + Q[j]                                             # every j distinct, no j an i
        max_cost = torch.maximum(max_cost, (key[sel] >> 32).to(torch.int32).view(torch.float32).max())
        remap = torch.arange(Vm, dtype=torch.int64, device=dev)
        remap[i] = j
        parent[i] = j
        live = remap[live]
        live = live[(live[:, 0] != live[:, 1]) & (live[:, 1] != live[:, 2]) & (live[:, 2] != live[:, 0])]
        rounds += 1
    kept = torch.unique(live)
    index = torch.full((Vm,), -1, dtype=torch.int64, device=dev)
    index[kept] = torch.arange(kept.shape[0], dtype=torch.int64, device=dev)
    root = parent
    for _ in range(64):                                                # pointer jumping: a chain of 2^64 collapses does not exist
        nxt = root[root]
        if torch.equal(nxt, root):
            break
        root = nxt
    stats = dict(faces_before=F0, faces=int(live.shape[0]), rounds=rounds, stalled=stalled, locked_vertices=locked_vertices,
                 max_cost=float(max_cost), degenerate_faces=degenerate, reached=int(live.shape[0]) <= target)
    return SimpleNamespace(vertices=V[kept].contiguous(), faces=index[live].to(torch.int32).contiguous(), kept=kept, vertex_map=index[root],
                           stats=stats)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m gaussianmesh_amd.mesh_simplify", description="in.obj -> a simplified out.obj")
    ap.add_argument("--mesh", required=True, help="the OBJ to simplify (a proxy_mesh, NeuS or MeshLab mesh)")
    ap.add_argument("--out", required=True, help="the OBJ to write")
    ap.add_argument("--target_faces", type=int)
    ap.add_argument("--ratio", type=float)
    ap.add_argument("--max_error", type=float)
    ap.add_argument("--min_cos", type=float, default=0.2)
    ap.add_argument("--max_rounds", type=int, default=1024)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mesh_simplify needs a HIP (cuda) device; there is no CPU path")
    from . import io as gio
    dev = torch.device("cuda")
    t0 = time.perf_counter()
    v, f = gio.read_obj(a.mesh)
    V, F = torch.as_tensor(np.asarray(v, np.float32), device=dev), torch.as_tensor(np.asarray(f, np.int32), device=dev)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    r = simplify(V, F, target_faces=a.target_faces, ratio=a.ratio, max_error=a.max_error, min_cos=a.min_cos, max_rounds=a.max_rounds)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    gio.write_obj(a.out, r.vertices.cpu().numpy(), r.faces.cpu().numpy())
    t3 = time.perf_counter()
    print(json.dumps(dict(vertices_before=int(V.shape[0]), faces_before=r.stats["faces_before"], vertices=int(r.vertices.shape[0]),
                          faces=r.stats["faces"], rounds=r.stats["rounds"], stalled=r.stats["stalled"], reached=r.stats["reached"], locked_vertices=r.stats["locked_vertices"],
                          max_cost=r.stats["max_cost"], seconds=dict(load=t1 - t0, simplify=t2 - t1, write=t3 - t2))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
