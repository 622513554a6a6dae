"""The definition of gm_mesh_quadrics / gm_mesh_collapse_round / mesh_simplify.simplify in numpy float32: no torch, no device.  Every
product and sum is one float32 operation in the order the header comment of csrc/gm_simplify.hip (and include/gmesh_hip.h) states, so
the device is held to these results bit for bit (tests/test_gpu_simplify.py); tests/test_simplify_ref_host.py checks the definition
against itself.  Also the meshes both test files use.

Where the trim lands: a collapse removes exactly two faces (its edge has two faces, the link condition keeps every other face of i
distinct), so the parity of the face count never changes: a run that is not stalled and not out of rounds ends at target_faces when
(faces_before - target_faces) is even and at target_faces - 1 when it is odd.
"""
import math

import numpy as np

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
K_RC = [(r, c) for r in range(4) for c in range(r, 4)]            # 00 01 02 03 11 12 13 22 23 33


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _normal(p0, p1, p2):
    x, y = p1 - p0, p2 - p0
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], -1)


def _expand(start, count):
    """(owner, position) of the ragged ranges [start[k], start[k] + count[k])"""
    count = np.asarray(count, np.int64)
    owner = np.repeat(np.arange(len(count), dtype=np.int64), count)
    first = np.cumsum(count) - count
    pos = np.arange(int(count.sum()), dtype=np.int64) - np.repeat(first, count) + np.repeat(np.asarray(start, np.int64), count)
    return owner, pos


def vertex_face_csr(faces, Vm):
    """(offsets int64 [Vm+1], face ids int64 [3F]): the faces at each vertex, ascending (deform.vertex_face_adjacency)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    vid = f.reshape(-1)
    fid = np.repeat(np.arange(len(f), dtype=np.int64), 3)
    order = np.argsort(vid, kind="stable")
    off = np.zeros(Vm + 1, np.int64)
    np.cumsum(np.bincount(vid, minlength=Vm), out=off[1:])
    return off, fid[order]


def edges_ref(faces, Vm):
    """(edges int64 [E,2] lo < hi sorted by lo Vm + hi, face count of each int64 [E])"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    k, cnt = np.unique(e.min(1) * Vm + e.max(1), return_counts=True)
    return np.stack([k // Vm, k % Vm], 1), cnt


def quadrics_ref(vertices, faces):
    """float32 [Vm,10]"""
    V = np.asarray(vertices, f32).reshape(-1, 3)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    Vm = len(V)
    Q = np.zeros((Vm, 10), f32)
    if len(F) == 0:
        return Q
    off, adj = vertex_face_csr(F, Vm)
    with np.errstate(all="ignore"):
        a = V[F[:, 0]]
        n = _normal(a, V[F[:, 1]], V[F[:, 2]])
        l = np.sqrt(_dot(n, n))
        ok = (l > 0) & (l <= FLT_MAX)
        u = n / l[:, None]
        p = np.concatenate([u, (-_dot(u, a))[:, None]], 1)
        area = l * f32(0.5)
        add = np.stack([area * (p[:, r] * p[:, c]) for r, c in K_RC], 1)
        cnt = off[1:] - off[:-1]
        for s in range(int(cnt.max())):
            vs = np.nonzero(cnt > s)[0]
            f = adj[off[vs] + s]
            g = ok[f]
            Q[vs[g]] = Q[vs[g]] + add[f[g]]
    return Q


def quadrics_f64(vertices, faces):
    """the same sums in float64 (degenerate faces skipped by the float32 rule), for the rounding check"""
    V32 = np.asarray(vertices, f32).reshape(-1, 3)
    V = V32.astype(np.float64)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    Q = np.zeros((len(V), 10))
    with np.errstate(all="ignore"):
        n32 = _normal(V32[F[:, 0]], V32[F[:, 1]], V32[F[:, 2]])
        l32 = np.sqrt(_dot(n32, n32))
        ok = (l32 > 0) & (l32 <= FLT_MAX)
    for f in np.nonzero(ok)[0]:
        a, b, c = V[F[f]]
        n = np.cross(b - a, c - a)
        l = np.linalg.norm(n)
        p = np.append(n / l, -np.dot(n / l, a))
        add = np.array([0.5 * l * p[r] * p[c] for r, c in K_RC])
        for v in F[f]:
            Q[v] += add
    return Q


def _direction(V, Q, F, off, adj, i, j, mc2, max_error):
    """(stands, cost) of the collapses i[k] -> j[k]"""
    n = len(i)
    cnt = off[i + 1] - off[i]
    owner, pos = _expand(off[i], cnt)
    ids = F[adj[pos]]
    io, jo = i[owner], j[owner]
    with np.errstate(all="ignore"):
        hasj = (ids == jo[:, None]).any(1)
        p = V[ids]
        n0 = _normal(p[:, 0], p[:, 1], p[:, 2])
        p1 = np.where((ids == io[:, None])[:, :, None], V[jo][:, None, :], p)
        n1 = _normal(p1[:, 0], p1[:, 1], p1[:, 2])
        d, sq = _dot(n0, n1), _dot(n0, n0) * _dot(n1, n1)
        dd = d * d
        good = (d > 0) & (dd <= FLT_MAX) & (sq <= FLT_MAX) & (dd >= mc2 * sq)
        flip_ok = np.bincount(owner[~good & ~hasj], minlength=n) == 0
        q = Q[i] + Q[j]
        x, y, z = V[j, 0], V[j, 1], V[j, 2]
        r0 = ((q[:, 0] * x + q[:, 1] * y) + q[:, 2] * z) + q[:, 3]
        r1 = ((q[:, 1] * x + q[:, 4] * y) + q[:, 5] * z) + q[:, 6]
        r2 = ((q[:, 2] * x + q[:, 5] * y) + q[:, 7] * z) + q[:, 8]
        r3 = ((q[:, 3] * x + q[:, 6] * y) + q[:, 8] * z) + q[:, 9]
        c = ((x * r0 + y * r1) + z * r2) + r3
        fin = np.abs(c) <= FLT_MAX
        cost = np.where(c > 0, c, f32(0)).astype(f32)
        ok = flip_ok & fin & ~(cost > max_error)
    return ok, cost


def round_ref(vertices, quadrics, faces, min_cos=0.2, max_error=None):
    """One round on the live faces: dict(edges [E,2], uses [E], locked bool [Vm], key uint64 [E], frm / to int64 [E] (-1: no
    candidate), selected bool [E], neighbours (row, col) of the closed vertex neighbourhoods)"""
    V = np.asarray(vertices, f32).reshape(-1, 3)
    Q = np.asarray(quadrics, f32).reshape(-1, 10)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    Vm = len(V)
    mc2 = f32(min_cos) * f32(min_cos)
    max_error = f32(np.inf) if max_error is None else f32(max_error)
    edges, uses = edges_ref(F, Vm)
    E = len(edges)
    off, adj = vertex_face_csr(F, Vm)
    locked = np.zeros(Vm, bool)
    locked[edges[uses != 2].reshape(-1)] = True
    # closed neighbourhoods: (v, w) for every pair of corners of one face, v == w included
    nk = np.unique((F[:, :, None] * Vm + F[:, None, :]).reshape(-1))
    nrow, ncol = nk // Vm, nk % Vm
    noff = np.zeros(Vm + 1, np.int64)
    np.cumsum(np.bincount(nrow, minlength=Vm), out=noff[1:])
    lo, hi = edges[:, 0], edges[:, 1]
    # link: distinct w outside {lo, hi} adjacent to both
    owner, pos = _expand(noff[lo], noff[lo + 1] - noff[lo])
    w = ncol[pos]
    q = hi[owner] * Vm + w
    at = np.minimum(np.searchsorted(nk, q), len(nk) - 1)
    both = (w != lo[owner]) & (w != hi[owner]) & (nk[at] == q)
    common = np.bincount(owner[both], minlength=E)
    # the edge part: a face of lo without hi whose other two corners (a < b) lie in one face of hi
    others = np.sort(np.stack([F[:, [1, 2]], F[:, [0, 2]], F[:, [0, 1]]], 1), axis=2)      # [F, corner, 2]: the corners besides it
    tri = np.unique(((F * Vm + others[:, :, 0]) * Vm + others[:, :, 1]).reshape(-1))        # (v, a, b) of every face at v
    owner, pos = _expand(off[lo], off[lo + 1] - off[lo])
    ids = F[adj[pos]]
    mine = ids == lo[owner][:, None]
    ab = others[adj[pos]][mine]                                      # a live face holds lo once
    q = (hi[owner] * Vm + ab[:, 0]) * Vm + ab[:, 1]
    at = np.minimum(np.searchsorted(tri, q), len(tri) - 1)
    folded = np.bincount(owner[~(ids == hi[owner][:, None]).any(1) & (tri[at] == q)], minlength=E) > 0
    base = (uses == 2) & (common == 2) & ~folded
    try_hi = np.nonzero(base & ~locked[hi])[0]                       # hi -> lo
    try_lo = np.nonzero(base & ~locked[lo])[0]
    ok_hi, ok_lo = np.zeros(E, bool), np.zeros(E, bool)
    c_hi, c_lo = np.zeros(E, f32), np.zeros(E, f32)
    ok_hi[try_hi], c_hi[try_hi] = _direction(V, Q, F, off, adj, hi[try_hi], lo[try_hi], mc2, max_error)
    ok_lo[try_lo], c_lo[try_lo] = _direction(V, Q, F, off, adj, lo[try_lo], hi[try_lo], mc2, max_error)
    cand = ok_hi | ok_lo
    take_lo = ok_lo & (~ok_hi | (c_lo < c_hi))
    frm = np.where(cand, np.where(take_lo, lo, hi), -1)
    to = np.where(cand, np.where(take_lo, hi, lo), -1)
    cost = np.where(take_lo, c_lo, c_hi).astype(f32)
    key = np.where(cand, (cost.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(E, dtype=np.uint64), NONE)
    vmin = np.full(Vm, NONE, np.uint64)
    ce = np.nonzero(cand)[0]
    np.minimum.at(vmin, lo[ce], key[ce])
    np.minimum.at(vmin, hi[ce], key[ce])
    rmin = vmin.copy()
    np.minimum.at(rmin, nrow, vmin[ncol])
    selected = np.zeros(E, bool)
    selected[ce] = key[ce] == np.minimum(rmin[lo[ce]], rmin[hi[ce]])
    return dict(edges=edges, uses=uses, locked=locked, key=key, frm=frm, to=to, selected=selected, cost=cost, neighbours=(nrow, ncol))


def resolve_target(n_faces, target_faces=None, ratio=None, max_error=None):
    """the face count a call asks for: target_faces, or floor(ratio * faces), or 0 when only max_error stops the run"""
    if target_faces is not None and ratio is not None:
        raise ValueError("simplify: give target_faces or ratio, not both")
    if target_faces is None and ratio is None:
        if max_error is None:
            raise ValueError("simplify: give target_faces, ratio or max_error")
        return 0
    if ratio is not None:
        ratio = float(ratio)
        if not (math.isfinite(ratio) and 0.0 < ratio <= 1.0):
            raise ValueError("simplify: ratio must be in (0, 1]; got %r" % (ratio,))
        return int(math.floor(ratio * n_faces))
    if int(target_faces) != target_faces or target_faces < 0:
        raise ValueError("simplify: target_faces must be a non-negative integer; got %r" % (target_faces,))
    return int(target_faces)


def simplify_ref(vertices, faces, target_faces=None, ratio=None, max_error=None, min_cos=0.2, max_rounds=1024, trace=None):
    """dict(vertices, faces int32, kept, vertex_map, rounds, stalled, faces_before, locked_vertices, max_cost).  trace(round index,
    live faces before, round_ref's dict plus quadrics_before / quadrics_after, applied mask, live faces after) is called after every
    applied round."""
    V = np.asarray(vertices, f32).reshape(-1, 3)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    Vm = len(V)
    target = resolve_target(len(F), target_faces, ratio, max_error)
    live = F[(F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 2] != F[:, 0])]        # faces with a repeated corner go first
    parent = np.arange(Vm, dtype=np.int64)
    rounds, stalled, max_cost, locked_vertices, n_live0 = 0, False, f32(0), 0, len(live)
    if len(live) > target:
        Q = quadrics_ref(V, live)
        e0, u0 = edges_ref(live, Vm)
        locked_vertices = len(np.unique(e0[u0 != 2]))
    while len(live) > target and rounds < max_rounds:
        r = round_ref(V, Q, live, min_cos, max_error)
        sel = r["selected"].copy()
        n = int(sel.sum())
        if n == 0:
            stalled = True
            break
        if len(live) - 2 * n < target:
            k = (len(live) - target + 1) // 2
            sel &= r["key"] <= np.sort(r["key"][sel])[k - 1]
        i, j = r["frm"][sel], r["to"][sel]
        r["quadrics_before"] = Q.copy()
        Q[j] = Q[i] + Q[j]
        r["quadrics_after"] = Q.copy()
        max_cost = max(max_cost, r["cost"][sel].max())
        remap = np.arange(Vm, dtype=np.int64)
        remap[i] = j
        parent[i] = j
        before = live
        live = remap[live]
        live = live[(live[:, 0] != live[:, 1]) & (live[:, 1] != live[:, 2]) & (live[:, 2] != live[:, 0])]
        if trace is not None:
            trace(rounds, before, r, sel, live)
        rounds += 1
    kept = np.unique(live)
    index = np.full(Vm, -1, np.int64)
    index[kept] = np.arange(len(kept))
    root = parent.copy()
    while True:
        nxt = root[root]
        if np.array_equal(nxt, root):
            break
        root = nxt
    return dict(vertices=V[kept], faces=index[live].astype(np.int32), kept=kept, vertex_map=index[root], rounds=rounds, stalled=stalled,
                faces_before=len(F), locked_vertices=locked_vertices, max_cost=float(max_cost), degenerate_faces=len(F) - n_live0,
                reached=len(live) <= target)


# ---- meshes ----
def tetrahedron():
    V = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], f32)
    return V, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)


def octahedron():
    V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)
    F = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    return V, np.array(F, np.int32)


def icosahedron():
    t = (1.0 + 5.0 ** 0.5) / 2.0
    V = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
                  [-t, 0, -1], [-t, 0, 1]], f32)
    F = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8], [3, 9, 4],
         [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    return V, np.array(F, np.int32)


def torus(nu, nv, R=2.0, r=0.7, offset=(0.0, 0.0, 0.0)):
    """scenes.torus_mesh in float32: nu nv vertices, 2 nu nv faces, 3 nu nv edges"""
    u = np.arange(nu) * (2 * math.pi / nu)
    v = np.arange(nv) * (2 * math.pi / nv)
    U, W = np.meshgrid(u, v, indexing="ij")
    X, Y, Z = (R + r * np.cos(W)) * np.cos(U), r * np.sin(W), (R + r * np.cos(W)) * np.sin(U)
    verts = np.stack([X, Y, Z], -1).reshape(-1, 3) + np.asarray(offset, np.float64)
    idx = np.arange(nu * nv).reshape(nu, nv)
    a, b, c, d = idx, np.roll(idx, -1, 0), np.roll(np.roll(idx, -1, 0), -1, 1), np.roll(idx, -1, 1)
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)], 0)
    return verts.astype(f32), faces.astype(np.int32)


def join(*meshes):
    Vs, Fs, n = [], [], 0
    for V, F in meshes:
        Vs.append(np.asarray(V, f32))
        Fs.append(np.asarray(F, np.int32) + n)
        n += len(V)
    return np.concatenate(Vs), np.concatenate(Fs).astype(np.int32)


def two_tori():
    return join(torus(12, 9), torus(10, 8, offset=(0.0, 5.0, 0.0)))


def grid_patch(a, b, height=None, origin=(0.0, 0.0, 0.0)):
    """(a + 1) (b + 1) vertices over a x b unit quads in the plane z = 0 (or z = height(x, y)): 2 a b faces, 3 a b + a + b edges"""
    x, y = np.meshgrid(np.arange(a + 1, dtype=np.float64), np.arange(b + 1, dtype=np.float64), indexing="ij")
    z = np.zeros_like(x) if height is None else height(x, y)
    V = np.stack([x, y, z], -1).reshape(-1, 3) + np.asarray(origin, np.float64)
    idx = np.arange((a + 1) * (b + 1)).reshape(a + 1, b + 1)
    p, q, r, s = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    F = np.concatenate([np.stack([p, q, r], -1).reshape(-1, 3), np.stack([p, r, s], -1).reshape(-1, 3)], 0)
    return V.astype(f32), F.astype(np.int32)


def flat_patch():
    """every cost is exactly +0: the edge-id half of the key decides"""
    return grid_patch(9, 7)


def bumpy_patch():
    return grid_patch(11, 9, height=lambda x, y: 0.6 * np.sin(0.9 * x) * np.cos(0.7 * y))


def edges_255():
    return torus(17, 5)                                               # 3 * 85


def edges_256():
    return join(torus(9, 9), grid_patch(1, 3, origin=(6.0, 0.0, 0.0)))      # 243 + 13


def edges_257():
    return join(torus(12, 7), grid_patch(1, 1, origin=(6.0, 0.0, 0.0)))     # 252 + 5


def nets(field):
    """the surface-nets mesh of one of tsdf_ref's fields"""
    import tsdf_ref as tr
    V, F = tr.surface_nets_ref(*field)
    return np.asarray(V, f32), np.asarray(F, np.int32)


def sphere_nets(n=20):
    import tsdf_ref as tr
    return nets(tr.sphere_field((n, n, n)))


def torus_nets():
    import tsdf_ref as tr
    return nets(tr.torus_field((24, 12, 24)))


def plane_nets():
    import tsdf_ref as tr
    return nets(tr.plane_field((9, 8, 7)))


def noise_nets():
    import tsdf_ref as tr
    return nets(tr.noise_field((9, 8, 7), seed=3))


def four_face_edge():
    """two tetrahedra that share the edge (0, 1): four faces on it, its ends locked"""
    V = np.array([[0, 0, 0], [0, 0, 1], [1, 0.2, 0.5], [0.3, 1, 0.5], [-1, -0.2, 0.5], [-0.3, -1, 0.4]], f32)
    F = [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2], [0, 4, 1], [0, 1, 5], [0, 5, 4], [1, 4, 5]]
    return V, np.array(F, np.int32)


def four_face_edge_fine():
    """the same defect inside a mesh with something to collapse: a torus and its point reflection about the middle of its edge (0, 1),
    which swaps that edge's ends: the two share the edge and nothing else"""
    V1, F1 = torus(10, 8)
    V2 = (V1[0] + V1[1]) - V1
    F2 = F1[:, ::-1].copy()                                            # the point reflection flips orientation: flip the rows back
    V, F = join((V1, F1), (V2, F2))
    n = len(V1)
    F = F.astype(np.int64)
    F[F == n + 0] = 1                                                  # copy 2's vertex 0 sits on p1, its vertex 1 on p0
    F[F == n + 1] = 0
    return V, F.astype(np.int32)                                       # (vertices n and n + 1 are left unreferenced)


def dirty_mesh():
    """what an OBJ from elsewhere may hold: a torus with two faces that repeat a corner (dropped before the first round) and one face
    given twice (kept: its edges then have three faces and their ends are locked)"""
    V, F = torus(12, 9)
    extra = np.array([[5, 5, 17], [30, 41, 30], F[50].tolist()], np.int32)
    return V, np.concatenate([F[:20], extra[:1], F[20:], extra[1:]]).astype(np.int32)


def zero_area_face():
    """an icosahedron with one vertex moved onto its neighbour: the faces holding both have zero area"""
    V, F = icosahedron()
    V = V.copy()
    V[5] = V[1]
    return V, F


def unreferenced_vertex(nu=16, nv=16):
    V, F = torus(nu, nv)
    return np.concatenate([V, np.array([[9, 9, 9]], f32)]), F


def nan_vertex():
    V, F = torus(14, 10)
    V = V.copy()
    V[37, 1] = np.nan
    return V, F


def fan(n=70):
    """a bipyramid over an n-gon: both apexes have valence n"""
    t = np.arange(n) * (2 * math.pi / n)
    ring = np.stack([np.cos(t), np.sin(t), 0.05 * np.cos(3 * t)], -1)
    V = np.concatenate([ring, [[0, 0, 0.8], [0, 0, -0.6]]]).astype(f32)
    k, k1 = np.arange(n), (np.arange(n) + 1) % n
    F = np.concatenate([np.stack([k, k1, np.full(n, n)], -1), np.stack([k1, k, np.full(n, n + 1)], -1)])
    return V, F.astype(np.int32)


BUILDERS = dict(tetrahedron=tetrahedron, octahedron=octahedron, icosahedron=icosahedron, torus_16x16=lambda: torus(16, 16),
                torus_17x15=lambda: torus(17, 15), torus_257=unreferenced_vertex, torus_7x5=lambda: torus(7, 5), sphere_nets=lambda: sphere_nets(12),
                torus_nets=torus_nets, plane_nets=plane_nets, noise_nets=noise_nets, four_face_edge=four_face_edge,
                four_face_edge_fine=four_face_edge_fine, two_tori=two_tori, zero_area_face=zero_area_face, nan_vertex=nan_vertex, fan=fan,
                flat_patch=flat_patch, bumpy_patch=bumpy_patch, edges_255=edges_255, edges_256=edges_256, edges_257=edges_257)


# ---- invariants the tests share ----
def closed_neighbourhood_sets(Vm, neighbours):
    nrow, ncol = neighbours
    out = [set() for _ in range(Vm)]
    for v, w in zip(nrow.tolist(), ncol.tolist()):
        out[v].add(w)
    return out


def face_normals64(V, F):
    v = np.asarray(V, np.float64)
    f = np.asarray(F, np.int64).reshape(-1, 3)
    return np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
