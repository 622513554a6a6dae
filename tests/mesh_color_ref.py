"""The definitions of gm_mesh_vertex_normals, gm_mesh_color_integrate and gm_mesh_color_spread restated in numpy (include/gmesh_hip.h).
Every product, sum and quotient is written out on np.float32 arrays in the header's order (numpy neither contracts nor reorders them, and
its float32 division is correctly rounded), so the arrays below are, bit for bit, what the device must produce.  Camera rows as in
tsdf_ref.camera_rows: views [K,4,4] stored transposed, tanfov [K,2]."""
import numpy as np

f32 = np.float32
ONE, HALF, ZERO = f32(1.0), f32(0.5), f32(0.0)


def adjacency(faces, Vm):
    """(offsets int32 [Vm+1], face ids int32 [3F]): the faces at each vertex in ascending face order (deform.vertex_face_adjacency)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    vid = f.reshape(-1)
    fid = np.repeat(np.arange(f.shape[0], dtype=np.int64), 3)
    order = np.argsort(vid, kind="stable")
    offsets = np.zeros(Vm + 1, np.int64)
    np.cumsum(np.bincount(vid, minlength=Vm), out=offsets[1:])
    return offsets.astype(np.int32), fid[order].astype(np.int32)


def _rounds(off):
    """the CSR walked in step: round r holds, for every vertex with more than r entries, (vertex, slot off[vertex] + r)"""
    off = np.asarray(off, np.int64)
    deg = off[1:] - off[:-1]
    for r in range(int(deg.max()) if len(deg) else 0):
        v = np.nonzero(deg > r)[0]
        yield v, off[v] + r


def vertex_normals_ref(vertices, faces, adj=None):
    """float32 [Vm,3]: N = 0, then N = N + cross(V[b] - V[a], V[c] - V[a]) over the vertex's faces in adjacency order"""
    V = np.asarray(vertices, f32).reshape(-1, 3)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    off, adj = adjacency(F, len(V)) if adj is None else adj
    N = np.zeros((len(V), 3), f32)
    with np.errstate(all="ignore"):
        for v, slot in _rounds(off):
            t = F[np.asarray(adj, np.int64)[slot]]
            a, b, c = V[t[:, 0]], V[t[:, 1]], V[t[:, 2]]
            e1, e2 = b - a, c - a
            cr = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                           e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
            assert cr.dtype == f32
            N[v] = N[v] + cr
    return N


def integrate_ref(csum, wsum, image, depth, alpha, views, tanfov, vertices, normals, alpha_min=0.5, depth_tol=0.0, two_sided=False):
    """(csum float32 [Vm,3], wsum float32 [Vm]) after the K views of image [K,3,H,W], depth / alpha [K,H,W]"""
    cs, ws = np.array(csum, f32, copy=True).reshape(-1, 3), np.array(wsum, f32, copy=True).reshape(-1)
    image, depth, alpha = np.asarray(image, f32), np.asarray(depth, f32), np.asarray(alpha, f32)
    K, H, W = depth.shape
    views, tanfov = np.asarray(views, f32).reshape(K, 4, 4), np.asarray(tanfov, f32).reshape(K, 2)
    P, N = np.asarray(vertices, f32).reshape(-1, 3), np.asarray(normals, f32).reshape(-1, 3)
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    NX, NY, NZ = N[:, 0], N[:, 1], N[:, 2]
    alpha_min, tol = f32(alpha_min), f32(depth_tol)
    fW, fH = f32(W), f32(H)
    for k in range(K):
        v, tx, ty = views[k], tanfov[k, 0], tanfov[k, 1]
        with np.errstate(all="ignore"):
            xv = ((X * v[0, 0] + Y * v[1, 0]) + Z * v[2, 0]) + v[3, 0]
            yv = ((X * v[0, 1] + Y * v[1, 1]) + Z * v[2, 1]) + v[3, 1]
            zv = ((X * v[0, 2] + Y * v[1, 2]) + Z * v[2, 2]) + v[3, 2]
            ok = zv > 0
            px = ((xv / (zv * tx) + ONE) * fW - ONE) * HALF
            py = ((yv / (zv * ty) + ONE) * fH - ONE) * HALF
            fx, fy = np.floor(px + HALF), np.floor(py + HALF)
            ok = ok & (fx >= 0) & (fx < fW) & (fy >= 0) & (fy < fH)
            ix, iy = np.where(ok, fx, 0).astype(np.int64), np.where(ok, fy, 0).astype(np.int64)
            a, d = alpha[k][iy, ix], depth[k][iy, ix]
            ok = ok & (a >= alpha_min)
            s = d / a - zv
            ok = ok & (s >= -tol) & (s <= tol)
            nvx = (NX * v[0, 0] + NY * v[1, 0]) + NZ * v[2, 0]
            nvy = (NX * v[0, 1] + NY * v[1, 1]) + NZ * v[2, 1]
            nvz = (NX * v[0, 2] + NY * v[1, 2]) + NZ * v[2, 2]
            dd = (nvx * xv + nvy * yv) + nvz * zv
            if not two_sided:
                ok = ok & (dd < 0)
            nn = (nvx * nvx + nvy * nvy) + nvz * nvz
            pp = (xv * xv + yv * yv) + zv * zv
            wgt = (dd * dd) / (nn * pp)
            ok = ok & (wgt > 0)
            c = image[k][:, iy, ix]                                     # [3,Vm]
            ok = ok & ((c - c) == 0).all(axis=0)
            new_c = cs + (wgt[None, :] * c).T
            new_w = ws + wgt
        assert new_c.dtype == f32 and new_w.dtype == f32 and wgt.dtype == f32 and s.dtype == f32
        cs, ws = np.where(ok[:, None], new_c, cs), np.where(ok, new_w, ws)
    return cs, ws


def resolve_ref(csum, wsum, min_weight=0.0, fallback=(0.5, 0.5, 0.5)):
    """(colors float32 [Vm,3], seen bool [Vm]): csum / wsum where wsum > 0 and wsum >= min_weight, fallback elsewhere"""
    cs, ws = np.asarray(csum, f32).reshape(-1, 3), np.asarray(wsum, f32).reshape(-1)
    with np.errstate(all="ignore"):
        seen = (ws > 0) & (ws >= f32(min_weight))
        q = cs / ws[:, None]
    return np.where(seen[:, None], q, np.asarray(fallback, f32)[None, :]).astype(f32), seen


def spread_ref(faces, seen, colors, iterations, fallback=(0.5, 0.5, 0.5), adj=None):
    """(colors float32 [Vm,3], has uint8 [Vm], counts int32 [2] = {filled, unreached}) after `iterations` Jacobi steps"""
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    seen = np.asarray(seen) != 0
    Vm = len(seen)
    off, adj = adjacency(F, Vm) if adj is None else adj
    adj = np.asarray(adj, np.int64)
    col = np.where(seen[:, None], np.asarray(colors, f32).reshape(-1, 3), ZERO).astype(f32)
    has = seen.copy()
    for _ in range(int(iterations)):
        s = np.zeros((Vm, 3), f32)
        n = np.zeros(Vm, np.int64)
        with np.errstate(all="ignore"):
            for v, slot in _rounds(off):
                t = F[adj[slot]]
                for q in range(3):
                    u = t[:, q]
                    take = (u != v) & has[u]
                    s[v] = np.where(take[:, None], s[v] + col[u], s[v])
                    n[v] += take
            upd = ~seen & (n > 0)
            mean = s / n.astype(f32)[:, None]
        assert mean.dtype == f32
        col, has = np.where(upd[:, None], mean, col), has | upd
    col = np.where(has[:, None], col, np.asarray(fallback, f32)[None, :]).astype(f32)
    counts = np.array([int((has & ~seen).sum()), int((~has).sum())], np.int32)
    return col, has.astype(np.uint8), counts


# ---- meshes of the tests ----
def octahedron():
    """(vertices float32 [6,3], faces int32 [8,3]) wound outwards: every vertex normal is 4 times its own position"""
    V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)
    F = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return V, F


def strip(n):
    """a strip of n quads along x, 2 (n + 1) vertices: vertex 2 i at (i, 0, 0), 2 i + 1 at (i, 1, 0); the quad i is (2i, 2i+2, 2i+3), (2i, 2i+3, 2i+1)"""
    V = np.array([[i, j, 0] for i in range(n + 1) for j in range(2)], f32)
    F = np.array([t for i in range(n) for t in ((2 * i, 2 * i + 2, 2 * i + 3), (2 * i, 2 * i + 3, 2 * i + 1))], np.int32)
    return V, F


def edge_distance(faces, Vm, sources):
    """int64 [Vm]: the number of edges between every vertex and the nearest source (-1: no path)"""
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    dist = np.full(Vm, -1, np.int64)
    dist[np.asarray(sources, np.int64)] = 0
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]], 0)
    e = np.concatenate([e, e[:, ::-1]], 0)
    step = 0
    while True:
        front = (dist[e[:, 0]] == step) & (dist[e[:, 1]] < 0)
        if not front.any():
            return dist
        step += 1
        dist[e[front, 1]] = step
