"""The definition of gm_closest_face restated in numpy (include/gmesh_hip.h): a float32 brute force over all faces.  Every product and
sum is written out per component on np.float32 arrays (numpy neither contracts nor reorders them, and its float32 division is correctly
rounded), so the arrays below are, bit for bit, what the device must produce - whatever its search structure."""
import numpy as np

f32 = np.float32


def _dot(ux, uy, uz, wx, wy, wz):
    return (ux * wx + uy * wy) + uz * wz


def face_distance(P, A, B, C):
    """(dist2, qx, qy, qz) of point rows P [..,3] against triangle rows (A, B, C) [..,3] (broadcast against each other), float32."""
    P, A, B, C = (np.asarray(x, f32) for x in (P, A, B, C))
    px, py, pz = P[..., 0], P[..., 1], P[..., 2]
    ax, ay, az = A[..., 0], A[..., 1], A[..., 2]
    bx, by, bz = B[..., 0], B[..., 1], B[..., 2]
    cx, cy, cz = C[..., 0], C[..., 1], C[..., 2]
    abx, aby, abz = bx - ax, by - ay, bz - az
    acx, acy, acz = cx - ax, cy - ay, cz - az
    cbx, cby, cbz = cx - bx, cy - by, cz - bz
    apx, apy, apz = px - ax, py - ay, pz - az
    d1, d2 = _dot(abx, aby, abz, apx, apy, apz), _dot(acx, acy, acz, apx, apy, apz)
    bpx, bpy, bpz = px - bx, py - by, pz - bz
    d3, d4 = _dot(abx, aby, abz, bpx, bpy, bpz), _dot(acx, acy, acz, bpx, bpy, bpz)
    cpx, cpy, cpz = px - cx, py - cy, pz - cz
    d5, d6 = _dot(abx, aby, abz, cpx, cpy, cpz), _dot(acx, acy, acz, cpx, cpy, cpz)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(all="ignore"):
        denom = f32(1.0) / ((va + vb) + vc)
        v, w = vb * denom, vc * denom
        t_ab, t_ac = d1 / (d1 - d3), d2 / (d2 - d6)
        x, y = d4 - d3, d5 - d6
        t_bc = x / (x + y)
        q = [(ax + abx * v) + acx * w, (ay + aby * v) + acy * w, (az + abz * v) + acz * w]                       # interior
        zero = f32(0.0)
        for m, alt in (((va <= zero) & (x >= zero) & (y >= zero), (bx + cbx * t_bc, by + cby * t_bc, bz + cbz * t_bc)),          # edge bc
                       ((vb <= zero) & (d2 >= zero) & (d6 <= zero), (ax + acx * t_ac, ay + acy * t_ac, az + acz * t_ac)),        # edge ac
                       ((vc <= zero) & (d1 >= zero) & (d3 <= zero), (ax + abx * t_ab, ay + aby * t_ab, az + abz * t_ab)),        # edge ab
                       ((d6 >= zero) & (d5 <= d6), (cx, cy, cz)), ((d3 >= zero) & (d4 <= d3), (bx, by, bz)),                     # vertices c, b
                       ((d1 <= zero) & (d2 <= zero), (ax, ay, az))):                                                              # vertex a
            q = [np.where(m, alt[k], q[k]) for k in range(3)]                                                     # the later line wins
        ex, ey, ez = px - q[0], py - q[1], pz - q[2]
        dist2 = (ex * ex + ey * ey) + ez * ez
    assert dist2.dtype == f32 and q[0].dtype == f32
    return dist2, q[0], q[1], q[2]


def closest_face_ref(points, vertices, faces, chunk=None):
    """(d2 float32 [N], face int64 [N], closest float32 [N,3]): per point the face with the smallest dist2, the lowest index among equals,
    a NaN dist2 never taken; no face left: face -1, d2 +inf, closest NaN."""
    P = np.ascontiguousarray(points, f32).reshape(-1, 3)
    V = np.ascontiguousarray(vertices, f32)
    F = np.asarray(faces, np.int64)
    A, B, C = V[F[:, 0]][None], V[F[:, 1]][None], V[F[:, 2]][None]
    N = len(P)
    chunk = max(1, min(512, 2000000 // max(1, len(F)))) if chunk is None else chunk        # ~2 M point-face pairs at a time
    d2 = np.full(N, np.inf, f32); idx = np.full(N, -1, np.int64); close = np.full((N, 3), np.nan, f32)
    for s in range(0, N, chunk):
        p = P[s:s + chunk][:, None, :]
        d, qx, qy, qz = face_distance(p, A, B, C)
        valid = ~np.isnan(d)
        key = np.where(valid, d, f32(np.inf))
        k = np.argmin(key, axis=1)                                   # the first (lowest index) of the smallest
        rows = np.arange(len(k))
        miss = ~valid[rows, k]                                       # the smallest is +inf and its first holder is a NaN face:
        if miss.any():                                               # take the first face with a real (infinite) dist2, if there is one
            first = np.argmax(valid[miss], axis=1)
            k[miss] = np.where(valid[miss].any(axis=1), first, -1)
        ok = k >= 0
        kk = np.where(ok, k, 0)
        d2[s:s + chunk] = np.where(ok, d[rows, kk], f32(np.inf))
        idx[s:s + chunk] = k
        for j, qc in enumerate((qx, qy, qz)):
            close[s:s + chunk, j] = np.where(ok, np.broadcast_to(qc, d.shape)[rows, kk], f32(np.nan))
    return d2, idx, close


def distance_to_face(points, vertices, faces, face_id):
    """dist2 float32 [N] of every point to ONE given face each (an O(N) evaluation of the same arithmetic)."""
    V = np.ascontiguousarray(vertices, f32)
    T = np.asarray(faces, np.int64)[np.asarray(face_id, np.int64)]
    return face_distance(np.ascontiguousarray(points, f32).reshape(-1, 3), V[T[:, 0]], V[T[:, 1]], V[T[:, 2]])[0]


# ---- the query families of the tests (seeded) ----
def near_surface(verts, faces, n, rng, sigma=0.05):
    """n points within N(0, sigma) of the surface along the face normal (sigma = 0: on the surface), float32"""
    verts = np.asarray(verts, np.float64)
    f = faces[rng.integers(len(faces), size=n)]
    a, b, c = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
    w = rng.dirichlet((1.0, 1.0, 1.0), size=n)
    nrm = np.cross(b - a, c - a); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    p = w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c
    if sigma:
        p = p + rng.normal(0.0, sigma, size=(n, 1)) * nrm
    return p.astype(f32)
