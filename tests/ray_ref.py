"""The definition of gm_ray_mesh restated in numpy (include/gmesh_hip.h): a float32 brute force over all faces.  Every product and sum
is written out per component on np.float32 arrays (numpy neither contracts nor reorders them, and its float32 division is correctly
rounded), so the arrays below are, bit for bit, what the device must produce.  The same lines run in float64 (dtype=np.float64) for the
sanity checks of the definition itself."""
import numpy as np

f32 = np.float32


def _dot(xx, xy, xz, yx, yy, yz):
    return (xx * yx + xy * yy) + xz * yz


def ray_face(O, D, A, B, C, t_min=0.0, t_max=np.inf, dtype=f32):
    """(hit, t, u, v) of ray rows (O, D) [..,3] against triangle rows (A, B, C) [..,3] (broadcast against each other) in dtype."""
    O, D, A, B, C = (np.asarray(x, dtype) for x in (O, D, A, B, C))
    t_min, t_max = dtype(t_min), dtype(t_max)
    ox, oy, oz = O[..., 0], O[..., 1], O[..., 2]
    dx, dy, dz = D[..., 0], D[..., 1], D[..., 2]
    ax, ay, az = A[..., 0], A[..., 1], A[..., 2]
    e1x, e1y, e1z = B[..., 0] - ax, B[..., 1] - ay, B[..., 2] - az
    e2x, e2y, e2z = C[..., 0] - ax, C[..., 1] - ay, C[..., 2] - az
    with np.errstate(all="ignore"):
        px, py, pz = dy * e2z - dz * e2y, dz * e2x - dx * e2z, dx * e2y - dy * e2x
        det = _dot(e1x, e1y, e1z, px, py, pz)
        sx, sy, sz = ox - ax, oy - ay, oz - az
        qx, qy, qz = sy * e1z - sz * e1y, sz * e1x - sx * e1z, sx * e1y - sy * e1x
        inv = dtype(1.0) / det
        u = _dot(sx, sy, sz, px, py, pz) * inv
        v = _dot(dx, dy, dz, qx, qy, qz) * inv
        t = _dot(e2x, e2y, e2z, qx, qy, qz) * inv
        zero, one = dtype(0.0), dtype(1.0)
        hit = (u >= zero) & (v >= zero) & ((u + v) <= one) & (t >= t_min) & (t <= t_max)            # every comparison False on NaN
    assert t.dtype == dtype and u.dtype == dtype and v.dtype == dtype
    return hit, t, u, v


def ray_mesh_ref(origins, dirs, vertices, faces, t_min=0.0, t_max=np.inf, chunk=None, dtype=f32):
    """(t dtype [R], face int64 [R], uv dtype [R,2]): per ray the hit with the smallest t, the lowest face index among equals, reported
    as t + 0 (so -0 becomes +0); no hit: face -1, t +inf, uv NaN."""
    O = np.ascontiguousarray(origins, dtype).reshape(-1, 3)
    D = np.ascontiguousarray(dirs, dtype).reshape(-1, 3)
    V = np.ascontiguousarray(vertices, dtype)
    F = np.asarray(faces, np.int64)
    A, B, C = V[F[:, 0]][None], V[F[:, 1]][None], V[F[:, 2]][None]
    R = len(O)
    chunk = max(1, min(512, 2000000 // max(1, len(F)))) if chunk is None else chunk                  # ~2 M ray-face pairs at a time
    out_t = np.full(R, np.inf, dtype); idx = np.full(R, -1, np.int64); uv = np.full((R, 2), np.nan, dtype)
    for s in range(0, R, chunk):
        hit, t, u, v = ray_face(O[s:s + chunk][:, None, :], D[s:s + chunk][:, None, :], A, B, C, t_min, t_max, dtype)
        t = t + dtype(0.0)                                           # -0 -> +0: both compare equal, the index decides between them
        key = np.where(hit, t, dtype(np.inf))
        k = np.argmin(key, axis=1)                                   # the first (lowest index) of the smallest
        rows = np.arange(len(k))
        stray = ~hit[rows, k]                                        # the smallest is +inf and its first holder is no hit: take the first
        if stray.any():                                              # hit (its t is +inf, accepted when t_max is), if there is one
            k[stray] = np.where(hit[stray].any(axis=1), np.argmax(hit[stray], axis=1), -1)
        ok = k >= 0
        kk = np.where(ok, k, 0)
        out_t[s:s + chunk] = np.where(ok, t[rows, kk], dtype(np.inf))
        idx[s:s + chunk] = k
        uv[s:s + chunk, 0] = np.where(ok, u[rows, kk], dtype(np.nan))
        uv[s:s + chunk, 1] = np.where(ok, v[rows, kk], dtype(np.nan))
    return out_t, idx, uv


# ---- the meshes and ray families of the tests (seeded) ----
def fit(faces, F):
    """F faces out of a list: a prefix, or the list repeated (then faces are present more than once)"""
    return np.resize(faces, (F, 3)).astype(np.int32)


def grid(F):
    """A regular grid in the plane z = 0, vertex coordinates multiples of 1/4, EVERY FACE PRESENT TWICE (the second copy behind the
    first in the list): every hit is an exact tie, the lowest index has to win."""
    n = int(np.ceil(np.sqrt(max(F, 2) / 4.0))) + 1
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2) * 0.25
    V = np.concatenate([g, np.zeros((n * n, 1))], 1).astype(f32)
    idx = np.arange(n * n).reshape(n, n)
    base = np.concatenate([np.stack([idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:]], -1).reshape(-1, 3),
                           np.stack([idx[:-1, :-1], idx[1:, 1:], idx[:-1, 1:]], -1).reshape(-1, 3)], 0)
    half = max(1, F // 2)
    return V, fit(np.concatenate([base[:half], base[:half]], 0), F)


def grid_rays(V, R, rng):
    """Rays at the grid of grid(): through vertices, edge midpoints (three directions) and interiors, straight down or slanted (by
    multiples of 1/4, so the products stay exact and the ties exact); kinds mixed in: parallel to the plane in it and above it
    (det = 0), origin ON the plane (t = +-0), origin beyond the plane (t < 0: no hit), a zero direction, a ray past the grid's edge."""
    n = int(round(np.sqrt(len(V))))
    i = rng.integers(max(n - 1, 1), size=(R, 2)).astype(np.float64)
    where = np.array([[0, 0], [0.5, 0], [0, 0.5], [0.5, 0.5], [0.25, 0.25], [0.75, 0.5]])[rng.integers(6, size=R)]
    target = np.concatenate([(i + where) * 0.25, np.zeros((R, 1))], 1)
    D = np.concatenate([rng.integers(-2, 3, size=(R, 2)) * 0.25, -np.ones((R, 1))], 1)
    D[rng.random(R) < 0.3, 2] = 1.0                                # from below as well: the test is two-sided
    height = rng.choice([1.0, 2.0, 0.5], size=R)
    O = target - D * height[:, None]
    kind = rng.integers(10, size=R)
    D[kind == 0, 2] = 0.0; O[kind == 0, 2] = 0.0                   # in the plane
    D[kind == 1, 2] = 0.0; O[kind == 1, 2] = 0.5                   # parallel above it
    O[kind == 2] = target[kind == 2]                               # origin on the plane: t = 0 with either sign
    O[kind == 3] = target[kind == 3] + D[kind == 3]                # origin beyond the plane: t = -1
    D[kind == 4] = 0.0                                             # no direction
    O[kind == 5, :2] += 40.0                                       # past the edge
    return O.astype(f32), D.astype(f32)


def torus(F, nu=24, nv=16):
    from gaussianmesh_amd import scenes
    verts, faces = scenes.torus_mesh(nu, nv)
    return verts.astype(f32), fit(faces, F)


def torus_rays(V, faces, R, rng):
    """Rays from a shell around the torus towards points of its faces (most pass through the surface two or four times), a share of them
    aimed past it"""
    Vd = np.asarray(V, np.float64)
    f = faces[rng.integers(len(faces), size=R)]
    w = rng.dirichlet((1.0, 1.0, 1.0), size=R)
    target = w[:, :1] * Vd[f[:, 0]] + w[:, 1:2] * Vd[f[:, 1]] + w[:, 2:] * Vd[f[:, 2]]
    O = rng.normal(size=(R, 3)); O *= rng.uniform(4.0, 7.0, size=(R, 1)) / np.linalg.norm(O, axis=1, keepdims=True)
    away = rng.random(R) < 0.15
    target[away] += rng.normal(0.0, 3.0, size=(int(away.sum()), 3))
    D = (target - O) * rng.uniform(0.3, 2.0, size=(R, 1))          # not normalised: t is in units of |d|
    return O.astype(f32), D.astype(f32)


def with_degenerate_faces(V, faces, rng, share=0.2):
    """a share of the faces made zero-area in place: two equal corners, or three"""
    faces = faces.copy()
    k = np.nonzero(rng.random(len(faces)) < share)[0]
    faces[k, 1] = faces[k, 0]
    faces[k[::2], 2] = faces[k[::2], 0]
    return faces
