"""The definitions of gm_tsdf_integrate and gm_surface_nets restated in numpy (include/gmesh_hip.h).  Every product, sum and quotient is
written out on np.float32 arrays in the header's order (numpy neither contracts nor reorders them, and its float32 division is correctly
rounded), so the arrays below are, bit for bit, what the device must produce.  Also here: the analytic volumes of the tests, ray-cast
depth maps of a mesh (through ray_ref's brute force), and the checks a proxy mesh has to pass (edge use, Euler characteristic,
components, signed volume)."""
import numpy as np

f32 = np.float32
ONE, HALF = f32(1.0), f32(0.5)


def voxel_centres(n, origin, voxel):
    """float32 [n]: origin + ((float)i + 0.5f) * voxel"""
    return f32(origin) + (np.arange(n, dtype=f32) + HALF) * f32(voxel)


def integrate_ref(tsdf, weight, depth, alpha, views, tanfov, origin, voxel, trunc, alpha_min=0.5, carve=True):
    """(tsdf, weight) float32 [nz,ny,nx] after the K views of depth / alpha [K,H,W], views [K,4,4] (stored transposed), tanfov [K,2]."""
    D, w = np.array(tsdf, f32, copy=True), np.array(weight, f32, copy=True)
    nz, ny, nx = D.shape
    depth, alpha = np.asarray(depth, f32), np.asarray(alpha, f32)
    K, H, W = depth.shape
    views, tanfov = np.asarray(views, f32).reshape(K, 4, 4), np.asarray(tanfov, f32).reshape(K, 2)
    voxel, trunc, alpha_min = f32(voxel), f32(trunc), f32(alpha_min)
    X = voxel_centres(nx, origin[0], voxel)[None, None, :]
    Y = voxel_centres(ny, origin[1], voxel)[None, :, None]
    Z = voxel_centres(nz, origin[2], voxel)[:, None, None]
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
            seen = a >= alpha_min
            s = d / a - zv
            q = s / trunc
            t = np.where(seen, np.where(q < ONE, q, ONE), ONE)
            update = ok & np.where(seen, s >= -trunc, bool(carve))
            w1 = w + ONE
            Dn = (D * w + t) / w1
        assert Dn.dtype == f32 and t.dtype == f32 and zv.dtype == f32
        D, w = np.where(update, Dn, D), np.where(update, w1, w)
    return D, w


def _corner(A, c):
    """the corner dx + 2 dy + 4 dz of every cell of a [nz,ny,nx] array"""
    nz, ny, nx = A.shape
    dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
    return A[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]


def _shift(A, axis, by):
    """A at g + by * e_axis (axis 0 = x), wrapped: the caller masks the samples that have no such neighbour"""
    return np.roll(A, -by, axis=2 - axis)


def surface_nets_ref(tsdf, weight, origin, voxel, min_weight=1.0):
    """(vertices float32 [V,3], faces int32 [F,3]) of the volume tsdf / weight [nz,ny,nx]"""
    D, Wt = np.asarray(tsdf, f32), np.asarray(weight, f32)
    nz, ny, nx = D.shape
    voxel = f32(voxel)
    inside = D < 0
    heavy = Wt >= f32(min_weight)
    all_heavy = np.ones((nz - 1, ny - 1, nx - 1), bool)
    neg = np.zeros((nz - 1, ny - 1, nx - 1), np.int32)
    for c in range(8):
        all_heavy &= _corner(heavy, c)
        neg += _corner(inside, c)
    active = all_heavy & (neg > 0) & (neg < 8)
    V = int(active.sum())
    vid = np.full((nz, ny, nx), -1, np.int64)
    cell_id = np.full(active.shape, -1, np.int64)
    cell_id[active] = np.arange(V)                                   # linear cell order, x fastest
    vid[:nz - 1, :ny - 1, :nx - 1] = cell_id
    act = vid >= 0
    # vertices
    s = [np.zeros(active.shape, f32) for _ in range(3)]
    count = np.zeros(active.shape, np.int32)
    with np.errstate(all="ignore"):
        for ax in range(3):
            lo = (1 << ax) - 1
            for e in range(4):
                ca = (e & lo) | ((e & ~lo) << 1)
                cb = ca | (1 << ax)
                da, db = _corner(D, ca), _corner(D, cb)
                cross = (da < 0) != (db < 0)
                t = da / (da - db)
                for k in range(3):
                    s[k] = np.where(cross, s[k] + (t if k == ax else f32((ca >> k) & 1)), s[k])
                count += cross
        fc = count.astype(f32)
        cz, cy, cx = np.meshgrid(np.arange(nz - 1, dtype=f32), np.arange(ny - 1, dtype=f32), np.arange(nx - 1, dtype=f32), indexing="ij")
        pos = [f32(origin[k]) + ((c + s[k] / fc) + HALF) * voxel for k, c in enumerate((cx, cy, cz))]
    vertices = np.stack([p[active] for p in pos], axis=1).astype(f32) if V else np.zeros((0, 3), f32)
    assert all(p.dtype == f32 for p in pos)
    # faces
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    idx, n = (ix, iy, iz), (nx, ny, nz)
    emit = np.zeros((nz, ny, nx, 3), bool)
    quads = np.zeros((nz, ny, nx, 3, 4), np.int64)
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        q = [_shift(_shift(vid, u, -1), v, -1), _shift(vid, v, -1), vid, _shift(vid, u, -1)]
        there = (idx[a] + 1 < n[a]) & (idx[u] >= 1) & (idx[v] >= 1)
        emit[..., a] = there & (q[0] >= 0) & (q[1] >= 0) & (q[2] >= 0) & (q[3] >= 0) & (inside != _shift(inside, a, 1))
        quads[..., a, :] = np.stack(q, axis=-1)
    rows = np.nonzero(emit.reshape(-1))[0]                           # the order of (g, a)
    q = quads.reshape(-1, 4)[rows]
    in0 = inside.reshape(-1)[rows // 3][:, None]
    first = np.where(in0, q[:, [0, 1, 2]], q[:, [0, 2, 1]])
    second = np.where(in0, q[:, [0, 2, 3]], q[:, [0, 3, 2]])
    faces = np.stack([first, second], axis=1).reshape(-1, 3).astype(np.int32)
    assert act.sum() == V
    return vertices, faces


# ---- analytic volumes: (tsdf, weight, origin, voxel) with samples at the voxel centres ----
def _grid_points(n, origin, voxel):
    nx, ny, nz = n
    x, y, z = (voxel_centres(m, o, voxel).astype(np.float64) for m, o in zip((nx, ny, nz), origin))
    return x[None, None, :], y[None, :, None], z[:, None, None]


def sphere_field(n=(24, 24, 24), radius=0.71, centre=(0.013, -0.021, 0.034)):
    nx, ny, nz = n
    voxel = 2.0 / max(n)
    origin = (-0.5 * nx * voxel, -0.5 * ny * voxel, -0.5 * nz * voxel)
    x, y, z = _grid_points(n, origin, voxel)
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius
    return (d / (3 * voxel)).astype(f32), np.ones((nz, ny, nx), f32), np.asarray(origin, f32), f32(voxel)


def torus_field(n=(40, 16, 40), R=0.6, r=0.22):
    nx, ny, nz = n
    voxel = 2.0 / max(nx, nz)
    origin = (-0.5 * nx * voxel + 0.003, -0.5 * ny * voxel + 0.007, -0.5 * nz * voxel - 0.005)
    x, y, z = _grid_points(n, origin, voxel)
    d = np.sqrt((np.sqrt(x * x + z * z) - R) ** 2 + y * y) - r
    return (d / (3 * voxel)).astype(f32), np.ones((nz, ny, nx), f32), np.asarray(origin, f32), f32(voxel)


def plane_field(n=(9, 8, 7), level=3):
    """D = iz - level exactly: the samples of layer `level` are exact zeros (outside), the surface lies on grid points"""
    nx, ny, nz = n
    d = np.broadcast_to((np.arange(nz, dtype=f32) - f32(level))[:, None, None], (nz, ny, nx)).copy()
    return d, np.ones((nz, ny, nx), f32), np.zeros(3, f32), f32(0.25)


def checker_field(n=(6, 5, 4)):
    """signs alternate from sample to sample: every cell is active and every grid edge crossed - the largest output a grid can give"""
    nx, ny, nz = n
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    d = np.where((ix + iy + iz) % 2 == 0, f32(-0.75), f32(0.5)).astype(f32)
    return d, np.ones((nz, ny, nx), f32), np.asarray((-1.0, 0.5, 2.0), f32), f32(0.125)


def positive_field(n=(5, 4, 3)):
    nx, ny, nz = n
    return np.full((nz, ny, nx), f32(0.5)), np.ones((nz, ny, nx), f32), np.zeros(3, f32), f32(1.0)


def noise_field(n, seed=0, observed=0.9):
    """a random field in [-1, 1) with a share of the samples unobserved (weight 0): many cells active at any grid size"""
    nx, ny, nz = n
    rng = np.random.default_rng(seed)
    d = rng.uniform(-1, 1, size=(nz, ny, nx)).astype(f32)
    w = (rng.random((nz, ny, nx)) < observed).astype(f32) * 2
    return d, w, np.asarray((0.5, -0.25, 1.0), f32), f32(0.0625)


# ---- depth maps of a mesh ----
def camera_rays(cam):
    """(origins, dirs) float32 [H*W,3] through every pixel centre of a scenes.camera_from_RT dict, directions with view z = 1 (a hit's t
    is its view depth): mesh_pick.camera_rays on the host"""
    W, H = cam["W"], cam["H"]
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    dv = np.stack([((2 * x + 1) / W - 1) * cam["tanx"], ((2 * y + 1) / H - 1) * cam["tany"], np.ones_like(x)], -1).reshape(-1, 3)
    dirs = dv @ np.asarray(cam["view"], np.float64)[:3, :3].T
    return np.broadcast_to(np.asarray(cam["campos"], f32), dirs.shape).copy(), dirs.astype(f32)


def raycast_maps(cams, vertices, faces):
    """(depth, alpha, views, tanfov): first-hit depth maps [K,H,W] of the mesh by ray_ref's brute force, alpha 1 on a hit and 0 on a miss"""
    import ray_ref as rr
    depth, alpha = [], []
    for cam in cams:
        o, d = camera_rays(cam)
        t, face, _ = rr.ray_mesh_ref(o, d, vertices, faces)
        hit = face >= 0
        depth.append(np.where(hit, t, f32(0)).reshape(cam["H"], cam["W"]).astype(f32))
        alpha.append(hit.reshape(cam["H"], cam["W"]).astype(f32))
    return np.stack(depth), np.stack(alpha), camera_rows(cams)[0], camera_rows(cams)[1]


def camera_rows(cams):
    return (np.stack([np.asarray(c["view"], f32) for c in cams]), np.asarray([[c["tanx"], c["tany"]] for c in cams], f32))


# ---- what a proxy mesh has to be ----
def edge_use(faces):
    """(edges int64 [E,2] with a < b, uses int64 [E]): how many faces hold each undirected edge"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    e = np.sort(e, axis=1)
    if len(e) == 0:
        return np.zeros((0, 2), np.int64), np.zeros(0, np.int64)
    return np.unique(e, axis=0, return_counts=True)


def boundary_edges(faces):
    return int((edge_use(faces)[1] == 1).sum())


def is_closed(faces):
    """every edge is used by exactly two faces, once in each direction"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    directed = len(np.unique(d, axis=0)) == len(d)                   # no directed edge twice: consistently wound
    return bool(len(f) > 0 and (edge_use(f)[1] == 2).all() and directed)


def euler_characteristic(n_vertices, faces):
    return int(n_vertices) - len(edge_use(faces)[0]) + len(np.asarray(faces).reshape(-1, 3))


def component_labels(n_vertices, faces):
    """label of every vertex: the smallest vertex id of its connected component (an unreferenced vertex is its own)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    label = np.arange(n_vertices, dtype=np.int64)
    while True:
        new = label.copy()
        m = label[f].min(axis=1) if len(f) else np.zeros(0, np.int64)
        for c in range(3):
            np.minimum.at(new, f[:, c], m)
        new = new[new]
        if np.array_equal(new, label):
            return label
        label = new


def n_components(n_vertices, faces):
    f = np.asarray(faces, np.int64).reshape(-1)
    return len(np.unique(component_labels(n_vertices, faces)[np.unique(f)]))


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return float((np.cross(v[f[:, 0]], v[f[:, 1]]) * v[f[:, 2]]).sum() / 6.0)


def keep_largest_ref(vertices, faces):
    """the component with the most faces (ties: the smallest vertex id), unreferenced vertices dropped, ids kept in order"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) == 0:
        return np.zeros((0, 3), f32), np.zeros((0, 3), np.int32)
    label = component_labels(len(vertices), f)[f[:, 0]]
    names, counts = np.unique(label, return_counts=True)
    best = names[np.argmax(counts)]                                   # the first of the largest: the smallest label
    f = f[label == best]
    used = np.unique(f)
    remap = np.full(len(vertices), -1, np.int64)
    remap[used] = np.arange(len(used))
    return np.asarray(vertices, f32)[used], remap[f].astype(np.int32)
