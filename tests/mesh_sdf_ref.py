"""The definitions of gm_mesh_winding and gm_mesh_signed_distance restated in numpy (include/gmesh_hip.h, csrc/gm_winding.hip): float64
from the float32 inputs, every product and sum written out per component, the faces summed in chunks of WN_CHUNK in face order and
the chunk sums in chunk order.  numpy neither contracts nor reorders, its sqrt and division are correctly rounded; its arctan2 is the
host library's, so the device's w agrees to a few ulp of pi per face, not bit for bit.  phi comes from closest_ref's float32 d2, which
the device matches bit for bit - so phi does too wherever the sign is decided (|w| away from 0.5)."""
import numpy as np

from closest_ref import closest_face_ref

WN_CHUNK = 1024
FOUR_PI = 4.0 * float.fromhex("0x1.921fb54442d18p+1")
f32, f64 = np.float32, np.float64


def _dot(xx, xy, xz, yx, yy, yz):
    return (xx * yx + xy * yy) + xz * yz


def face_omega(P, A, B, C):
    """omega float64 of point rows P [..,3] against triangle rows (A, B, C) [..,3] (float32, broadcast against each other)"""
    P, A, B, C = (np.asarray(x, f32).astype(f64) for x in (P, A, B, C))
    px, py, pz = P[..., 0], P[..., 1], P[..., 2]
    ax, ay, az = A[..., 0] - px, A[..., 1] - py, A[..., 2] - pz
    bx, by, bz = B[..., 0] - px, B[..., 1] - py, B[..., 2] - pz
    cx, cy, cz = C[..., 0] - px, C[..., 1] - py, C[..., 2] - pz
    la, lb, lc = np.sqrt(_dot(ax, ay, az, ax, ay, az)), np.sqrt(_dot(bx, by, bz, bx, by, bz)), np.sqrt(_dot(cx, cy, cz, cx, cy, cz))
    nx, ny, nz = by * cz - bz * cy, bz * cx - bx * cz, bx * cy - by * cx
    det = _dot(ax, ay, az, nx, ny, nz)
    den = (((la * lb) * lc + _dot(ax, ay, az, bx, by, bz) * lc) + _dot(bx, by, bz, cx, cy, cz) * la) + _dot(cx, cy, cz, ax, ay, az) * lb
    return 2.0 * np.arctan2(det, den)


def winding_ref(points, vertices, faces, rows=None):
    """w float64 [N]: per point the chunked sum of the definition over 4 pi"""
    P = np.ascontiguousarray(points, f32).reshape(-1, 3)
    V = np.ascontiguousarray(vertices, f32)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    A, B, C = V[F[:, 0]][None], V[F[:, 1]][None], V[F[:, 2]][None]
    w = np.empty(len(P), f64)
    rows = max(1, 500000 // max(1, len(F))) if rows is None else rows            # ~0.5 M point-face pairs at a time
    for s in range(0, len(P), rows):
        om = face_omega(P[s:s + rows][:, None, :], A, B, C)                     # [rows, F]
        total = np.zeros(om.shape[0], f64)
        for k in range(0, om.shape[1], WN_CHUNK):
            part = np.zeros(om.shape[0], f64)
            for j in range(k, min(k + WN_CHUNK, om.shape[1])):                  # face order, from 0.0
                part = part + om[:, j]
            total = total + part                                                # chunk order, from 0.0
        w[s:s + rows] = total / FOUR_PI
    return w


def signed_distance_ref(points, vertices, faces):
    """(phi float32 [N], face int64 [N], closest float32 [N,3], w float64 [N])"""
    d2, face, close = closest_face_ref(points, vertices, faces)
    w = winding_ref(points, vertices, faces)
    with np.errstate(invalid="ignore"):
        root = np.sqrt(d2)                                                      # float32, correctly rounded
        phi = np.where(np.abs(w) > 0.5, -root, root).astype(f32)
    phi = np.where(d2 == 0, f32(0.0), phi)
    phi = np.where(np.isnan(w) | (face < 0), f32(np.nan), phi).astype(f32)
    return phi, face, close, w


def lattice_points_ref(origin, voxel, shape):
    """the positions mesh_sdf.grid_values samples, float32 [nz*ny*nx, 3] in its flat order: fl(fl(fl(float32(i) + 0.5f) * voxel) + origin)"""
    nz, ny, nx = shape
    o, h = np.asarray(origin, f64).astype(f32), f32(voxel)
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    idx = np.stack([ix, iy, iz], -1).reshape(-1, 3).astype(f32)
    pts = (idx + f32(0.5)) * h + o[None]
    assert pts.dtype == f32
    return pts


def grid_values_ref(vertices, faces, origin, voxel, shape):
    """phi float32 [nz,ny,nx] of the lattice"""
    return signed_distance_ref(lattice_points_ref(origin, voxel, shape), vertices, faces)[0].reshape(shape)


# ---- the meshes of the tests ----
def tetrahedron():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], f32)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)         # wound outwards
    return v, f


def cube(lo=(-0.5, -0.5, -0.5), hi=(0.5, 0.5, 0.5)):
    """12 triangles wound outwards; faces 2k, 2k + 1 are one side: -x, +x, -y, +y, -z, +z"""
    lo, hi = np.asarray(lo, f64), np.asarray(hi, f64)
    v = np.array([[(hi if (i >> k) & 1 else lo)[k] for k in range(3)] for i in range(8)], f32)      # bit 0: x, bit 1: y, bit 2: z
    quads = [(0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6)]
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return v, f


def merged(*meshes):
    vs, fs, off = [], [], 0
    for v, f in meshes:
        vs.append(np.asarray(v, f32)); fs.append(np.asarray(f, np.int32) + off); off += len(v)
    return np.concatenate(vs, 0), np.concatenate(fs, 0)
