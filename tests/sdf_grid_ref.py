"""The prepared signed-distance grid of dynamics.SdfGrid restated in numpy: `prepare` in float32, operation for operation what
gm_sdf_grid_prepare does (csrc/gm_sdf.hip), so the device is held to it bit for bit; `sample` in float64, the trilinear interpolation of
all four channels and the normalised gradient of csrc/gm_sdf.h's sdf_sample (numpy has no fma: the device differs in the last bits).
numpy only."""
import numpy as np

F = np.float32


def prepare(values, voxel, weight=None, min_weight=1.0, scale=1.0):
    """values float32 [nz,ny,nx] (+ weight of the same shape) -> float32 [nz,ny,nx,4]: (phi, gx, gy, gz) on valid samples - not NaN and
    weight >= min_weight - four NaNs elsewhere; phi = value * scale; per axis over the valid in-grid neighbours (phi+ - phi-) / (2 voxel),
    a one-sided difference / voxel, or 0"""
    v = np.asarray(values, F)
    voxel, scale, two = F(voxel), F(scale), F(2.0) * F(voxel)
    valid = ~np.isnan(v)
    if weight is not None:
        with np.errstate(invalid="ignore"):
            valid &= np.asarray(weight, F) >= F(min_weight)
    with np.errstate(invalid="ignore", over="ignore"):
        phi = (v * scale).astype(F)
    out = np.full(v.shape + (4,), np.nan, F)
    out[..., 0] = phi
    for a, axis in ((0, 2), (1, 1), (2, 0)):                           # x is the last array axis
        up, upv = np.roll(phi, -1, axis), np.roll(valid, -1, axis)
        dn, dnv = np.roll(phi, 1, axis), np.roll(valid, 1, axis)
        last, first = [slice(None)] * 3, [slice(None)] * 3
        last[axis], first[axis] = -1, 0
        upv[tuple(last)] = False                                       # beyond the grid: no neighbour
        dnv[tuple(first)] = False
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            both, hi, lo = ((up - dn) / two).astype(F), ((up - phi) / voxel).astype(F), ((phi - dn) / voxel).astype(F)
        out[..., 1 + a] = np.where(upv & dnv, both, np.where(upv, hi, np.where(dnv, lo, F(0.0))))
    out[~valid] = np.nan
    return out


def sample(grid, origin, voxel, points):
    """(phi float64 [N], n float64 [N,3]) of points [N,3] (any float; read as given) in the prepared grid: NaN outside
    0 <= g_a < n_a - 1, next to a sample whose phi is NaN, and where the interpolated gradient has no length"""
    G = np.asarray(grid, F)
    nz, ny, nx = G.shape[:3]
    X = np.asarray(points, np.float64).reshape(-1, 3)
    o, h = np.asarray(origin, F).astype(np.float64), float(F(voxel))
    N = len(X)
    phi, n = np.full(N, np.nan), np.full((N, 3), np.nan)
    with np.errstate(invalid="ignore"):
        g = (X - o) / h - 0.5
        inside = ((g >= 0.0) & (g < np.array([nx - 1, ny - 1, nz - 1], np.float64))).all(axis=1)
    rows = np.flatnonzero(inside)
    if not len(rows):
        return phi, n
    g = g[rows]
    i = np.floor(g).astype(np.int64)
    f = g - i
    c = np.empty((len(rows), 2, 2, 2, 4))
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                c[:, dz, dy, dx] = G[i[:, 2] + dz, i[:, 1] + dy, i[:, 0] + dx].astype(np.float64)
    known = ~np.isnan(c[..., 0]).reshape(len(rows), -1).any(axis=1)
    fx, fy, fz = f[:, 0, None], f[:, 1, None], f[:, 2, None]
    with np.errstate(invalid="ignore"):
        a = c[:, :, :, 0] + fx[:, None, None] * (c[:, :, :, 1] - c[:, :, :, 0])       # [rows, dz, dy, 4]
        b = a[:, :, 0] + fy[:, None] * (a[:, :, 1] - a[:, :, 0])                       # [rows, dz, 4]
        q = b[:, 0] + fz * (b[:, 1] - b[:, 0])                                         # [rows, 4]
        s = np.sqrt(q[:, 1] ** 2 + q[:, 2] ** 2 + q[:, 3] ** 2)
        ok = known & (s > 0.0) & np.isfinite(s)
        unit = q[:, 1:] / s[:, None]
    phi[rows[ok]] = q[ok, 0]
    n[rows[ok]] = unit[ok]
    return phi, n
