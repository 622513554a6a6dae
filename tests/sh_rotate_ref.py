"""The definition gm_sh_rotate is held to, in float64 numpy: c' is the unique coefficient row with
    SH_deg(d) . c' == SH_deg(A^T d) . c    for every unit direction d,
SH_deg the polynomial of csrc/gm_sh.h (restated here), A any 3x3 matrix.  Band l of that polynomial is homogeneous of degree l in
(x, y, z), so the right side, restricted to the unit sphere, is a polynomial of degree <= deg and lies in the span of the same
(deg+1)^2 functions: c' exists, is unique, and any exact method finds it.  Here: least squares over 96 Fibonacci directions."""
import numpy as np

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435]
BANDS = ((0, 1), (1, 4), (4, 9), (9, 16))


def basis(d):
    """The 16 functions of sh_channel (gm_sh.h) at directions d [..., 3] (NOT normalised here) -> [..., 16], float64."""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return np.stack([C0 * np.ones_like(x), -C1 * y, C1 * z, -C1 * x,
                     C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy),
                     C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy), C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
                     C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy), C3[6] * x * (xx - 3 * yy)], -1)


def fibonacci_directions(K):
    """K unit directions on a Fibonacci spiral: z_j = 1 - (2 j + 1) / K, azimuth j pi (1 + sqrt 5)."""
    i = np.arange(K) + 0.5
    phi = np.arccos(1 - 2 * i / K)
    th = np.pi * (1 + 5 ** 0.5) * i
    return np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1)


def eval_sh(d, c, deg=3):
    """SH_deg(d) . c: d [T,3], c [N,M,3] -> [N,T,3] (no + 0.5, no clamp)."""
    n = (deg + 1) ** 2
    return np.einsum("tk,nkc->ntc", basis(d)[:, :n], np.asarray(c, np.float64)[:, :n])


def eval_sh_rotated(d, A, c, deg=3):
    """SH_deg(A^T d) . c per row: d [T,3], A [N,3,3], c [N,M,3] -> [N,T,3]."""
    n = (deg + 1) ** 2
    dr = np.einsum("nji,tj->nti", np.asarray(A, np.float64), np.asarray(d, np.float64))
    return np.einsum("ntk,nkc->ntc", basis(dr)[..., :n], np.asarray(c, np.float64)[:, :n])


def rotate_sh_ref(c, A, deg=3, K=96):
    """c [N,M,3], A [N,3,3] -> c' [N,M,3] float64: coefficients k < (deg+1)^2 re-expressed, the others copied."""
    c = np.asarray(c, np.float64)
    out = c.copy()
    n = (deg + 1) ** 2
    if deg == 0 or len(c) == 0:
        return out
    D = fibonacci_directions(K)
    B = basis(D)[:, :n]                                     # [K, n], well conditioned (K = 96: below 1.1)
    f = eval_sh_rotated(D, A, c, deg)                       # [N, K, 3]
    sol = np.linalg.lstsq(B, f.transpose(1, 0, 2).reshape(K, -1), rcond=None)[0]
    out[:, :n] = sol.reshape(n, len(c), 3).transpose(1, 0, 2)
    return out


def random_rotations(n, rng):
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)


def blended_matrices(n, rng):
    """Dirichlet blends of three random rotations: what a barycentric blend of per-vertex rotations looks like, not orthogonal."""
    w = rng.dirichlet([1, 1, 1], size=n)
    return sum(w[:, k, None, None] * random_rotations(n, rng) for k in range(3))


def random_coefficients(n, rng, M=16):
    """DC ~ N(0, 0.5), the others ~ N(0, 0.1) (scenes.make_cloud's rows)."""
    return rng.normal(size=(n, M, 3)) * np.array([0.5] + [0.1] * (M - 1))[None, :, None]


def unit_directions(n, rng):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)
