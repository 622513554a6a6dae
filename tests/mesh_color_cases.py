"""Inputs of the mesh colour tests, shared by the host and the device files: the hand-built 8 x 8 case in which every decision of
gm_mesh_color_integrate falls EXACTLY on its edge, the two-quad occlusion case, orbit views of a torus with ray-cast maps, and random
sums and states for the spread.  Everything is numpy, computed once and handed out read-only."""
import functools

import numpy as np

import mesh_color_ref as mr
import tsdf_ref as tr

f32 = np.float32
ALPHA_MIN, DEPTH_TOL = 0.5, 0.25
UNDER_HALF = np.nextafter(f32(0.5), f32(0))


def _lock(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def edge_case():
    """An identity camera at the origin looking along +z, tan 1, 8 x 8 maps: a vertex (x, y, z) lands on px = 4 x / z + 3.5, and with
    coordinates that are multiples of powers of two every product of the definition is exact, so each case below sits exactly ON its
    edge or one ulp beyond it.  Away from its cases' pixels the view shows a wall at depth 1 with alpha 1.
    dict(names, P, N, pixel int [n,2] (the pixel a vertex that is not skipped before step 3 reads; -1: none), image, depth, alpha,
    views, tans, expect(alpha_min, two_sided) -> bool [n])"""
    H = W = 8
    alpha, depth = np.ones((1, H, W), f32), np.ones((1, H, W), f32)
    iy, ix = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    image = np.stack([(ix + 1) / 16.0, (iy + 1) / 16.0, np.full((H, W), 0.25) + (ix + 8 * iy) / 256.0]).astype(f32)[None]
    names, P, N, pixel, rule = [], [], [], [], []
    front = (0.0, 0.0, -1.0)

    def at(i, j, z=1.0):
        return ((i - 3.5) / 4.0 * z, (j - 3.5) / 4.0 * z, z)

    def add(name, p, n, pix, when):
        """when: "always", "never", "a0" (only with alpha_min == 0), "two" (only two-sided)"""
        names.append(name); P.append(p); N.append(n); pixel.append(pix); rule.append(when)

    add("plain", at(1, 1), front, (1, 1), "always")
    add("zv == 0", (0.0, 0.0, 0.0), front, (-1, -1), "never")
    add("zv == -0", (0.0, 0.0, -0.0), front, (-1, -1), "never")
    add("zv < 0", (0.0, 0.0, -1.0), front, (-1, -1), "never")
    z = 2.0 ** -10
    add("zv small", at(5, 4, z), front, (5, 4), "always")
    depth[0, 4, 5] = z
    lo, hi = float(np.nextafter(f32(-1), f32(-2))), 1.0 - 2.0 ** -22
    y2, x5 = at(0, 2)[1], at(5, 0)[0]
    add("left border: px + 0.5 == 0", (-1.0, y2, 1.0), front, (0, 2), "always")
    add("left of it by an ulp", (lo, y2, 1.0), front, (-1, -1), "never")
    add("right border: px + 0.5 == W", (1.0, y2, 1.0), front, (-1, -1), "never")
    add("right, inside by an ulp of px", (hi, y2, 1.0), front, (7, 2), "always")
    add("top border: py + 0.5 == 0", (x5, -1.0, 1.0), front, (5, 0), "always")
    add("above it by an ulp", (x5, lo, 1.0), front, (-1, -1), "never")
    add("bottom border: py + 0.5 == H", (x5, 1.0, 1.0), front, (-1, -1), "never")
    add("bottom, inside by an ulp of py", (at(6, 0)[0], hi, 1.0), front, (6, 7), "always")
    # px + 0.5 == 4 exactly: floor takes pixel 4, and one ulp less takes pixel 3, which shows nothing
    y6 = at(0, 6)[1]
    add("px + 0.5 an exact integer", (0.0, y6, 1.0), front, (4, 6), "always")
    add("an ulp below it", (-(2.0 ** -24), y6, 1.0), front, (3, 6), "never")
    alpha[0, 6, 3], depth[0, 6, 3] = 0, 0
    add("a == alpha_min", at(2, 3), front, (2, 3), "always")
    alpha[0, 3, 2], depth[0, 3, 2] = 0.5, 0.5
    add("a an ulp below alpha_min", at(3, 3), front, (3, 3), "a0")
    alpha[0, 3, 3], depth[0, 3, 3] = UNDER_HALF, UNDER_HALF
    add("a == 0", at(5, 3), front, (5, 3), "never")                   # with alpha_min == 0: a >= 0 holds, and 0 / 0 - zv is NaN
    alpha[0, 3, 5], depth[0, 3, 5] = 0, 0
    add("s == +tol", at(1, 5), front, (1, 5), "always")
    depth[0, 5, 1] = 1.25
    add("s an ulp above +tol", at(2, 5), front, (2, 5), "never")
    depth[0, 5, 2] = np.nextafter(f32(1.25), f32(2))
    add("s == -tol", at(3, 5), front, (3, 5), "always")
    depth[0, 5, 3] = 0.75
    add("s an ulp below -tol", at(4, 5), front, (4, 5), "never")
    depth[0, 5, 4] = np.nextafter(f32(0.75), f32(0))
    add("d == 0", at(6, 1), (1.0, 1.0, 0.0), (6, 1), "never")          # 0.625 - 0.625: grazing; two-sided its weight is 0
    add("d == -2^-20", at(6, 1), (1.0, 1.0, -(2.0 ** -20)), (6, 1), "always")
    add("facing away", at(6, 2), (0.0, 0.0, 1.0), (6, 2), "two")
    add("zero normal", at(6, 4), (0.0, 0.0, 0.0), (6, 4), "never")
    add("NaN colour", at(1, 7), front, (1, 7), "never")
    image[0, 0, 7, 1] = np.nan
    add("inf colour", at(2, 7), front, (2, 7), "never")
    image[0, 2, 7, 2] = np.inf
    add("NaN depth", at(3, 7), front, (3, 7), "never")
    depth[0, 7, 3] = np.nan
    add("NaN alpha", at(4, 7), front, (4, 7), "never")
    alpha[0, 7, 4] = np.nan
    add("NaN normal", at(1, 2), (np.nan, 0.0, -1.0), (1, 2), "never")
    add("NaN position", (np.nan, 0.0, 1.0), front, (-1, -1), "never")
    rule = np.array(rule)

    def expect(alpha_min, two_sided):
        return (rule == "always") | ((rule == "a0") & (alpha_min <= UNDER_HALF)) | ((rule == "two") & bool(two_sided))

    out = dict(names=names, P=np.array(P, f32), N=np.array(N, f32), pixel=np.array(pixel), image=image, depth=depth, alpha=alpha,
               views=np.eye(4, dtype=f32)[None], tans=np.ones((1, 2), f32), expect=expect)
    _lock(out["P"], out["N"], image, depth, alpha, out["views"], out["tans"])
    return out


@functools.lru_cache(maxsize=None)
def occlusion_case():
    """two parallel quads over the pixels 2 .. 5 of the edge case's camera, at z = 1 and z = 2, both wound towards the camera; the maps
    are the front one's: (V, F, image, depth, alpha, views, tans); vertices 0..3 front, 4..7 back"""
    H = W = 8
    corners = [(2, 2), (5, 2), (5, 5), (2, 5)]
    V = np.array([((i - 3.5) / 4.0 * z, (j - 3.5) / 4.0 * z, z) for z in (1.0, 2.0) for i, j in corners], f32)
    F = np.array([(0, 2, 1), (0, 3, 2), (4, 6, 5), (4, 7, 6)], np.int32)
    depth, alpha = np.ones((1, H, W), f32), np.ones((1, H, W), f32)
    image = np.full((1, 3, H, W), 0.75, f32)
    return _lock(V, F, image, depth, alpha, np.eye(4, dtype=f32)[None], np.ones((1, 2), f32))


def torus(nu=24, nv=16):
    """scenes.torus_mesh wound OUTWARDS (the generator's rows point inwards), float32"""
    from gaussianmesh_amd import scenes
    V, F = scenes.torus_mesh(nu, nv)
    return V.astype(f32), np.ascontiguousarray(F[:, [0, 2, 1]])


@functools.lru_cache(maxsize=None)
def orbit_case(K, H, W, seed=0):
    """K cameras on an orbit ABOVE a 24 x 16 torus - its underside stays unseen -, ray-cast depth and alpha of the torus itself and a
    random image: (V, F, N, image, depth, alpha, views, tans)"""
    from gaussianmesh_amd import scenes
    V, F = torus()
    cams = [scenes.orbit_camera(k, K, W, H, radius=6.5, height=4.5, fovx_deg=50.0) for k in range(K)]
    depth, alpha, views, tans = tr.raycast_maps(cams, V, F)
    rng = np.random.default_rng(seed + 100 * K + H)
    image = rng.uniform(0, 1, size=(K, 3, H, W)).astype(f32)
    soft = rng.choice(np.array([0.25, 0.5, 0.75, 1.0], f32), size=alpha.shape)          # the rasterizer's maps: alpha below 1, depth alpha-weighted
    alpha = (alpha * soft).astype(f32)
    depth = (depth * alpha).astype(f32)
    N = mr.vertex_normals_ref(V, F)
    return _lock(V, F, N, image, depth, alpha, views, tans)


def mesh_of(Vm, seed=0):
    """(V float32 [Vm,3], F int32 [F,3]) with exactly Vm vertices: a jittered strip, and for an odd count a last vertex without faces
    (Vm == 1: that vertex alone, no faces)"""
    rng = np.random.default_rng(seed + Vm)
    n = Vm // 2 - 1
    if n < 1:
        return _lock(rng.uniform(-1, 1, size=(Vm, 3)).astype(f32), np.zeros((0, 3), np.int32))
    V, F = mr.strip(n)
    V = np.concatenate([V, np.full((Vm - len(V), 3), 3.0, f32)]).astype(f32)
    V = (V + rng.normal(0, 0.2, size=V.shape)).astype(f32)
    return _lock(V, F)


def torus_tol():
    """depth_tol of the torus cases: well above the depth a vertex's pixel centre differs by on a 32-pixel map, well below the tube"""
    return 0.35


def random_vertices(Vm, K, H, W, seed):
    """Vm vertices scattered through the torus's orbit views with random normals, half of them zero-faced (no mesh needed):
    (P, N, csum0, wsum0) - a state to start from that is not empty"""
    rng = np.random.default_rng(seed)
    P = rng.uniform(-2.5, 2.5, size=(Vm, 3)).astype(f32)
    N = rng.normal(size=(Vm, 3)).astype(f32)
    csum0 = rng.uniform(0, 2, size=(Vm, 3)).astype(f32)
    wsum0 = rng.uniform(0, 2, size=(Vm,)).astype(f32)
    return _lock(P, N, csum0, wsum0)


def spread_state(Vm, seen_share, seed):
    """(seen uint8 [Vm], colors float32 [Vm,3]): colours everywhere - the unseen rows hold values that must not matter"""
    rng = np.random.default_rng(seed)
    seen = (rng.random(Vm) < seen_share).astype(np.uint8) * rng.integers(1, 255, size=Vm).astype(np.uint8)     # any non-zero byte is seen
    colors = rng.uniform(0, 1, size=(Vm, 3)).astype(f32)
    return _lock(seen, colors)
