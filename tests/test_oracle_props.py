"""Structural properties of the oracle: binning order, fast path == staged path, knn vs a KD-tree, deform invariants."""
import numpy as np
import pytest

from helpers import small_scene


def test_higher_msb(oracle):
    # rasterizer_impl.cu:35-50 on the tile counts of 256^2, 1080p and 4K
    assert [oracle.higher_msb(n) for n in (256, 8160, 32400, 1, 2, 3)] == [9, 13, 15, 1, 2, 2]


def test_binning_is_stable_tile_depth_order(oracle):
    sc, cam = small_scene(P=800, W=100, H=60, seed=2)
    sc["means"][10:20] = sc["means"][10]           # identical depths -> ties must stay in Gaussian-index order
    fw = oracle.forward_full(sc, cam, np.zeros(3, np.float32))
    keys, pl, geo = fw["bins"]["keys"], fw["bins"]["point_list"], fw["geo"]
    assert (np.diff(keys.astype(np.uint64).view(np.int64)) >= 0).all()
    same = keys[1:] == keys[:-1]
    assert (pl[1:][same] > pl[:-1][same]).all()    # ties: ascending Gaussian id
    assert fw["bins"]["R"] == int(geo["tiles"].sum())
    rg = fw["bins"]["ranges"]
    n = (rg[:, 1] - rg[:, 0]).sum()
    assert n == fw["bins"]["R"]
    depth_bits = geo["depths"].view(np.uint32)[pl]
    assert np.array_equal(keys & np.uint64(0xFFFFFFFF), depth_bits.astype(np.uint64))


@pytest.mark.parametrize("pre", [False, True])
def test_fast_forward_equals_staged(oracle, pre):
    sc, cam = small_scene(P=700, W=90, H=70, seed=5)
    bg = np.array([1, 0.5, 0.25], np.float32)
    fw = oracle.forward_full(sc, cam, bg, use_precomp_cov=pre, use_precomp_color=pre)
    col, radii, R = oracle.forward_fast(sc, cam, bg, use_precomp_cov=pre, use_precomp_color=pre)
    assert R == fw["bins"]["R"] and np.array_equal(radii, fw["geo"]["radii"]) and np.array_equal(col, fw["color"])


def test_linearity_in_background_and_colour(oracle):
    """Image is affine in (bg, colours) for fixed geometry: C = sum w_i c_i + T bg."""
    sc, cam = small_scene(P=300, W=48, H=48, seed=6)
    z = np.zeros(3, np.float32)
    a = oracle.forward_full(sc, cam, z, use_precomp_color=True)["color"]
    sc2 = dict(sc); sc2["colors_precomp"] = 2 * sc["colors_precomp"]
    b = oracle.forward_full(sc2, cam, z, use_precomp_color=True)
    assert np.allclose(b["color"], 2 * a, atol=1e-6)
    c = oracle.forward_full(sc, cam, np.ones(3, np.float32), use_precomp_color=True)
    assert np.allclose(c["color"] - a, c["final_T"].reshape(1, cam["H"], cam["W"]), atol=1e-6)


def test_knn_against_kdtree(oracle):
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(0)
    pts = rng.normal(size=(3000, 3)).astype(np.float32)
    out = oracle.knn_mean_dist2(pts)
    d, _ = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=4)
    assert np.allclose(out, (d[:, 1:] ** 2).mean(1), rtol=1e-5)


def test_deform_invariants(oracle):
    from gaussianmesh_amd import scenes
    verts, faces = scenes.torus_mesh(20, 12)
    cl = scenes.bind_cloud_to_mesh(500, verts, faces, seed=1)
    cov = scenes.cov3d_from_scale_rot(cl["scales"], cl["rots"]).astype(np.float32)
    Vm = verts.shape[0]
    I = np.tile(np.eye(3, dtype=np.float32), (Vm, 1, 1))
    # identity
    p, c, r = oracle.deform(cl["tri"], cl["weights"], np.zeros((Vm, 3), np.float32), I, I, cov, cl["means"])
    assert np.array_equal(p, cl["means"]) and np.allclose(c, cov, atol=1e-7) and np.allclose(r, np.eye(3))
    # rigid motion x -> Q x + t with the reference convention: per-vertex R such that RS = R^T S maps the covariance,
    # i.e. the blended rotation is stored transposed (edittool/__init__.py:122): pass R = Q^T
    a = 0.7
    Q = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t = np.array([0.3, -0.2, 0.5])
    V1 = verts @ Q.T + t
    Rv = np.tile(Q.T.astype(np.float32), (Vm, 1, 1))
    p, c, r = oracle.deform(cl["tri"], cl["weights"], (V1 - verts).astype(np.float32), Rv, I, cov, cl["means"])
    assert np.allclose(c, Q @ cov.astype(np.float64) @ Q.T, atol=1e-6)
    assert np.allclose(r, Q, atol=1e-6)
    # positions move by the barycentric blend of the vertex displacements
    tri = cl["tri"]; w = cl["weights"]
    dV = V1 - verts
    exp = cl["means"] + (w[:, :, None] * dV[tri]).sum(1)
    assert np.allclose(p, exp, atol=1e-5)
    # uniform scale s: R = I, S = s I -> cov * s^2
    p, c, r = oracle.deform(cl["tri"], cl["weights"], (0.5 * verts).astype(np.float32), I, 1.5 * I, cov, cl["means"])
    assert np.allclose(c, 2.25 * cov, rtol=1e-6)


def test_twist_frames_are_polar_decompositions():
    from gaussianmesh_amd import scenes
    verts, _ = scenes.torus_mesh(16, 10)
    V1, R, S = scenes.twist_bend_frame(verts, t=5, period=64)
    assert np.allclose(R @ R.transpose(0, 2, 1), np.eye(3), atol=1e-10)
    assert np.allclose(S, S.transpose(0, 2, 1), atol=1e-10)
    assert np.allclose(np.linalg.det(R), 1.0)
    V0, R0, S0 = scenes.twist_bend_frame(verts, t=0)
    assert np.allclose(V0, verts) and np.allclose(R0, np.eye(3)) and np.allclose(S0, np.eye(3))


def test_mesh_rs_oracle_invariants():
    """oracle/mesh_oracle.py (the checker of gm_mesh_rs): identity, rigid motion, uniform scale, affine map."""
    from oracle import mesh_oracle
    from gaussianmesh_amd import scenes
    verts, faces = scenes.torus_mesh(24, 16)
    I = np.eye(3)
    R, S = mesh_oracle.mesh_rs(verts, verts, faces)
    assert np.abs(R - I).max() <= 1e-12 and np.abs(S - I).max() <= 1e-12
    c, s = np.cos(0.8), np.sin(0.8)
    Q = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    R, S = mesh_oracle.mesh_rs(verts, verts @ Q.T + 3.0, faces)
    assert np.abs(R - Q.T).max() <= 1e-10 and np.abs(S - I).max() <= 1e-10
    R, S = mesh_oracle.mesh_rs(verts, 0.6 * verts, faces)
    assert np.abs(R - I).max() <= 1e-10 and np.abs(S - 0.6 * I).max() <= 1e-10
    A = Q @ np.array([[1.3, 0.2, 0.0], [0.0, 0.9, 0.1], [0.1, 0.0, 1.2]])
    R, S = mesh_oracle.mesh_rs(verts, verts @ A.T, faces)
    assert np.abs(np.einsum("nji,njk->nik", R, S) - A).max() <= 1e-6      # (the 1e-9 normal regulariser)
    assert np.abs(np.linalg.det(R) - 1).max() <= 1e-10 and np.abs(S - S.transpose(0, 2, 1)).max() <= 1e-12


def _census_walk(W, H, bins, geo):
    """orc_power_census restated in numpy float32 (the same expression, evaluation order and stop): the list of (pixel, list position)"""
    f = np.float32
    xy, co = geo["xy"].astype(f), geo["conic_op"].astype(f)
    gx = (W + 15) // 16
    out = []
    for t, (r0, r1) in enumerate(bins["ranges"]):
        for y in range(16 * (t // gx), min(16 * (t // gx) + 16, H)):
            for x in range(16 * (t % gx), min(16 * (t % gx) + 16, W)):
                T = f(1)
                for e in range(r0, r1):
                    g = bins["point_list"][e]
                    dx, dy = xy[g, 0] - f(x), xy[g, 1] - f(y)
                    power = f(-0.5) * (co[g, 0] * dx * dx + co[g, 2] * dy * dy) - co[g, 1] * dx * dy
                    if power > 0:
                        if co[g, 3] >= f(1) / f(255):
                            out.append((y * W + x, e))
                        continue
                    alpha = min(f(0.99), co[g, 3] * f(np.exp(power)))
                    if alpha < f(1) / f(255):
                        continue
                    if T * (f(1) - alpha) < f(1e-4):
                        break
                    T = T * (f(1) - alpha)
    return out


def test_power_census_counts_a_constructed_scene(oracle):
    """orc_power_census on hand-made lists (20x18 pixels, four tiles; only tile 0 has a list) with a known answer.  Entry 3 has the
    indefinite conic (1, 0, -1) centred on (7.5, 7.5): power = (dy^2 - dx^2) / 2, exact in float32, > 0 on the 4 x 28 = 112 pixels of the
    tile with |dy| > |dx|.  Entry 0 takes alpha = 0.99 everywhere (T = 0.01); entry 1 stops column 3 (alpha = 0.99 at dx = 0, < 1/255
    elsewhere), whose 6 pixels with |dy| > 4.5 therefore never reach entry 3: 106 pairs.  Entry 2 is entry 3's twin below 1/255 opacity
    (skipped by every pixel with power clamped to 0 as well): no pair.  Then a random scene against a numpy restatement of the walk."""
    W, H = 20, 18
    xy = np.array([[7.5, 7.5], [3.0, 7.5], [7.5, 7.5], [7.5, 7.5]], np.float32)
    co = np.array([[1e-6, 0, 1e-6, 1.0], [100.0, 0, 1e-6, 1.0], [1, 0, -1, 1 / 300], [1, 0, -1, 0.5]], np.float32)
    ranges = np.zeros((4, 2), np.uint32); ranges[0] = [0, 4]
    bins = dict(R=4, point_list=np.arange(4, dtype=np.uint32), ranges=ranges)
    geo = dict(xy=xy, conic_op=co)
    pixel, pos = oracle.power_census(W, H, bins, geo)
    assert len(pixel) == 106 and (pos == 3).all()
    y, x = pixel // W, pixel % W
    assert (np.abs(y - 7.5) > np.abs(x - 7.5)).all() and not ((x == 3) & (np.abs(y - 7.5) > 4.5)).any()
    assert len(np.unique(pixel)) == 106 and (x < 16).all() and (y < 16).all()
    assert sorted(zip(pixel.tolist(), pos.tolist())) == sorted(_census_walk(W, H, bins, geo))
    # without the stopper every pixel of the tile reaches entry 3: 112
    keep = np.array([0, 2, 3], np.uint32)
    ranges[0] = [0, 3]
    assert len(oracle.power_census(W, H, dict(R=3, point_list=keep, ranges=ranges), geo)[0]) == 112
    # opacity exactly 1/255 counts, just below does not
    co2 = co.copy(); co2[3, 3] = np.float32(1) / np.float32(255)
    assert len(oracle.power_census(W, H, dict(R=3, point_list=keep, ranges=ranges), dict(xy=xy, conic_op=co2))[0]) == 112
    co2[3, 3] = np.nextafter(co2[3, 3], np.float32(0))
    assert len(oracle.power_census(W, H, dict(R=3, point_list=keep, ranges=ranges), dict(xy=xy, conic_op=co2))[0]) == 0
    # random lists over a ragged 37 x 29 image, conics of both signs, against the numpy walk (order: tile, pixel, list position)
    rng = np.random.default_rng(4)
    W, H, P = 37, 29, 60
    xy = rng.uniform(-4, 40, (P, 2)).astype(np.float32)
    co = np.stack([rng.uniform(0.01, 0.5, P), rng.uniform(-0.6, 0.6, P), rng.uniform(0.01, 0.5, P), rng.uniform(0, 1, P)], 1).astype(np.float32)
    gx, gy = 3, 2
    lists = [rng.choice(P, int(rng.integers(0, 30)), replace=False) for _ in range(gx * gy)]
    ranges = np.cumsum([0] + [len(l) for l in lists]).astype(np.uint32)
    bins = dict(R=int(ranges[-1]), point_list=np.concatenate(lists).astype(np.uint32), ranges=np.stack([ranges[:-1], ranges[1:]], 1).copy())
    pixel, pos = oracle.power_census(W, H, bins, dict(xy=xy, conic_op=co))
    ref = _census_walk(W, H, bins, dict(xy=xy, conic_op=co))
    assert len(ref) > 50 and list(zip(pixel.tolist(), pos.tolist())) == ref
