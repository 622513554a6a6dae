"""-m gpu: gm_surface_nets and gm_tsdf_integrate against their definition - the numpy float32 restatement of tests/tsdf_ref.py, bit for bit
in values, ids and order - on every grid size where a scan block can go wrong and on volumes and maps made to hurt; then the surface
above them: TsdfVolume, from_cloud on a torus cloud (mesh = the reference's on the downloaded maps; closed, one component, genus 1; binds;
drags), and the CLI."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import tsdf_ref as tr

pytestmark = pytest.mark.gpu
f32 = np.float32
BLOCK = 256                     # SN_BLOCK of csrc/gm_tsdf.hip: samples per workgroup of every scan pass
FILL = -7


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


def _origin(o):
    return (C.c_float * 3)(*[float(x) for x in o])


# ---- surface nets ----
def _device_nets(tsdf, weight, origin, voxel, min_weight=1.0, max_v=None, max_f=None):
    """gm_surface_nets through ctypes: (vertex buffer, face buffer, counts); the buffers pre-filled with FILL, the workspace at an odd
    address; capacities default to the largest output the grid can give"""
    from gaussianmesh_amd import _lib
    lib = _lib.lib()
    nz, ny, nx = tsdf.shape
    cells = (nx - 1) * (ny - 1) * (nz - 1)
    max_v = cells if max_v is None else max_v
    max_f = 6 * nx * ny * nz if max_f is None else max_f
    V = torch.full((max(max_v, 1), 3), float(FILL), device="cuda")
    F = torch.full((max(max_f, 1), 3), FILL, dtype=torch.int32, device="cuda")
    counts = torch.full((2,), FILL, dtype=torch.int32, device="cuda")
    nbytes = lib.gm_surface_nets_workspace_bytes(nx, ny, nz)
    ws = torch.empty((nbytes + 64,), dtype=torch.uint8, device="cuda")
    d, w = _dev(tsdf), _dev(weight)
    _lib.check(lib.gm_surface_nets(nx, ny, nz, _origin(origin), float(voxel), d.data_ptr(), w.data_ptr(), float(min_weight), max_v, V.data_ptr(),
                                   max_f, F.data_ptr(), counts.data_ptr(), ws.data_ptr() + 4, nbytes, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return V.cpu().numpy()[:max_v], F.cpu().numpy()[:max_f], counts.cpu().numpy()


def _same_mesh(got, ref, what):
    (V, F, counts), (rV, rF) = got, ref
    assert counts.tolist() == [len(rV), len(rF)], "%s: counts %s, reference %d vertices %d faces" % (what, counts.tolist(), len(rV), len(rF))
    assert np.array_equal(F[:len(rF)], rF), "%s: face rows differ" % what
    assert np.array_equal(_bits(V[:len(rV)]), _bits(rV)), "%s: vertex bits differ" % what
    assert (V[len(rV):] == FILL).all() and (F[len(rF):] == FILL).all(), "%s: rows beyond the counts were written" % what


FIELDS = {
    "sphere": lambda n: tr.sphere_field(n),
    "torus": lambda n: tr.torus_field(n, R=0.55, r=0.25),
    "plane": lambda n: tr.plane_field(n, level=n[2] // 2),
    "checker": lambda n: tr.checker_field(n),
    "positive": lambda n: tr.positive_field(n),
    "noise": lambda n: tr.noise_field(n, seed=n[0] + 7 * n[1]),
}
# sample counts at one scan block -1 / exact / +2 (257 is prime) and at the second level of block sums -1 / exact / +4 (65537 is prime);
# (4,6,18) and (5,9,9): 255 and 256 CELLS, all active under the checkerboard
GRIDS = [(2, 2, 2), (3, 3, 3), (5, 7, 9), (33, 17, 65), (64, 64, 64), (3, 5, 17), (4, 8, 8), (2, 3, 43), (15, 17, 257), (32, 32, 64), (20, 29, 113),
         (4, 6, 18), (5, 9, 9)]


@pytest.mark.parametrize("n", GRIDS, ids=lambda n: "%dx%dx%d" % n)
def test_extraction_bit_for_bit(n):
    assert [g[0] * g[1] * g[2] for g in GRIDS[5:11]] == [BLOCK - 1, BLOCK, BLOCK + 2, BLOCK * BLOCK - 1, BLOCK * BLOCK, BLOCK * BLOCK + 4]
    total = 0
    for name, make in FIELDS.items():
        tsdf, w, origin, voxel = make(n)
        ref = tr.surface_nets_ref(tsdf, w, origin, voxel, 1.0)
        total += len(ref[0]) + len(ref[1])
        _same_mesh(_device_nets(tsdf, w, origin, voxel), ref, "%s %s" % (name, n))
        if name == "checker":
            cells = (n[0] - 1) * (n[1] - 1) * (n[2] - 1)
            assert len(ref[0]) == cells                                # every cell active
    assert total > 0


def test_half_observed_volume_gives_the_reference_open_boundary():
    tsdf, w, origin, voxel = tr.sphere_field((33, 17, 29), radius=0.35)
    w[:, :, 16:] = 0
    ref = tr.surface_nets_ref(tsdf, w, origin, voxel, 1.0)
    assert len(ref[0]) > 200 and tr.boundary_edges(ref[1]) > 20
    _same_mesh(_device_nets(tsdf, w, origin, voxel), ref, "half-observed sphere")
    # min_weight is a threshold on the weight itself
    w2 = np.random.default_rng(3).integers(0, 4, size=w.shape).astype(f32)
    for mw in (0.0, 1.0, 2.5, 3.0, 4.0):
        ref = tr.surface_nets_ref(tsdf, w2, origin, voxel, mw)
        _same_mesh(_device_nets(tsdf, w2, origin, voxel, min_weight=mw), ref, "min_weight %g" % mw)
    assert len(ref[0]) == 0 and len(ref[1]) == 0                       # nothing weighs 4: the empty result


def test_capacity_short_of_need_reports_the_counts_and_writes_the_prefix():
    tsdf, w, origin, voxel = tr.torus_field((40, 18, 40), R=0.6, r=0.225)
    rV, rF = tr.surface_nets_ref(tsdf, w, origin, voxel, 1.0)
    for max_v, max_f in ((len(rV) - 1, len(rF) - 1), (len(rV), len(rF) - 3), (BLOCK, 2 * BLOCK + 1), (1, 1), (0, 0), (len(rV), len(rF))):
        V, F, counts = _device_nets(tsdf, w, origin, voxel, max_v=max_v, max_f=max_f)
        assert counts.tolist() == [len(rV), len(rF)], (max_v, max_f)
        assert np.array_equal(_bits(V), _bits(rV[:max_v])) and np.array_equal(F, rF[:max_f]), (max_v, max_f)


def test_extraction_gives_the_same_bits_twice():
    tsdf, w, origin, voxel = tr.noise_field((33, 17, 65), seed=5)
    one, two = _device_nets(tsdf, w, origin, voxel), _device_nets(tsdf, w, origin, voxel)
    assert all(np.array_equal(a.view(np.uint32) if a.dtype == f32 else a, b.view(np.uint32) if b.dtype == f32 else b) for a, b in zip(one, two))


# ---- fusion ----
def _device_integrate(tsdf, weight, depth, alpha, views, tans, origin, voxel, trunc, alpha_min=0.5, carve=True, one_at_a_time=False):
    from gaussianmesh_amd import _lib
    lib = _lib.lib()
    nz, ny, nx = tsdf.shape
    K, H, W = depth.shape
    D, Wt = _dev(tsdf), _dev(weight)
    d, a, v, t = _dev(depth), _dev(alpha), _dev(np.asarray(views, f32).reshape(K, 16)), _dev(np.asarray(tans, f32).reshape(K, 2))
    s = torch.cuda.current_stream().cuda_stream
    call = lambda k, kk: _lib.check(lib.gm_tsdf_integrate(kk, H, W, d[k:].data_ptr(), a[k:].data_ptr(), v[k:].data_ptr(), t[k:].data_ptr(), nx, ny, nz,
                                                          _origin(origin), float(voxel), float(trunc), float(alpha_min), int(carve), D.data_ptr(),
                                                          Wt.data_ptr(), s))
    if one_at_a_time:
        for k in range(K):
            call(k, 1)
    else:
        call(0, K)
    torch.cuda.synchronize()
    return D.cpu().numpy(), Wt.cpu().numpy()


def _same_volume(got, ref, what):
    assert np.array_equal(_bits(got[1]), _bits(ref[1])), "%s: %d weights differ" % (what, (got[1] != ref[1]).sum())
    bad = np.nonzero(_bits(got[0]) != _bits(ref[0]))
    assert len(bad[0]) == 0, "%s: %d tsdf values differ, first at %s: device %r reference %r" % (
        what, len(bad[0]), [int(b[0]) for b in bad], got[0][bad][0], ref[0][bad][0])


def _orbit_case(n, H, W, K, seed):
    """K orbit cameras around a grid of n voxels that they see whole or in part, depth maps around the distance to its middle with
    alpha from a pool that sits on both sides of 0.5; a non-empty volume to start from"""
    from gaussianmesh_amd import scenes
    rng = np.random.default_rng(seed)
    nx, ny, nz = n
    voxel = 2.0 / max(n)
    origin = np.array([-0.5 * nx * voxel + 0.013, -0.5 * ny * voxel - 0.007, -0.5 * nz * voxel + 0.021], f32)
    cams = [scenes.orbit_camera(k, K, W, H, radius=(2.6, 1.7, 3.5)[k % 3], height=(1.2, -0.8, 0.3)[k % 3], fovx_deg=(60.0, 35.0)[k % 2]) for k in range(K)]
    views, tans = tr.camera_rows(cams)
    dist = np.array([np.linalg.norm(c["campos"]) for c in cams], f32)
    depth = (dist[:, None, None] + rng.normal(0, 0.4, size=(K, H, W))).astype(f32)
    alpha = rng.choice(np.array([0.0, 0.2, 0.49999997, 0.5, 0.50000006, 0.8, 1.0], f32), size=(K, H, W))
    depth = (depth * alpha).astype(f32)                               # the rasterizer's map: depth is alpha-weighted
    tsdf0 = rng.uniform(-1, 1, size=(nz, ny, nx)).astype(f32)
    w0 = rng.integers(0, 3, size=(nz, ny, nx)).astype(f32)
    return tsdf0, w0, depth, alpha, views, tans, origin, voxel


@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("HW", [(23, 37), (64, 64)], ids=["37x23", "64x64"])
@pytest.mark.parametrize("n", [(5, 7, 9), (32, 32, 32)], ids=["5x7x9", "32x32x32"])
def test_fusion_bit_for_bit(n, HW, K):
    tsdf0, w0, depth, alpha, views, tans, origin, voxel = _orbit_case(n, HW[0], HW[1], K, seed=K + HW[0])
    trunc = 3 * voxel
    for carve in (True, False):
        ref = tr.integrate_ref(tsdf0, w0, depth, alpha, views, tans, origin, voxel, trunc, 0.5, carve)
        assert (ref[1] > w0).any() and (ref[1] < w0 + K).any()          # views taken, views skipped
        got = _device_integrate(tsdf0, w0, depth, alpha, views, tans, origin, voxel, trunc, 0.5, carve)
        _same_volume(got, ref, "n %s maps %s K %d carve %s" % (n, HW, K, carve))
        each = _device_integrate(tsdf0, w0, depth, alpha, views, tans, origin, voxel, trunc, 0.5, carve, one_at_a_time=True)
        _same_volume(each, got, "one view at a time")
    zero = np.zeros_like(tsdf0)
    _same_volume(_device_integrate(zero, zero, depth, alpha, views, tans, origin, voxel, trunc),
                 tr.integrate_ref(zero, zero, depth, alpha, views, tans, origin, voxel, trunc), "from the empty volume")


def _exact_case(H=8, W=8):
    """An identity camera at the origin looking along +z and a grid whose centres are multiples of 1/8: every product is exact, so
    the cases below occur EXACTLY - z == 0 (skipped), pixel coordinates on halves (floor(px + 0.5) decides), a column just outside
    each image edge, s == -trunc, 0 and trunc, alpha at and beside alpha_min, depth 0 with alpha 0"""
    n = (21, 19, 9)
    voxel, trunc = 0.125, 0.375
    origin = np.array([-(10 + 0.5) * voxel, -(9 + 0.5) * voxel, -0.5 * voxel], f32)       # centres: x -1.25 .. 1.25, y -1.125 .. 1.125, z 0 .. 1
    views = np.eye(4, dtype=f32)[None]
    tans = np.array([[1.0, 1.0]], f32)
    rng = np.random.default_rng(11)
    alpha = rng.choice(np.array([0.0, 0.25, 0.49999997, 0.5, 0.50000006, 1.0], f32), size=(1, H, W))
    z = rng.integers(0, 17, size=(1, H, W)).astype(f32) * f32(0.125)                      # expected depths on the grid's own layers and beyond
    depth = (z * alpha).astype(f32)                                                       # (alpha 0 -> depth 0)
    return n, voxel, trunc, origin, views, tans, depth, alpha


def test_fusion_cases_that_occur_exactly():
    n, voxel, trunc, origin, views, tans, depth, alpha = _exact_case()
    nx, ny, nz = n
    zero = np.zeros((nz, ny, nx), f32)
    # the case holds what it promises (float64 restatement of the exact quantities)
    X, Z = tr.voxel_centres(nx, origin[0], voxel), tr.voxel_centres(nz, origin[2], voxel)
    assert Z[0] == 0 and Z[8] == 1 and X[0] == -1.25
    px = ((X / (Z[8] * f32(1)) + 1) * 8 - 1) * 0.5                                        # on the layer z = 1
    assert (px == np.floor(px)).sum() >= 8 and (px - np.floor(px) == 0.5).sum() >= 8      # pixel centres and exact halves
    assert px.min() == -1.5 and px.max() == 8.5                                           # -1.5 -> -1: outside; -0.5 -> pixel 0; 7.5 -> 8: outside
    for carve in (True, False):
        for alpha_min in (0.5, 0.0, 0.50000006):
            ref = tr.integrate_ref(zero, zero, depth, alpha, views, tans, origin, voxel, trunc, alpha_min, carve)
            got = _device_integrate(zero, zero, depth, alpha, views, tans, origin, voxel, trunc, alpha_min, carve)
            _same_volume(got, ref, "exact case carve %s alpha_min %g" % (carve, alpha_min))
    ref = tr.integrate_ref(zero, zero, depth, alpha, views, tans, origin, voxel, trunc, 0.5, True)
    assert (ref[1][0] == 0).all()                                                         # the layer z == 0 is skipped
    # on the layer z = 1: px = -1.5, -1 (floor(-0.5) = -1) are outside, -0.5 is pixel 0; 7 is pixel 7, 7.5 (floor(8) = 8), 8 and 8.5 are outside
    assert (ref[1][8][:, :2] == 0).all() and (ref[1][8][:, -3:] == 0).all()
    assert (ref[1][8][:, 2] == 1).any() and (ref[1][8][:, -4] == 1).any()
    seen = ref[1] == 1
    assert (ref[0][seen] == 1).any() and (ref[0][seen] == 0).any() and (ref[0][seen] == -1).any()      # s == trunc, 0, -trunc (kept)
    # s just beyond -trunc is unobserved: on the layer z = 1 a pixel with expected depth 0.5 leaves its voxels untouched
    d2, a2 = np.full((1, 8, 8), f32(0.5)), np.ones((1, 8, 8), f32)
    ref = tr.integrate_ref(zero, zero, d2, a2, views, tans, origin, voxel, trunc, 0.5, True)
    assert (ref[1][8] == 0).all() and (ref[1][7][9, 10] == 1) and ref[0][7][9, 10] == -1 and (ref[1][4][9, 10] == 1) and ref[0][4][9, 10] == 0
    _same_volume(_device_integrate(zero, zero, d2, a2, views, tans, origin, voxel, trunc), ref, "a wall at 0.5")


def test_camera_inside_the_grid_and_nan_maps():
    from gaussianmesh_amd import scenes
    n = (17, 13, 15)
    voxel = 0.125
    origin = np.array([-1.0, -0.8, -0.9], f32)
    cams = [scenes.look_at_camera((0.05, 0.02, -0.03), (1.0, 0.3, 0.2), 37, 23), scenes.look_at_camera((-0.3, -0.2, 0.1), (1.0, 0.0, 0.5), 37, 23)]
    views, tans = tr.camera_rows(cams)
    rng = np.random.default_rng(2)
    alpha = rng.choice(np.array([0.0, 0.3, 0.7, 1.0], f32), size=(2, 23, 37))
    depth = (rng.uniform(0.1, 1.5, size=(2, 23, 37)).astype(f32) * alpha).astype(f32)
    depth[0, 3, 5], alpha[1, 7, 9] = np.nan, np.nan                                       # a NaN skips the view (alpha) or the sample (depth)
    zero = np.zeros((n[2], n[1], n[0]), f32)
    ref = tr.integrate_ref(zero, zero, depth, alpha, views, tans, origin, voxel, 0.375)
    assert (ref[1] == 0).sum() > 500 and (ref[1] == 2).sum() > 50 and not np.isnan(ref[0]).any()      # behind both cameras / seen by both
    _same_volume(_device_integrate(zero, zero, depth, alpha, views, tans, origin, voxel, 0.375), ref, "cameras inside the grid")


# ---- the Python surface ----
def test_volume_class_groups_views_by_resolution_and_refuses_cpu_maps():
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd._lib import GmeshError
    from gaussianmesh_amd.proxy_mesh import TsdfVolume
    from gaussianmesh_amd.renderer import Camera
    a = _orbit_case((12, 9, 11), 23, 37, 3, seed=1)
    b = _orbit_case((12, 9, 11), 64, 64, 2, seed=2)
    origin, voxel = a[6], a[7]
    hi = origin.astype(np.float64) + np.array([12, 9, 11]) * voxel
    vol = TsdfVolume(origin, hi, voxel_size=voxel)
    assert (vol.nx, vol.ny, vol.nz) == (12, 9, 11) and vol.trunc == float(f32(3 * voxel)) and vol.voxel == float(f32(voxel))
    cams_a = [scenes.orbit_camera(k, 3, 37, 23, radius=(2.6, 1.7, 3.5)[k % 3], height=(1.2, -0.8, 0.3)[k % 3], fovx_deg=(60.0, 35.0)[k % 2]) for k in range(3)]
    cams_b = [scenes.orbit_camera(k, 2, 64, 64, radius=(2.6, 1.7, 3.5)[k % 3], height=(1.2, -0.8, 0.3)[k % 3], fovx_deg=(60.0, 35.0)[k % 2]) for k in range(2)]
    cams = [Camera(c, "cuda") for c in cams_a[:2]] + cams_b + [Camera(cams_a[2], "cuda")]                 # objects and dicts, three runs of a resolution
    depth = [_dev(a[2][0]), _dev(a[2][1])[None], _dev(b[2][0]), _dev(b[2][1]), _dev(a[2][2])]
    alpha = [_dev(a[3][0]), _dev(a[3][1])[None], _dev(b[3][0]), _dev(b[3][1]), _dev(a[3][2])]
    vol.integrate(cams, depth, alpha)
    zero = np.zeros((11, 9, 12), f32)
    ref = tr.integrate_ref(zero, zero, a[2][:2], a[3][:2], a[4][:2], a[5][:2], origin, vol.voxel, vol.trunc)
    ref = tr.integrate_ref(*ref, b[2], b[3], b[4], b[5], origin, vol.voxel, vol.trunc)
    ref = tr.integrate_ref(*ref, a[2][2:], a[3][2:], a[4][2:], a[5][2:], origin, vol.voxel, vol.trunc)
    _same_volume((vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy()), ref, "TsdfVolume.integrate")
    assert vol.views == 5
    V, F = vol.extract(keep="all")
    rV, rF = tr.surface_nets_ref(ref[0], ref[1], origin, vol.voxel, 1.0)
    assert V.is_cuda and F.dtype == torch.int32 and np.array_equal(_bits(V.cpu().numpy()), _bits(rV)) and np.array_equal(F.cpu().numpy(), rF)
    Vl, Fl = vol.extract(keep="largest")
    lV, lF = tr.keep_largest_ref(rV, rF)
    assert np.array_equal(_bits(Vl.cpu().numpy()), _bits(lV)) and np.array_equal(Fl.cpu().numpy(), lF) and vol.stats["components"] >= 1
    with pytest.raises(GmeshError):
        vol.integrate(cams[:1], [torch.zeros(23, 37)], [torch.zeros(23, 37)])
    with pytest.raises(ValueError):
        vol.integrate(cams[:1], [_dev(b[2][0])], [_dev(b[3][0])])                          # a 37 x 23 camera with 64 x 64 maps
    with pytest.raises(ValueError):
        vol.extract(keep="some")


def test_extract_retries_when_the_guess_is_short():
    from gaussianmesh_amd.proxy_mesh import TsdfVolume
    tsdf, w, origin, voxel = tr.checker_field((40, 30, 20))                                # 21 489 vertices: far more than a surface's share
    vol = TsdfVolume(origin, origin.astype(np.float64) + np.array([40, 30, 20]) * float(voxel), voxel_size=float(voxel))
    vol.tsdf.copy_(_dev(tsdf)); vol.weight.copy_(_dev(w))
    V, F = vol.extract(keep="all")
    rV, rF = tr.surface_nets_ref(tsdf, w, origin, vol.voxel, 1.0)
    assert len(rV) == 39 * 29 * 19 > max(4096, 8 * 40 * 30)
    assert np.array_equal(_bits(V.cpu().numpy()), _bits(rV)) and np.array_equal(F.cpu().numpy(), rF)


# ---- end to end: a torus cloud -> its proxy mesh -> an edit ----
E2E = dict(P=40000, nu=48, nv=32, K=12, W=128, H=128, resolution=48)


def _torus_cloud(P, nu, nv, seed=5):
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.bg_model import PlainGaussians, inverse_sigmoid
    verts, faces = scenes.torus_mesh(nu, nv)
    cl = scenes.bind_cloud_to_mesh(P, verts, faces, seed=seed)
    model = PlainGaussians(3, device="cuda")
    model._set_params(_dev(cl["means"]), _dev(cl["shs"]), torch.log(_dev(cl["scales"])), _dev(cl["rots"]), inverse_sigmoid(_dev(cl["opac"])))
    model.active_sh_degree = 3
    return model, cl, verts.astype(f32), faces


def _orbit(K, W, H):
    from gaussianmesh_amd import scenes
    return [scenes.orbit_camera(k, K, W, H, radius=6.5, height=(4.5, -4.5)[k % 2]) for k in range(K)]


def _mesh_report(V, F):
    edges, uses = tr.edge_use(F)
    f = F.astype(np.int64)
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    key = lambda e: np.sort(e[:, 0] * max(len(V), 1) + e[:, 1])
    return dict(vertices=len(V), faces=len(F), odd_edges=int((uses % 2 == 1).sum()), four_edges=int((uses == 4).sum()),
                oriented=bool(np.array_equal(key(directed), key(directed[:, ::-1]))), components=tr.n_components(len(V), F),
                euler=tr.euler_characteristic(len(V), F))


def e2e_run(P, nu, nv, K, W, H, resolution, tmp=None):
    """the whole path once; returns what the test asserts on (also called by measurement scripts)"""
    from types import SimpleNamespace
    from gaussianmesh_amd import proxy_mesh as pm
    from gaussianmesh_amd.renderer import Camera, bg_render
    model, cl, verts, faces = _torus_cloud(P, nu, nv)
    cam_dicts = _orbit(K, W, H)
    cams = [Camera(c, "cuda") for c in cam_dicts]
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    lo, hi, voxel = pm.default_bounds(model, resolution)
    out = dict(model=model, cl=cl, cams=cam_dicts, bounds=(lo, hi))
    with torch.no_grad():
        maps = [bg_render(c, model, pipe, torch.zeros(3, device="cuda"), return_aux=True) for c in cams]
    depth, alpha = [m["depth"] for m in maps], [m["alpha"] for m in maps]
    vol = pm.TsdfVolume(lo, hi, voxel_size=voxel, trunc=3.0 * voxel)
    vol.integrate(cams, depth, alpha)
    out["vol"] = vol
    out["maps"] = (torch.cat(depth).cpu().numpy(), torch.cat(alpha).cpu().numpy())
    out["all"] = tuple(x.cpu().numpy() for x in vol.extract(keep="all"))
    out["largest"] = vol.extract(keep="largest")
    out["stats"] = dict(vol.stats)
    out["from_cloud"] = pm.from_cloud(model, cam_dicts, resolution=resolution)
    return out


@functools.lru_cache(maxsize=None)
def _e2e():
    return e2e_run(**E2E)


def test_end_to_end_device_mesh_equals_the_reference_on_the_downloaded_maps():
    r = _e2e()
    vol, (depth, alpha) = r["vol"], r["maps"]
    assert depth.shape == (12, 128, 128) and 0.1 < (alpha > 0.5).mean() < 0.6
    views, tans = tr.camera_rows(r["cams"])
    zero = np.zeros((vol.nz, vol.ny, vol.nx), f32)
    assert max(vol.nx, vol.ny, vol.nz) == 48
    ref = tr.integrate_ref(zero, zero, depth, alpha, views, tans, vol.origin, vol.voxel, vol.trunc, 0.5, True)
    _same_volume((vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy()), ref, "fused torus cloud")
    rV, rF = tr.surface_nets_ref(ref[0], ref[1], vol.origin, vol.voxel, 1.0)
    assert np.array_equal(_bits(r["all"][0]), _bits(rV)) and np.array_equal(r["all"][1], rF)
    lV, lF = tr.keep_largest_ref(rV, rF)
    V, F = r["largest"]
    assert np.array_equal(_bits(V.cpu().numpy()), _bits(lV)) and np.array_equal(F.cpu().numpy(), lF)
    assert torch.equal(r["from_cloud"][0], V) and torch.equal(r["from_cloud"][1], F)      # from_cloud is these steps


def test_end_to_end_mesh_is_closed_genus_one_binds_and_drags():
    """Closed as in test_proxy_mesh_host: no edge held by an odd number of faces, every directed edge with its opposite (naive surface
    nets gives an edge four faces where the surface passes diagonally through a grid face)."""
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.deform import SingleObjectDeform
    from gaussianmesh_amd.mesh_bind import bind_points
    r = _e2e()
    V, F = r["largest"]
    v, f = V.cpu().numpy(), F.cpu().numpy()
    rep = _mesh_report(v, f)
    print("proxy mesh of the torus cloud:", rep, r["stats"])
    assert 2000 < rep["vertices"] < 9000 and rep["faces"] >= 2 * rep["vertices"]
    assert rep["odd_edges"] == 0 and rep["oriented"] and rep["components"] == 1 and rep["euler"] == 0
    assert tr.signed_volume(v, f) > 0
    # the cloud binds to it, near its surface
    cl = r["cl"]
    pts = _dev(cl["means"])
    b = bind_points(pts, V, F)
    assert b["tri"].shape == (len(pts), 3) and np.isfinite(b["weights"]).all() and float(np.sqrt(b["sqr_distance"].max())) < 0.6
    # and ArapSolver takes it: one drag of a few handles completes and moves the mesh and the cloud
    cov = scenes.cov3d_from_scale_rot(cl["scales"], cl["rots"])
    o = SingleObjectDeform(pts, _dev(cov), _dev(cl["opac"]), _dev(cl["shs"]), _dev(b["tri"], torch.int32), _dev(b["weights"]), V)
    ids = np.array([int(np.argmax(v[:, 0])), int(np.argmin(v[:, 0])), int(np.argmax(v[:, 2])), int(np.argmin(v[:, 2]))])
    o.set_handles(ids, faces=F)
    target = v[ids].copy()
    target[0] += (0.3, 0.4, 0.0)
    pos = o.drag(_dev(target))[0]
    torch.cuda.synchronize()
    moved = o.mesh_vertex_current.cpu().numpy()
    assert np.isfinite(moved).all() and np.array_equal(moved[ids], target.astype(f32)) and np.abs(moved - v).max() >= 0.4
    assert torch.isfinite(pos).all() and float((pos - pts).abs().max()) > 0.1


def test_cli_writes_the_same_mesh(tmp_path, capsys):
    from gaussianmesh_amd import io as gio
    from gaussianmesh_amd import proxy_mesh as pm
    r = _e2e()
    ply, cj, obj = str(tmp_path / "cloud.ply"), str(tmp_path / "cameras.json"), str(tmp_path / "proxy.obj")
    r["model"].save_ply(ply)
    entries = []
    for k, c in enumerate(r["cams"]):
        Rt = c["view"].T.astype(np.float64)
        entries.append(gio.camera_to_json(k, Rt[:3, :3].T, Rt[:3, 3], c["W"], c["H"], c["fovx"], c["fovy"], "v%d" % k))
    with open(cj, "w") as fh:
        json.dump(entries, fh)
    lo, hi = r["bounds"]
    assert pm.main(["--gaussian", ply, "--cameras", cj, "--out", obj, "--resolution", "48", "--bounds"] + [repr(float(x)) for x in (*lo, *hi)]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    v, f = gio.read_obj(obj)
    assert line["vertices"] == len(v) and line["faces"] == len(f) and line["boundary_edges"] == 0 and set(line["seconds"]) == {"load", "render_fuse", "extract", "write"}
    # the same arrays as the module call on the cameras the CLI read back (a cameras.json round trip moves the last bits of a view)
    V, F = pm.from_cloud(r["model"], gio.load_cameras_json(cj), resolution=48, bounds=(lo, hi))
    assert np.array_equal(v, V.cpu().numpy().astype(np.float64)) and np.array_equal(f, F.cpu().numpy())
    assert os.path.getsize(obj) > 100000
