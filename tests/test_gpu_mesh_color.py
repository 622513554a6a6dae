"""-m gpu: gm_mesh_vertex_normals, gm_mesh_color_integrate and gm_mesh_color_spread against their definition - the numpy float32
restatement of tests/mesh_color_ref.py, bit for bit - at every vertex count where a workgroup edge can go wrong, on square and
non-square maps, for one view and several, with every decision hit exactly on its edge; on guard-banded, poisoned buffers; then the
surface above them: VertexColors, color_from_cloud, from_cloud(vertex_colors=True) on a two-coloured torus cloud, both CLIs and the
preview."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import mesh_color_cases as mc
import mesh_color_ref as mr
import poison
import tsdf_ref as tr

pytestmark = pytest.mark.gpu
f32 = np.float32
FILL = -7
SIZES = (1, 255, 256, 257)          # vertices: one, and a 256-thread workgroup less one / exactly / plus one
FALLBACK = (0.125, 0.25, 0.375)


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _dev(a, dt=torch.float32):
    return torch.as_tensor(np.array(a, order="C"), dtype=dt, device="cuda")      # (a copy: the shared cases are read-only)


def _same(got, ref, what):
    bad = np.nonzero(_bits(got) != _bits(ref))
    assert len(bad[0]) == 0, "%s: %d values differ, first at %s: device %r reference %r" % (
        what, len(bad[0]), [int(b[0]) for b in bad], np.asarray(got)[bad][0], np.asarray(ref)[bad][0])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _adj(F, Vm):
    off, adj = mr.adjacency(F, Vm)
    return _dev(off, torch.int32), _dev(adj, torch.int32)


# ---- the three calls through ctypes ----
def _device_normals(V, F):
    from gaussianmesh_amd import _lib
    Vd, Fd = _dev(V), _dev(F, torch.int32)
    off, adj = _adj(F, len(V))
    out = torch.full((len(V), 3), float(FILL), device="cuda")
    _lib.check(_lib.lib().gm_mesh_vertex_normals(len(V), len(F), Vd.data_ptr(), Fd.data_ptr(), off.data_ptr(), adj.data_ptr(), out.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _device_integrate(csum, wsum, image, depth, alpha, views, tans, P, N, alpha_min=0.5, tol=0.25, two_sided=False, one_at_a_time=False):
    from gaussianmesh_amd import _lib
    lib = _lib.lib()
    K, H, W = depth.shape
    cs, ws = _dev(np.array(csum, f32)), _dev(np.array(wsum, f32))
    im, d, a, v, t = _dev(image), _dev(depth), _dev(alpha), _dev(np.asarray(views, f32).reshape(K, 16)), _dev(np.asarray(tans, f32).reshape(K, 2))
    Pd, Nd = _dev(P), _dev(N)
    call = lambda k, kk: _lib.check(lib.gm_mesh_color_integrate(kk, H, W, im[k:].data_ptr(), d[k:].data_ptr(), a[k:].data_ptr(), v[k:].data_ptr(),
                                                                t[k:].data_ptr(), len(P), Pd.data_ptr(), Nd.data_ptr(), float(alpha_min), float(tol),
                                                                int(two_sided), cs.data_ptr(), ws.data_ptr(), _stream()))
    if one_at_a_time:
        for k in range(K):
            call(k, 1)
    else:
        call(0, K)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Pd.cpu().numpy()), _bits(P)) and np.array_equal(_bits(Nd.cpu().numpy()), _bits(N)), "the inputs changed"
    return cs.cpu().numpy(), ws.cpu().numpy()


def _device_spread(F, Vm, seen, colors, iterations, fallback=FALLBACK):
    """(colors, has, counts): out_has and out_counts pre-filled with FILL, the workspace at an odd address and full of 0xA5"""
    from gaussianmesh_amd import _lib
    lib = _lib.lib()
    Fd = _dev(F, torch.int32)
    off, adj = _adj(F, Vm)
    sn, col = _dev(seen, torch.uint8), _dev(np.array(colors, f32))
    has = torch.full((max(Vm, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    counts = torch.full((2,), FILL, dtype=torch.int32, device="cuda")
    nbytes = lib.gm_mesh_color_spread_workspace_bytes(Vm)
    ws = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    _lib.check(lib.gm_mesh_color_spread(Vm, len(F), Fd.data_ptr(), off.data_ptr(), adj.data_ptr(), sn.data_ptr(), int(iterations),
                                        (C.c_float * 3)(*fallback), col.data_ptr(), has.data_ptr(), counts.data_ptr(), ws.data_ptr() + 4, nbytes,
                                        _stream()))
    torch.cuda.synchronize()
    assert np.array_equal(sn.cpu().numpy(), seen), "seen changed"
    return col.cpu().numpy(), has.cpu().numpy()[:Vm], counts.cpu().numpy()


def _same_spread(got, ref, what):
    assert got[2].tolist() == ref[2].tolist(), "%s: counts %s, reference %s" % (what, got[2].tolist(), ref[2].tolist())
    assert np.array_equal(got[1], ref[1]), "%s: %d states differ" % (what, (got[1] != ref[1]).sum())
    _same(got[0], ref[0], what)


# ---- normals ----
def test_normals_bit_for_bit():
    V, F = mc.torus()
    ref = mr.vertex_normals_ref(V, F)
    _same(_device_normals(V, F), ref, "torus 24 x 16")
    assert (np.abs(ref).sum(1) > 0).all()
    Vo, Fo = mr.octahedron()
    Vo = np.concatenate([Vo, [[7, 7, 7]]]).astype(f32)
    got = _device_normals(Vo, Fo)
    _same(got, mr.vertex_normals_ref(Vo, Fo), "octahedron and a vertex without faces")
    assert np.array_equal(_bits(got[:6]), _bits(4 * Vo[:6])) and np.array_equal(_bits(got[6]), _bits(np.zeros(3, f32)))
    for Vm in SIZES:
        Vs, Fs = mc.mesh_of(Vm)
        assert len(Vs) == Vm
        _same(_device_normals(Vs, Fs), mr.vertex_normals_ref(Vs, Fs), "%d vertices" % Vm)
    # NaN and inf positions go through as the arithmetic says: NaN where the reference has one (inf - inf makes a NaN whose sign and
    # payload are the hardware's own, not the definition's), the same bits everywhere else
    Vn = np.array(mc.mesh_of(256)[0])
    Vn[7, 1], Vn[100, 0] = np.nan, np.inf
    got, ref = _device_normals(Vn, mc.mesh_of(256)[1]), mr.vertex_normals_ref(Vn, mc.mesh_of(256)[1])
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and 6 < np.isnan(ref).sum() < 60
    _same(np.where(np.isnan(ref), f32(0), got), np.where(np.isnan(ref), f32(0), ref), "NaN and inf positions")


# ---- integration ----
@pytest.mark.parametrize("HW", [(8, 8), (7, 13), (32, 32)], ids=["8x8", "13x7", "32x32"])
def test_integration_bit_for_bit(HW):
    H, W = HW
    taken = skipped = 0
    for K in (1, 3, 6):
        V, F, N, image, depth, alpha, views, tans = mc.orbit_case(K, H, W)
        for Vm in SIZES:
            P, Nr, cs0, ws0 = mc.random_vertices(Vm, K, H, W, seed=Vm + K)
            for two_sided in (False, True):
                what = "maps %s K %d Vm %d two_sided %s" % (HW, K, Vm, two_sided)
                ref = mr.integrate_ref(cs0, ws0, image, depth, alpha, views, tans, P, Nr, 0.5, 3.0, two_sided)
                got = _device_integrate(cs0, ws0, image, depth, alpha, views, tans, P, Nr, 0.5, 3.0, two_sided)
                _same(got[1], ref[1], what + ": wsum")
                _same(got[0], ref[0], what + ": csum")
                taken, skipped = taken + int((ref[1] != ws0).sum()), skipped + int((ref[1] == ws0).sum())
        # the torus itself, with its own normals, from the empty state: K views in one call are K calls of one; twice the same bits
        zero3, zero = np.zeros((len(V), 3), f32), np.zeros(len(V), f32)
        ref = mr.integrate_ref(zero3, zero, image, depth, alpha, views, tans, V, N, 0.5, mc.torus_tol())
        got = _device_integrate(zero3, zero, image, depth, alpha, views, tans, V, N, 0.5, mc.torus_tol())
        _same(got[1], ref[1], "torus K %d: wsum" % K)
        _same(got[0], ref[0], "torus K %d: csum" % K)
        each = _device_integrate(zero3, zero, image, depth, alpha, views, tans, V, N, 0.5, mc.torus_tol(), one_at_a_time=True)
        again = _device_integrate(zero3, zero, image, depth, alpha, views, tans, V, N, 0.5, mc.torus_tol())
        for other, name in ((each, "one view at a time"), (again, "a second run")):
            _same(other[0], got[0], name)
            _same(other[1], got[1], name)
        seen = ref[1] > 0
        assert seen.any() and not seen[V[:, 1] < -0.69].any()         # the orbit is above: a band of the torus stays unseen
    assert taken > 0 and skipped > 0


@pytest.mark.parametrize("two_sided", [False, True], ids=["one-sided", "two-sided"])
@pytest.mark.parametrize("alpha_min", [0.5, 0.0])
def test_every_decision_edge_on_the_device(alpha_min, two_sided):
    c = mc.edge_case()
    n = len(c["names"])
    zero3, zero = np.zeros((n, 3), f32), np.zeros(n, f32)
    args = (c["image"], c["depth"], c["alpha"], c["views"], c["tans"], c["P"], c["N"], alpha_min, mc.DEPTH_TOL, two_sided)
    ref = mr.integrate_ref(zero3, zero, *args)
    got = _device_integrate(zero3, zero, *args)
    want = c["expect"](alpha_min, two_sided)
    assert [c["names"][i] for i in np.nonzero((got[1] > 0) != want)[0]] == []
    _same(got[1], ref[1], "edge case: wsum")
    _same(got[0], ref[0], "edge case: csum")
    # a skipped view leaves a non-empty state's bits alone
    rng = np.random.default_rng(1)
    cs0, ws0 = rng.uniform(0, 1, size=(n, 3)).astype(f32), rng.uniform(0, 1, size=n).astype(f32)
    got = _device_integrate(cs0, ws0, *args)
    assert np.array_equal(_bits(got[0][~want]), _bits(cs0[~want])) and np.array_equal(_bits(got[1][~want]), _bits(ws0[~want]))
    _same(got[1], mr.integrate_ref(cs0, ws0, *args)[1], "edge case on a state")


def test_occlusion_on_the_device():
    V, F, image, depth, alpha, views, tans = mc.occlusion_case()
    N = _device_normals(V, F)
    _same(N, mr.vertex_normals_ref(V, F), "two quads")
    got = _device_integrate(np.zeros((8, 3), f32), np.zeros(8, f32), image, depth, alpha, views, tans, V, N, 0.5, mc.DEPTH_TOL)
    assert (got[1][:4] > 0).all() and (got[1][4:] == 0).all() and (got[0][4:] == 0).all()


# ---- spread ----
@functools.lru_cache(maxsize=None)
def _torus_seen():
    """the torus after six views of 32 x 32: (F, seen uint8, colours) - the underside unseen"""
    V, F, N, image, depth, alpha, views, tans = mc.orbit_case(6, 32, 32)
    cs, ws = mr.integrate_ref(np.zeros((len(V), 3), f32), np.zeros(len(V), f32), image, depth, alpha, views, tans, V, N, 0.5, mc.torus_tol())
    col, seen = mr.resolve_ref(cs, ws, fallback=(np.nan, np.nan, np.nan))          # what the unseen rows hold must not matter
    return F, seen.astype(np.uint8), col


@pytest.mark.parametrize("iterations", [0, 1, 2, 64])
def test_spread_bit_for_bit(iterations):
    F, seen, col = _torus_seen()
    ref = mr.spread_ref(F, seen, col, iterations, FALLBACK)
    got = _device_spread(F, len(seen), seen, col, iterations)
    _same_spread(got, ref, "torus, %d iterations" % iterations)
    dist = mr.edge_distance(F, len(seen), np.nonzero(seen)[0])
    assert np.array_equal(got[1] != 0, dist <= iterations) and dist.max() == 2    # the unseen band is five rings wide
    assert _device_spread(F, len(seen), seen, col, iterations)[0].tobytes() == got[0].tobytes()       # twice the same bits
    if iterations == 64:
        assert ref[2].tolist() == [int((seen == 0).sum()), 0]
    for Vm in SIZES:
        Vs, Fs = mc.mesh_of(Vm)
        for share in (0.0, 0.1, 0.9):
            sn, cl = mc.spread_state(Vm, share, seed=Vm)
            _same_spread(_device_spread(Fs, Vm, sn, cl, iterations), mr.spread_ref(Fs, sn, cl, iterations, FALLBACK), "%d vertices, %g seen, %d iterations" % (Vm, share, iterations))


def test_spread_of_an_empty_mesh_and_of_a_mesh_without_faces():
    got = _device_spread(np.zeros((0, 3), np.int32), 0, np.zeros(0, np.uint8), np.zeros((0, 3), f32), 5)
    assert got[2].tolist() == [0, 0]
    sn, cl = mc.spread_state(300, 0.5, seed=2)
    F0 = np.zeros((0, 3), np.int32)
    _same_spread(_device_spread(F0, 300, sn, cl, 3), mr.spread_ref(F0, sn, cl, 3, FALLBACK), "300 vertices without faces")


# ---- guard bands ----
def test_all_three_stay_inside_guard_banded_buffers_and_write_all_they_return():
    """every output and the workspace AT ITS EXACT QUERIED SIZE between poisoned guard bands (tests/poison.py): the bands are intact
    afterwards, and the results do not depend on what the buffers held"""
    from gaussianmesh_amd import _lib
    lib = _lib.lib()
    V, F, N, image, depth, alpha, views, tans = mc.orbit_case(3, 7, 13)
    Fsn, seen, col = _torus_seen()
    for Vm, Vs, Fs in [(len(V), V, F)] + [(n,) + tuple(mc.mesh_of(n)) for n in (1, 255, 257)]:
        Vd, Fd = _dev(Vs), _dev(Fs, torch.int32)
        off, adj = _adj(Fs, Vm)
        P, Nr, cs0, ws0 = mc.random_vertices(Vm, 3, 7, 13, seed=Vm)
        Pd, Nd, c0, w0 = _dev(P), _dev(Nr), _dev(cs0), _dev(ws0)
        im, d, a, v, t = _dev(image), _dev(depth), _dev(alpha), _dev(views.reshape(3, 16)), _dev(tans)
        sn, cl = (seen, col) if Vm == len(V) else mc.spread_state(Vm, 0.2, seed=Vm)
        snd, cld = _dev(sn, torch.uint8), _dev(np.nan_to_num(cl))
        nbytes = lib.gm_mesh_color_spread_workspace_bytes(Vm)
        fb = (C.c_float * 3)(*FALLBACK)

        def route():
            out = torch.empty((Vm, 3), dtype=torch.float32, device="cuda")
            _lib.check(lib.gm_mesh_vertex_normals(Vm, len(Fs), Vd.data_ptr(), Fd.data_ptr(), off.data_ptr(), adj.data_ptr(), out.data_ptr(), _stream()))
            cs, ws = torch.empty_like(c0).copy_(c0), torch.empty_like(w0).copy_(w0)
            _lib.check(lib.gm_mesh_color_integrate(3, 7, 13, im.data_ptr(), d.data_ptr(), a.data_ptr(), v.data_ptr(), t.data_ptr(), Vm, Pd.data_ptr(),
                                                   Nd.data_ptr(), 0.5, 3.0, 1, cs.data_ptr(), ws.data_ptr(), _stream()))
            colors = torch.empty_like(cld).copy_(cld)
            has = torch.empty((Vm,), dtype=torch.uint8, device="cuda")
            counts = torch.empty((2,), dtype=torch.int32, device="cuda")
            work = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
            _lib.check(lib.gm_mesh_color_spread(Vm, len(Fs), Fd.data_ptr(), off.data_ptr(), adj.data_ptr(), snd.data_ptr(), 3, fb, colors.data_ptr(),
                                                has.data_ptr(), counts.data_ptr(), work.data_ptr(), nbytes, _stream()))
            return out, cs, ws, colors, has, counts

        runs = poison.run_under_fills(route)                           # a damaged band raises GuardViolation
        assert all(p.handed_out == 7 and p.unguarded == 0 for p, _ in runs)
        assert poison.differing(runs) == [], "%d vertices: a result depends on the buffers' old contents" % Vm
        out = [x.cpu().numpy() for x in runs[-1][1]]
        _same(out[0], mr.vertex_normals_ref(Vs, Fs), "guard-banded normals")
        ref = mr.integrate_ref(cs0, ws0, image, depth, alpha, views, tans, P, Nr, 0.5, 3.0, True)
        _same(out[1], ref[0], "guard-banded csum")
        _same(out[2], ref[1], "guard-banded wsum")
        _same_spread((out[3], out[4], out[5]), mr.spread_ref(Fs, sn, np.nan_to_num(cl), 3, FALLBACK), "guard-banded spread")


# ---- the Python surface ----
def test_vertex_colors_groups_views_by_resolution_refuses_cpu_and_resolves_as_the_reference():
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd import mesh_color as mcol
    from gaussianmesh_amd._lib import GmeshError
    from gaussianmesh_amd.renderer import Camera
    a, b = mc.orbit_case(3, 7, 13), mc.orbit_case(1, 32, 32)
    V, F, N = a[0], a[1], a[2]
    cam = lambda k, K, W, H: scenes.orbit_camera(k, K, W, H, radius=6.5, height=4.5, fovx_deg=50.0)
    cams = [Camera(cam(0, 3, 13, 7), "cuda"), cam(1, 3, 13, 7), cam(0, 1, 32, 32), Camera(cam(2, 3, 13, 7), "cuda")]     # objects and dicts, three runs
    images = [_dev(a[3][0]), _dev(a[3][1]), _dev(b[3][0]), _dev(a[3][2])]
    depth = [_dev(a[4][0]), _dev(a[4][1])[None], _dev(b[4][0]), _dev(a[4][2])]
    alpha = [_dev(a[5][0]), _dev(a[5][1])[None], _dev(b[5][0]), _dev(a[5][2])]
    vc = mcol.VertexColors(_dev(V), _dev(F, torch.int32))
    _same(vc.normals.cpu().numpy(), N, "VertexColors.normals")
    _same(mcol.vertex_normals(_dev(V), _dev(F, torch.int32)).cpu().numpy(), N, "vertex_normals")
    lo, hi = V.min(0).astype(np.float64), V.max(0).astype(np.float64)
    assert vc.default_depth_tol == float(f32(0.01 * np.linalg.norm(hi - lo))) and vc.stats is None
    assert vc.integrate(cams, images, depth, alpha, depth_tol=mc.torus_tol()) is vc and vc.views == 4
    zero3, zero = np.zeros((len(V), 3), f32), np.zeros(len(V), f32)
    ref = mr.integrate_ref(zero3, zero, a[3][:2], a[4][:2], a[5][:2], a[6][:2], a[7][:2], V, N, 0.5, mc.torus_tol())
    ref = mr.integrate_ref(*ref, b[3], b[4], b[5], b[6], b[7], V, N, 0.5, mc.torus_tol())
    ref = mr.integrate_ref(*ref, a[3][2:], a[4][2:], a[5][2:], a[6][2:], a[7][2:], V, N, 0.5, mc.torus_tol())
    _same(vc.wsum.cpu().numpy(), ref[1], "VertexColors.integrate: wsum")
    _same(vc.csum.cpu().numpy(), ref[0], "VertexColors.integrate: csum")
    # a stacked [K,3,H,W] tensor is the same as a list
    vc2 = mcol.VertexColors(_dev(V), _dev(F, torch.int32)).integrate(cams[:2], _dev(a[3][:2]), _dev(a[4][:2]), _dev(a[5][:2]), depth_tol=mc.torus_tol())
    r2 = mr.integrate_ref(zero3, zero, a[3][:2], a[4][:2], a[5][:2], a[6][:2], a[7][:2], V, N, 0.5, mc.torus_tol())
    _same(vc2.csum.cpu().numpy(), r2[0], "stacked maps")
    # resolve: plain, with a threshold, and spread
    col, seen = mr.resolve_ref(ref[0], ref[1], 0.0, FALLBACK)
    got = vc.resolve(fallback=FALLBACK)
    assert got.is_cuda and got.dtype == torch.float32
    _same(got.cpu().numpy(), col, "resolve")
    assert vc.stats == dict(seen=int(seen.sum()), filled=0, unreached=int((~seen).sum())) and 0 < seen.sum() < len(V)
    col_w, seen_w = mr.resolve_ref(ref[0], ref[1], 0.5, FALLBACK)
    _same(vc.resolve(min_weight=0.5, fallback=FALLBACK).cpu().numpy(), col_w, "resolve(min_weight)")
    assert vc.stats["seen"] == int(seen_w.sum()) < int(seen.sum())
    for spread, n in ((2, 2), (True, len(V)), (0, 0)):
        sp = mr.spread_ref(F, seen, col, n, FALLBACK)
        _same(vc.resolve(spread=spread, fallback=FALLBACK).cpu().numpy(), sp[0], "resolve(spread=%r)" % (spread,))
        assert vc.stats == dict(seen=int(seen.sum()), filled=int(sp[2][0]), unreached=int(sp[2][1]))
    assert vc.stats["unreached"] == len(V) - int(seen.sum()) and mcol.SPREAD_MAX >= len(V)
    _same(vc.csum.cpu().numpy(), ref[0], "resolve left the sums alone")
    with pytest.raises(GmeshError):
        vc.integrate(cams[:1], [torch.zeros(3, 7, 13)], [_dev(a[4][0])], [_dev(a[5][0])])
    with pytest.raises(GmeshError):
        vc.integrate(cams[:1], [_dev(a[3][0])], [torch.zeros(7, 13)], [torch.zeros(7, 13)])
    with pytest.raises(GmeshError):
        mcol.VertexColors(torch.as_tensor(np.array(V)), torch.as_tensor(np.array(F)))
    with pytest.raises(ValueError):
        vc.integrate(cams[:1], [_dev(b[3][0])], [_dev(b[4][0])], [_dev(b[5][0])])         # a 13 x 7 camera with 32 x 32 maps
    with pytest.raises(ValueError):
        vc.resolve(spread=-1)


# ---- end to end: a torus cloud, red where x > 0 and blue where x < 0 ----
E2E = dict(P=40000, nu=48, nv=32, K=12, W=128, H=128, resolution=48)          # test_gpu_tsdf.py's recipe
SH_C0 = 0.28209479177387814


@functools.lru_cache(maxsize=None)
def _e2e():
    from gaussianmesh_amd import proxy_mesh as pm
    from gaussianmesh_amd import mesh_color as mcol
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.bg_model import PlainGaussians, inverse_sigmoid
    verts, faces = scenes.torus_mesh(E2E["nu"], E2E["nv"])
    cl = scenes.bind_cloud_to_mesh(E2E["P"], verts, faces, seed=5)
    shs = np.zeros_like(cl["shs"])
    red = cl["means"][:, 0] > 0
    rgb = np.where(red[:, None], np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0]))
    shs[:, 0] = (rgb - 0.5) / SH_C0                                     # the DC band alone: the colour does not depend on the view
    model = PlainGaussians(3, device="cuda")
    model._set_params(_dev(cl["means"]), _dev(shs), torch.log(_dev(cl["scales"])), _dev(cl["rots"]), inverse_sigmoid(_dev(cl["opac"])))
    model.active_sh_degree = 3
    cams = [scenes.orbit_camera(k, E2E["K"], E2E["W"], E2E["H"], radius=6.5, height=(4.5, -4.5)[k % 2]) for k in range(E2E["K"])]
    lo, hi, voxel = pm.default_bounds(model, E2E["resolution"])
    plain = pm.from_cloud(model, cams, resolution=E2E["resolution"])
    coloured = pm.from_cloud(model, cams, resolution=E2E["resolution"], vertex_colors=True)
    trunc = float(f32(3.0 * voxel))
    colors, vc = mcol._color_from_cloud(model, cams, plain[0], plain[1], None, None, 8, 0.5, trunc, False, True, None)
    return dict(model=model, cams=cams, bounds=(lo, hi), trunc=trunc, plain=plain, coloured=coloured, colors=colors, stats=vc.stats)


def test_end_to_end_the_mesh_is_unchanged_and_red_where_the_cloud_is_red():
    from gaussianmesh_amd import mesh_color as mcol
    r = _e2e()
    (V0, F0), (V, F, colors) = r["plain"], r["coloured"]
    assert len(r["coloured"]) == 3 and torch.equal(V, V0) and torch.equal(F, F0) and V.dtype == torch.float32
    assert colors.is_cuda and colors.dtype == torch.float32 and colors.shape == V.shape
    assert poison.same_bits(colors, r["colors"])                       # from_cloud's colours are color_from_cloud's on that mesh
    assert poison.same_bits(colors, mcol.color_from_cloud(r["model"], r["cams"], V, F, depth_tol=r["trunc"]))
    v, c = V.cpu().numpy(), colors.cpu().numpy()
    east, west = v[:, 0] > 0.5, v[:, 0] < -0.5
    print("coloured proxy mesh: %d vertices, %s; x > 0.5: mean rgb %s, x < -0.5: mean rgb %s" % (len(v), r["stats"], c[east].mean(0), c[west].mean(0)))
    assert east.sum() > 500 and west.sum() > 500 and np.isfinite(c).all()
    assert c[east][:, 0].mean() > c[east][:, 2].mean() and c[west][:, 2].mean() > c[west][:, 0].mean()
    assert r["stats"]["unreached"] == 0 and r["stats"]["seen"] + r["stats"]["filled"] == len(v) and r["stats"]["seen"] > 0


def _write_scene(r, tmp_path):
    from gaussianmesh_amd import io as gio
    ply, cj = str(tmp_path / "cloud.ply"), str(tmp_path / "cameras.json")
    r["model"].save_ply(ply)
    entries = []
    for k, c in enumerate(r["cams"]):
        Rt = c["view"].T.astype(np.float64)
        entries.append(gio.camera_to_json(k, Rt[:3, :3].T, Rt[:3, 3], c["W"], c["H"], c["fovx"], c["fovy"], "v%d" % k))
    with open(cj, "w") as fh:
        json.dump(entries, fh)
    return ply, cj


def test_both_clis(tmp_path, capsys):
    from gaussianmesh_amd import io as gio
    from gaussianmesh_amd import mesh_color as mcol
    from gaussianmesh_amd import proxy_mesh as pm
    r = _e2e()
    ply, cj = _write_scene(r, tmp_path)
    obj, obj2, obj3 = str(tmp_path / "proxy.obj"), str(tmp_path / "plain.obj"), str(tmp_path / "recoloured.obj")
    lo, hi = r["bounds"]
    args = ["--gaussian", ply, "--cameras", cj, "--resolution", "48", "--bounds"] + [repr(float(x)) for x in (*lo, *hi)]
    assert pm.main(args + ["--out", obj2]) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(plain) == {"vertices", "faces", "components_dropped", "boundary_edges", "grid", "views", "seconds"}
    assert set(plain["seconds"]) == {"load", "render_fuse", "extract", "write"} and gio.read_obj_colors(obj2) is None
    assert pm.main(args + ["--out", obj, "--vertex_colors"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(line) == set(plain) | {"colored_vertices", "spread_vertices", "uncolored_vertices"}
    assert set(line["seconds"]) == set(plain["seconds"]) | {"color"} and line["seconds"]["color"] > 0
    # the same arrays as the module call on the cameras the CLI read back (a cameras.json round trip moves the last bits of a view)
    cams = gio.load_cameras_json(cj)
    V, F, colors = pm.from_cloud(r["model"], cams, resolution=48, bounds=(lo, hi), vertex_colors=True)
    v, f = gio.read_obj(obj)
    c = gio.read_obj_colors(obj)
    assert np.array_equal(v, V.cpu().numpy().astype(np.float64)) and np.array_equal(f, F.cpu().numpy())
    assert c.dtype == f32 and np.array_equal(_bits(c), _bits(colors.cpu().numpy()))
    assert all(len(l.split()) == 7 for l in open(obj) if l.startswith("v "))
    assert open(obj2).read().splitlines() == [" ".join(l.split()[:4]) for l in open(obj).read().splitlines()]     # the geometry records are the plain run's
    assert line["colored_vertices"] + line["spread_vertices"] + line["uncolored_vertices"] == line["vertices"] == len(v) and line["uncolored_vertices"] == 0
    # --color_spread 0: what no view coloured keeps the fallback grey
    assert pm.main(args + ["--out", obj, "--vertex_colors", "--color_spread", "0"]) == 0
    zero = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert zero["spread_vertices"] == 0 and zero["uncolored_vertices"] == line["spread_vertices"] and zero["colored_vertices"] == line["colored_vertices"]
    assert (gio.read_obj_colors(obj) == 0.5).all(axis=1).sum() >= zero["uncolored_vertices"]
    # the colouring CLI on the written mesh reproduces the colours
    gio.write_obj(obj, v, f, c)
    voxel = float((np.asarray(hi, np.float64) - np.asarray(lo, np.float64)).max()) / 48                   # fuse_cloud's, from the bounds
    vol_trunc = pm.TsdfVolume(lo, hi, voxel_size=voxel, trunc=3.0 * voxel).trunc
    assert mcol.main(["--gaussian", ply, "--cameras", cj, "--mesh", obj, "--out", obj3, "--depth_tol", repr(vol_trunc)]) == 0
    again = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(again) == {"vertices", "seen", "filled", "unreached", "seconds"} and again["vertices"] == len(v)
    assert [again[k] for k in ("seen", "filled", "unreached")] == [line[k] for k in ("colored_vertices", "spread_vertices", "uncolored_vertices")]
    assert np.array_equal(_bits(gio.read_obj_colors(obj3)), _bits(c)) and np.array_equal(gio.read_obj(obj3)[0], v)


# ---- the preview ----
def test_render_preview_shows_the_interpolated_colour_of_the_pick_and_the_background_on_a_miss():
    from gaussianmesh_amd import mesh_color as mcol
    from gaussianmesh_amd import mesh_pick, scenes
    from gaussianmesh_amd.renderer import Camera
    V, F = mc.torus()
    rng = np.random.default_rng(4)
    colors = rng.uniform(0, 1, size=V.shape).astype(f32)
    cam_d = scenes.orbit_camera(1, 5, 40, 24, radius=6.5, height=4.5, fovx_deg=50.0)
    cam = Camera(cam_d, "cuda")
    Vd, Fd, cd = _dev(V), _dev(F, torch.int32), _dev(colors)
    bg = (0.25, 0.5, 0.75)
    img = mcol.render_preview(cam, Vd, Fd, cd, bg_color=bg)
    assert img.shape == (3, 24, 40) and img.is_cuda and img.dtype == torch.float32
    assert poison.same_bits(img, mcol.render_preview(cam_d, Vd, Fd, cd, bg_color=bg))      # a camera dict is the same camera
    y, x = np.meshgrid(np.arange(24), np.arange(40), indexing="ij")
    pix = _dev(np.stack([x.reshape(-1), y.reshape(-1)], 1))
    p = mesh_pick.pick(cam, pix, Vd, Fd)
    o, d = mesh_pick.camera_rays(cam, pix)
    t, face, uv = mesh_pick.ray_mesh_hits(o, d, Vd, Fd)
    assert torch.equal(face, p["face"])
    face, uv, got = face.cpu().numpy(), uv.cpu().numpy().astype(np.float64), img.cpu().numpy().reshape(3, -1).T
    hit = face >= 0
    assert 100 < hit.sum() < hit.size - 100
    tri = F[face[hit]]
    u, v = uv[hit, 0:1], uv[hit, 1:2]
    want = (1 - u - v) * colors[tri[:, 0]] + u * colors[tri[:, 1]] + v * colors[tri[:, 2]]
    # against float64: 1 - u - v rounds twice (2 x 6e-8, times a colour below 1), three products and two sums of numbers below 1 round
    # once each (5 x 6e-8): 4.2e-7 at the most
    assert np.abs(got[hit] - want).max() < 4.2e-7
    assert (got[~hit] == np.array(bg, f32)).all()
    assert (mcol.render_preview(cam, Vd, Fd, cd).cpu().numpy().reshape(3, -1).T[~hit] == 0).all()         # black unless given
