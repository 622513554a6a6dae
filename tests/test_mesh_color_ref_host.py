"""Mesh colour on the host: the four entry points of csrc/gm_mesh_color.hip are exported, in sync with the header, and refuse bad
arguments before any GPU work; the numpy definition (tests/mesh_color_ref.py) gives the normals, the per-view decisions - every edge hit
exactly, both sides checked -, the occlusion and the spread their meaning; coloured OBJ files round-trip; the Python surface has no CPU
path."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mesh_color_cases as mc
import mesh_color_ref as mr

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _ulps(a, b):
    """distance in float32 steps between finite values of one sign"""
    return np.abs(_bits(a).astype(np.int64) - _bits(b).astype(np.int64))


# ---- 1. the ABI ----
ENTRY_POINTS = (("gm_mesh_vertex_normals", "int", 8), ("gm_mesh_color_integrate", "int", 17), ("gm_mesh_color_spread_workspace_bytes", "size_t", 1),
                ("gm_mesh_color_spread", "int", 14))


def test_entry_points_are_declared_typed_and_in_sync():
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    names = _lib.header_symbols()
    txt = open(_lib.HEADER).read()
    for name, ret, n in ENTRY_POINTS:
        assert name in names and name in _lib.SIGNATURES and hasattr(l, name), name
        m = re.search(r"\b%s\s+%s\(([^)]*)\);" % (ret, name), txt)
        assert m and len(m.group(1).split(",")) == n == len(_lib.SIGNATURES[name][1]), name
    assert set(names) == set(_lib.SIGNATURES)
    assert l.gm_abi_version() == 3 and "#define GM_ABI_VERSION 3" in txt
    assert "gm_mesh_color.hip" in open(os.path.join(_lib.CSRC, "Makefile")).read()


def test_unit_neither_waits_nor_allocates_nor_uses_atomics():
    from gaussianmesh_amd import _lib
    src = open(os.path.join(_lib.CSRC, "gm_mesh_color.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("hipMalloc", "hipFree", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy", "atomic", "__threadfence"):
        assert word not in code, word
    assert "#pragma clang fp contract(off)" in code
    assert "tests/mesh_color_ref.py" in src and "REACH" in src


def test_workspace_query_is_monotonic_and_positive():
    from gaussianmesh_amd import _lib
    q = _lib.lib().gm_mesh_color_spread_workspace_bytes
    assert q(0) > 0 and q(-5) == q(0)
    sizes = [0, 1, 2, 255, 256, 257, 1000, 65536, 65537, 1 << 20]
    for a, b in zip(sizes, sizes[1:]):
        assert q(a) <= q(b)
    assert 13 * (1 << 20) < q(1 << 20) < 13.1 * (1 << 20)             # a second colour array, a state byte, eight bytes a workgroup


M = 1 << 24                                                           # bogus non-null "pointers", 16 MiB apart


def test_normals_refuse_before_any_gpu_work():
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    def call(Vm=100, F=200, V=1 * M, faces=2 * M, off=3 * M, adj=4 * M, out=5 * M):
        return l.gm_mesh_vertex_normals(Vm, F, V, faces, off, adj, out, None)
    err = lambda: l.gm_last_error()
    assert call(Vm=-1) == 1 and b"negative" in err()
    assert call(F=-1) == 1 and b"negative" in err()
    assert call(F=(1 << 31) // 3 + 1) == 1 and b"fit an int" in err()
    assert call(Vm=0, V=None, out=None) == 0                          # nothing to do
    for k in ("V", "faces", "off", "adj", "out"):
        assert call(**{k: None}) == 1 and b"null pointer" in err(), k
    assert call(out=1 * M) == 1 and b"vertices overlaps out_normals" in err()
    assert call(out=1 * M + 12 * 99) == 1 and b"vertices overlaps out_normals" in err()    # the last vertex
    assert call(out=2 * M - 12 * 99) == 1 and b"faces overlaps out_normals" in err()
    assert call(out=3 * M + 4 * 100) == 1 and b"adj_offsets overlaps out_normals" in err()  # the entry Vm of the offsets
    assert call(out=4 * M) == 1 and b"adj_faces overlaps out_normals" in err()


def test_integrate_refuses_before_any_gpu_work():
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    def call(K=2, H=8, W=8, image=1 * M, depth=2 * M, alpha=3 * M, views=4 * M, tans=5 * M, Vm=100, V=6 * M, N=7 * M, alpha_min=0.5, tol=0.25, two=0,
             csum=8 * M, wsum=9 * M):
        return l.gm_mesh_color_integrate(K, H, W, image, depth, alpha, views, tans, Vm, V, N, alpha_min, tol, two, csum, wsum, None)
    err = lambda: l.gm_last_error()
    for kw in (dict(K=-1), dict(H=0), dict(W=0), dict(H=-3), dict(W=(1 << 24) + 1)):
        assert call(**kw) == 1 and b"invalid sizes" in err(), kw
    assert call(Vm=-1) == 1 and b"negative" in err()
    assert call(alpha_min=float("nan")) == 1 and b"NaN" in err()
    assert call(tol=float("nan")) == 1 and b"NaN" in err()
    assert call(tol=-0.125) == 1 and b"depth_tol" in err()
    for k in ("image", "depth", "alpha", "views", "tans", "V", "N", "csum", "wsum"):
        assert call(**{k: None}) == 1 and b"null pointer" in err(), k
    # K == 0 and Vm == 0 are valid, and then the pointers they would index are not looked at
    assert call(K=0, image=None, depth=None, alpha=None, views=None, tans=None) == 0
    assert call(Vm=0, V=None, N=None, csum=None, wsum=None) == 0
    assert call(K=0, tol=0.0, alpha_min=float("-inf")) == 0           # depth_tol == 0 and any alpha_min that is a number are valid
    inputs = (("image", 1 * M), ("depth", 2 * M), ("alpha", 3 * M), ("views", 4 * M), ("tanfov", 5 * M), ("vertices", 6 * M), ("normals", 7 * M))
    for what, at in inputs:
        assert call(csum=at) == 1 and what.encode() + b" overlaps csum" in err(), what
        assert call(wsum=at) == 1 and what.encode() + b" overlaps wsum" in err(), what
    assert call(wsum=8 * M) == 1 and b"csum overlaps wsum" in err()
    assert call(wsum=8 * M + 12 * 100 - 1) == 1 and b"csum overlaps wsum" in err()
    assert call(wsum=1 * M + 4 * 2 * 3 * 64 - 4) == 1 and b"image overlaps wsum" in err()  # the last float of the images
    assert call(wsum=4 * M + 64) == 1 and b"views overlaps wsum" in err()                  # the second view's rows


def test_spread_refuses_before_any_gpu_work():
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    need = l.gm_mesh_color_spread_workspace_bytes(100)
    fb = (C.c_float * 3)(0.5, 0.5, 0.5)
    def call(Vm=100, F=200, faces=1 * M, off=2 * M, adj=3 * M, seen=4 * M, iterations=3, fallback=fb, colors=5 * M, has=6 * M, counts=7 * M, ws=8 * M,
             ws_bytes=need):
        return l.gm_mesh_color_spread(Vm, F, faces, off, adj, seen, iterations, fallback, colors, has, counts, ws, ws_bytes, None)
    err = lambda: l.gm_last_error()
    assert call(Vm=-1) == 1 and b"negative" in err()
    assert call(F=-1) == 1 and b"negative" in err()
    assert call(iterations=-1) == 1 and b"iterations" in err()
    for k in ("faces", "off", "adj", "seen", "fallback", "colors", "has", "counts", "ws"):
        assert call(**{k: None}) == 1 and b"null pointer" in err(), k
    for k, what in (("faces", b"faces"), ("off", b"adj_offsets"), ("adj", b"adj_faces"), ("seen", b"seen")):
        at = dict(faces=1 * M, off=2 * M, adj=3 * M, seen=4 * M)[k]
        assert call(colors=at) == 1 and what + b" overlaps colors" in err(), k
        assert call(has=at) == 1 and what + b" overlaps out_has" in err(), k
        assert call(counts=at) == 1 and what + b" overlaps out_counts" in err(), k
        assert call(ws=at - need + 1) == 1 and what + b" overlaps workspace" in err(), k
    assert call(has=5 * M + 12 * 100 - 1) == 1 and b"colors overlaps out_has" in err()
    assert call(counts=6 * M + 99) == 1 and b"out_has overlaps out_counts" in err()
    assert call(ws=7 * M + 7) == 1 and b"out_counts overlaps workspace" in err()
    assert call(ws=5 * M - need + 1) == 1 and b"colors overlaps workspace" in err()
    # an undersized workspace: GM_ERR_BUFFER, still before any GPU work
    assert call(ws_bytes=need - 1) == 3 and b"workspace too small" in err()
    assert call(ws_bytes=0) == 3
    assert call(iterations=0, ws_bytes=need - 1) == 3                                       # iterations == 0 got past the scalars


# ---- 2. the reference: normals ----
def test_normals_of_a_closed_octahedron_are_exact_and_an_isolated_vertex_gets_zero():
    V, F = mr.octahedron()
    V = np.concatenate([V, [[7, 7, 7]]]).astype(f32)                   # a vertex no face names
    N = mr.vertex_normals_ref(V, F)
    assert np.array_equal(_bits(N[:6]), _bits(4 * V[:6]))              # four faces of cross product (1, 1, 1)-like each: outward, exact
    assert np.array_equal(_bits(N[6]), _bits(np.zeros(3, f32))) and not np.signbit(N[6]).any()
    off, adj = mr.adjacency(F, 7)
    assert off.tolist() == [0, 4, 8, 12, 16, 20, 24, 24] and adj[:4].tolist() == [0, 3, 4, 7]
    from gaussianmesh_amd.deform import vertex_face_adjacency
    o2, a2 = vertex_face_adjacency(F, 7)
    assert np.array_equal(off, o2) and np.array_equal(adj, a2)
    # a scaled, shifted copy: area-weighted means quadratic in the scale, and the shift leaves nothing
    N2 = mr.vertex_normals_ref(V * f32(0.5) + f32(2.0), F)
    assert np.array_equal(_bits(N2[:6]), _bits(V[:6]))
    Vt, Ft = mc.torus()
    import tsdf_ref as tr
    assert tr.signed_volume(Vt, Ft) > 0 and tr.is_closed(Ft)
    Nt = mr.vertex_normals_ref(Vt, Ft)
    centre = np.stack([2 * Vt[:, 0] / np.hypot(Vt[:, 0], Vt[:, 2]), np.zeros(len(Vt)), 2 * Vt[:, 2] / np.hypot(Vt[:, 0], Vt[:, 2])], 1)
    assert (((Vt - centre) * Nt).sum(1) > 0).all()                    # outward everywhere


# ---- 3. the reference: one view, every decision on its edge ----
@pytest.mark.parametrize("two_sided", [False, True], ids=["one-sided", "two-sided"])
@pytest.mark.parametrize("alpha_min", [0.5, 0.0])
def test_every_decision_edge_exactly_and_on_both_sides(alpha_min, two_sided):
    c = mc.edge_case()
    n = len(c["names"])
    zero3, zero = np.zeros((n, 3), f32), np.zeros(n, f32)
    cs, ws = mr.integrate_ref(zero3, zero, c["image"], c["depth"], c["alpha"], c["views"], c["tans"], c["P"], c["N"], alpha_min, mc.DEPTH_TOL, two_sided)
    want = c["expect"](alpha_min, two_sided)
    got = ws > 0
    assert [c["names"][i] for i in np.nonzero(got != want)[0]] == []
    assert np.array_equal(_bits(ws[~want]), _bits(zero[~want])) and np.array_equal(_bits(cs[~want]), _bits(zero3[~want]))    # a skipped view adds nothing at all
    # a taken view read the pixel the case names: the colours are that pixel's, the weight cos^2
    col, seen = mr.resolve_ref(cs, ws)
    assert np.array_equal(seen, want)
    for i in np.nonzero(want)[0]:
        px, py = c["pixel"][i]
        assert (_ulps(col[i], c["image"][0, :, py, px]) <= 2).all(), c["names"][i]
        assert 0 < ws[i] <= 1, c["names"][i]
    names = c["names"]
    assert ws[names.index("d == -2^-20")] < 1e-11 and ws[names.index("plain")] == f32(1.0) / (f32(0.625) ** 2 * 2 + 1)      # cos^2 = z^2 / |P|^2
    assert want.sum() == {(0.5, False): 11, (0.5, True): 12, (0.0, False): 12, (0.0, True): 13}[(alpha_min, two_sided)]
    # the exact quantities the cases promise (float64 restatement)
    P = c["P"].astype(np.float64)
    with np.errstate(all="ignore"):
        px = 4 * P[:, 0] / P[:, 2] + 3.5
    assert px[names.index("left border: px + 0.5 == 0")] == -0.5 and px[names.index("right border: px + 0.5 == W")] == 7.5
    assert px[names.index("px + 0.5 an exact integer")] == 3.5 and -0.5 - 1e-6 < px[names.index("left of it by an ulp")] < -0.5


def test_views_accumulate_as_state():
    """K views in one call are K calls of one view, and a taken view twice doubles the sums exactly"""
    V, F, N, image, depth, alpha, views, tans = mc.orbit_case(3, 13, 7)
    zero3, zero = np.zeros((len(V), 3), f32), np.zeros(len(V), f32)
    whole = mr.integrate_ref(zero3, zero, image, depth, alpha, views, tans, V, N, 0.5, mc.torus_tol())
    each = (zero3, zero)
    for k in range(3):
        each = mr.integrate_ref(*each, image[k:k + 1], depth[k:k + 1], alpha[k:k + 1], views[k:k + 1], tans[k:k + 1], V, N, 0.5, mc.torus_tol())
    assert np.array_equal(_bits(whole[0]), _bits(each[0])) and np.array_equal(_bits(whole[1]), _bits(each[1]))
    assert (whole[1] > 0).any() and (whole[1] == 0).any()


# ---- 4. occlusion, constant colour ----
def test_the_back_quad_stays_unseen_behind_the_front_one():
    V, F, image, depth, alpha, views, tans = mc.occlusion_case()
    N = mr.vertex_normals_ref(V, F)
    assert (N[:, 2] < 0).all() and (N[:, :2] == 0).all()               # both wound towards the camera
    cs, ws = mr.integrate_ref(np.zeros((8, 3), f32), np.zeros(8, f32), image, depth, alpha, views, tans, V, N, 0.5, mc.DEPTH_TOL)
    assert (ws[:4] > 0).all() and (ws[4:] == 0).all() and (cs[4:] == 0).all()
    col, seen = mr.resolve_ref(cs, ws, fallback=(0.0, 1.0, 0.0))
    assert seen.tolist() == [True] * 4 + [False] * 4 and (col[4:] == (0.0, 1.0, 0.0)).all() and (_ulps(col[:4], f32(0.75)) <= 2).all()
    # with the back quad's own depth in the map, it is the front one that is off the rendered surface
    cs, ws = mr.integrate_ref(np.zeros((8, 3), f32), np.zeros(8, f32), image, depth * 2, alpha, views, tans, V, N, 0.5, mc.DEPTH_TOL)
    assert (ws[:4] == 0).all() and (ws[4:] > 0).all()


def test_a_constant_image_gives_every_seen_vertex_that_colour():
    """The colour of a vertex k views took is fl(sum of fl(w_j c)) / fl(sum of w_j): k products and k - 1 additions above (relative error
    at most k u to first order, u = 2^-24, all terms positive), k - 1 additions below, one division - 2 k u in all, and u is at most one
    step of a float32: within 2 steps per view.  One view - the issue's figure - is within 2."""
    V, F, N, image, depth, alpha, views, tans = mc.orbit_case(6, 32, 32)
    const = np.broadcast_to(np.array([0.3, 0.6, 0.9], f32)[None, :, None, None], image.shape)
    want = np.array([0.3, 0.6, 0.9], f32)
    zero3, zero = np.zeros((len(V), 3), f32), np.zeros(len(V), f32)
    total = 0
    for k in range(6):
        cs, ws = mr.integrate_ref(zero3, zero, const[k:k + 1], depth[k:k + 1], alpha[k:k + 1], views[k:k + 1], tans[k:k + 1], V, N, 0.5, mc.torus_tol())
        col, seen = mr.resolve_ref(cs, ws)
        total += int(seen.sum())
        assert seen.sum() > 20 and (_ulps(col[seen], np.broadcast_to(want, col[seen].shape)) <= 2).all(), k
    cs, ws = mr.integrate_ref(zero3, zero, const, depth, alpha, views, tans, V, N, 0.5, mc.torus_tol())
    col, seen = mr.resolve_ref(cs, ws)
    print("torus, 6 views of 32 x 32: %d of %d vertices seen, %.1f views each" % (seen.sum(), len(V), total / max(seen.sum(), 1)))
    assert 100 < seen.sum() < len(V) - 50                              # the orbit is above: the underside stays unseen
    assert not seen[V[:, 1] < -0.69].any()
    assert (_ulps(col[seen], np.broadcast_to(want, col[seen].shape)) <= 2 * 6).all()
    assert (col[~seen] == 0.5).all()


# ---- 5. spread ----
def test_spread_reaches_exactly_n_edges_and_leaves_the_seen_alone():
    V, F = mr.strip(9)                                                 # 20 vertices; the two ends are seen
    lone_V, lone_F = mr.strip(2)                                       # and a component nobody saw
    Fa = np.concatenate([F, lone_F + 20]).astype(np.int32)
    Vm = 20 + 6 + 1                                                    # and a vertex without faces
    seen = np.zeros(Vm, np.uint8)
    seen[[0, 1, 18, 19]] = (1, 7, 255, 1)
    rng = np.random.default_rng(0)
    colors = rng.uniform(0, 1, size=(Vm, 3)).astype(f32)
    dist = mr.edge_distance(Fa, Vm, np.nonzero(seen)[0])
    assert dist.max() == 4 and (dist[20:] == -1).all()
    fb = (0.125, 0.25, 0.375)
    for n in (0, 1, 2, 3, 4, 5, 40):
        col, has, counts = mr.spread_ref(Fa, seen, colors, n, fb)
        reach = (dist >= 0) & (dist <= n)
        assert np.array_equal(has != 0, reach), n
        assert counts.tolist() == [int(reach.sum()) - 4, int((~reach).sum())], n
        assert np.array_equal(_bits(col[seen != 0]), _bits(colors[seen != 0])), n           # seen values never move
        assert (col[~reach] == np.array(fb, f32)).all(), n
        assert ((col[reach] >= colors[seen != 0].min(0)) & (col[reach] <= colors[seen != 0].max(0))).all(), n    # means of means of the seen
    assert counts.tolist() == [16, 7]
    # the unseen rows of the input do not matter
    other = colors.copy()
    other[seen == 0] = np.nan
    again = mr.spread_ref(Fa, seen, other, 40, fb)
    assert np.array_equal(_bits(again[0]), _bits(col))
    # one step next to one seen neighbour through two faces: the neighbour counts twice, the mean is still its colour
    V2, F2 = mr.strip(1)
    s2 = np.array([1, 0, 0, 0], np.uint8)
    c2, h2, n2 = mr.spread_ref(F2, s2, colors[:4], 1, fb)
    assert h2.tolist() == [1, 1, 1, 1] and n2.tolist() == [3, 0] and np.array_equal(_bits(c2), _bits(np.broadcast_to(colors[0], (4, 3))))


# ---- 6. coloured OBJ files ----
def test_coloured_obj_round_trip(tmp_path):
    from gaussianmesh_amd import io as gio
    V, F = mc.torus(7, 5)
    rng = np.random.default_rng(3)
    colors = rng.uniform(0, 1, size=V.shape).astype(f32)
    colors[0] = (0.0, 1.0, np.nextafter(f32(1), f32(0)))
    colors[1] = (1e-30, 0.1, 1.0 / 3.0)
    plain, coloured, old = str(tmp_path / "plain.obj"), str(tmp_path / "coloured.obj"), str(tmp_path / "old.obj")
    gio.write_obj(plain, V, F)
    gio.write_obj(coloured, V, F, colors)
    with open(old, "w") as f:                                          # the records write_obj has always written
        for v in np.asarray(V, np.float64):
            f.write("v %.17g %.17g %.17g\n" % (v[0], v[1], v[2]))
        for t in np.asarray(F, np.int64):
            f.write("f %d %d %d\n" % (t[0] + 1, t[1] + 1, t[2] + 1))
    assert open(plain, "rb").read() == open(old, "rb").read()
    assert gio.read_obj_colors(plain) is None
    v, f = gio.read_obj(coloured)
    assert np.array_equal(v, V.astype(np.float64)) and np.array_equal(f, F) and np.array_equal(_bits(v.astype(f32)), _bits(V))
    back = gio.read_obj_colors(coloured)
    assert back.dtype == f32 and back.shape == V.shape and np.array_equal(_bits(back), _bits(colors))
    lines = open(coloured).read().splitlines()
    assert all(len(l.split()) == 7 for l in lines if l.startswith("v ")) and [l for l in lines if l.startswith("f ")] == [
        l for l in open(plain).read().splitlines() if l.startswith("f ")]
    with pytest.raises(ValueError):
        gio.write_obj(coloured, V, F, colors[:-1])


# ---- 7. the Python surface ----
def test_no_cpu_path():
    import torch
    from gaussianmesh_amd import mesh_color as mcol
    from gaussianmesh_amd import proxy_mesh as pm
    from gaussianmesh_amd._lib import GmeshError
    V, F = mr.octahedron()
    Vt, Ft = torch.as_tensor(V), torch.as_tensor(F)
    with pytest.raises(GmeshError):
        mcol.vertex_normals(Vt, Ft)
    with pytest.raises(GmeshError):
        mcol.VertexColors(Vt, Ft)
    with pytest.raises(GmeshError):
        mcol.VertexColors(V, F)                                        # host arrays neither
    with pytest.raises(GmeshError):
        mcol.render_preview(dict(W=4, H=4), Vt, Ft, torch.zeros(6, 3))
    import inspect
    assert inspect.signature(pm.from_cloud).parameters["vertex_colors"].default is False
    assert mcol.SPREAD_MAX == 1024
