"""Host side of growing a pick into a surface region: mesh_region.surface_graph against its edge-by-edge restatement and on hand-made
meshes, the float32 Dijkstra of tests/geodesic_ref.py - the definition the device is held to in test_gpu_geodesic.py - against a Jacobi
iteration, how round an unfolded "disc" is, region_handles, gm_mesh_geodesic's declaration and refusals (before any GPU work), and the
--pick_sequence reader's two new keys."""
import json
import math
import os
import re

import numpy as np
import pytest

import geodesic_ref as gr
from gaussianmesh_amd import _lib, scenes
from gaussianmesh_amd.mesh_region import SurfaceGraph, region_handles, surface_graph

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _entries(csr):
    off, cols, lens = csr
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return {(int(p), int(q)): l for p, q, l in zip(rows, cols, lens)}


# ---- surface_graph ----
@pytest.mark.parametrize("unfold", [False, True])
def test_surface_graph_shape_and_restatement(unfold):
    V, F = scenes.torus_mesh(40, 30)
    off, cols, lens = csr = surface_graph(V, F, unfold=unfold)
    assert off.dtype == np.int32 and cols.dtype == np.int32 and lens.dtype == f32
    assert off.shape == (1201,) and off[0] == 0 and off[-1] == len(cols) == len(lens)
    rows = np.repeat(np.arange(1200), np.diff(off))
    assert (rows != cols).all()                                                          # no diagonal
    assert ((np.diff(cols) > 0) | (np.diff(rows) > 0)).all()                             # columns ascend within a row
    e = _entries(csr)
    assert all(_bits(e[(q, p)]) == _bits(l) for (p, q), l in e.items())                  # symmetric, to the bit
    assert (np.diff(off) == (12 if unfold else 6)).all()                                 # a regular torus: 6 edges a vertex, 6 unfolded across them
    ref = gr.surface_graph_ref(V, F, unfold=unfold)
    assert all(np.array_equal(a, b) for a, b in zip(csr[:2], ref[:2])) and np.array_equal(_bits(lens), _bits(ref[2]))
    # a real edge's length is the float64 norm rounded once
    V64 = V.astype(f32).astype(np.float64)
    real = {(int(p), int(q)) for face in F for p, q in zip(face, np.roll(face, -1))}
    for (p, q) in list(real)[:500]:
        assert e[(p, q)] == f32(np.sqrt(((V64[p] - V64[q]) ** 2).sum())) or unfold      # (unfolded: a virtual edge may be shorter, below)
    if not unfold:
        assert set(e) == real | {(q, p) for p, q in real}


def _fold(angle, apex=(0.5, 1.0), other=(0.5, 1.0)):
    """two triangles on the edge (0, 1) = (0,0,0)-(1,0,0): c = vertex 2 in the plane z = 0 at apex, e = vertex 3 folded down by `angle`
    about the edge from the flat position (other[0], -other[1], 0)"""
    V = np.array([[0, 0, 0], [1, 0, 0], [apex[0], apex[1], 0], [other[0], -other[1] * math.cos(angle), other[1] * math.sin(angle)]], f32)
    return V, np.array([[0, 1, 2], [1, 0, 3]], np.int32)


@pytest.mark.parametrize("angle", [0.0, 0.4, math.pi / 2, 2.5, 3.0])
def test_unfolded_edge_does_not_depend_on_the_fold(angle):
    V, F = _fold(angle)
    e = _entries(surface_graph(V, F))
    assert len(e) == 12 and (2, 3) in e                                                  # five real edges and the virtual one, both ways
    assert abs(float(e[(2, 3)]) - 2.0) <= 2e-7 * 2                                        # the flat distance from c to e, whatever the angle
    assert (2, 3) not in _entries(surface_graph(V, F, unfold=False))
    assert np.array_equal(_bits(surface_graph(V, F)[2]), _bits(gr.surface_graph_ref(V, F)[2]))


def test_unfolding_refuses_what_is_no_straight_line():
    # non-convex unfolding: the line from c to e passes outside the shared edge (x* = 1.4 > L = 1, x* = -0.4 < 0): no virtual edge
    for apex, other in (((1.8, 1.0), (1.0, 1.0)), ((-0.8, 1.0), (0.0, 1.0))):
        V, F = _fold(0.3, apex, other)
        assert (2, 3) not in _entries(surface_graph(V, F)) and len(surface_graph(V, F)[1]) == 10
    # x* exactly at an end of the edge (the line passes through vertex a): the open interval refuses it
    V, F = _fold(0.0, (0.0, 1.0), (0.0, 1.0))
    assert (2, 3) not in _entries(surface_graph(V, F))
    # a boundary edge (one face) adds nothing; neither does an edge of three faces, but each pair across a two-face edge still does
    V = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0], [0.5, 0, 1]], f32)
    assert len(surface_graph(V, [[0, 1, 2]])[1]) == 6
    three = _entries(surface_graph(V, [[0, 1, 2], [1, 0, 3], [0, 1, 4]]))
    assert not {(2, 3), (2, 4), (3, 4)} & set(three) and len(three) == 14
    # a degenerate wing (e on the edge's line: ey = 0), a zero-length edge, the same face twice (c == e): nothing, and no warning
    V = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.25, 0, 0], [0, 0, 0]], f32)
    with np.errstate(all="raise"):
        assert (2, 3) not in _entries(surface_graph(V, [[0, 1, 2], [1, 0, 3]]))
        assert len(surface_graph(V, [[0, 4, 2], [4, 0, 1]])[1]) > 0
        assert len(surface_graph(V, [[0, 1, 2], [0, 1, 2]])[1]) == 6
        assert len(surface_graph(V, [[0, 0, 2]])[1]) == 2                                # p == q is no edge
    for g in (surface_graph(V, np.zeros((0, 3), np.int32)), surface_graph(np.zeros((0, 3), f32), np.zeros((0, 3), np.int32))):
        assert len(g[1]) == 0 and not g[0].any()


def test_duplicate_keeps_the_minimum():
    """two triangles folded by 2 rad about (0, 1), and a third face that makes the pair of their apexes (2, 3) a REAL edge: the chord
    through the air (0.54) beats the path unfolded over the edge (1.0); flat, both are the same number and the entry appears once"""
    for angle in (2.0, 0.0):
        V = np.array([[0, 0, 0], [1, 0, 0], [0.5, 0.5, 0], [0.5, -0.5 * math.cos(angle), 0.5 * math.sin(angle)], [2, 2, 2]], f32)
        F = np.array([[0, 1, 2], [1, 0, 3], [2, 3, 4]], np.int32)
        assert abs(float(_entries(surface_graph(V, F[:2]))[(2, 3)]) - 1.0) <= 2e-7           # the virtual edge alone
        csr = surface_graph(V, F)
        e = _entries(csr)
        chord = f32(np.linalg.norm(V[2].astype(np.float64) - V[3].astype(np.float64)))
        assert (chord < 0.55 if angle else chord == 1.0) and e[(2, 3)] == e[(3, 2)] == chord and len(e) == len(csr[1]) == 16
        assert np.array_equal(_bits(csr[2]), _bits(gr.surface_graph_ref(V, F)[2]))
    assert len(surface_graph(V, [[0, 1, 2], [2, 1, 0]], unfold=False)[1]) == 6                # an edge listed by two faces appears once


def test_surface_graph_refusals():
    V, F = scenes.torus_mesh(8, 6)
    for bad_v in (V[:, :2], V.reshape(-1)):
        with pytest.raises(ValueError, match="vertices"):
            surface_graph(bad_v, F)
    for bad_f in (F[:, :2], F.reshape(-1), F.astype(f32)):
        with pytest.raises(ValueError, match="faces"):
            surface_graph(V, bad_f)
    for ident in (-1, 48):
        bad = F.copy(); bad[3, 1] = ident
        with pytest.raises(ValueError, match="face index outside"):
            surface_graph(V, bad)
    g = SurfaceGraph(V, F, device="cpu")                                                 # the set-up is host work
    assert g.Vm == 48 and np.array_equal(g.csr[1], surface_graph(V, F)[1])
    with pytest.raises(_lib.GmeshError, match="no CPU path"):
        g.distances([[0]])


# ---- the reference itself ----
def test_dijkstra_equals_jacobi_bit_for_bit():
    rng = np.random.default_rng(5)
    g = gr.random_graph(400, rng)
    for srcs in ([0], [17, 250, 399]):
        d = gr.dijkstra32(*g, [srcs])[0]
        j, _ = gr.jacobi32(*g, srcs)
        assert np.array_equal(_bits(d), _bits(j)) and np.isinf(d).any() and np.isfinite(d).sum() > 100
        cut = np.sort(d[np.isfinite(d)])[60]
        dc, jc = gr.dijkstra32(*g, [srcs], max_distance=cut)[0], gr.jacobi32(*g, srcs, max_distance=cut)[0]
        assert np.array_equal(_bits(dc), _bits(jc)) and np.array_equal(_bits(dc), _bits(np.where(d <= cut, d, np.inf)))
    V, F = scenes.torus_mesh(40, 30)
    for unfold, sweeps in ((False, 37), (True, 26)):
        g = surface_graph(V, F, unfold=unfold)
        j, n = gr.jacobi32(*g, [0])
        assert np.array_equal(_bits(gr.dijkstra32(*g, [[0]])[0]), _bits(j)) and n <= sweeps + 1 and np.isfinite(j).all()
    both = gr.dijkstra32(*g, [[0], [600], [0, 600], []])
    assert np.array_equal(_bits(both[2]), _bits(np.minimum(both[0], both[1]))) and np.isinf(both[3]).all()


def test_unfolded_discs_are_round():
    """planar 41 x 41 grid, one diagonal per cell, points 5 to 20 cells from the source: the worst path / Euclidean distance is 1.4142 on
    the edges alone (the hexagon) and 1.0824 with the unfolded edges"""
    V, F = gr.grid_mesh(41)
    src = 20 * 41 + 20
    euclid = np.linalg.norm(V.astype(np.float64) - V[src].astype(np.float64), axis=1)
    ring = (euclid >= 5) & (euclid <= 20)
    worst = {}
    for unfold in (False, True):
        d = gr.dijkstra32(*surface_graph(V, F, unfold=unfold), [[src]])[0]
        worst[unfold] = float((d[ring] / euclid[ring]).max())
        assert (d[ring] / euclid[ring]).min() >= 1 - 1e-6
    print("worst distance / Euclidean: edges only %.4f, unfolded %.4f" % (worst[False], worst[True]))
    assert worst[True] < 1.09 and worst[False] > 1.41


# ---- region_handles ----
def _rows(*rows):
    return np.array(rows, f32)


def test_region_handles_order_and_owners():
    inf = math.inf
    dh = _rows([0.0, 0.5, 1.0, 2.0, 3.0, inf, 9.0, 1.0], [3.0, 2.0, 1.5, 0.5, 0.0, inf, 9.0, 1.0 + 2 ** -20])
    da = _rows([inf, inf, inf, inf, inf, 4.0, 1.0, inf], [inf, inf, inf, inf, inf, 0.0, 0.5, inf])
    ids, owner = region_handles(dh, None, 1.0)
    assert ids.dtype == np.int64 and owner.dtype == np.int32
    assert ids.tolist() == [0, 1, 2, 7, 3, 4] and owner.tolist() == [0, 0, 0, 0, 1, 1]   # pick order, ascending inside; the radius is inclusive
    ids, owner = region_handles(dh, da, 1.0)
    assert ids.tolist() == [0, 1, 2, 7, 3, 4, 6, 5] and owner.tolist() == [0, 0, 0, 0, 1, 1, -1, -1]     # anchor 0 holds 6; anchor 1 adds only 5
    ids, owner = region_handles(dh[:1], None, 0.5, free_radius=2.0)
    assert ids.tolist() == [0, 1, 4, 5, 6] and owner.tolist() == [0, 0, -1, -1, -1]      # beyond 2.0, the unreachable vertex included; 3 (= 2.0) is free
    ids, owner = region_handles(dh, da, 0.5, free_radius=2.5)
    assert ids.tolist() == [0, 1, 3, 4, 5, 6] and owner.tolist() == [0, 0, 1, 1, -1, -1]  # held once each: by the anchor, then by distance
    ids, owner = region_handles(dh[:1], None, 0.0)
    assert ids.tolist() == [0] and owner.tolist() == [0]
    import torch
    t_ids, t_owner = region_handles(torch.as_tensor(dh), torch.as_tensor(da), 1.0)
    assert t_ids.tolist() == [0, 1, 2, 7, 3, 4, 6, 5]


def test_region_handles_refusals():
    dh = _rows([0.0, 0.5, 1.0, 2.0, 3.0], [3.0, 2.0, 1.0, 0.5, 0.0])
    da = _rows([5.0, 5.0, 5.0, 0.75, 0.0])
    with pytest.raises(ValueError, match=r"handle 0 and handle 1 overlap \(vertex 2 "):
        region_handles(dh, None, 1.0)
    with pytest.raises(ValueError, match=r"handle 1 meets the region of anchor 0 \(vertex 3 "):
        region_handles(dh, da, 0.75)
    with pytest.raises(ValueError, match="free_radius 0.25 is below grab_radius 0.5"):
        region_handles(dh, None, 0.5, free_radius=0.25)
    for grab, free in ((-1.0, None), (math.nan, None), (0.5, math.nan), (0.5, -2.0)):
        with pytest.raises(ValueError, match="must be >= 0 and not NaN"):
            region_handles(dh, None, grab, free_radius=free)
    with pytest.raises(ValueError, match="d_handles"):
        region_handles(np.zeros((0, 5), f32), None, 1.0)
    assert region_handles(dh, None, 0.5, free_radius=0.5)[0].tolist() == [0, 1, 3, 4, 2]  # the radii may be equal


# ---- the C ABI ----
def test_geodesic_is_declared_and_typed():
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for name, ret, n in (("gm_mesh_geodesic", "int", 15), ("gm_mesh_geodesic_workspace_bytes", "size_t", 3)):
        m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)" % (ret, name), txt)
        assert m and len(m.group(1).split(",")) == n == len(_lib.SIGNATURES[name][1])
    assert _lib.lib().gm_abi_version() == 3


def test_geodesic_refuses_before_any_gpu_work():
    """every refusal below happens with host pointers that would fault if anything were launched with them"""
    l = _lib.lib()
    p = 4096                                                                             # not NULL, and nothing anyone may read
    good = dict(Vm=10, off=p, cols=p, lens=p, B=2, soff=p, src=p, cut=math.inf, sweeps=4, resume=0, dist=p, uns=p, ws=p, nbytes=1 << 20)

    def call(**kw):
        a = dict(good, **kw)
        return l.gm_mesh_geodesic(a["Vm"], a["off"], a["cols"], a["lens"], a["B"], a["soff"], a["src"], a["cut"], a["sweeps"], a["resume"], a["dist"],
                                  a["uns"], a["ws"], a["nbytes"], None)
    for kw, word in ((dict(Vm=-1), "negative size"), (dict(B=-1), "negative size"), (dict(sweeps=0), "sweeps"), (dict(sweeps=-3), "sweeps"),
                     (dict(B=0), "source sets"), (dict(B=65536), "source sets"), (dict(cut=math.nan), "max_distance"), (dict(cut=-1.0), "max_distance"),
                     (dict(cut=-math.inf), "max_distance")) + tuple((({k: None}), "null pointer") for k in ("off", "cols", "lens", "soff", "src", "dist", "uns", "ws")):
        assert call(**kw) == 1 and word in l.gm_last_error().decode(), kw                # GM_ERR_INVALID_ARG
    need = l.gm_mesh_geodesic_workspace_bytes(10, 2, 4)
    assert call(nbytes=need - 1) == 3 and "workspace too small" in l.gm_last_error().decode()      # GM_ERR_BUFFER
    assert call(Vm=0) == 0 and call(Vm=0, B=0, off=None, cols=None, lens=None, soff=None, src=None, dist=None, uns=None, ws=None, nbytes=0) == 0
    sizes = [l.gm_mesh_geodesic_workspace_bytes(1000, 3, s) for s in (0, 1, 2, 64, 65, 1024, 100000)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] >= 4 * 100001
    assert l.gm_mesh_geodesic_workspace_bytes(1, 1, 64) == l.gm_mesh_geodesic_workspace_bytes(10 ** 6, 8, 64)      # in place: O(sweeps)


def test_geodesic_unit_neither_waits_nor_allocates():
    """gm_mesh_geodesic's "no host synchronisation, no device allocation", and no workgroup waiting for another: its translation unit
    names no such runtime call, and its kernels hold no loop on memory another workgroup writes"""
    src = open(os.path.join(_lib.CSRC, "gm_geodesic.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("hipMalloc", "hipFree", "hipMemcpy", "hipMemset", "Synchronize", "hipEventQuery", "hipStreamQuery", "hipStreamWaitEvent", "while",
                 "atomicMin", "atomicCAS", "atomicExch", "__threadfence"):
        assert word not in code, word
    assert code.count("atomicAdd(") == 1 and "float" not in code.split("atomicAdd(")[1].split(";")[0]       # one integer atomic a workgroup
    assert "gm_geodesic.hip" in open(os.path.join(_lib.CSRC, "Makefile")).read()


# ---- --pick_sequence ----
def test_pick_sequence_radii(tmp_path):
    from gaussianmesh_amd.edit_sequence import read_pick_sequence
    path = str(tmp_path / "picks.json")
    good = dict(camera_id=1, handles=[[10, 20], [30.5, 8]], anchors=[[5, 5]], offsets=[[[1, 0], [0, 1]], [[2, 0], [0, 2]]])

    def read(**kw):
        with open(path, "w") as fh:
            json.dump(dict(good, **kw), fh)
        return read_pick_sequence(path)
    plain = read()
    assert len(plain) == 4 and plain[0] == 1 and plain[1].shape == (2, 2) and plain[2].shape == (1, 2) and plain[3].shape == (2, 2, 2)      # as before
    out = read(grab_radius=0.5, free_radius=2)
    assert len(out) == 5 and out[4] == (0.5, 2.0) and all(np.array_equal(a, b) for a, b in zip(out[:4], plain))
    assert read(grab_radius=0.25)[4] == (0.25, None) and read(free_radius=1.5)[4] == (0.0, 1.5) and read(grab_radius=0, free_radius=0)[4] == (0.0, 0.0)
    for kw, word in ((dict(grab_radius=-0.5), '"grab_radius"'), (dict(grab_radius="1"), '"grab_radius"'), (dict(grab_radius=None), '"grab_radius"'),
                     (dict(grab_radius=True), '"grab_radius"'), (dict(grab_radius=[1]), '"grab_radius"'), (dict(grab_radius=float("nan")), '"grab_radius"'),
                     (dict(free_radius=float("inf")), '"free_radius"'), (dict(grab_radius=1, free_radius=-1), '"free_radius"'),
                     (dict(grab_radius=1.0, free_radius=0.5), '"free_radius" 0.5 is below "grab_radius" 1')):
        with pytest.raises(SystemExit, match=word):
            read(**kw)
    with pytest.raises(SystemExit, match='"offsets"'):                                  # the old refusals still come first
        read(grab_radius=1, offsets=[])
