"""Mesh simplification on the host: the numpy definition of gm_mesh_quadrics / gm_mesh_collapse_round / simplify (tests/simplify_ref.py)
against itself and against the invariants the design rests on - the selected set of a round is 2-ring independent, a closed mesh stays
closed, borders stay, the trim lands where the parity argument says -, the new ABI rows, and every refusal that is decided before any
GPU work.  The device is held to the definition bit for bit in test_gpu_simplify.py."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simplify_ref as sr
import tsdf_ref as tr

f32 = np.float32
CLOSED = ("octahedron", "icosahedron", "torus_16x16", "torus_7x5", "sphere_nets", "two_tori", "fan", "edges_255")


def _runs():
    """each closed builder simplified to a quarter, with the trace of every round; computed once"""
    if not _runs.cache:
        for name in CLOSED:
            V, F = sr.BUILDERS[name]()
            rounds = []
            res = sr.simplify_ref(V, F, ratio=0.25, trace=lambda k, before, r, sel, after: rounds.append((before, r, sel, after)))
            _runs.cache[name] = (V, F, res, rounds)
    return _runs.cache


_runs.cache = {}


# ---- 1. quadrics ----
@pytest.mark.parametrize("name", sorted(sr.BUILDERS))
def test_quadrics_match_float64_within_rounding(name):
    V, F = sr.BUILDERS[name]()
    Q, Q64 = sr.quadrics_ref(V, F), sr.quadrics_f64(V, F)
    fin = np.isfinite(Q64).all(1)
    assert np.array_equal(np.isfinite(Q).all(1), fin)
    # a face's term: ~10 roundings of values up to area * max(1, |a|)^2; a vertex sums at most its valence of them
    F64 = np.asarray(F, np.int64)
    scale = np.zeros(len(V))
    n = np.linalg.norm(sr.face_normals64(np.nan_to_num(V), F64), axis=1)
    reach = np.maximum(1.0, np.abs(np.nan_to_num(V)).max()) ** 2
    np.add.at(scale, F64.reshape(-1), np.repeat(0.5 * n * reach, 3))
    val = np.bincount(F64.reshape(-1), minlength=len(V))
    tol = (16 + val)[:, None] * np.finfo(f32).eps * scale[:, None] + 1e-30
    assert (np.abs(Q[fin] - Q64[fin]) <= tol[fin]).all()
    assert (Q[val == 0] == 0).all()


def test_quadric_of_a_plane_vanishes_on_it():
    V, F = sr.flat_patch()
    Q = sr.quadrics_ref(V, F)
    r = sr.round_ref(V, Q, F)
    cand = r["frm"] >= 0
    assert cand.any() and (r["cost"][cand] == 0).all()                # every cost ties: the edge id decides
    assert np.array_equal(r["key"][cand], np.nonzero(cand)[0].astype(np.uint64))


def test_degenerate_faces_add_nothing():
    V, F = sr.zero_area_face()
    Q = sr.quadrics_ref(V, F)
    assert np.isfinite(Q).all()
    keep = np.array([not (1 in f and 5 in f) for f in F.tolist()])
    assert np.array_equal(Q, sr.quadrics_ref(V, F[keep]))
    V, F = sr.nan_vertex()
    Q = sr.quadrics_ref(V, F)
    assert np.isfinite(Q).all()                                        # faces at the NaN vertex are skipped, not summed


# ---- 2. one round ----
@pytest.mark.parametrize("name", sorted(sr.BUILDERS))
def test_selected_set_is_two_ring_independent(name):
    """no end of a selected edge lies in the closed neighbourhood of an end of another selected edge: what makes a round's collapses
    commute.  Checked on EVERY round of a run that goes on until it stalls (up to 67 rounds, on torus_nets): the later rounds have the
    irregular valences and the summed quadrics."""
    V, F = sr.BUILDERS[name]()
    seen = []
    res = sr.simplify_ref(V, F, target_faces=0, trace=lambda k, before, r, sel, after: seen.append(r))
    assert res["stalled"] and len(seen) == res["rounds"]
    if name in ("tetrahedron", "four_face_edge"):                      # nothing may collapse there: say so instead of passing on an empty trace
        r = sr.round_ref(V, sr.quadrics_ref(V, F), F)
        assert seen == [] and not r["selected"].any() and (r["frm"] == -1).all() and (r["key"] == sr.NONE).all()
        return
    assert len(seen) >= 1
    for r in seen:
        N = sr.closed_neighbourhood_sets(len(V), r["neighbours"])
        sel = np.nonzero(r["selected"])[0]
        assert len(sel) > 0
        for e in sel.tolist():
            assert not r["locked"][r["frm"][e]] and r["uses"][e] == 2
        ends = {}
        for e in sel.tolist():
            for x in (int(r["frm"][e]), int(r["to"][e])):
                assert x not in ends, "two selected edges share an end"
                ends[x] = e
        for e in sel.tolist():
            i, j = int(r["frm"][e]), int(r["to"][e])
            for u in N[i] | N[j]:
                assert ends.get(u, e) == e, "an end of edge %d lies in the neighbourhood of edge %d" % (ends[u], e)


def test_tie_removes_the_larger_id_and_key_holds_cost_and_edge():
    V, F = sr.flat_patch()                                             # every cost is 0: wherever both directions stand, hi goes
    r = sr.round_ref(V, sr.quadrics_ref(V, F), F)
    c = np.nonzero(r["frm"] >= 0)[0]
    lo, hi = r["edges"][c, 0], r["edges"][c, 1]
    both = ~r["locked"][lo] & ~r["locked"][hi]
    assert both.any() and (r["frm"][c][both] == hi[both]).all() and (r["to"][c][both] == lo[both]).all()
    only_lo = r["locked"][hi] & ~r["locked"][lo]
    assert only_lo.any() and (r["frm"][c][only_lo] == lo[only_lo]).all()
    V2, F2 = sr.torus(16, 16)
    r2 = sr.round_ref(V2, sr.quadrics_ref(V2, F2), F2)
    c = np.nonzero(r2["frm"] >= 0)[0]
    assert len(c) and (np.sort(np.stack([r2["frm"][c], r2["to"][c]], 1), 1) == r2["edges"][c]).all()
    assert np.array_equal((r2["key"][c] >> np.uint64(32)).astype(np.uint32), r2["cost"][c].view(np.uint32))
    assert ((r2["key"][c] & np.uint64(0xFFFFFFFF)) == c.astype(np.uint64)).all()
    assert (r2["key"][r2["frm"] < 0] == sr.NONE).all() and (r2["to"][r2["frm"] < 0] == -1).all()


def test_max_error_and_min_cos_reject():
    V, F = sr.torus(16, 16)
    Q = sr.quadrics_ref(V, F)
    free = sr.round_ref(V, Q, F, min_cos=0.0)
    cost = free["cost"][free["frm"] >= 0]
    bound = float(np.median(cost))
    r = sr.round_ref(V, Q, F, min_cos=0.0, max_error=bound)
    c = r["frm"] >= 0
    assert 0 < c.sum() < (free["frm"] >= 0).sum() and (r["cost"][c] <= f32(bound)).all()
    assert (sr.round_ref(V, Q, F, min_cos=1.0)["frm"] >= 0).sum() <= (sr.round_ref(V, Q, F, min_cos=0.2)["frm"] >= 0).sum() <= c.size


# ---- 3. whole runs ----
@pytest.mark.parametrize("name", CLOSED)
def test_closed_mesh_stays_closed_through_every_round(name):
    V, F, res, rounds = _runs()[name]
    Vm = len(V)
    chi0, comps0 = tr.euler_characteristic(len(np.unique(F)), F), tr.n_components(Vm, F)
    assert rounds
    for before, r, sel, after in rounds:
        n = int(sel.sum())
        assert n > 0
        assert len(after) == len(before) - 2 * n                                    # F - 2 per collapse
        assert len(np.unique(after)) == len(np.unique(before)) - n                  # V - 1 per collapse
        assert tr.is_closed(after)
        assert tr.euler_characteristic(len(np.unique(after)), after) == chi0 and tr.n_components(Vm, after) == comps0
        assert (after[:, 0] != after[:, 1]).all() and (after[:, 1] != after[:, 2]).all() and (after[:, 2] != after[:, 0]).all()
        assert len(np.unique(np.sort(after, 1), axis=0)) == len(after)              # no two faces over the same vertices
        # every surviving face against itself before the round
        remap = np.arange(Vm)
        remap[r["frm"][sel]] = r["to"][sel]
        moved = remap[before]
        alive = (moved[:, 0] != moved[:, 1]) & (moved[:, 1] != moved[:, 2]) & (moved[:, 2] != moved[:, 0])
        assert np.array_equal(moved[alive], after)
        n0, n1 = sr.face_normals64(V, before[alive]), sr.face_normals64(V, after)
        assert ((n0 * n1).sum(1) > 0).all()
    assert res["stalled"] or len(res["faces"]) <= len(F) // 4          # (the small solids stall: nothing closed has fewer than four faces)
    assert len(res["faces"]) < len(F) and (len(F) < 256 or not res["stalled"])


def test_plane_patch_keeps_its_border_and_stalls_there():
    V, F = sr.plane_nets()
    e0, u0 = sr.edges_ref(F, len(V))
    border = e0[u0 == 1]
    assert len(border) == 26
    res = sr.simplify_ref(V, F, target_faces=2)
    assert res["stalled"] and res["locked_vertices"] == len(np.unique(border))
    kept = res["kept"]
    assert set(np.unique(border).tolist()) == set(kept.tolist())       # only border vertices are left
    e1, u1 = sr.edges_ref(kept[res["faces"]], len(V))
    have = set(map(tuple, e1[u1 == 1].tolist()))
    assert set(map(tuple, border.tolist())) == have                    # and every border edge is still a border edge


def test_tetrahedron_never_changes():
    V, F = sr.tetrahedron()
    for kw in (dict(target_faces=2), dict(target_faces=0, min_cos=0.0), dict(max_error=1e9)):
        res = sr.simplify_ref(V, F, **kw)
        assert res["stalled"] and res["rounds"] == 0 and np.array_equal(res["faces"], F) and np.array_equal(res["vertices"], V)


def test_four_face_edge_ends_stay():
    V, F = sr.four_face_edge()
    res = sr.simplify_ref(V, F, target_faces=0)
    assert {0, 1} <= set(res["kept"].tolist())
    V, F = sr.four_face_edge_fine()
    res = sr.simplify_ref(V, F, ratio=0.25)
    assert {0, 1} <= set(res["kept"].tolist()) and res["locked_vertices"] == 2
    e, u = sr.edges_ref(res["kept"][res["faces"]], len(V))
    assert (u == 4).sum() == 1 and e[u == 4].tolist() == [[0, 1]]


def test_nan_vertex_neighbourhood_is_never_collapsed():
    V, F = sr.nan_vertex()
    bad = 37
    ring = np.unique(F[(F == bad).any(1)])
    res = sr.simplify_ref(V, F, ratio=0.25)
    assert set(ring.tolist()) <= set(res["kept"].tolist())
    assert res["rounds"] > 0 and np.isfinite(res["max_cost"])


@pytest.mark.parametrize("target", [240, 241, 600, 601, 2, 3])
def test_trim_lands_on_target_or_one_below_by_parity(target):
    """a collapse removes exactly two faces, so the parity of the face count is fixed: target when (F - target) is even, target - 1 else"""
    V, F = sr.torus(20, 15)                                            # 600 faces
    res = sr.simplify_ref(V, F, target_faces=target)
    if target >= len(F):
        assert res["rounds"] == 0 and np.array_equal(res["faces"], F)
        return
    if res["stalled"]:
        assert len(res["faces"]) > target
        return
    assert len(res["faces"]) == (target if (len(F) - target) % 2 == 0 else target - 1)


def test_target_at_or_above_returns_the_input():
    V, F = sr.unreferenced_vertex(7, 5)
    res = sr.simplify_ref(V, F, target_faces=len(F))
    assert res["rounds"] == 0 and not res["stalled"] and np.array_equal(res["faces"], F)
    assert res["vertex_map"][-1] == -1 and len(res["kept"]) == len(V) - 1
    assert sr.simplify_ref(V, F, ratio=1.0)["rounds"] == 0


@pytest.mark.parametrize("name", ["torus_16x16", "torus_257", "sphere_nets", "two_tori", "plane_nets", "four_face_edge_fine"])
def test_kept_and_vertex_map(name):
    V, F = sr.BUILDERS[name]()
    steps = []
    res = sr.simplify_ref(V, F, ratio=0.25, trace=lambda k, before, r, sel, after: steps.append((before, r["frm"][sel], r["to"][sel])))
    kept, vmap = res["kept"], res["vertex_map"]
    assert (np.diff(kept) > 0).all()
    assert np.array_equal(res["vertices"].view(np.uint32), V[kept].view(np.uint32))
    assert np.array_equal(vmap[kept], np.arange(len(kept)))
    used = np.zeros(len(V), bool)
    used[np.unique(F)] = True
    assert (vmap[~used] == -1).all() and (vmap[used] >= 0).all()
    # a removed vertex ends where a walk along edges (each one an edge of the mesh when it was collapsed) takes it
    parent = np.arange(len(V))
    for before, i, j in steps:
        e, _ = sr.edges_ref(before, len(V))
        have = set(map(tuple, e.tolist()))
        for a, b in zip(i.tolist(), j.tolist()):
            assert (min(a, b), max(a, b)) in have
        parent[i] = j
    for v in np.nonzero(used)[0]:
        x = v
        while parent[x] != x:
            x = parent[x]
        assert kept[vmap[v]] == x
    assert tr.n_components(len(kept), res["faces"]) == tr.n_components(len(V), F)


def test_input_faces_with_a_repeated_corner_go_first_and_duplicates_lock():
    V, F = sr.dirty_mesh()
    clean = F[(F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 2] != F[:, 0])]
    assert len(clean) == len(F) - 2
    a, b = sr.simplify_ref(V, F, target_faces=100), sr.simplify_ref(V, clean, target_faces=100)
    assert a["degenerate_faces"] == 2 and b["degenerate_faces"] == 0 and a["faces_before"] == len(F)
    for k in ("faces", "kept", "vertex_map"):
        assert np.array_equal(a[k], b[k]), k
    assert a["rounds"] == b["rounds"] > 0 and a["reached"] and not a["stalled"]
    dup = set(F[-1].tolist())                                          # the face given twice: three-face edges, its corners locked
    assert a["locked_vertices"] == 3 and dup <= set(a["kept"].tolist())
    out = a["kept"][a["faces"]]
    assert (np.sort(out, 1) == np.sort(F[-1])).all(1).sum() == 2
    untouched = sr.simplify_ref(V, F, target_faces=len(F))             # zero rounds: still without the two degenerate faces
    assert untouched["rounds"] == 0 and np.array_equal(untouched["kept"][untouched["faces"]], clean) and untouched["reached"]
    assert not sr.simplify_ref(*sr.plane_nets(), target_faces=2)["reached"]


def test_runs_are_repeatable():
    V, F = sr.torus(16, 16)
    a, b = sr.simplify_ref(V, F, ratio=0.25), sr.simplify_ref(V, F, ratio=0.25)
    assert np.array_equal(a["faces"], b["faces"]) and np.array_equal(a["vertex_map"], b["vertex_map"]) and a["rounds"] == b["rounds"]


# ---- 4. the ABI ----
def test_entry_points_are_declared_typed_and_in_sync():
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    names = _lib.header_symbols()
    txt = open(_lib.HEADER).read()
    for name, ret, n in (("gm_mesh_quadrics", "int", 8), ("gm_mesh_collapse_round_workspace_bytes", "size_t", 1), ("gm_mesh_collapse_round", "int", 20)):
        assert name in names and name in _lib.SIGNATURES and hasattr(l, name), name
        m = re.search(r"\b%s\s+%s\(([^)]*)\);" % (ret, name), txt)
        assert m and len(m.group(1).split(",")) == n == len(_lib.SIGNATURES[name][1]), name
    assert set(names) == set(_lib.SIGNATURES)
    assert l.gm_abi_version() == 3 and "#define GM_ABI_VERSION 3" in txt
    assert "gm_simplify.hip" in open(os.path.join(_lib.CSRC, "Makefile")).read()


def test_unit_neither_waits_nor_allocates():
    from gaussianmesh_amd import _lib
    src = open(os.path.join(_lib.CSRC, "gm_simplify.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("hipMalloc", "hipFree", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy", "while (atomic", "__threadfence"):
        assert word not in code, word
    assert "#pragma clang fp contract(off)" in code


def test_workspace_query_is_monotonic_and_positive():
    from gaussianmesh_amd import _lib
    q = _lib.lib().gm_mesh_collapse_round_workspace_bytes
    assert q(0) > 0 and q(-3) == q(0)
    sizes = [0, 1, 255, 256, 257, 7500, 10 ** 6]
    assert all(q(a) <= q(b) for a, b in zip(sizes, sizes[1:]))
    assert 9 * 10 ** 6 <= q(10 ** 6) < 9 * 10 ** 6 + 4096


# ---- 5. refusals, all before any GPU work ----
def test_quadrics_refuses_before_any_gpu_work():
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    M = 1 << 24
    def call(Vm=100, V=1 * M, F=200, faces=2 * M, off=3 * M, adj=4 * M, Q=5 * M):
        return l.gm_mesh_quadrics(Vm, V, F, faces, off, adj, Q, None)
    err = lambda: l.gm_last_error()
    assert call(Vm=-1) == 1 and call(F=-1) == 1 and b"negative size" in err()
    assert call(F=(1 << 31) // 3 + 1) == 1
    for k in ("V", "faces", "off", "adj", "Q"):
        assert call(**{k: None}) == 1 and b"null pointer" in err(), k
    assert call(Q=1 * M + 12 * 100 - 1) == 1 and b"vertices overlaps out_quadrics" in err()
    assert call(Q=2 * M - 40 * 100 + 1) == 1 and b"faces overlaps out_quadrics" in err()
    assert call(Q=3 * M + 4 * 100) == 1 and b"vf_offsets overlaps out_quadrics" in err()
    assert call(Q=4 * M + 12 * 200 - 4) == 1 and b"vf_faces overlaps out_quadrics" in err()
    assert call(Vm=0, V=None, faces=None, off=None, adj=None, Q=None) == 0       # nothing to do: launches nothing


def test_collapse_round_refuses_before_any_gpu_work():
    """bogus non-null "pointers": every refusal is decided on the arguments alone"""
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    M = 1 << 24
    need = l.gm_mesh_collapse_round_workspace_bytes(100)
    names = ("V", "Q", "faces", "off", "adj", "edges", "uses", "sel", "frm", "to", "key", "count", "ws")
    def call(Vm=100, F=200, E=300, min_cos=0.2, max_error=float("inf"), ws_bytes=need, **kw):
        p = {n: (k + 1) * M for k, n in enumerate(names)}
        p.update(kw)
        return l.gm_mesh_collapse_round(Vm, p["V"], p["Q"], F, p["faces"], p["off"], p["adj"], E, p["edges"], p["uses"], min_cos, max_error,
                                        p["sel"], p["frm"], p["to"], p["key"], p["count"], p["ws"], ws_bytes, None)
    err = lambda: l.gm_last_error()
    assert call(Vm=-1) == 1 and call(F=-1) == 1 and call(E=-1) == 1 and b"negative size" in err()
    for bad in (-0.1, float("nan"), float("inf")):
        assert call(min_cos=bad) == 1 and b"min_cos" in err(), bad
    for bad in (-1.0, float("nan")):
        assert call(max_error=bad) == 1 and b"max_error" in err(), bad
    assert call(Vm=0) == 1 and call(F=0) == 1 and b"empty mesh" in err()
    for n in names:
        assert call(**{n: None}) == 1 and b"null pointer" in err(), n
    assert call(key=11 * M + 4) == 1 and b"aligned" in err()
    out = dict(sel=300, frm=1200, to=1200, key=2400, count=4)
    for n, nbytes in out.items():                                      # each output onto the last byte of an input, and onto the workspace
        assert call(**{n: 1 * M + 12 * 100 - (8 if n == "key" else 1)}) == 1 and b"vertices overlaps" in err(), n
        assert call(**{n: 13 * M + (need // 8) * 8 - 8}) == 1 and b"overlaps workspace" in err(), n
    assert call(frm=8 * M + 296) == 1 and b"out_selected overlaps out_from" in err()
    assert call(ws=7 * M - need + 1) == 1 and b"edge_faces overlaps workspace" in err()
    # an undersized workspace: GM_ERR_BUFFER, still before any GPU work; zero edges: nothing to do
    assert call(ws_bytes=need - 1) == 3 and b"workspace too small" in err()
    assert call(ws_bytes=0) == 3
    assert call(E=0, edges=None, uses=None, sel=None, frm=None, to=None, key=None, count=None) == 0


def test_python_refusals():
    from gaussianmesh_amd._lib import GmeshError
    from gaussianmesh_amd import mesh_simplify as ms
    V, F = (torch.as_tensor(x) for x in sr.octahedron())
    for kw in (dict(), dict(target_faces=4, ratio=0.5), dict(ratio=0.0), dict(ratio=1.5), dict(ratio=float("nan")), dict(target_faces=-1),
               dict(target_faces=2.5), dict(target_faces=4, max_error=float("nan")), dict(target_faces=4, max_error=-1.0),
               dict(target_faces=4, max_error=float("inf")), dict(target_faces=4, min_cos=float("nan")), dict(target_faces=4, min_cos=-0.1),
               dict(target_faces=4, min_cos=1.5), dict(target_faces=4, max_rounds=-1)):
        with pytest.raises(ValueError):
            ms.simplify(V, F, **kw)
        if "min_cos" not in kw and "max_rounds" not in kw and not ("max_error" in kw and "target_faces" in kw):
            with pytest.raises(ValueError):
                sr.simplify_ref(V.numpy(), F.numpy(), **kw)
    for kw in (dict(target_faces=True), dict(ratio=True), dict(target_faces=4, min_cos=False), dict(target_faces=4, max_error=True),
               dict(target_faces=4, max_rounds=True), dict(target_faces="4"), dict(target_faces=4, min_cos=None), dict(target_faces=4, max_rounds=2.5)):
        with pytest.raises(ValueError):                                # bool is no number here, nor is a string
            ms.simplify(V, F, **kw)
    with pytest.raises(GmeshError, match="no CPU path"):
        ms.simplify(V, F, target_faces=4)
    # any real scalar passes the parameter checks (and then meets the device check): numpy scalars, 0-d tensors
    for kw in (dict(target_faces=np.int64(4)), dict(target_faces=torch.tensor(4)), dict(ratio=np.float32(0.5)), dict(ratio=torch.tensor(0.5)),
               dict(target_faces=4, max_error=np.float32(0.1), min_cos=np.float64(0.2)), dict(max_error=torch.tensor(0.1), max_rounds=np.int32(7)),
               dict(target_faces=4.0)):
        with pytest.raises(GmeshError, match="no CPU path"):
            ms.simplify(V, F, **kw)
    assert ms.resolve_target(100, ratio=np.float32(0.255)) == sr.resolve_target(100, ratio=np.float32(0.255)) == 25
    with pytest.raises(GmeshError, match="no CPU path"):
        ms.simplify(V.numpy(), F.numpy(), target_faces=4)
    with pytest.raises(GmeshError, match="no CPU path"):
        ms.quadrics(V, F)
    assert ms.resolve_target(100, ratio=0.255) == sr.resolve_target(100, ratio=0.255) == 25
    assert ms.resolve_target(100, max_error=1.0) == sr.resolve_target(100, max_error=1.0) == 0
