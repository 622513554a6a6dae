"""Mesh simplification on the device, held to the numpy definition (tests/simplify_ref.py) bit for bit: gm_mesh_quadrics, one round of
gm_mesh_collapse_round (all 64 key bits, directions, selected flags, the count), whole runs of mesh_simplify.simplify; then what it is
for - from_cloud(..., target_faces=N) gives a mesh that binds and drags -, both CLIs in fresh child processes, and the C-level refusals
on guard-banded buffers.  No comparison leaves an element out."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simplify_ref as sr
import tsdf_ref as tr
from poison import FILLS, differing, poisoned, run_under_fills

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, f32)).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return sr.BUILDERS[name]()


# ---- 1. quadrics ----
@pytest.mark.parametrize("name", sorted(sr.BUILDERS))
def test_quadrics_bit_for_bit(name):
    """every builder: 255 / 256 / 257 vertices (torus_17x15, torus_16x16, torus_257), the valence-70 fan, zero-area faces, a NaN vertex,
    an unreferenced vertex.  The output is allocated inside poison.poisoned: pre-filled with each fill, guard bands checked.
    (gm_mesh_quadrics takes no workspace.)"""
    from gaussianmesh_amd import mesh_simplify as ms
    V, F = _mesh(name)
    ref = sr.quadrics_ref(V, F)
    dV, dF = _dev(V), _dev(F, torch.int32)
    runs = run_under_fills(lambda: ms.quadrics(dV, dF))
    assert differing(runs) == []
    got = runs[0][1].cpu().numpy()
    assert got.shape == ref.shape and np.array_equal(_bits(got), _bits(ref)), "%d of %d values differ" % ((_bits(got) != _bits(ref)).sum(), ref.size)


# ---- 2. one round ----
def _device_round(V, Q, F, min_cos=0.2, max_error=None):
    """gm_mesh_collapse_round on the live faces F with the module's own bookkeeping; outputs from torch.empty (guarded inside
    poison.poisoned), the workspace one byte into its buffer"""
    from gaussianmesh_amd import _lib
    from gaussianmesh_amd import mesh_simplify as ms
    l = _lib.lib()
    dV, dQ, dF = _dev(V), _dev(Q), _dev(F, torch.int64)
    edges, uses, off, adj = ms._bookkeeping(dF, len(V))
    F32 = dF.to(torch.int32).contiguous()
    E = edges.shape[0]
    o = dict(device="cuda")
    sel, frm, to = torch.empty((E,), dtype=torch.uint8, **o), torch.empty((E,), dtype=torch.int32, **o), torch.empty((E,), dtype=torch.int32, **o)
    key, count = torch.empty((E,), dtype=torch.int64, **o), torch.empty((1,), dtype=torch.int32, **o)
    need = l.gm_mesh_collapse_round_workspace_bytes(len(V))
    ws = torch.empty((need + 1,), dtype=torch.uint8, **o)[1:]
    assert ws.data_ptr() % 2 == 1
    rc = l.gm_mesh_collapse_round(len(V), dV.data_ptr(), dQ.data_ptr(), F32.shape[0], F32.data_ptr(), off.data_ptr(), adj.data_ptr(), E,
                                  edges.data_ptr(), uses.data_ptr(), min_cos, float("inf") if max_error is None else max_error, sel.data_ptr(),
                                  frm.data_ptr(), to.data_ptr(), key.data_ptr(), count.data_ptr(), ws.data_ptr(), need,
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0, l.gm_last_error()
    torch.cuda.synchronize()
    return dict(edges=edges, uses=uses, off=off, adj=adj, selected=sel, frm=frm, to=to, key=key, count=count)


def _same_round(got, ref, F, Vm, what):
    n = lambda t: t.cpu().numpy()
    assert np.array_equal(n(got["edges"]), ref["edges"]) and np.array_equal(n(got["uses"]), ref["uses"]), what + ": bookkeeping"
    off, adj = sr.vertex_face_csr(F, Vm)
    assert np.array_equal(n(got["off"]), off) and np.array_equal(n(got["adj"]), adj), what + ": CSR"
    assert np.array_equal(n(got["key"]).view(np.uint64), ref["key"]), what + ": %d keys differ" % (n(got["key"]).view(np.uint64) != ref["key"]).sum()
    assert np.array_equal(n(got["frm"]), ref["frm"]) and np.array_equal(n(got["to"]), ref["to"]), what + ": directions"
    assert np.array_equal(n(got["selected"]).astype(bool), ref["selected"]) and n(got["selected"]).max(initial=0) <= 1, what + ": selected"
    assert int(got["count"].item()) == int(ref["selected"].sum()), what + ": count"


@functools.lru_cache(maxsize=None)
def _two_rounds(name):
    """the states before the first and the second round of a run of the definition: [(faces, quadrics)]"""
    V, F = _mesh(name)
    F = np.asarray(F, np.int64)
    states = [(F, sr.quadrics_ref(V, F))]
    sr.simplify_ref(V, F, target_faces=0, max_rounds=1, trace=lambda k, before, r, sel, after: states.append((after, r["quadrics_after"])))
    return states


@pytest.mark.parametrize("name", sorted(sr.BUILDERS))
def test_round_bit_for_bit(name):
    """the first round of every builder and the second (quadrics that are sums, irregular valences): 768 edges (torus_16x16), 255 / 256 /
    257 (edges_*), the flat patch where every cost ties, locked borders and four-face edges, the NaN vertex"""
    V, _ = _mesh(name)
    states = _two_rounds(name)
    assert len(states) == 2 or name in ("tetrahedron", "four_face_edge")
    for k, (F, Q) in enumerate(states):
        what = "%s round %d" % (name, k)
        ref = sr.round_ref(V, Q, F)
        runs = run_under_fills(lambda: _device_round(V, Q, F))
        assert differing(runs) == [], what
        _same_round(runs[0][1], ref, F, len(V), what)
    if name == "flat_patch":
        ref = sr.round_ref(V, states[0][1], states[0][0])
        assert ref["selected"].any() and (ref["cost"][ref["frm"] >= 0] == 0).all()


@pytest.mark.parametrize("min_cos,max_error", [(0.0, None), (0.9, None), (0.2, 0.002), (0.0, 0.0)])
def test_round_parameters_bit_for_bit(min_cos, max_error):
    for name in ("torus_16x16", "bumpy_patch", "sphere_nets"):
        V, _ = _mesh(name)
        F, Q = _two_rounds(name)[1]
        ref = sr.round_ref(V, Q, F, min_cos, max_error)
        _same_round(_device_round(V, Q, F, min_cos, max_error), ref, F, len(V), "%s min_cos=%r max_error=%r" % (name, min_cos, max_error))


# ---- 3. whole runs ----
RUNS = {
    "torus 40x30 to a quarter": (lambda: sr.torus(40, 30), dict(ratio=0.25)),
    "torus 40x30 to a tenth": (lambda: sr.torus(40, 30), dict(ratio=0.1)),
    "sphere nets 20^3 to an eighth": (lambda: sr.sphere_nets(20), dict(ratio=0.125)),
    "plane patch to 2 (stalls)": (sr.plane_nets, dict(target_faces=2)),
    "four-face edge": (sr.four_face_edge_fine, dict(ratio=0.25)),
    "two tori": (sr.two_tori, dict(ratio=0.2)),
    "NaN vertex": (sr.nan_vertex, dict(ratio=0.25)),
    "max_error alone": (lambda: sr.torus(24, 16), dict(max_error=0.004)),
    "min_cos 0": (lambda: sr.torus(24, 16), dict(ratio=0.2, min_cos=0.0)),
    "min_cos 0.2": (lambda: sr.torus(24, 16), dict(ratio=0.2, min_cos=0.2)),
    "odd target": (lambda: sr.torus(24, 16), dict(target_faces=301)),
    "unreferenced vertex, target above": (sr.unreferenced_vertex, dict(target_faces=10 ** 6)),
    "tetrahedron": (sr.tetrahedron, dict(target_faces=2)),
    "repeated corners and a duplicate face": (sr.dirty_mesh, dict(target_faces=100)),
    "numpy and tensor parameters": (lambda: sr.torus(24, 16), dict(ratio=np.float32(0.2), min_cos=torch.tensor(0.2), max_error=np.float64(10.0),
                                                                   max_rounds=np.int64(500))),
}


@pytest.mark.parametrize("case", sorted(RUNS))
def test_whole_run_equals_the_definition(case):
    from gaussianmesh_amd import mesh_simplify as ms
    build, kw = RUNS[case]
    V, F = build()
    ref = sr.simplify_ref(V, F, **kw)
    dV, dF = _dev(V), _dev(F, torch.int32)
    a, b = ms.simplify(dV, dF, **kw), ms.simplify(dV, dF, **kw)
    for r in (a, b):
        assert r.vertices.dtype == torch.float32 and r.faces.dtype == torch.int32 and r.kept.dtype == torch.int64 and r.vertex_map.dtype == torch.int64
        assert np.array_equal(r.faces.cpu().numpy(), ref["faces"]), case
        assert np.array_equal(r.kept.cpu().numpy(), ref["kept"]) and np.array_equal(r.vertex_map.cpu().numpy(), ref["vertex_map"]), case
        assert np.array_equal(_bits(r.vertices.cpu().numpy()), _bits(ref["vertices"])), case
        st = r.stats
        assert (st["rounds"], st["stalled"], st["faces_before"], st["faces"], st["locked_vertices"], st["degenerate_faces"], st["reached"]) == \
               (ref["rounds"], ref["stalled"], ref["faces_before"], len(ref["faces"]), ref["locked_vertices"], ref["degenerate_faces"],
                ref["reached"]), case
        assert f32(st["max_cost"]) == f32(ref["max_cost"]), case
    # what the cases are there for
    if case == "plane patch to 2 (stalls)":
        assert ref["stalled"] and len(ref["faces"]) > 2 and not ref["reached"]
    if case == "repeated corners and a duplicate face":
        assert ref["degenerate_faces"] == 2 and ref["locked_vertices"] == 3 and ref["rounds"] > 0 and ref["reached"]
    if case == "two tori":
        assert tr.n_components(len(ref["kept"]), ref["faces"]) == 2
    if case == "NaN vertex":
        ring = np.unique(F[(F == 37).any(1)])
        assert set(ring.tolist()) <= set(ref["kept"].tolist()) and ref["rounds"] > 0
    if case == "four-face edge":
        assert {0, 1} <= set(ref["kept"].tolist())
    if case == "max_error alone":
        assert ref["stalled"] and ref["rounds"] > 0 and ref["max_cost"] <= f32(0.004)
    if case == "odd target":
        assert len(ref["faces"]) == 300
    if case in ("unreferenced vertex, target above", "tetrahedron"):
        assert ref["rounds"] == 0 and np.array_equal(ref["faces"], F)


def test_face_ids_out_of_range_are_refused():
    from gaussianmesh_amd import mesh_simplify as ms
    V, F = sr.octahedron()
    for bad in (-1, 6):
        G = F.copy()
        G[3, 1] = bad
        with pytest.raises(ValueError, match="face ids"):
            ms.simplify(_dev(V), _dev(G, torch.int32), target_faces=4)


# ---- 4. downstream: a torus cloud -> its proxy mesh, simplified -> an edit ----
E2E = dict(P=40000, nu=48, nv=32, K=12, W=128, H=128, resolution=48, target=3000)


@functools.lru_cache(maxsize=None)
def _e2e():
    from gaussianmesh_amd import proxy_mesh as pm
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.bg_model import PlainGaussians, inverse_sigmoid
    verts, faces = scenes.torus_mesh(E2E["nu"], E2E["nv"])
    cl = scenes.bind_cloud_to_mesh(E2E["P"], verts, faces, seed=5)
    model = PlainGaussians(3, device="cuda")
    model._set_params(_dev(cl["means"]), _dev(cl["shs"]), torch.log(_dev(cl["scales"])), _dev(cl["rots"]), inverse_sigmoid(_dev(cl["opac"])))
    model.active_sh_degree = 3
    cams = [scenes.orbit_camera(k, E2E["K"], E2E["W"], E2E["H"], radius=6.5, height=(4.5, -4.5)[k % 2]) for k in range(E2E["K"])]
    vol = pm.fuse_cloud(model, cams, resolution=E2E["resolution"])
    assert vol.simplified is None
    dense = vol.extract()                                              # the call as it was before target_faces existed
    stats_dense = dict(vol.stats)
    assert vol.simplified is None
    coarse = vol.extract(target_faces=E2E["target"])
    return dict(model=model, cl=cl, cams=cams, vol=vol, dense=dense, stats_dense=stats_dense, coarse=coarse, stats=dict(vol.stats),
                simplified=vol.simplified)


def _report(V, F):
    edges, uses = tr.edge_use(F)
    f = F.astype(np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    key = lambda e: np.sort(e[:, 0] * max(len(V), 1) + e[:, 1])
    return dict(vertices=len(V), faces=len(F), odd_edges=int((uses % 2 == 1).sum()), oriented=bool(np.array_equal(key(d), key(d[:, ::-1]))),
                components=tr.n_components(len(V), F), euler=tr.euler_characteristic(len(V), F))


def test_from_cloud_with_a_target_gives_a_usable_proxy():
    from gaussianmesh_amd import proxy_mesh as pm
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.deform import SingleObjectDeform
    from gaussianmesh_amd.mesh_bind import bind_points
    r = _e2e()
    N = E2E["target"]
    (Vd, Fd), (V, F), s = r["dense"], r["coarse"], r["simplified"]
    # target_faces=None: bitwise what it was, and no new key in the stats
    again = pm.from_cloud(r["model"], r["cams"], resolution=E2E["resolution"], target_faces=None)
    plain = pm.from_cloud(r["model"], r["cams"], resolution=E2E["resolution"])
    assert torch.equal(again[0], Vd) and torch.equal(again[1], Fd) and torch.equal(plain[0], Vd) and torch.equal(plain[1], Fd)
    assert set(r["stats_dense"]) == {"vertices", "faces", "components", "components_dropped"}
    # from_cloud(target_faces=N) is extract(target_faces=N)
    fc = pm.from_cloud(r["model"], r["cams"], resolution=E2E["resolution"], target_faces=N)
    assert torch.equal(fc[0], V) and torch.equal(fc[1], F)
    v, f, vd, fd = V.cpu().numpy(), F.cpu().numpy(), Vd.cpu().numpy(), Fd.cpu().numpy()
    rep, rep_dense = _report(v, f), _report(vd, fd)
    print("dense:", rep_dense, "simplified:", rep, r["stats"])
    assert len(fd) > 2 * N
    assert r["stats"]["faces_before_simplify"] == len(fd) and r["stats"]["simplify_rounds"] == s.stats["rounds"] > 0
    assert r["stats"]["seconds_simplify"] > 0 and r["stats"]["simplify_reached"] is True and not r["stats"]["simplify_stalled"]
    assert len(f) <= N or s.stats["stalled"]
    assert rep["odd_edges"] == 0 and rep["oriented"] and rep["components"] == 1 and rep["euler"] == 0 == rep_dense["euler"]      # closed, genus 1
    assert tr.signed_volume(v, f) > 0
    kept = s.kept.cpu().numpy()
    assert np.array_equal(_bits(v), _bits(vd[kept])) and (np.diff(kept) > 0).all()             # rows of the unsimplified extraction
    vmap = s.vertex_map.cpu().numpy()
    assert vmap.shape == (len(vd),) and vmap.min() >= 0 and np.array_equal(vmap[kept], np.arange(len(kept)))
    # the whole stage equals the definition on the dense mesh
    ref = sr.simplify_ref(vd, fd, target_faces=N)
    assert np.array_equal(f, ref["faces"]) and np.array_equal(kept, ref["kept"]) and np.array_equal(vmap, ref["vertex_map"])
    # a run that ends above the target says so: a flag and a warning, and the mesh it got to; an extract without a target forgets it
    vol = r["vol"]
    with pytest.warns(RuntimeWarning, match="above target_faces=%d" % N):
        short = vol.extract(target_faces=N, simplify_max_rounds=2)
    assert vol.stats["simplify_reached"] is False and vol.stats["simplify_rounds"] == 2 and N < short[1].shape[0] < len(fd)
    assert vol.simplified.stats["faces"] == short[1].shape[0]
    back = vol.extract()
    assert vol.simplified is None and torch.equal(back[1], Fd) and "simplify_reached" not in vol.stats
    # the cloud binds to it, and a drag solves on it
    cl = r["cl"]
    pts = _dev(cl["means"])
    b = bind_points(pts, V, F)
    assert b["tri"].shape == (len(pts), 3) and np.isfinite(b["weights"]).all() and float(np.sqrt(b["sqr_distance"].max())) < 0.6
    cov = scenes.cov3d_from_scale_rot(cl["scales"], cl["rots"])
    o = SingleObjectDeform(pts, _dev(cov), _dev(cl["opac"]), _dev(cl["shs"]), _dev(b["tri"], torch.int32), _dev(b["weights"]), V)
    ids_dense = np.array([int(np.argmax(vd[:, 0])), int(np.argmin(vd[:, 0])), int(np.argmax(vd[:, 2])), int(np.argmin(vd[:, 2]))])
    ids = np.unique(vmap[ids_dense])                                   # picks on the dense mesh carried over by vertex_map
    assert len(ids) == 4
    o.set_handles(ids, faces=F)
    target = v[ids].copy()
    target[0] += (0.3, 0.4, 0.0)
    pos = o.drag(_dev(target))[0]
    torch.cuda.synchronize()
    moved = o.mesh_vertex_current.cpu().numpy()
    free = np.ones(len(v), bool)
    free[ids] = False
    assert np.isfinite(moved).all() and np.array_equal(moved[ids], target.astype(f32))            # the handles are where they were put
    assert np.abs(moved - v)[free].max() > 0.1                                                    # and the mesh followed the 0.5 drag
    assert torch.isfinite(pos).all() and float((pos - pts).abs().max()) > 0.1


# ---- 5. the CLIs, each in a fresh child process ----
def _child(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m"] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_mesh_simplify_cli(tmp_path):
    from gaussianmesh_amd import io as gio
    V, F = sr.torus(24, 16)
    src, out = str(tmp_path / "in.obj"), str(tmp_path / "out.obj")
    gio.write_obj(src, V, F)
    line = _child(["gaussianmesh_amd.mesh_simplify", "--mesh", src, "--out", out, "--target_faces", "200", "--min_cos", "0.2", "--max_error", "10"])
    ref = sr.simplify_ref(V, F, target_faces=200, min_cos=0.2, max_error=10.0)
    v, f = gio.read_obj(out)
    assert np.array_equal(f, ref["faces"]) and np.array_equal(v, ref["vertices"].astype(np.float64))
    assert (line["faces_before"], line["faces"], line["vertices"], line["rounds"], line["stalled"]) == (768, 200, len(v), ref["rounds"], False)
    assert line["reached"] is True
    assert set(line["seconds"]) == {"load", "simplify", "write"}


def test_proxy_mesh_cli_with_target_faces(tmp_path):
    from gaussianmesh_amd import io as gio
    r = _e2e()
    ply, cj, obj = str(tmp_path / "cloud.ply"), str(tmp_path / "cameras.json"), str(tmp_path / "proxy.obj")
    r["model"].save_ply(ply)
    entries = []
    for k, c in enumerate(r["cams"]):
        Rt = c["view"].T.astype(np.float64)
        entries.append(gio.camera_to_json(k, Rt[:3, :3].T, Rt[:3, 3], c["W"], c["H"], c["fovx"], c["fovy"], "v%d" % k))
    with open(cj, "w") as fh:
        json.dump(entries, fh)
    line = _child(["gaussianmesh_amd.proxy_mesh", "--gaussian", ply, "--cameras", cj, "--out", obj, "--resolution", "48", "--target_faces",
                   str(E2E["target"])])
    v, f = gio.read_obj(obj)
    assert line["vertices"] == len(v) and line["faces"] == len(f) <= E2E["target"] < line["faces_before_simplify"]
    assert line["simplify_rounds"] > 0 and line["boundary_edges"] == 0 and line["simplify_reached"] is True
    assert set(line["seconds"]) == {"load", "render_fuse", "extract", "write", "simplify"} and 0 < line["seconds"]["simplify"] <= line["seconds"]["extract"]
    rep = _report(np.asarray(v, f32), f)
    assert rep["odd_edges"] == 0 and rep["components"] == 1 and rep["euler"] == 0


# ---- 6. C-level refusals leave the outputs alone ----
def test_refusals_touch_nothing():
    from gaussianmesh_amd import _lib
    from gaussianmesh_amd import mesh_simplify as ms
    l = _lib.lib()
    V, F = _mesh("torus_7x5")
    dV, dF = _dev(V), _dev(F, torch.int64)
    edges, uses, off, adj = ms._bookkeeping(dF, len(V))
    F32 = dF.to(torch.int32).contiguous()
    Q = ms.quadrics(dV, F32)
    E, Vm, nF = edges.shape[0], len(V), len(F)
    need = l.gm_mesh_collapse_round_workspace_bytes(Vm)
    for fill in FILLS[1:]:
        with poisoned(fill) as p:
            o = dict(device="cuda")
            sel, frm, to = torch.empty((E,), dtype=torch.uint8, **o), torch.empty((E,), dtype=torch.int32, **o), torch.empty((E,), dtype=torch.int32, **o)
            key, count = torch.empty((E,), dtype=torch.int64, **o), torch.empty((1,), dtype=torch.int32, **o)
            ws = torch.empty((need,), dtype=torch.uint8, **o)
            Qo = torch.empty((Vm, 10), dtype=torch.float32, **o)
            outs = (sel, frm, to, key, count, ws, Qo)
            def call(Vm=Vm, nF=nF, E=E, min_cos=0.2, max_error=float("inf"), ws_bytes=need, **kw):
                a = dict(V=dV.data_ptr(), Q=Q.data_ptr(), faces=F32.data_ptr(), off=off.data_ptr(), adj=adj.data_ptr(), edges=edges.data_ptr(),
                         uses=uses.data_ptr(), sel=sel.data_ptr(), frm=frm.data_ptr(), to=to.data_ptr(), key=key.data_ptr(), count=count.data_ptr(),
                         ws=ws.data_ptr())
                a.update(kw)
                return l.gm_mesh_collapse_round(Vm, a["V"], a["Q"], nF, a["faces"], a["off"], a["adj"], E, a["edges"], a["uses"], min_cos, max_error,
                                                a["sel"], a["frm"], a["to"], a["key"], a["count"], a["ws"], ws_bytes, None)
            assert call(Vm=-1) == 1 and call(nF=-1) == 1 and call(E=-1) == 1
            assert call(min_cos=float("nan")) == 1 and call(min_cos=-1.0) == 1 and call(max_error=float("nan")) == 1 and call(max_error=-1.0) == 1
            for n in ("V", "Q", "faces", "off", "adj", "edges", "uses", "sel", "frm", "to", "key", "count", "ws"):
                assert call(**{n: None}) == 1, n
            assert call(frm=sel.data_ptr()) == 1 and call(to=frm.data_ptr()) == 1 and call(count=key.data_ptr()) == 1       # outputs on each other
            assert call(sel=dV.data_ptr()) == 1 and call(ws=Q.data_ptr()) == 1 and call(key=edges.data_ptr()) == 1           # and on inputs
            assert call(ws_bytes=need - 1) == 3 and call(ws_bytes=0) == 3
            assert call(E=0) == 0                                                                                            # launches nothing
            q = lambda Vm=Vm, nF=nF, **kw: l.gm_mesh_quadrics(Vm, kw.get("V", dV.data_ptr()), nF, kw.get("faces", F32.data_ptr()), off.data_ptr(),
                                                              adj.data_ptr(), kw.get("Q", Qo.data_ptr()), None)
            assert q(Vm=-1) == 1 and q(nF=-1) == 1 and q(V=None) == 1 and q(Q=None) == 1 and q(faces=None) == 1
            assert q(Q=dV.data_ptr()) == 1 and q(Q=F32.data_ptr()) == 1
            assert q(Vm=0) == 0
            torch.cuda.synchronize()
            for t in outs:
                assert bool((t.reshape(-1).view(torch.uint8) == fill).all()), "a refused call wrote to an output"
        assert p.handed_out == 7
