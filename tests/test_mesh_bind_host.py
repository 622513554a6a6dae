"""Host side of binding a plain Gaussian cloud to a proxy mesh: gm_closest_face's declaration, typing and refusals (before any GPU
work), the Python refusals, bind_points on given faces against the lines of edittool.load_mesh it restates, and the float32 brute force
of tests/closest_ref.py - the definition the device is held to in test_gpu_mesh_bind.py - against the project's float64 host search."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from gaussianmesh_amd import _lib, edittool, scenes
from gaussianmesh_amd.deform import barycentric_weights

import closest_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_args(name, ret="int"):
    text = open(os.path.join(ROOT, "include", "gmesh_hip.h")).read()
    m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, name), text)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name, ret, n", [("gm_closest_face", "int", 12), ("gm_closest_face_workspace_bytes", "size_t", 2)])
def test_header_declares_and_lib_types_the_entry_points(name, ret, n):
    assert name in _lib.header_symbols()
    assert len(_declared_args(name, ret)) == n
    assert len(_lib.SIGNATURES[name][1]) == n
    assert hasattr(_lib.lib(), name)


def test_abi_version_unchanged():
    assert _lib.lib().gm_abi_version() == 3
    assert "#define GM_ABI_VERSION 3" in open(os.path.join(ROOT, "include", "gmesh_hip.h")).read()


def test_closest_face_refuses_before_any_gpu_work():
    l = _lib.lib()
    a = 1 << 24                                               # a non-null "pointer": never dereferenced, every call is refused first
    big = 1 << 30
    call = lambda N=10, P=a, Vm=8, V=a, F=5, T=a, d2=a, face=a, close=a, ws=a, nbytes=big: l.gm_closest_face(N, P, Vm, V, F, T, d2, face, close, ws, nbytes, None)
    for kw in (dict(N=-1), dict(Vm=-1), dict(F=-1)):
        assert call(**kw) == 1 and b"negative" in l.gm_last_error(), kw
    assert call(F=0) == 1 and b"F == 0" in l.gm_last_error()
    assert call(Vm=0) == 1 and b"Vm == 0" in l.gm_last_error()
    for kw in (dict(P=None), dict(V=None), dict(T=None), dict(d2=None), dict(face=None), dict(ws=None)):
        assert call(**kw) == 1 and b"null" in l.gm_last_error(), kw
    need = l.gm_closest_face_workspace_bytes(10, 5)
    assert need > 0
    assert call(nbytes=need - 1) == 3 and b"workspace" in l.gm_last_error()
    assert l.gm_closest_face(0, None, 0, None, 0, None, None, None, None, None, 0, None) == 0          # N == 0: nothing to do, nothing launched


def test_workspace_bytes_are_monotonic_in_both_sizes():
    l = _lib.lib()
    sizes = [1, 2, 63, 64, 65, 4095, 4096, 4097, 100000, 1000000, (3 << 19) - 1, 3 << 19, (3 << 19) + 1, 2000000, (4 << 20) - 1, 4 << 20, (4 << 20) + 1, 6000000]
    for fixed in (1, 15000, 1600000, 5000000):
        in_n = [l.gm_closest_face_workspace_bytes(n, fixed) for n in sizes]
        in_f = [l.gm_closest_face_workspace_bytes(fixed, f) for f in sizes]
        assert in_n == sorted(in_n) and in_f == sorted(in_f), fixed
    assert l.gm_closest_face_workspace_bytes(0, 0) == l.gm_closest_face_workspace_bytes(1, 1) > 0


def test_the_kernel_file_waits_for_nothing_and_allocates_nothing():
    """gm_closest_face's "no host synchronisation, no device allocation": its translation unit names no such runtime call"""
    text = open(os.path.join(ROOT, "gaussianmesh_amd", "csrc", "gm_closest.hip")).read()
    assert "gm_closest.hip" in open(os.path.join(ROOT, "gaussianmesh_amd", "csrc", "Makefile")).read()
    hits = re.findall(r"hipMemcpy\w*|hip\w*Synchronize|hipMalloc\w*|hipFree\w*|GM_LAUNCH_CHECK", text)
    assert not hits, hits
    assert "#pragma clang fp contract(off)" in text


def _small_mesh():
    verts, faces = scenes.torus_mesh(8, 6)
    return verts.astype(np.float32), faces


def test_python_refusals():
    from gaussianmesh_amd.mesh_bind import bind_points, closest_faces
    verts, faces = _small_mesh()
    pts = torch.zeros((4, 3))
    with pytest.raises(_lib.GmeshError, match="no CPU path"):
        closest_faces(pts, verts, faces)                                               # CPU tensors: no CPU path
    with pytest.raises(_lib.GmeshError, match="no CPU path"):
        bind_points(pts, verts, faces)
    with pytest.raises(_lib.GmeshError, match="no CPU path"):
        bind_points(pts.numpy(), verts, faces)
    with pytest.raises(ValueError, match=r"\[N,3\]"):
        closest_faces(torch.zeros((4, 2)), verts, faces)
    with pytest.raises(ValueError, match=r"\[N,3\]"):
        bind_points(torch.zeros((4, 2)), verts, faces, face_id=np.zeros(4, np.int64))
    with pytest.raises(ValueError, match=r"\[Vm,3\]"):
        closest_faces(pts, verts[:, :2], faces)
    with pytest.raises(ValueError, match=r"\[F,3\]"):
        closest_faces(pts, verts, faces[:, :2])
    bad = faces.copy(); bad[3, 1] = len(verts)
    for fn in (closest_faces, bind_points):
        with pytest.raises(ValueError, match="face index outside"):
            fn(pts, verts, bad)
        neg = faces.copy(); neg[0, 0] = -1
        with pytest.raises(ValueError, match="face index outside"):
            fn(pts, verts, neg)
    with pytest.raises(ValueError, match="integer"):
        closest_faces(pts, verts, faces.astype(np.float32))
    with pytest.raises(ValueError, match="empty"):
        closest_faces(pts, verts, faces[:0])
    with pytest.raises(ValueError, match="one entry per point"):
        bind_points(pts, verts, faces, face_id=np.zeros(3, np.int64))
    with pytest.raises(ValueError, match="face_id outside"):
        bind_points(pts, verts, faces, face_id=np.full(4, len(faces), np.int64))


def test_from_plain_refuses_a_cpu_device(tmp_path):
    with pytest.raises(_lib.GmeshError, match="no CPU path"):
        edittool.SingleObjectDeform.from_plain(str(tmp_path / "missing.ply"), str(tmp_path / "missing.obj"), device="cpu")
    assert hasattr(edittool.ObjectVisualTool, "add_plain_gaussian") and hasattr(edittool.SceneVisualTool, "add_plain_gaussian")


def test_bind_points_on_given_faces_restates_load_mesh():
    """bind_points(..., face_id=given) = the no-face-id branch of edittool.load_mesh (normals, bias, distance, intersection, barycentric
    weights) on those faces, number for number: the same numpy expressions give the same bits."""
    from gaussianmesh_amd.mesh_bind import bind_points
    rng = np.random.default_rng(3)
    vertex, triangles = scenes.torus_mesh(12, 9)
    pos = cr.near_surface(vertex, triangles, 500, rng)
    index_tri = rng.integers(len(triangles), size=500)
    # edittool.load_mesh, the branch `if self.index_tri is None`, with index_tri given
    normals = np.cross(vertex[triangles[:, 1]] - vertex[triangles[:, 0]], vertex[triangles[:, 2]] - vertex[triangles[:, 0]])
    normals /= np.linalg.norm(normals, axis=1)[:, None]
    bias = -(vertex[triangles[:, 0]] * normals).sum(axis=1)
    gpos = pos.astype(np.float64)
    n_g, b_g = normals[index_tri], bias[index_tri]
    distance = -((n_g * gpos).sum(axis=1) + b_g)
    intersection = gpos + distance[:, None] * n_g
    tri = triangles[index_tri]
    coord = barycentric_weights(intersection, vertex[tri[:, 0]], vertex[tri[:, 1]], vertex[tri[:, 2]])
    for points in (torch.from_numpy(pos), pos):
        b = bind_points(points, vertex, triangles, face_id=index_tri)
        assert b["weights"].dtype == np.float32 and b["tri"].dtype == np.int32 and b["face_id"].dtype == np.int64
        assert np.array_equal(b["face_id"], index_tri) and np.array_equal(b["tri"], tri)
        assert np.array_equal(b["weights"].view(np.uint32), coord.astype(np.float32).view(np.uint32))
        assert b["sqr_distance"].shape == (500,) and np.isnan(b["sqr_distance"]).all()            # no search was made
    assert np.abs(coord.sum(axis=1) - 1).max() < 1e-12


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "gaussianmesh_amd.edit_sequence", "--object_origin_mesh", "m.obj", "--camera_path", ".",
                           "--render_path", "out", "--mesh_sequence", "seq"] + list(args), cwd=ROOT, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=300)


def test_cli_wants_exactly_one_kind_of_object_file():
    r = _cli()
    assert r.returncode == 2 and "--object_gaussian" in r.stdout and "--object_plain_gaussian" in r.stdout, r.stdout[-2000:]
    r = _cli("--object_gaussian", "o.ply", "--object_plain_gaussian", "p.ply")
    assert r.returncode == 2 and "not allowed with" in r.stdout, r.stdout[-2000:]


# ---- the float32 definition against the float64 host search ----
C_MEASURED = 0.508            # largest excess of the helper on the inputs below, in units of 2^-24 ext (the far-away family; per family:
C_GATE = 4 * C_MEASURED       # near 0.003, on 0, ball 0.112, far 0.508, shifted 0.282); the gate: four times that


def query_families(n=2000, seed=0):
    """(faces, [(name, vertices float32, points float32)]): torus_mesh(40, 30) and the five query families"""
    rng = np.random.default_rng(seed)
    verts, faces = scenes.torus_mesh(40, 30)
    verts = verts.astype(np.float32)
    ball = rng.normal(0, 2.0, size=(n, 3)).astype(np.float32)
    fams = [("near", verts, cr.near_surface(verts, faces, n, rng)), ("on", verts, cr.near_surface(verts, faces, n, rng, sigma=0.0)),
            ("ball", verts, ball), ("far", verts, (ball * np.float32(150)).astype(np.float32)),
            ("shifted", (verts + np.float32(1000)).astype(np.float32), (cr.near_surface(verts, faces, n, rng) + np.float32(1000)).astype(np.float32))]
    return faces, fams


def _distance64_to(P, V, F, k):
    """float64 distance of every point to the one face k names (edittool's own function, a face at a time)"""
    out = np.empty(len(P))
    for f in np.unique(k):
        rows = np.nonzero(k == f)[0]
        out[rows] = edittool.point_mesh_squared_distance(P[rows], V, F[f:f + 1])[0]
    return np.sqrt(out)


def test_float32_definition_against_the_float64_host_search():
    """tests/closest_ref.py (float32, the arithmetic of include/gmesh_hip.h) against edittool.point_mesh_squared_distance (float64) on the
    same float32-representable inputs: scenes.torus_mesh(40, 30), 2 000 points per family - within N(0, 0.05) of the surface, on the
    surface, a Gaussian ball of sigma 2, that ball x 150, mesh and near-surface points shifted by +1000.
    (i) near the surface the face differs from the float64 one for at most 0.5 % of the points (a foot on a shared edge; measured 1 of
        2 000).  The other families hold genuine ties by the hundred and get no index check.
    (ii) everywhere the float64 distance to the face the helper chose exceeds the float64 minimum by at most C_GATE 2^-24 ext, ext =
        max |vertex coordinate| + max |point coordinate|.  Measured largest excess: 0.508 (x 2^-24 ext; per family 0.003 / 0 / 0.112 /
        0.508 / 0.282); the gate is four times that, 2.032: rounding excess scales with ext, the factor covers other seeds."""
    faces, fams = query_families()
    worst = {}
    for name, V, P in fams:
        d2, k, q = cr.closest_face_ref(P, V, faces)
        assert d2.dtype == np.float32 and (k >= 0).all()
        s64, k64, _ = edittool.point_mesh_squared_distance(P.astype(np.float64), V.astype(np.float64), faces)
        if name == "near":
            differ = int((k != k64).sum())
            print("near-surface: %d of %d faces differ from the float64 search" % (differ, len(k)))
            assert differ <= 0.005 * len(k), differ
        ext = float(np.abs(V).max() + np.abs(P).max())
        excess = _distance64_to(P.astype(np.float64), V.astype(np.float64), faces, k) - np.sqrt(s64)
        worst[name] = float(excess.max() / (2.0 ** -24 * ext))
        # the helper's d2 is the float32 value of the distance to the face it chose, and q lies at that distance
        assert np.allclose(np.sqrt(d2.astype(np.float64)), np.sqrt(s64) + excess, rtol=0, atol=64 * 2.0 ** -24 * ext)
        assert np.array_equal(cr.distance_to_face(P, V, faces, k).view(np.uint32), d2.view(np.uint32))
    print("largest excess per family, in 2^-24 ext:", {n: round(c, 3) for n, c in worst.items()})
    assert max(worst.values()) <= C_GATE, worst
    assert min(worst.values()) >= 0.0


def test_helper_on_degenerate_faces_and_ties():
    """NaN never wins, ties go to the lowest index, no usable face gives (-1, +inf, NaN)"""
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 2]], np.float32)
    tri = np.array([0, 1, 2])
    F = np.array([[3, 3, 3], [0, 0, 1], tri, tri, [0, 2, 1]])           # three equal vertices, no area, a face twice, the same face reversed
    P = np.array([[0.25, 0.25, 1.0], [5, 5, 5]], np.float32)
    d2, k, q = cr.closest_face_ref(P, V, F)
    assert k[0] == 2 and d2[0] == 1.0 and np.array_equal(q[0], np.array([0.25, 0.25, 0], np.float32))
    d2, k, q = cr.closest_face_ref(P, V, F[1:2])                          # only the face without area (a = b): for the first point the edge ab
    assert k[0] == -1 and np.isinf(d2[0]) and np.isnan(q[0]).all()        # branch holds with d1 = d3 = 0, so t_ab = 0 / 0; the second is
    assert k[1] == 0 and d2[1] == 66.0                                    # closest to vertex c = (1, 0, 0), a branch without a division
    d2, k, q = cr.closest_face_ref(P, V, F[:1])                           # three equal vertices: every d is 0, the vertex a branch holds
    assert (k == 0).all() and d2[1] == 27.0
