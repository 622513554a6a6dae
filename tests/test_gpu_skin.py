"""-m gpu: gm_skin_weights / gm_skin_pose (skinning.SkinBinding, skinning.skin_vertices) against the float64 reference of
tests/skin_ref.py on the cases of tests/skin_cases.py: the full weights against the dense solve, compaction as a restatement, both
blends, batches, repeatability on poisoned memory, refusals, and the edit surface on top (SingleObjectDeform.attach_skeleton /
pose_sequence, ObjectVisualTool.pose_one_gaussian, render_sequence over the posed meshes, edit_sequence --pose_sequence)."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import skin_cases as sc
import skin_ref
from poison import differing, run_under_fills, same_bits
from test_gpu_arap import _scene64, _tool
from test_gpu_edit_sequence import _gate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIGHT = dict(cg_iterations=2000, cg_tolerance=1e-10)
_made = {}


def _skeleton(name):
    from gaussianmesh_amd.skinning import Skeleton
    return Skeleton(*sc.skeleton(name))


def _binding(mesh, skeleton, keep=4):
    """the tight binding of a case with its full columns, built once"""
    from gaussianmesh_amd.skinning import SkinBinding
    if (mesh, skeleton, keep) not in _made:
        V0, faces = sc.mesh(mesh)
        _made[(mesh, skeleton, keep)] = SkinBinding(V0, faces, _skeleton(skeleton), max_influences=keep, want_full=True, **TIGHT)
    return _made[(mesh, skeleton, keep)]


def _dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


def _ulp(v):
    """one float32 ulp at the largest magnitude of v"""
    return float(np.spacing(np.float32(np.abs(v).max())))


# ---- 1. the full weights against the dense solve ----
@pytest.mark.parametrize("mesh, skeleton", sc.CASES, ids=sc.IDS)
def test_full_weights_against_the_dense_solve(mesh, skeleton):
    """max |w_hip - w_dense| <= 10 x what the numpy restatement of the same PCG (same start, same stopping rule, cg_tolerance 1e-10)
    leaves against the dense solve on this case; the factor covers the summation order of a 1024-thread workgroup.  Largest figures
    seen: INTEGRATION.md section AE."""
    s, want = sc.system(mesh, skeleton), sc.dense(mesh, skeleton)
    restated, _, _ = s.pcg(TIGHT["cg_iterations"], TIGHT["cg_tolerance"])
    figure = float(np.abs(restated - want).max())
    assert figure <= 1e-7
    bound = 10.0 * figure
    b = _binding(mesh, skeleton)
    full, stats = b.full.cpu().numpy(), b.stats.cpu().numpy()
    err = float(np.abs(full - want).max())
    print("%s-%s: max |w_hip - w_dense| = %.3g, the restatement's = %.3g (bound %.3g); CG steps at most %d, residual at most %.3g"
          % (mesh, skeleton, err, figure, bound, int(stats[:, 0].max()), stats[:, 1].max()))
    assert full.shape == want.shape and np.isfinite(full).all() and err <= bound
    assert stats.shape == (s.J, 2) and (stats[:, 1] <= TIGHT["cg_tolerance"]).all()
    assert (stats[:, 0] == np.round(stats[:, 0])).all() and (stats[:, 0] >= 0).all() and (stats[:, 0] <= TIGHT["cg_iterations"]).all()
    assert full.min() >= -bound and full.max() <= 1.0 + bound
    assert np.abs(full.sum(axis=0) - 1.0).max() <= s.J * bound
    assert np.array_equal(full[:, ~s.unknown], s.p[:, ~s.unknown])     # a row that is no unknown keeps p


# ---- 2. compaction is a restatement ----
@pytest.mark.parametrize("keep", [1, 2, 3, 4])
@pytest.mark.parametrize("mesh, skeleton", [("torus_96", "ring5"), ("torus_96", "star17"), ("unreferenced", "ring5"), ("torus_96", "one_bone"),
                                            ("flat_257", "chain3"), ("two_tori", "inside")])
def test_compaction_is_the_rule_applied_to_the_devices_own_columns(mesh, skeleton, keep):
    s = sc.system(mesh, skeleton)
    b = _binding(mesh, skeleton, keep)
    ids, w = skin_ref.compact(b.full.cpu().numpy(), s.unknown, s.near, keep)
    got_ids, got_w = b.bone_ids.cpu().numpy(), b.bone_w.cpu().numpy()
    assert got_ids.dtype == np.int32 and got_w.dtype == np.float32
    assert np.array_equal(got_ids, ids) and np.array_equal(got_w.view(np.uint32), w.view(np.uint32))
    if skeleton == "one_bone":
        assert (got_ids == 0).all() and (got_w == np.array([1, 0, 0, 0], np.float32)).all()
    if mesh == "unreferenced":
        assert (got_ids[-1] == np.nonzero(s.near[:, -1])[0][0]).all() and got_w[-1].tolist() == [1.0, 0.0, 0.0, 0.0]
    if skeleton == "ring5" and keep == 4:
        assert (got_w[s.unknown, 3] > 0).all()                         # five bones, four kept: one is dropped at every unknown row


# ---- 3. the pose against the reference ----
POSED = [("torus_1073", "ring5"), ("torus_96", "star17"), ("flat_257", "chain3"), ("flat_255", "chain3"), ("unreferenced", "ring5"), ("two_tori", "inside")]


@pytest.mark.parametrize("blend", ["linear", "dqs"])
@pytest.mark.parametrize("mesh, skeleton", POSED, ids=["%s-%s" % c for c in POSED])
def test_pose_against_the_reference(mesh, skeleton, blend):
    """both sides compute in float64 from the same float32 inputs and round once: one float32 ulp of the largest coordinate"""
    b = _binding(mesh, skeleton)
    ids, w = b.bone_ids.cpu().numpy(), b.bone_w.cpu().numpy()
    V0 = sc.mesh(mesh)[0]
    for T in (1, 5, 70):
        M = b.skeleton.bone_transforms(*sc.pose(skeleton, T, seed=T))
        got = b.pose(M, blend=blend)
        assert got.shape == (T, len(V0), 3) and got.dtype is torch.float32
        want = skin_ref.blend(V0, ids, w, M, blend)
        err, ulp = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max()), _ulp(want)
        print("%s-%s %s T = %d: max |x_hip - x_ref| = %.3g (one ulp: %.3g)" % (mesh, skeleton, blend, T, err, ulp))
        assert err <= ulp
        assert same_bits(b.pose_skeleton(*sc.pose(skeleton, T, seed=T), blend=blend), got)
    assert float(np.abs(want - V0).max()) > 0.1                        # the poses move the mesh


@pytest.mark.parametrize("blend", ["linear", "dqs"])
def test_identity_and_rigid_poses(blend):
    for mesh, skeleton in (("torus_1073", "ring5"), ("flat_257", "chain3"), ("unreferenced", "ring5")):
        b = _binding(mesh, skeleton)
        V0 = sc.mesh(mesh)[0]
        rest = b.pose_skeleton(np.zeros((2, b.skeleton.Nj, 3)), blend=blend)
        assert same_bits(rest[0], _dev(V0)) and same_bits(rest[1], _dev(V0))
        # the root alone turns: one rigid motion for all bones.  A quarter turn, whose float32 matrix is a rotation to 1e-16 (a general
        # one is a rotation to 6e-8 only, which the unit quaternion of dqs takes out again: the linear blend gets one of those too)
        for turn in ((0.0, math.pi / 2, 0.0),) + (((0.4, -0.9, 0.3),) if blend == "linear" else ()):
            rot = np.zeros((1, b.skeleton.Nj, 3))
            rot[0, 0] = turn
            tr = np.array([[0.3, 0.1, -0.2]])
            M = b.skeleton.bone_transforms(rot, tr)
            assert np.array_equal(M[0], np.broadcast_to(M[0, 0], M[0].shape))
            A, t = M[0, 0, :, :3].astype(np.float64), M[0, 0, :, 3].astype(np.float64)
            want = V0.astype(np.float64) @ A.T + t
            got = b.pose(M, blend=blend)[0].cpu().numpy().astype(np.float64)
            assert float(np.abs(got - want).max()) <= _ulp(want)


def _ring(n=64, radius=0.5, height=0.5):
    a = np.arange(n) * (2 * math.pi / n)
    return np.stack([radius * np.cos(a), np.full(n, height), radius * np.sin(a)], 1).astype(np.float32)


def _about_y(angle, t=(0.0, 0.0, 0.0)):
    c, s = math.cos(angle), math.sin(angle)
    return np.array([[c, 0, s, t[0]], [0, 1, 0, t[1]], [-s, 0, c, t[2]]], np.float32)


def test_a_half_twist_keeps_its_radius_under_dqs_and_collapses_under_linear():
    """a ring of points about the y axis, half owned by a bone that stays and half by one that turns 180 degrees about y"""
    from gaussianmesh_amd.skinning import skin_vertices
    ring = _ring()
    ids = np.tile(np.array([0, 1, 0, 0], np.int32), (len(ring), 1))
    w = np.tile(np.array([0.5, 0.5, 0, 0], np.float32), (len(ring), 1))
    M = np.stack([_about_y(0.0), _about_y(math.pi)], 0)[None]
    M[np.abs(M) < 1e-6] = 0.0                                          # (cos pi, sin pi exactly)
    radius = lambda x: np.hypot(x[:, 0], x[:, 2])
    dqs = skin_vertices(_dev(ring), ids, w, M, "dqs")[0].cpu().numpy().astype(np.float64)
    lin = skin_vertices(_dev(ring), ids, w, M, "linear")[0].cpu().numpy().astype(np.float64)
    assert np.abs(radius(dqs) - 0.5).max() <= 1e-6 and np.abs(dqs[:, 1] - 0.5).max() <= 1e-6
    assert radius(lin).max() <= 1e-6 and np.abs(lin[:, 1] - 0.5).max() <= 1e-6
    for kind, got in (("dqs", dqs), ("linear", lin)):
        assert float(np.abs(got - skin_ref.blend(ring, ids, w, M, kind)[0]).max()) <= _ulp(ring)


def test_antipodal_quaternions_take_the_short_way():
    """+170 and -170 degrees about y: the quaternions with w >= 0 have a negative dot product, so the second is negated and the blend is
    the half turn between them (the short way, 20 degrees apart) - without the rule it would be the identity"""
    from gaussianmesh_amd.skinning import skin_vertices
    ring = _ring(height=-0.3)
    ids = np.tile(np.array([0, 1, 0, 0], np.int32), (len(ring), 1))
    w = np.tile(np.array([0.5, 0.5, 0, 0], np.float32), (len(ring), 1))
    M = np.stack([_about_y(math.radians(170.0), (0.1, 0.2, 0.3)), _about_y(math.radians(-170.0), (0.1, 0.2, 0.3))], 0)[None]
    got = skin_vertices(_dev(ring), ids, w, M, "dqs")[0].cpu().numpy().astype(np.float64)
    want = skin_ref.blend_dqs(ring, ids, w, M)[0]
    assert float(np.abs(got - want).max()) <= _ulp(want)
    half = ring.astype(np.float64) * [-1, 1, -1]                       # the half turn about y; the translation: both bones' t turned alike
    moved = got - half
    assert np.abs(moved - moved[0]).max() <= 1e-6 and np.abs(got - ring).max() > 0.5


# ---- 4. batches and memory ----
@pytest.mark.parametrize("blend", ["linear", "dqs"])
def test_a_frame_does_not_depend_on_its_batch(blend):
    b = _binding("torus_1073", "ring5")
    M = b.skeleton.bone_transforms(*sc.pose("ring5", 70, seed=7))
    full = b.pose(M, blend=blend)
    single = torch.stack([b.pose(M[t:t + 1], blend=blend)[0] for t in range(70)], 0)
    assert same_bits(full, single) and not same_bits(single[20], single[21])
    pick = [3, 60, 3, 17, 0, 69]
    assert same_bits(b.pose(M[pick], blend=blend), single[pick])
    assert same_bits(b.pose(M[::-1].copy(), blend=blend), single.flip(0))
    big = torch.full((72, 1073, 3), 7.0, device="cuda")
    got = b.pose(M, blend=blend, out=big[1:71])
    assert got.data_ptr() == big[1].data_ptr() and same_bits(got, single) and bool((big[0] == 7.0).all()) and bool((big[71] == 7.0).all())


@pytest.mark.parametrize("mesh, skeleton", [("torus_1073", "ring5"), ("unreferenced", "ring5"), ("flat_257", "chain3"), ("torus_96", "star17")])
def test_same_bits_from_call_to_call_and_on_poisoned_memory(mesh, skeleton):
    """two runs give the same bits; so do runs whose every allocation (ids, weights, columns, stats, the workspace, the meshes) was filled
    with 0x00, 0xFF and 0x5A beforehand, and no guard band around any of them is touched"""
    from gaussianmesh_amd.skinning import SkinBinding
    V0, faces = sc.mesh(mesh)
    skel = _skeleton(skeleton)
    M = skel.bone_transforms(*sc.pose(skeleton, 3, seed=3))

    def route():
        b = SkinBinding(V0, faces, skel, want_full=True)
        return b.bone_ids, b.bone_w, b.full, b.stats, b.pose(M, blend="dqs"), b.pose(M, blend="linear")
    first = route()
    assert same_bits(first, route())
    runs = run_under_fills(route)
    assert all(r[0].handed_out >= 7 for r in runs)
    assert differing(runs) == [] and same_bits(runs[0][1], first)


# ---- 5. refusals ----
def test_python_refusals_launch_nothing():
    from gaussianmesh_amd import _lib
    from gaussianmesh_amd.skinning import SkinBinding, Skeleton, skin_vertices
    V0, faces = sc.mesh("torus_96")
    skel = _skeleton("ring5")
    for kw in (dict(heat=0.0), dict(heat=float("nan")), dict(heat=True), dict(max_influences=0), dict(max_influences=5), dict(max_influences=2.0)):
        with pytest.raises(ValueError, match="SkinBinding"):
            SkinBinding(V0, faces, skel, **kw)
    with pytest.raises(ValueError, match="skeleton"):
        SkinBinding(V0, faces, sc.skeleton("ring5"))
    with pytest.raises(_lib.GmeshError):
        SkinBinding(V0, faces, skel, device="cpu")
    for kw, what in ((dict(cg_iterations=0), "cg_iterations"), (dict(cg_tolerance=-1.0), "cg_tolerance"), (dict(cg_tolerance=float("nan")), "cg_tolerance")):
        with pytest.raises(_lib.GmeshError, match=what):
            SkinBinding(V0, faces, skel, **kw)
    b = _binding("torus_96", "ring5")
    good = skel.bone_transforms(*sc.pose("ring5", 2))
    out = torch.full((2, 96, 3), 5.0, device="cuda")
    scaled = good.copy()
    scaled[1, 3, :, :3] *= 1.001
    mirrored = good.copy()
    mirrored[0, 2, 0, :3] *= -1.0
    for bad in (scaled, mirrored):
        with pytest.raises(ValueError, match="frame %d, bone %d" % ((1, 3) if bad is scaled else (0, 2))):
            b.pose(bad, blend="dqs", out=out)
    for bad in (good[:, :4], good[:, :, :, :3], good.astype(np.int32), good[:0], np.full_like(good, np.nan)):
        with pytest.raises(ValueError, match="transforms"):
            b.pose(bad, blend="linear", out=out)
    with pytest.raises(ValueError, match="blend"):
        b.pose(good, blend="cubic", out=out)
    for bad_out in (out[:1], out.double(), out.cpu(), torch.empty((2, 3, 96), device="cuda").transpose(1, 2)):
        with pytest.raises(ValueError, match="out"):
            b.pose(good, out=bad_out)
    rest, ids, w = b.rest, b.bone_ids, b.bone_w
    for args in ((rest, ids[:50], w, good), (rest, ids.float(), w, good), (rest, ids, w.int(), good), (rest, ids, w[:, :3], good),
                 (rest, ids + 5, w, good), (rest, ids - 1, w, good), (rest[:, :2], ids, w, good), (rest, ids, w, good[0])):
        with pytest.raises(ValueError, match="skin_vertices"):
            skin_vertices(*args)
    with pytest.raises(_lib.GmeshError):
        skin_vertices(rest.cpu(), ids, w, good)
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    assert float((b.pose(scaled, blend="linear") - b.pose(good, blend="linear")).abs().max()) > 0     # linear takes what dqs refuses


def test_c_refusals_launch_nothing():
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    size = l.gm_skin_weights_workspace_bytes
    assert size(0, 5) == 0 and size(96, 0) == 0 and size(96, 257) == 0 and size(-1, 5) == 0
    assert 0 < size(96, 1) < size(96, 2) < size(97, 2) < size(7500, 256) and size(96, 5) >= 5 * 96 * 33
    b = _binding("torus_96", "ring5")
    g = b.mesh
    V0, faces = sc.mesh("torus_96")
    from gaussianmesh_amd.dynamics import vertex_masses
    area = _dev(vertex_masses(V0, faces, 1.0), torch.float64)
    a, e = (_dev(x) for x in b.skeleton.bones)
    ids = torch.full((96, 4), -7, dtype=torch.int32, device="cuda")
    w = torch.full((96, 4), 5.0, device="cuda")
    full = torch.full((5, 96), 5.0, dtype=torch.float64, device="cuda")
    stats = torch.full((5, 2), -3.0, dtype=torch.float64, device="cuda")
    ws = torch.empty((size(96, 5),), dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def weights(Vm=96, J=5, heat=1.0, cg=2000, tol=1e-10, keep=4, nbytes=None, **kw):
        t = dict(off=g.off, cols=g.cols, w=g.w, V0=g.rest, area=area, a=a, b=e, ids=ids, ow=w, full=full, stats=stats, ws=ws)
        t.update(kw)
        q = {k: (v.data_ptr() if torch.is_tensor(v) else v) for k, v in t.items()}
        return l.gm_skin_weights(Vm, J, q["off"], q["cols"], q["w"], q["V0"], q["area"], q["a"], q["b"], heat, cg, tol, keep, q["ids"], q["ow"],
                                 q["full"], q["stats"], q["ws"], ws.numel() if nbytes is None else nbytes, stream)
    for kw, rc in ((dict(Vm=0), 1), (dict(J=0), 1), (dict(J=257), 1), (dict(heat=0.0), 1), (dict(heat=float("inf")), 1), (dict(cg=0), 1),
                   (dict(tol=-1.0), 1), (dict(keep=0), 1), (dict(keep=5), 1), (dict(area=None), 1), (dict(a=None), 1), (dict(ids=None), 1),
                   (dict(ow=None), 1), (dict(ws=None), 1), (dict(ow=ids), 1), (dict(full=stats), 1), (dict(ws=full), 1), (dict(ids=g.rest), 1),
                   (dict(nbytes=size(96, 5) - 1), 3), (dict(nbytes=0), 3)):
        assert weights(**kw) == rc and b"gm_skin_weights" in l.gm_last_error(), (kw, l.gm_last_error())
    out = torch.full((2, 96, 3), 5.0, device="cuda")
    M = _dev(b.skeleton.bone_transforms(*sc.pose("ring5", 2)))

    def pose(T=2, Vm=96, J=5, blend=1, **kw):
        t = dict(V0=g.rest, ids=b.bone_ids, w=b.bone_w, M=M, out=out)
        t.update(kw)
        q = {k: (v.data_ptr() if torch.is_tensor(v) else v) for k, v in t.items()}
        return l.gm_skin_pose(T, Vm, J, q["V0"], q["ids"], q["w"], q["M"], blend, q["out"], stream)
    for kw in (dict(T=0), dict(Vm=0), dict(J=0), dict(J=257), dict(blend=2), dict(blend=-1), dict(V0=None), dict(ids=None), dict(w=None), dict(M=None),
               dict(out=None), dict(out=g.rest), dict(out=M), dict(out=b.bone_w)):
        assert pose(**kw) == 1 and b"gm_skin_pose" in l.gm_last_error(), (kw, l.gm_last_error())
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((ids == -7).all()) and bool((w == 5.0).all()) and bool((full == 5.0).all()) and bool((stats == -3.0).all())
    assert weights() == 0 and pose() == 0                              # and the same calls, unrefused, write everything
    torch.cuda.synchronize()
    assert same_bits((ids, w, full, stats), (b.bone_ids, b.bone_w, b.full, b.stats)) and same_bits(out, b.pose(M, blend="dqs"))
    assert weights(full=None, stats=None) == 0                         # both are optional
    torch.cuda.synchronize()
    assert same_bits((ids, w), (b.bone_ids, b.bone_w))


# ---- 6. the edit surface ----
def _scene_skeleton(verts):
    """five bones round the centre circle of the scene's torus, and three poses of them"""
    from gaussianmesh_amd.skinning import Skeleton
    V = np.asarray(verts, np.float64)
    radius = float(np.hypot(V[:, 0], V[:, 2]).mean())
    ang = 0.2 + np.arange(6) * (2 * math.pi / 6)
    skel = Skeleton(np.stack([radius * np.cos(ang), np.full(6, 0.02), radius * np.sin(ang)], 1), [-1, 0, 1, 2, 3, 4])
    rng = np.random.default_rng(11)
    return skel, rng.uniform(-0.4, 0.4, (3, 6, 3)), rng.uniform(-0.2, 0.2, (3, 3))


def test_pose_sequence_is_the_binding_and_leaves_the_object_at_the_last_pose(tmp_path):
    from gaussianmesh_amd.deform import SingleObjectDeform as TensorObject
    from gaussianmesh_amd.skinning import SkinBinding
    d = str(tmp_path)
    _scene64(d)
    tool, other = _tool(d), _tool(d)
    o, q = tool.gaussians_list[0], other.gaussians_list[0]
    skel, rot, tr = _scene_skeleton(o.vertex.cpu().numpy())
    with pytest.raises(ValueError, match="attach_skeleton"):
        o.pose_sequence(rot, tr)
    binding = o.attach_skeleton(skel)
    assert isinstance(binding, SkinBinding) and o.attach_skeleton(skel) is binding and binding.mesh is o.mesh_graph
    assert o.attach_skeleton(skel, max_influences=2) is not binding
    o.attach_skeleton(skel)
    want = SkinBinding(o.vertex, o.faces, skel).pose_skeleton(rot, tr)
    got = o.pose_sequence(rot, tr)
    assert got.shape == (3, o.vertex.shape[0], 3) and same_bits(got, want)
    assert torch.equal(o.mesh_vertex_current, want[-1])
    exp = q.deform_vertices(want[-1])
    assert all(torch.equal(g, e) for g, e in zip(o.deform_vertices(o.mesh_vertex_current), exp))
    assert all(torch.equal(g, e) for g, e in zip(o.pose(rot[1], tr[1], blend="linear"), q.deform_vertices(SkinBinding(o.vertex, o.faces, skel).pose_skeleton(rot[1:2], tr[1:2], blend="linear")[0])))
    third = _tool(d)
    assert third.pose_one_gaussian("Nobody", rot, tr, skeleton=skel) is None
    assert same_bits(third.pose_one_gaussian("Object", rot, tr, skeleton=skel), want)
    assert same_bits(third.pose_one_gaussian("Object", rot[:2], blend="linear"), SkinBinding(o.vertex, o.faces, skel).pose_skeleton(rot[:2], blend="linear"))
    t = TensorObject(o.gaussian_pos, o.gaussian_cov, o.gaussian_o, o.gaussian_feature, o.gaussian_triangles, o.coord, o.vertex, name="T")
    with pytest.raises(ValueError, match="no faces"):
        t.attach_skeleton(skel)
    t.attach_skeleton(skel, faces=o.faces.cpu().numpy())
    assert same_bits(t.pose_sequence(rot, tr), want)


def test_render_sequence_over_the_posed_meshes(tmp_path):
    d = str(tmp_path)
    _scene64(d)
    tool, ref_tool = _tool(d), _tool(d)
    o = tool.gaussians_list[0]
    skel, rot, tr = _scene_skeleton(o.vertex.cpu().numpy())
    o.attach_skeleton(skel)
    meshes = o.pose_sequence(rot, tr)
    cams = tool.get_camera(d)
    got = list(tool.render_sequence([(cams[k % 3], {"Object": meshes[k]}) for k in range(3)], frames_per_launch=4))
    assert len(got) == 3
    for k in range(3):
        ref_tool.gaussians_list[0].deform_vertices(meshes[k])
        assert got[k].shape == (3, 64, 64)
        _gate(got[k], ref_tool.render_gaussian(cams[k % 3]), "frame %d vs deform_vertices + render_gaussian" % k)
        assert float((got[k] - 1.0).abs().max()) > 0.1                 # the object is in the picture


def _cli(d, out, *source):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "gaussianmesh_amd.edit_sequence", "--object_gaussian", os.path.join(d, "object.ply"),
                        "--object_origin_mesh", os.path.join(d, "rest.obj"), "--camera_path", d, "--render_path", out, "--save_meshes"] + list(source),
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]


def test_cli_pose_sequence_writes_the_posed_meshes(tmp_path):
    from gaussianmesh_amd import io as gio
    from gaussianmesh_amd.skinning import SkinBinding
    d = str(tmp_path)
    _scene64(d)
    verts, faces = gio.read_obj(os.path.join(d, "rest.obj"))
    skel, rot, tr = _scene_skeleton(verts)
    skel.write(os.path.join(d, "skeleton.json"))
    json.dump({"rotations": rot.tolist(), "root_translation": tr.tolist()}, open(os.path.join(d, "pose.json"), "w"))
    out = os.path.join(d, "renders")
    _cli(d, out, "--pose_sequence", os.path.join(d, "pose.json"), "--skeleton", os.path.join(d, "skeleton.json"), "--skin_blend", "linear",
         "--skin_influences", "3", "--skin_heat", "1.5")
    back = type(skel).read(os.path.join(d, "skeleton.json"))
    want = SkinBinding(verts.astype(np.float32), faces, back, heat=1.5, max_influences=3).pose_skeleton(rot, tr, blend="linear").cpu().numpy().astype(np.float64)
    assert sorted(os.listdir(out)) == ["%05d.%s" % (k, e) for k in range(3) for e in ("obj", "png")]
    for k in range(3):
        v, f = gio.read_obj(os.path.join(out, "%05d.obj" % k))
        assert np.array_equal(f, faces) and np.array_equal(v, want[k]), k
        assert os.path.getsize(os.path.join(out, "%05d.png" % k)) > 100


def test_cli_without_the_new_flags_is_byte_for_byte_what_it_was(tmp_path):
    """two invocations over a folder of meshes, the second naming the old flags' defaults: the same files, byte for byte (the pose path
    is entered only behind --pose_sequence)"""
    from gaussianmesh_amd import io as gio
    d = str(tmp_path)
    _scene64(d)
    verts, faces = gio.read_obj(os.path.join(d, "rest.obj"))
    seq = os.path.join(d, "seq")
    os.makedirs(seq)
    for k in range(2):
        gio.write_obj(os.path.join(seq, "%d.obj" % (k + 1)), verts + [0.0, 0.1 * (k + 1), 0.0], faces)
    plain, zero = os.path.join(d, "plain"), os.path.join(d, "zero")
    _cli(d, plain, "--mesh_sequence", seq)
    _cli(d, zero, "--mesh_sequence", seq, "--inbetweens", "0", "--arap_batch", "1")
    names = sorted(os.listdir(plain))
    assert names == sorted(os.listdir(zero)) == ["%05d.%s" % (k, e) for k in range(2) for e in ("obj", "png")]
    for n in names:
        assert open(os.path.join(plain, n), "rb").read() == open(os.path.join(zero, n), "rb").read(), n
