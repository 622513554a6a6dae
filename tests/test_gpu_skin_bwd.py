"""-m gpu: gm_skin_pose_bwd and what stands on it (INTEGRATION.md section AF) - the gradient against autograd through the float64
restatement of tests/skin_bwd_ref.py, painted weights at the wave's edge and on all four Shepperd branches, frame independence,
repeatability on poisoned memory, the autograd wiring (skin_pose_differentiable, Skeleton.bone_transforms_torch, checked=), the C
refusals, inverse kinematics (SkinBinding.solve_ik, drag_skeleton) and the fit of a skeleton's pose to three views
(pose_fit.SkeletonPoseFitter).
THE BOUND of every gradient comparison: |g_hip - g_ref| <= 2^-30 max |g_ref| per frame.  Both sides are float64 from the same float32
inputs and differ by summation order: at most 4 x 1073 terms at u = 2^-53 whose absolute sum was at most 10.4 max |g_ref| on these
cases (the linear blend), about 2^-38; 2^-30 leaves 2^8 for the dqs chain through the normalisations."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import skin_bwd_ref as ref
import skin_cases as sc
from poison import differing, run_under_fills, same_bits
from test_gpu_skin import _binding, _dev, _scene_skeleton

pytestmark = pytest.mark.gpu
BOUND = 2.0 ** -30
CASES = [("torus_1073", "ring5"), ("torus_96", "star17"), ("flat_255", "chain3"), ("flat_256", "chain3"), ("flat_257", "chain3"),
         ("unreferenced", "ring5"), ("two_tori", "inside"), ("torus_96", "one_bone")]


def _g_out(T, Vm):
    return np.random.default_rng(7).standard_normal((T, Vm, 3)).astype(np.float32)


def _bwd(rest, ids, w, M, g_out, blend, incidence=None):
    """gm_skin_pose_bwd on device tensors -> float64 [T,J,3,4]"""
    from gaussianmesh_amd.skinning import BLENDS, _pose_bwd, bone_incidence
    M = _dev(M)
    return _pose_bwd(rest, ids, w, M, BLENDS.index(blend), _dev(g_out), incidence or bone_incidence(ids, w, M.shape[1]))


def _compare(what, got, want):
    """the bound, frame by frame; returns the largest |g_hip - g_ref| / max |g_ref|"""
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float64 and np.isfinite(got).all()
    worst = 0.0
    for t in range(len(want)):
        scale = float(np.abs(want[t]).max())
        err = float(np.abs(got[t] - want[t]).max())
        worst = max(worst, err / scale)
        assert scale > 0 and err <= BOUND * scale, "%s frame %d: |g_hip - g_ref| = %.3g, bound %.3g" % (what, t, err, BOUND * scale)
    print("%s: max |g_hip - g_ref| / max |g_ref| = %.3g = 2^%.1f (bound 2^-30)" % (what, worst, math.log2(worst) if worst else -math.inf))
    return worst


# ---- 1. the gradient against the reference ----
@pytest.mark.parametrize("blend", ["linear", "dqs"])
@pytest.mark.parametrize("mesh, skeleton", CASES, ids=["%s-%s" % c for c in CASES])
def test_gradient_against_the_reference(mesh, skeleton, blend):
    b = _binding(mesh, skeleton)
    ids, w = b.bone_ids.cpu().numpy(), b.bone_w.cpu().numpy()
    V0 = sc.mesh(mesh)[0]
    for T in (1, 5):
        M = b.skeleton.bone_transforms(*sc.pose(skeleton, T, seed=T))
        ref.check_gradient_position(V0, ids, w, M)                     # the device's own weights, too, sit away from every decision
        g = _g_out(T, len(V0))
        got = _bwd(b.rest, b.bone_ids, b.bone_w, M, g, blend, b.incidence)
        _compare("%s-%s %s T = %d" % (mesh, skeleton, blend, T), got, ref.gradient(V0, ids, w, M, g, blend))


# ---- 2. painted weights ----
def _painted_edges():
    """J = 4: bones 0, 1, 2 with 63, 64 and 65 entries, bone 3 named by nobody; vertex 0 names bone 0 in slots 0 and 2; rows 95 .. 99
    carry no weight at all.  Weights are not normalised."""
    rng = np.random.default_rng(21)
    Vm = 100
    V0 = rng.uniform(-1, 1, (Vm, 3)).astype(np.float32)
    ids, w = np.zeros((Vm, 4), np.int32), np.zeros((Vm, 4), np.float32)
    rnd = lambda n: rng.uniform(0.1, 1.0, n).astype(np.float32)
    ids[:, 1], ids[:, 3] = 1, 2
    w[:62, 0] = rnd(62)                                                # bone 0: 62 rows in slot 0 ...
    w[0, 2] = 0.37                                                     # ... and vertex 0 once more in slot 2: 63
    w[:64, 1] = rnd(64)                                                # bone 1: 64
    w[30:95, 3] = rnd(65)                                              # bone 2: 65
    return V0, ids, w


def _rigid(rotvecs, seed):
    """float32 [T,J,3,4] of rotation vectors [T,J,3] and random translations"""
    from gaussianmesh_amd.skinning import axis_angle_matrices
    rotvecs = np.asarray(rotvecs, np.float64)
    t = np.random.default_rng(seed).uniform(-0.5, 0.5, rotvecs.shape[:2] + (3, 1))
    return np.concatenate([axis_angle_matrices(rotvecs), t], axis=3).astype(np.float32)


@pytest.mark.parametrize("blend", ["linear", "dqs"])
def test_painted_weights_at_the_wave_edge(blend):
    from gaussianmesh_amd.skinning import bone_incidence, skin_pose_differentiable, skin_vertices
    V0, ids, w = _painted_edges()
    M = _rigid(np.random.default_rng(22).uniform(-0.6, 0.6, (2, 4, 3)), 23)
    off, ent = bone_incidence(_dev(ids, torch.int32), _dev(w), 4)
    assert np.diff(off.cpu().numpy()).tolist() == [63, 64, 65, 0] and {0, 2} <= set(ent.cpu().numpy()[:63].tolist())
    ref.check_gradient_position(V0, ids, w, M)
    Md = _dev(M).requires_grad_(True)
    out = skin_pose_differentiable(_dev(V0), ids, w, Md, blend)
    assert same_bits(out.detach(), skin_vertices(_dev(V0), ids, w, M, blend))
    assert same_bits(out.detach()[:, 95:], _dev(V0[95:]).expand(2, 5, 3))          # no weight: the forward keeps x
    g = _g_out(2, 100)
    (out * _dev(g)).sum().backward()
    assert Md.grad.dtype is torch.float32 and Md.grad.shape == Md.shape
    got = _bwd(_dev(V0), _dev(ids, torch.int32), _dev(w), M, g, blend)
    assert same_bits(Md.grad, got.float())
    assert bool((got[:, 3] == 0).all()) and not bool(torch.signbit(got[:, 3]).any())        # the bone nobody names: exact zeros
    _compare("painted edges %s" % blend, got, ref.gradient(V0, ids, w, M, g, blend))
    g2 = g.copy()
    g2[:, 95:] += 3.0                                                  # rows without weight hand nothing to any bone
    assert same_bits(_bwd(_dev(V0), _dev(ids, torch.int32), _dev(w), M, g2, blend), got)


@pytest.mark.parametrize("blend", ["linear", "dqs"])
def test_painted_weights_on_the_four_shepperd_branches(blend):
    rng = np.random.default_rng(31)
    Vm = 70
    V0 = rng.uniform(-1, 1, (Vm, 3)).astype(np.float32)
    ids = np.stack([rng.permutation(4) for _ in range(Vm)]).astype(np.int32)
    w = rng.uniform(0.1, 1.0, (Vm, 4)).astype(np.float32)
    rot = np.array([[[0.3, 0.05, -0.04], [3.0, 0.05, -0.04], [0.05, 3.0, -0.04], [0.05, -0.04, 3.0]],
                    [[-0.2, 0.1, 0.15], [2.9, -0.1, 0.07], [-0.06, 3.05, 0.1], [0.08, 0.1, 2.95]]])
    M = _rigid(rot, 32)
    info = {}
    x, idt, wt = ref.tensors(V0, ids, w)
    ref.dqs(x, idt, wt, torch.as_tensor(M.astype(np.float64)), info)
    assert info["which"].tolist() == [[0, 1, 2, 3], [0, 1, 2, 3]]     # each branch is taken, on the reference's word
    ref.check_gradient_position(V0, ids, w, M)
    g = _g_out(2, Vm)
    got = _bwd(_dev(V0), _dev(ids, torch.int32), _dev(w), M, g, blend)
    _compare("four branches %s" % blend, got, ref.gradient(V0, ids, w, M, g, blend))


# ---- 3. frames and memory ----
@pytest.mark.parametrize("blend", ["linear", "dqs"])
def test_a_frames_gradient_does_not_depend_on_its_batch(blend):
    b = _binding("torus_1073", "ring5")
    M = b.skeleton.bone_transforms(*sc.pose("ring5", 5, seed=5))
    g = _g_out(5, 1073)
    run = lambda m, go: _bwd(b.rest, b.bone_ids, b.bone_w, np.ascontiguousarray(m), np.ascontiguousarray(go), blend, b.incidence)
    full = run(M, g)
    single = torch.stack([run(M[t:t + 1], g[t:t + 1])[0] for t in range(5)], 0)
    assert same_bits(full, single) and not same_bits(single[1], single[2])
    assert same_bits(run(M[::-1], g[::-1]), single.flip(0))
    assert same_bits(run(M[[3, 0, 3]], g[[3, 0, 3]]), single[[3, 0, 3]])


@pytest.mark.parametrize("mesh, skeleton", [("torus_1073", "ring5"), ("flat_257", "chain3"), ("unreferenced", "ring5")])
def test_same_bits_from_call_to_call_and_on_poisoned_memory(mesh, skeleton):
    """two runs give the same bits; so do runs whose every allocation (the output, the workspace, the incidence lists) was filled with
    0x00, 0xFF and 0x5A beforehand, and no guard band around any of them is touched"""
    from gaussianmesh_amd.skinning import bone_incidence
    b = _binding(mesh, skeleton)
    M = b.skeleton.bone_transforms(*sc.pose(skeleton, 3, seed=3))
    g = _g_out(3, b.Vm)

    def route():
        inc = bone_incidence(b.bone_ids, b.bone_w, b.J)
        Md = _dev(M).requires_grad_(True)
        (b.pose_differentiable(Md, "dqs") * _dev(g)).sum().backward()
        return _bwd(b.rest, b.bone_ids, b.bone_w, M, g, "dqs", inc), _bwd(b.rest, b.bone_ids, b.bone_w, M, g, "linear", inc), Md.grad
    first = route()
    assert same_bits(first, route())
    runs = run_under_fills(route)
    assert all(r[0].handed_out >= 6 for r in runs)                     # an output and a workspace per backward, the forward's mesh
    assert differing(runs) == [] and same_bits(runs[0][1], first)


# ---- 4. the autograd wiring ----
@pytest.mark.parametrize("blend", ["linear", "dqs"])
def test_autograd_wiring(blend):
    b = _binding("flat_257", "chain3")
    sk = b.skeleton
    rot, tr = sc.pose("chain3", 2, seed=2)
    M = sk.bone_transforms(rot, tr)
    g = _g_out(2, 257)
    # the forward is pose(), the backward the C call, in the dtype of the transforms
    for dt in (torch.float32, torch.float64):
        Md = _dev(M, dt).requires_grad_(True)
        out = b.pose_differentiable(Md, blend)
        assert out.dtype is torch.float32 and same_bits(out.detach(), b.pose(M, blend=blend))
        (out * _dev(g)).sum().backward()
        direct = _bwd(b.rest, b.bone_ids, b.bone_w, M, g, blend, b.incidence)
        assert Md.grad.dtype is dt and same_bits(Md.grad, direct.to(dt))
    assert same_bits(b.pose(M, blend=blend, checked=False), b.pose(M, blend=blend))
    from gaussianmesh_amd.skinning import skin_vertices
    assert same_bits(skin_vertices(b.rest, b.bone_ids, b.bone_w, M, blend, checked=False), b.pose(M, blend=blend))
    if blend == "dqs":                                                 # checked=False spares exactly the rotation check
        scaled = M.copy()
        scaled[0, 1, :, :3] *= 1.01
        with pytest.raises(ValueError, match="frame 0, bone 1"):
            b.pose(scaled, blend="dqs")
        assert bool(torch.isfinite(b.pose(scaled, blend="dqs", checked=False)).all())
    # d loss / d rotations through the forward kinematics in torch
    r = _dev(rot, torch.float64).requires_grad_(True)
    t = _dev(tr, torch.float64).requires_grad_(True)
    V1 = b.pose_differentiable(sk.bone_transforms_torch(r, t), blend)
    assert same_bits(V1.detach(), b.pose(M, blend=blend))              # the float32 rounding of the torch FK is the numpy FK's
    (V1 * _dev(g)).sum().backward()
    rr, tt = torch.tensor(rot, requires_grad=True), torch.tensor(tr, requires_grad=True)
    M64 = ref.fk(*sc.skeleton("chain3"), rr, tt)
    gM = ref.gradient(sc.mesh("flat_257")[0], b.bone_ids.cpu().numpy(), b.bone_w.cpu().numpy(), M64.detach().numpy().astype(np.float32), g, blend)
    want_r, want_t = torch.autograd.grad(M64, (rr, tt), grad_outputs=torch.as_tensor(gM))
    for name, got, want in (("rotations", r.grad, want_r), ("root_translation", t.grad, want_t)):
        err, scale = float((got.cpu() - want).abs().max()), float(want.abs().max())
        print("%s d loss / d %s: |hip - ref| / max |ref| = %.3g" % (blend, name, err / scale))
        assert err <= BOUND * scale
    with pytest.raises(ValueError, match="transforms"):
        b.pose_differentiable(_dev(M)[:, :1], blend)
    with pytest.raises(ValueError, match="transforms"):
        b.pose_differentiable(torch.as_tensor(M), blend)
    with pytest.raises(ValueError, match="blend"):
        b.pose_differentiable(_dev(M), "cubic")


# ---- 5. the C refusals ----
def test_c_refusals_launch_nothing():
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    size = l.gm_skin_pose_bwd_workspace_bytes
    assert size(0, 96, 5, 1) == 0 and size(2, 0, 5, 1) == 0 and size(2, 96, 0, 1) == 0 and size(2, 96, 257, 1) == 0 and size(2, 96, 5, 2) == 0
    assert 0 < size(1, 96, 5, 0) < size(1, 96, 5, 1) < size(2, 96, 5, 1) < size(2, 1073, 5, 1) <= size(2, 1073, 256, 1)
    assert size(2, 96, 5, 1) >= 2 * 96 * 8 * 8 and size(2, 96, 5, 0) >= 2 * 96 * 3 * 8
    b = _binding("torus_96", "ring5")
    M = _dev(b.skeleton.bone_transforms(*sc.pose("ring5", 2)))
    g = _dev(_g_out(2, 96))
    off, ent = b.incidence
    out = torch.full((2, 5, 3, 4), 5.0, dtype=torch.float64, device="cuda")
    ws = torch.empty((size(2, 96, 5, 1),), dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(T=2, Vm=96, J=5, blend=1, nbytes=None, **kw):
        t = dict(V0=b.rest, ids=b.bone_ids, w=b.bone_w, M=M, g=g, off=off, ent=ent, out=out, ws=ws)
        t.update(kw)
        q = {k: (v.data_ptr() if torch.is_tensor(v) else v) for k, v in t.items()}
        return l.gm_skin_pose_bwd(T, Vm, J, q["V0"], q["ids"], q["w"], q["M"], blend, q["g"], q["off"], q["ent"], q["out"], q["ws"],
                                  ws.numel() if nbytes is None else nbytes, stream)
    as_bytes = lambda t: t.view(torch.uint8).reshape(-1)
    for kw, rc in ((dict(T=0), 1), (dict(Vm=0), 1), (dict(J=0), 1), (dict(J=257), 1), (dict(blend=2), 1), (dict(blend=-1), 1), (dict(V0=None), 1),
                   (dict(ids=None), 1), (dict(w=None), 1), (dict(M=None), 1), (dict(g=None), 1), (dict(off=None), 1), (dict(ent=None), 1),
                   (dict(out=None), 1), (dict(ws=None), 1), (dict(out=M), 1), (dict(out=g), 1), (dict(out=b.rest), 1), (dict(out=off), 1),
                   (dict(out=ent), 1), (dict(ws=out), 1), (dict(ws=g, nbytes=g.numel() * 4), 1), (dict(out=as_bytes(ws)[256:]), 1),
                   (dict(nbytes=size(2, 96, 5, 1) - 1), 3), (dict(nbytes=0), 3)):
        assert call(**kw) == rc and b"gm_skin_pose_bwd" in l.gm_last_error(), (kw, l.gm_last_error())
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    assert call() == 0                                                 # and the same call, unrefused, writes everything
    torch.cuda.synchronize()
    assert same_bits(out, _bwd(b.rest, b.bone_ids, b.bone_w, M.cpu().numpy(), g.cpu().numpy(), "dqs", b.incidence))
    assert call(blend=0, nbytes=size(2, 96, 5, 0)) == 0                # the linear blend asks for less
    torch.cuda.synchronize()
    assert same_bits(out, _bwd(b.rest, b.bone_ids, b.bone_w, M.cpu().numpy(), g.cpu().numpy(), "linear", b.incidence))


# ---- 6. inverse kinematics ----
PICKS = [0, 15, 240, 255, 120, 136, 256, 60]


@pytest.mark.parametrize("blend", ["linear", "dqs"])
def test_ik_reaches_an_attainable_pose(blend):
    """targets that a pose attains, from rest, 40 iterations: final / first objective <= 1e-6.  The restatement under the same optimiser
    reaches 2.0e-11 (linear) and 2.0e-10 (dqs) at 40 iterations and 4e-8 / 2e-7 at 20; the float32 rounding of the device's vertices
    puts the floor near 1e-13: more than three decades of margin."""
    b = _binding("flat_257", "chain3")
    targets = b.pose_skeleton(*sc.pose("chain3", 1, seed=3), blend=blend)[0][PICKS]
    rot, tr, history = b.solve_ik(PICKS, targets, iterations=40, blend=blend)
    assert rot.shape == (3, 3) and tr.shape == (3,) and rot.dtype is torch.float64 and len(history) == 41 and np.isfinite(history).all()
    print("IK %s: objective %.3g -> %.3g, ratio %.3g" % (blend, history[0], history[-1], history[-1] / history[0]))
    assert history[0] > 1e-3 and history[-1] / history[0] <= 1e-6
    reached = b.pose_skeleton(rot[None], tr[None], blend=blend)[0][PICKS]
    assert abs(0.5 * float(((reached.double() - targets.double()) ** 2).sum()) - history[-1]) <= 1e-12 + 1e-6 * history[-1]
    held = b.solve_ik(PICKS, targets, rotations=rot, root_translation=tr, iterations=2, blend=blend, fit_translation=False)
    assert torch.equal(held[1], tr) and len(held[2]) == 3 and np.isfinite(held[2]).all()
    for bad in (dict(vertex_ids=[0, 257]), dict(vertex_ids=[]), dict(targets=targets[:3]), dict(iterations=0), dict(damping=-1.0), dict(blend="cubic"),
                dict(rotations=np.zeros((2, 3)))):
        with pytest.raises(ValueError, match="solve_ik"):
            b.solve_ik(**{**dict(vertex_ids=PICKS, targets=targets), **bad})


def test_drag_skeleton_leaves_the_object_at_the_pose_it_returns(tmp_path):
    from test_gpu_arap import _scene64, _tool
    d = str(tmp_path)
    _scene64(d)
    tool, other = _tool(d), _tool(d)
    o, q = tool.gaussians_list[0], other.gaussians_list[0]
    skel, rot, tr = _scene_skeleton(o.vertex.cpu().numpy())
    picks = [0, 7, 19, 33]
    for call in (lambda: o.drag_skeleton(picks, o.vertex[picks]), lambda: o.fit_skeleton_pose([], 1)):
        with pytest.raises(ValueError, match="call attach_skeleton\\(skeleton\\) first"):
            call()
    assert tool.drag_skeleton_one_gaussian("Nobody", picks, o.vertex[picks], skeleton=skel) is None
    q.attach_skeleton(skel)
    targets = q.skin.pose_skeleton(rot[:1], tr[:1])[0][picks]
    got_rot, got_tr, history = tool.drag_skeleton_one_gaussian("Object", picks, targets, skeleton=skel, iterations=10)
    assert history[-1] < history[0] and len(history) == 11
    q.pose(got_rot, got_tr)
    assert torch.equal(o.mesh_vertex_current, q.mesh_vertex_current)
    assert torch.equal(o.mesh_vertex_current, o.skin.pose_skeleton(got_rot[None], got_tr[None])[0])
    again = o.drag_skeleton(picks, targets, iterations=3)              # continues from the pose it is in
    assert again[2][0] == pytest.approx(history[-1], rel=1e-9, abs=1e-15)


# ---- 7. the fit ----
def test_fit_a_skeleton_pose_from_three_views(tmp_path):
    """the setup of test_fit_a_twisted_torus_from_three_views with a skeleton under the torus: five bones, rotations within 0.4 rad,
    targets rendered from obj.pose(...), 60 steps of SkeletonPoseFitter from rest at its default lr.  No ratio is asserted; on an MI355X
    the losses went 0.2357 -> 0.1536, 0.2438 -> 0.1802, 0.2347 -> 0.1831 (ratio 0.724) and the vertex RMS 2.2156 -> 1.4752 (0.666)."""
    from gpu_utils import T
    from gaussianmesh_amd import GaussianRasterizer, scenes
    from gaussianmesh_amd.deform import SingleObjectDeform
    from gaussianmesh_amd.edit_sequence import read_pose_sequence
    from gaussianmesh_amd.renderer import Camera, _settings
    W, H, steps = 96, 64, 60
    verts, faces = scenes.torus_mesh(24, 16)
    cl = scenes.bind_cloud_to_mesh(4000, verts, faces, seed=5)
    cov = scenes.cov3d_from_scale_rot(cl["scales"], cl["rots"]).astype(np.float32)
    obj = SingleObjectDeform(T(cl["means"]), T(cov), T(cl["opac"]), T(cl["shs"]), T(cl["tri"], dtype=torch.int32), T(cl["weights"]), T(verts))
    dev = obj.vertex.device
    skel, rots, trs = _scene_skeleton(verts)
    obj.attach_skeleton(skel, faces=T(faces, dtype=torch.int32))
    cams = [Camera(scenes.orbit_camera(k, 3, W, H, radius=6.0), dev) for k in range(3)]
    bg = torch.ones(3, device=dev)
    views = []
    with torch.no_grad():
        obj.pose(rots[0], trs[0])
        V1, R, S = obj.deform_state
        target_mesh = obj.mesh_vertex_current.clone()
        for cam in cams:
            pos, rgb, cov6 = obj.deform_and_shade(V1, R, S, cam.camera_center)
            image, radii = GaussianRasterizer(_settings(cam, bg, 1.0, 3, False))(pos, torch.zeros_like(pos), obj.gaussian_o, colors_precomp=rgb,
                                                                                 cov3D_precomp=cov6)
            assert int((radii > 0).sum()) > 1000
            views.append((cam, image.clone()))
    obj.deform_state = None
    fitter = obj.fit_skeleton_pose(views, steps, from_current=False)   # the fit starts at rest
    losses = torch.stack(fitter.losses).cpu().numpy()
    assert losses.shape == (steps,) and np.isfinite(losses).all()
    rot, tr = fitter.pose.rotations.detach(), fitter.pose.root_translation.detach()
    rms = lambda a: float(((a - target_mesh) ** 2).sum(1).mean().sqrt())
    start, end = rms(obj.vertex), rms(obj.mesh_vertex_current)
    print("skeleton pose fit, %d steps at lr %g: loss per view first -> last %s; ratio %.3f; vertex RMS error %.4f -> %.4f, ratio %.3f" % (
        steps, fitter.lr, ", ".join("%.4f -> %.4f" % (losses[k], losses[steps - 3 + k]) for k in range(3)), losses[-3:].mean() / losses[:3].mean(),
        start, end, end / start))
    for k in range(3):                                                 # steps k and 57 + k saw the same view
        assert losses[steps - 3 + k] < losses[k], k
    assert end < start
    # the object is left exactly at pose(fitted)
    fresh = SingleObjectDeform(T(cl["means"]), T(cov), T(cl["opac"]), T(cl["shs"]), T(cl["tri"], dtype=torch.int32), T(cl["weights"]), T(verts))
    fresh.attach_skeleton(skel, faces=T(faces, dtype=torch.int32))
    fresh.pose(rot, tr)
    assert all(torch.equal(a, e) for a, e in zip(obj.deform_state, fresh.deform_state)) and obj.gaussian_deform_pos.shape == (4000, 3)
    path = str(tmp_path / "pose.json")
    fitter.write_pose(path)
    back_rot, back_tr = read_pose_sequence(path, joints=skel.Nj)
    assert np.array_equal(back_rot, rot.cpu().numpy()[None]) and np.array_equal(back_tr, tr.cpu().numpy()[None])
    assert set(json.load(open(path))) == {"rotations", "root_translation"}
