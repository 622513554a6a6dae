"""-m "not gpu": the host side of the skinning backward (INTEGRATION.md section AF).  tests/skin_bwd_ref.py, the float64 torch
restatement whose autograd defines gm_skin_pose_bwd, against the numpy reference of the forward and against finite differences;
Skeleton.bone_transforms_torch against the numpy forward kinematics, and its gradient at rest; bone_incidence on CPU tensors; the
general position of the cases test_gpu_skin_bwd.py compares on; the host refusals of the new Python entry points."""
import types

import numpy as np
import pytest
import torch

import skin_bwd_ref as ref
import skin_cases as sc
import skin_ref

GRADIENT_CASES = [("torus_1073", "ring5"), ("torus_96", "star17"), ("flat_255", "chain3"), ("flat_256", "chain3"), ("flat_257", "chain3"),
                  ("unreferenced", "ring5"), ("two_tori", "inside"), ("torus_96", "one_bone")]
IDS = ["%s-%s" % c for c in GRADIENT_CASES]


def _transforms(skeleton, T):
    from gaussianmesh_amd.skinning import Skeleton
    return Skeleton(*sc.skeleton(skeleton)).bone_transforms(*sc.pose(skeleton, T, seed=T))


@pytest.mark.parametrize("mesh, skeleton", GRADIENT_CASES, ids=IDS)
def test_the_restatement_is_the_numpy_reference(mesh, skeleton):
    ids, w = ref.reference_weights(mesh, skeleton)
    V0 = sc.mesh(mesh)[0]
    x, idt, wt = ref.tensors(V0, ids, w)
    for T in (1, 5):
        M = _transforms(skeleton, T)
        for kind in ("linear", "dqs"):
            got = ref.blend(x, idt, wt, torch.as_tensor(M.astype(np.float64)), kind).numpy()
            err = float(np.abs(got - skin_ref.blend(V0, ids, w, M, kind)).max())
            print("%s-%s T = %d %s: restatement against skin_ref.blend %.3g" % (mesh, skeleton, T, kind, err))
            assert err <= 1e-13


@pytest.mark.parametrize("kind", ["linear", "dqs"])
def test_gradcheck_of_the_restatement(kind):
    ids, w = ref.reference_weights("torus_96", "star17")
    x, idt, wt = ref.tensors(sc.mesh("torus_96")[0], ids, w)
    M = torch.as_tensor(_transforms("star17", 2).astype(np.float64)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda m: ref.blend(x, idt, wt, m, kind), (M,), eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("mesh, skeleton", GRADIENT_CASES, ids=IDS)
def test_the_cases_sit_away_from_every_decision(mesh, skeleton):
    """what test_gpu_skin_bwd.py compares on, with the reference's weights (the device's differ from them by its PCG's 1e-8)"""
    ids, w = ref.reference_weights(mesh, skeleton)
    for T in (1, 5):
        figures = ref.check_gradient_position(sc.mesh(mesh)[0], ids, w, _transforms(skeleton, T))
        print("%s-%s T = %d: Shepperd margin %.3g, |q_k . q_0| %.3g, |b_r| %.3g" % ((mesh, skeleton, T) + figures))


@pytest.mark.parametrize("skeleton", ["ring5", "chain3", "star17", "inside", "one_bone"])
def test_forward_kinematics_in_torch_is_the_numpy_one(skeleton):
    from gaussianmesh_amd.skinning import Skeleton
    sk = Skeleton(*sc.skeleton(skeleton))
    for T in (1, 5):
        rot, tr = sc.pose(skeleton, T, seed=T)
        got = sk.bone_transforms_torch(torch.as_tensor(rot), torch.as_tensor(tr))
        assert got.dtype is torch.float64 and tuple(got.shape) == (T, sk.J, 3, 4)
        A, t = sk.joint_transforms(rot, tr)
        p = sk.parents[1:]
        want = np.concatenate([A[:, p], t[:, p, :, None]], axis=3)
        err = float(np.abs(got.numpy() - want).max())
        print("%s T = %d: torch FK against numpy %.3g; the restatement's %.3g" % (
            skeleton, T, err, float(np.abs(ref.fk(*sc.skeleton(skeleton), torch.as_tensor(rot), torch.as_tensor(tr)).numpy() - want).max())))
        assert err <= 1e-12
        assert np.array_equal(got.numpy().astype(np.float32).view(np.uint32), sk.bone_transforms(rot, tr).view(np.uint32))
    assert np.array_equal(sk.bone_transforms_torch(torch.as_tensor(rot)).numpy().astype(np.float32), sk.bone_transforms(rot))


def test_the_gradient_at_rest_is_finite_and_central_differences():
    from gaussianmesh_amd.skinning import Skeleton
    sk = Skeleton(*sc.skeleton("chain3"))
    probe = torch.as_tensor(np.random.default_rng(3).standard_normal((1, sk.J, 3, 4)))
    f = lambda r, t: (sk.bone_transforms_torch(r, t) * probe).sum()
    r = torch.zeros((1, sk.Nj, 3), dtype=torch.float64, requires_grad=True)
    t = torch.zeros((1, 3), dtype=torch.float64, requires_grad=True)
    gr, gt = torch.autograd.grad(f(r, t), (r, t))
    assert bool(torch.isfinite(gr).all()) and bool(torch.isfinite(gt).all()) and float(gr.abs().max()) > 0.1
    h = 1e-5
    with torch.no_grad():
        for k in range(sk.Nj):
            for a in range(3):
                e = torch.zeros_like(r)
                e[0, k, a] = h
                fd = float(f(e, t) - f(-e, t)) / (2 * h)
                assert abs(fd - float(gr[0, k, a])) <= 1e-8, (k, a, fd, float(gr[0, k, a]))     # (the series' odd terms: O(h^2) = 1e-10)
    assert bool(torch.isfinite(torch.autograd.grad(f(torch.full_like(r, 1e-5).requires_grad_(True), t), t)[0]).all())


def test_bone_incidence_lists_every_nonzero_slot_once():
    from gaussianmesh_amd.skinning import bone_incidence
    rng = np.random.default_rng(5)
    Vm, J = 300, 7
    ids = rng.integers(0, J - 1, (Vm, 4))                              # bone J - 1 is named by nobody
    w = rng.uniform(0.1, 1.0, (Vm, 4)).astype(np.float32)
    w[rng.uniform(size=(Vm, 4)) < 0.4] = 0.0
    ids[7] = 2                                                         # one bone in all four slots
    w[7] = [0.5, 0.0, 0.25, 0.25]
    w[11] = 0.0                                                        # a row nobody moves
    off, ent = bone_incidence(torch.as_tensor(ids, dtype=torch.int32), torch.as_tensor(w), J)
    assert off.dtype is torch.int32 and ent.dtype is torch.int32 and tuple(off.shape) == (J + 1,)
    off, ent = off.numpy(), ent.numpy()
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(ent) == int((w != 0).sum())
    assert off[J] == off[J - 1]                                        # the unused bone: empty
    assert len(np.unique(ent)) == len(ent)
    for j in range(J):
        mine = ent[off[j]:off[j + 1]]
        assert (np.diff(mine) > 0).all()
        assert (ids.reshape(-1)[mine] == j).all() and (w.reshape(-1)[mine] != 0).all()
    assert set(ent[off[2]:off[3]]) >= {28, 30, 31} and 29 not in ent and not set(range(44, 48)) & set(ent)
    out = bone_incidence(torch.as_tensor(ids - 3), torch.as_tensor(w), J)[1].numpy()      # ids forced into [0, J) as the kernels force them
    assert len(out) == len(ent)
    empty = bone_incidence(torch.zeros((5, 4), dtype=torch.int64), torch.zeros((5, 4)), 3)
    assert empty[0].tolist() == [0, 0, 0, 0] and empty[1].numel() == 0


def test_host_refusals():
    from gaussianmesh_amd import _lib
    from gaussianmesh_amd.pose_fit import SkeletonPose, SkeletonPoseFitter
    from gaussianmesh_amd.skinning import Skeleton, bone_incidence, skin_pose_differentiable
    sk = Skeleton(*sc.skeleton("chain3"))
    good = torch.zeros((2, 3, 3), dtype=torch.float64)
    for bad in (good[:, :2], good[0], good[:0], good.to(torch.int64), good.numpy(), torch.zeros((2, 3, 3, 3), dtype=torch.float64)):
        with pytest.raises(ValueError, match="bone_transforms_torch: rotations"):
            sk.bone_transforms_torch(bad)
    for bad in (torch.zeros((3, 3)), torch.zeros(3), np.zeros((2, 3)), torch.zeros((2, 3), dtype=torch.int32)):
        with pytest.raises(ValueError, match="root_translation"):
            sk.bone_transforms_torch(good, bad)
    ids, w = torch.zeros((6, 4), dtype=torch.int32), torch.ones((6, 4))
    for args in ((ids[:, :3], w[:, :3], 2), (ids, w[:5], 2), (ids.float(), w, 2), (ids, w.int(), 2), (ids, w, 0), (ids, w, 257)):
        with pytest.raises(ValueError, match="bone_incidence"):
            bone_incidence(*args)
    with pytest.raises(_lib.GmeshError, match="skin_pose_differentiable"):
        skin_pose_differentiable(torch.zeros((6, 3)), ids, w, torch.zeros((1, 2, 3, 4)))
    with pytest.raises(ValueError, match="attach_skeleton"):
        SkeletonPoseFitter(types.SimpleNamespace(skin=None))
    binding = types.SimpleNamespace(rest=torch.zeros((6, 3)), skeleton=sk)
    with pytest.raises(ValueError, match="blend"):
        SkeletonPose(binding, blend="cubic")
    with pytest.raises(ValueError, match="rotations"):
        SkeletonPose(binding, rotations=np.zeros((2, 3)))
    pose = SkeletonPose(binding, rotations=np.full((3, 3), 0.1), root_translation=[1.0, 2.0, 3.0])
    assert pose.rotations.dtype is torch.float64 and pose.root_translation.tolist() == [1.0, 2.0, 3.0] and len(list(pose.parameters())) == 2
