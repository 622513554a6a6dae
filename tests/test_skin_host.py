"""Host half of the skinning stage (gaussianmesh_amd/skinning.py): Skeleton's refusals and files, forward kinematics, edit_sequence's
reader and flag refusals, and the float64 reference of tests/skin_ref.py on the cases of tests/skin_cases.py - the properties the GPU
tests then lean on.  No device anywhere."""
import json
import math
import os

import numpy as np
import pytest

import skin_cases as sc
import skin_ref


def _skeleton(name):
    from gaussianmesh_amd.skinning import Skeleton
    return Skeleton(*sc.skeleton(name))


# ---- Skeleton ----
def test_skeleton_refusals_name_the_joint():
    from gaussianmesh_amd.skinning import Skeleton
    j = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], np.float32)
    s = Skeleton(j, [-1, 0, 1], names=["hip", "knee", "foot"])
    assert (s.Nj, s.J) == (3, 2) and s.joints.dtype == np.float32 and s.parents.dtype == np.int64
    a, b = s.bones
    assert np.array_equal(a, j[[0, 1]]) and np.array_equal(b, j[[1, 2]])
    for parents, what in (([0, 0, 1], "joint 0"), ([-1, 1, 1], "joint 1"), ([-1, 0, 2], "joint 2"), ([-1, 0, -1], "joint 2"), ([-1, 0, 5], "joint 2")):
        with pytest.raises(ValueError, match=what):
            Skeleton(j, parents)
    bad = j.copy()
    bad[1, 2] = np.nan
    with pytest.raises(ValueError, match="joint 1"):
        Skeleton(bad, [-1, 0, 1])
    for joints, parents in ((j[:1], [-1]), (j[:, :2], [-1, 0, 1]), (j, [-1, 0]), (j, [-1.0, 0.0, 1.0]), (np.zeros((258, 3)), [-1] + list(range(257)))):
        with pytest.raises(ValueError, match="Skeleton"):
            Skeleton(joints, parents)
    with pytest.raises(ValueError, match="names"):
        Skeleton(j, [-1, 0, 1], names=["a"])


def test_skeleton_read_write_round_trip(tmp_path):
    from gaussianmesh_amd.skinning import Skeleton
    joints, parents = sc.skeleton("star17")
    path = str(tmp_path / "s.json")
    for names in (None, ["j%d" % k for k in range(len(joints))]):
        Skeleton(joints, parents, names).write(path)
        doc = json.load(open(path))
        assert set(doc) == ({"joints", "parents"} if names is None else {"joints", "parents", "names"})
        back = Skeleton.read(path)
        assert np.array_equal(back.joints, joints) and np.array_equal(back.parents, parents) and back.names == names
    for text in ("{", "[1, 2]", '{"joints": [[0, 0, 0], [1, 0, 0]]}', '{"joints": [[0, 0, 0], [1, 0, 0]], "parents": [0, 0]}',
                 '{"joints": [[0, 0], [1, 0]], "parents": [-1, 0]}', '{"joints": "x", "parents": [-1, 0]}'):
        open(path, "w").write(text)
        with pytest.raises(ValueError, match="s.json"):
            Skeleton.read(path)
    with pytest.raises(ValueError, match="cannot read"):
        Skeleton.read(str(tmp_path / "none.json"))


# ---- forward kinematics ----
def test_identity_pose_gives_identity_transforms():
    for name in ("ring5", "star17", "one_bone"):
        s = _skeleton(name)
        eye = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)
        for rot in (np.zeros((3, s.Nj, 3)), np.tile(np.eye(3), (3, s.Nj, 1, 1))):
            M = s.bone_transforms(rot)
            assert M.shape == (3, s.J, 3, 4) and M.dtype == np.float32 and np.array_equal(M, np.broadcast_to(eye, M.shape))


def test_root_rotation_is_one_rigid_motion_for_every_bone():
    s = _skeleton("ring5")
    rot = np.zeros((2, s.Nj, 3))
    rot[0, 0], rot[1, 0] = (0.3, -1.1, 0.4), (0.0, 2.5, 0.0)
    tr = np.array([[0.2, -0.1, 0.5], [0.0, 0.0, 0.0]])
    M = s.bone_transforms(rot, tr).astype(np.float64)
    c = s.joints[0].astype(np.float64)
    for t in range(2):
        R = skin_ref.rotation_matrix(rot[t, 0])
        want = np.concatenate([R, (c - R @ c + tr[t])[:, None]], 1)
        assert np.abs(M[t] - want).max() <= 4e-7                       # float32 rounding of entries below 4
        assert np.array_equal(M[t], np.broadcast_to(M[t, 0], M[t].shape))
    leaf = np.zeros((1, s.Nj, 3))
    leaf[0, s.Nj - 1] = (0.5, 0.5, 0.5)                                # a leaf joint's rotation moves nothing
    assert np.array_equal(s.bone_transforms(leaf), s.bone_transforms(np.zeros((1, s.Nj, 3))))
    for bad_rot, bad_tr in ((np.zeros((2, s.Nj + 1, 3)), None), (np.zeros((0, s.Nj, 3)), None), (np.zeros((2, s.Nj, 3)), np.zeros((3, 3))),
                            (np.full((1, s.Nj, 3), np.nan), None)):
        with pytest.raises(ValueError, match="bone_transforms"):
            s.bone_transforms(bad_rot, bad_tr)


def test_two_quarter_turns_against_a_hand_computed_matrix():
    """joints (0,0,0) -> (1,0,0) -> (2,0,0) -> (3,0,0); joint 0 turns 90 degrees about z, joint 1 turns 90 degrees about x.  Bone 0 moves
    with G_0 = Rz: x -> (-y, x, z).  Bone 1 moves with G_1 = Rz o (Rx about (1,0,0)): Rx about (1,0,0) is x -> (x, -z, y) (the centre
    lies on the axis), then Rz: (x, y, z) -> (z, x, y), no translation.  Bone 2 moves with G_2 = G_1 (joint 2 does not turn)."""
    from gaussianmesh_amd.skinning import Skeleton
    s = Skeleton([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]], [-1, 0, 1, 2])
    h = math.pi / 2
    rot = np.array([[[0, 0, h], [h, 0, 0], [0, 0, 0], [0, 0, 0]]])
    M = s.bone_transforms(rot)[0].astype(np.float64)
    want0 = np.array([[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0]], np.float64)
    want1 = np.array([[0, 0, 1, 0], [1, 0, 0, 0], [0, 1, 0, 0]], np.float64)
    assert np.abs(M[0] - want0).max() <= 1e-7 and np.abs(M[1] - want1).max() <= 1e-7 and np.abs(M[2] - want1).max() <= 1e-7
    # the same through matrices, and against the reference's 4 x 4 chain on a bent skeleton
    from gaussianmesh_amd.skinning import axis_angle_matrices
    assert np.array_equal(s.bone_transforms(axis_angle_matrices(rot)), s.bone_transforms(rot))
    mats = np.stack([skin_ref.rotation_matrix(r) for r in rot[0]], 0)[None]
    assert np.abs(s.bone_transforms(mats).astype(np.float64) - s.bone_transforms(rot)).max() <= 1e-7
    for name in ("ring5", "star17", "inside"):
        k = _skeleton(name)
        r, tr = sc.pose(name, 3)
        want = skin_ref.bone_transforms(k.joints, k.parents, r, tr)
        assert np.abs(k.bone_transforms(r, tr).astype(np.float64) - want).max() <= 1e-6


# ---- edit_sequence: the reader and the flags ----
def test_pose_sequence_reader(tmp_path):
    from gaussianmesh_amd.edit_sequence import read_pose_sequence
    path = str(tmp_path / "pose.json")
    rot, tr = sc.pose("chain3", 4)
    json.dump({"rotations": rot.tolist(), "root_translation": tr.tolist()}, open(path, "w"))
    got_r, got_t = read_pose_sequence(path, joints=3)
    assert np.array_equal(got_r, rot) and np.array_equal(got_t, tr)
    json.dump({"rotations": rot.tolist()}, open(path, "w"))
    assert read_pose_sequence(path)[1] is None
    with pytest.raises(SystemExit, match="pose.json.*rotations"):
        read_pose_sequence(path, joints=4)
    for doc in ("{", "[]", {"rotations": []}, {"rotations": [[1, 2, 3]]}, {"rotations": [[[1, 2]]]}, {"rotations": "x"},
                {"rotations": [[[0, 0, float("nan")]]]}, {"rotations": rot.tolist(), "root_translation": tr[:2].tolist()},
                {"rotations": rot.tolist(), "root_translation": "x"}):
        open(path, "w").write(doc if isinstance(doc, str) else json.dumps(doc))
        with pytest.raises(SystemExit, match="pose.json"):
            read_pose_sequence(path)
    with pytest.raises(SystemExit, match="cannot read"):
        read_pose_sequence(str(tmp_path / "none.json"))


def test_edit_sequence_flag_refusals(tmp_path):
    from gaussianmesh_amd.edit_sequence import main
    base = ["--object_gaussian", "o.ply", "--object_origin_mesh", "m.obj", "--camera_path", "c", "--render_path", str(tmp_path / "out")]
    pose = str(tmp_path / "pose.json")
    json.dump({"rotations": np.zeros((2, 3, 3)).tolist()}, open(pose, "w"))
    for extra, what in ((["--skeleton", "s.json"], "--skeleton"), (["--skin_blend", "linear"], "--skin_blend"), (["--skin_heat", "2"], "--skin_heat"),
                        (["--skin_influences", "2"], "--skin_influences")):
        with pytest.raises(SystemExit, match=what + " belongs to --pose_sequence"):
            main(base + ["--mesh_sequence", "d"] + extra)
    posed = base + ["--pose_sequence", pose]
    with pytest.raises(SystemExit, match="needs --skeleton"):
        main(posed)
    posed += ["--skeleton", "s.json"]
    for extra, what in ((["--dynamics"], "--dynamics"), (["--arap_batch", "2"], "--arap_batch"), (["--skin_heat", "0"], "--skin_heat"),
                        (["--skin_heat", "inf"], "--skin_heat"), (["--skin_influences", "5"], "--skin_influences"),
                        (["--skin_influences", "0"], "--skin_influences")):
        with pytest.raises(SystemExit, match=what):
            main(posed + extra)
    with pytest.raises(SystemExit):                                    # (argparse: one source only, one blend of the two)
        main(posed + ["--mesh_sequence", "d"])
    with pytest.raises(SystemExit):
        main(posed + ["--skin_blend", "cubic"])
    open(pose, "w").write("{")
    with pytest.raises(SystemExit, match="pose.json"):
        main(posed)
    assert not os.path.exists(str(tmp_path / "out"))


# ---- the reference ----
@pytest.mark.parametrize("mesh, skeleton", sc.CASES, ids=sc.IDS)
def test_reference_weights_are_a_partition_of_unity_in_general_position(mesh, skeleton):
    s, full = sc.system(mesh, skeleton), sc.dense(mesh, skeleton)
    margin, gap = sc.check_general_position(mesh, skeleton)
    print("%s-%s: Vm %d, J %d, unknowns %d, threshold margin %.3g, cut gap %.3g, weights in [%.3g, %.3g]"
          % (mesh, skeleton, s.Vm, s.J, int(s.unknown.sum()), margin, gap, full.min(), full.max()))
    assert full.shape == (s.J, s.Vm) and np.isfinite(full).all()
    assert full.min() >= -1e-12 and full.max() <= 1.0 + 1e-12
    assert np.abs(full.sum(axis=0) - 1.0).max() <= 1e-10
    assert (s.near.sum(axis=0) >= 1).all()
    if mesh == "unreferenced":
        assert not s.unknown[-1] and s.unknown[:-1].all() and np.array_equal(full[:, -1], s.p[:, -1])
    else:
        assert s.unknown.all()
    # the restatement of the PCG reaches the dense solve, and the residual it reports is the true one
    x, steps, res = s.pcg(2000, 1e-10)
    assert np.abs(x - full).max() <= 1e-7 and (res <= 1e-10).all() and (steps < 2000).all()
    b = np.where(s.unknown, s.h * s.p, 0.0)
    true = np.stack([np.where(s.unknown, b[j] - s.apply(x[j]), 0.0) for j in range(s.J)], 0)
    norm = np.linalg.norm(b, axis=1)
    assert (np.linalg.norm(true, axis=1) <= 2e-10 * np.maximum(norm, 1e-300) + 1e-300).all()


def test_a_bones_weights_fall_off_along_the_mesh():
    """bone 0 of ring5 on the 1073-vertex torus: the mean weight of the vertices whose angle round the torus lies in a sector falls from
    the bone's own sector to the opposite one, and the vertex nearest the bone's middle carries more than 0.8"""
    s, full = sc.system("torus_1073", "ring5"), sc.dense("torus_1073", "ring5")
    V0 = sc.mesh("torus_1073")[0].astype(np.float64)
    mid = 0.5 * (s.a[0] + s.b[0])
    at = math.atan2(mid[2], mid[0])
    turn = np.abs((np.arctan2(V0[:, 2], V0[:, 0]) - at + math.pi) % (2 * math.pi) - math.pi)     # 0 at the bone, pi opposite
    means = [float(full[0][(turn >= lo) & (turn < lo + math.pi / 6)].mean()) for lo in np.arange(6) * math.pi / 6]
    print("mean weight of bone 0 by sector:", " ".join("%.4f" % m for m in means))
    assert all(a > b for a, b in zip(means, means[1:])) and means[0] > 0.7 and means[-1] < 0.05
    assert full[0][np.argmin(((V0 - mid) ** 2).sum(axis=1))] > 0.8


def test_compaction_keeps_the_largest_and_renormalises():
    s, full = sc.system("torus_96", "ring5"), sc.dense("torus_96", "ring5")
    for keep in (1, 2, 3, 4):
        ids, w = skin_ref.compact(full, s.unknown, s.near, keep)
        assert ids.dtype == np.int32 and w.dtype == np.float32 and ids.shape == w.shape == (96, 4)
        assert np.abs(w.astype(np.float64).sum(axis=1) - 1.0).max() <= 4 * 6e-8
        assert (np.diff(w, axis=1) <= 0).all() and (w[:, keep:] == 0).all() and (w[:, :keep] > 0).all()
        assert np.array_equal(ids[:, 0], full.argmax(axis=0))
        assert (ids[:, keep:] == ids[:, :1]).all()
        for i in range(96):
            assert len(set(ids[i, :keep])) == keep
    one = skin_ref.compact(sc.dense("torus_96", "one_bone"), np.ones(96, bool), np.ones((1, 96), bool), 4)
    assert (one[0] == 0).all() and (one[1] == np.array([1, 0, 0, 0], np.float32)).all()
    u = sc.system("unreferenced", "ring5")
    ids, w = skin_ref.compact(sc.dense("unreferenced", "ring5"), u.unknown, u.near, 4)
    assert (ids[-1] == np.nonzero(u.near[:, -1])[0][0]).all() and w[-1].tolist() == [1.0, 0.0, 0.0, 0.0]


def test_blends_agree_where_a_row_has_one_influence():
    s, full = sc.system("torus_96", "ring5"), sc.dense("torus_96", "ring5")
    V0 = sc.mesh("torus_96")[0]
    ids, w = skin_ref.compact(full, s.unknown, s.near, 1)
    joints, parents = sc.skeleton("ring5")
    M = skin_ref.bone_transforms(joints, parents, *sc.pose("ring5", 3)).astype(np.float32)
    lin, dqs = skin_ref.blend_linear(V0, ids, w, M), skin_ref.blend_dqs(V0, ids, w, M)
    assert np.abs(lin - dqs).max() <= 1e-6                             # (the float32 transforms are rotations to 1e-7 only)
    own = M[:, ids[:, 0]].astype(np.float64)                           # [T,Vm,3,4]
    rigid = np.einsum("tvab,vb->tva", own[..., :3], V0.astype(np.float64)) + own[..., 3]
    assert np.abs(lin - rigid).max() <= 1e-12
    # and with four influences they differ, the identity pose returning the rest vertices exactly under both
    ids4, w4 = skin_ref.compact(full, s.unknown, s.near, 4)
    assert np.abs(skin_ref.blend_linear(V0, ids4, w4, M) - skin_ref.blend_dqs(V0, ids4, w4, M)).max() > 1e-4
    eye = skin_ref.bone_transforms(joints, parents, np.zeros((1, 6, 3))).astype(np.float32)
    for kind in ("linear", "dqs"):
        assert np.array_equal(skin_ref.blend(V0, ids4, w4, eye, kind).astype(np.float32)[0], V0)
