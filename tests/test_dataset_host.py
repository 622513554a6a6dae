"""Host side of training from a dataset: both readers, load_view and GroundTruth.float_target against tests/golden/dataset_expected.npz
(what the reference's readers, loadCam and Camera returned for tests/golden/dataset/, make_golden_dataset.py), the first model's host
tensors against mesh_init.npz (create_from_pcd executed), the ABI of the two 8-bit loss entry points, and the CLI's refusals."""
import json
import os
import re
import shutil

import numpy as np
import pytest
import torch

_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_DATA = os.path.join(_GOLD, "dataset")
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def exp():
    return np.load(os.path.join(_GOLD, "dataset_expected.npz"))


def _scene(name, **kw):
    from gaussianmesh_amd import dataset
    return dataset.load_scene(os.path.join(_DATA, name), **kw)


@pytest.mark.parametrize("name", ["blender", "colmap"])
def test_reader_matches_the_reference(name, exp):
    """Poses, fields of view, sizes, names, split and nerf_normalization: the readers use the reference's numpy operations in its
    order, so everything is compared EXACTLY (float64 bits)."""
    from gaussianmesh_amd import dataset
    sc = _scene(name, eval=True, is_exist_bg=True)
    assert sc.kind == {"blender": "Blender", "colmap": "Colmap"}[name]
    for split, views in (("train", sc.train_cameras), ("test", sc.test_cameras)):
        key = "%s_%s_" % (name, split)
        assert [v.image_name for v in views] == list(exp[key + "names"])
        assert [v.uid for v in views] == list(exp[key + "uid"])
        assert np.array_equal(np.array([v.R for v in views]), exp[key + "R"])
        assert np.array_equal(np.array([v.T for v in views]), exp[key + "T"])
        assert np.array_equal(np.array([v.FovX for v in views]), exp[key + "FovX"])
        assert np.array_equal(np.array([v.FovY for v in views]), exp[key + "FovY"])
        assert np.array_equal(np.array([(v.width, v.height) for v in views]), exp[key + "size"])
    assert np.array_equal(sc.nerf_normalization["translate"], exp[name + "_translate"])
    assert sc.nerf_normalization["radius"] == float(exp[name + "_radius"])
    # the eval split: Blender holds out transforms_val.json, COLMAP every 8th view of the name-sorted list
    if name == "colmap":
        assert [v.image_name for v in sc.test_cameras] == ["view_00", "view_08"] and len(sc.train_cameras) == 7
    else:
        assert len(sc.train_cameras) == 4 and len(sc.test_cameras) == 2
    plain = _scene(name)
    assert [v.image_name for v in plain.train_cameras] == list(exp[name + "_noeval_train_names"])
    assert len(plain.test_cameras) == int(exp[name + "_noeval_n_test"]) == 0
    assert plain.nerf_normalization["radius"] == float(exp[name + "_noeval_radius"])
    # cameras.json: the reference's entries (test cameras first), through io.camera_to_json - the same numpy operations
    assert dataset.cameras_json_entries(sc) == json.loads(str(exp[name + "_cameras_json"]))


@pytest.mark.parametrize("name", ["blender", "colmap"])
def test_load_view_planes_sizes_and_camera(name, exp):
    """8-bit planes EXACTLY (the reference's float image is bytes / 255: compared as float32(bytes) / 255 bit for bit), at -r 1 and
    -r 2.  The camera matrices come from scenes.camera_from_RT, which is not the reference's sequence of operations:
      view        world2view2 solves A c = -t once where getWorld2View2 inverts the 4x4 twice      bound: 4 ulp of the largest entry
      proj        float64 tan / divisions narrowed to float32, and a numpy float32 matmul, where the reference fills a float32
                  matrix and multiplies with bmm                                                   bound: 8 ulp of the largest entry
      centre      inverse of the float32 view matrix by numpy instead of jt.linalg.inv             bound: 8 ulp of the largest entry
    (a float32 product or inverse of 4x4 matrices of O(1) condition carries a few ulps of its largest entry)."""
    from gaussianmesh_amd import dataset
    sc = _scene(name, eval=True, is_exist_bg=True)
    lut = np.arange(256, dtype=np.float32) / np.float32(255.0)
    for split, views in (("train", sc.train_cameras), ("test", sc.test_cameras)):
        for i, v in enumerate(views):
            for r in (1, 2):
                key = "%s_%s_%d_r%d_" % (name, split, i, r)
                cam, gt = dataset.load_view(v, resolution=r, device="cpu")
                ref_img, ref_mask = exp[key + "image"], exp[key + "mask"]
                assert gt.rgb.dtype == torch.uint8 and tuple(gt.rgb.shape) == ref_img.shape
                assert (cam.image_height, cam.image_width) == ref_img.shape[1:]
                if r == 2:
                    assert (cam.image_width, cam.image_height) == (round(v.width / 2), round(v.height / 2))
                assert np.array_equal(lut[gt.rgb.numpy()].view(np.int32), ref_img.view(np.int32)), key
                mine = lut[gt.mask.numpy()]
                if name == "blender":            # the reference carries the alpha on three equal planes; one plane here
                    assert mine.shape[0] == 1 and ref_mask.shape[0] == 3
                    mine = np.broadcast_to(mine, ref_mask.shape)
                assert mine.shape == ref_mask.shape and np.array_equal(np.ascontiguousarray(mine).view(np.int32), ref_mask.view(np.int32)), key
                if r == 1:
                    assert np.array_equal(np.array([cam.FoVx, cam.FoVy]), exp[key + "fov"])
                    for mat, ref, ulps in ((cam.world_view_transform, exp[key + "view"], 4), (cam.full_proj_transform, exp[key + "proj"], 8),
                                           (cam.camera_center, exp[key + "center"], 8)):
                        err = np.abs(mat.numpy().astype(np.float64) - ref.astype(np.float64)).max()
                        assert err <= ulps * ULP * np.abs(ref).max(), (key, err)
    masks = {v.image_name: dataset.load_view_arrays(v, 1)[1].shape[0] for v in sc.train_cameras + sc.test_cameras}
    if name == "colmap":                         # an RGB mask keeps its three planes, an L mask its one
        assert masks["view_02"] == 3 and masks["view_01"] == 1 and set(masks.values()) == {1, 3}
        v = sc.train_cameras[0]
        for r in (-1, 13):                       # loadCam's other size rules
            rgb, _ = dataset.load_view_arrays(v, r)
            assert np.array_equal(lut[rgb].view(np.int32), exp["colmap_train_0_r%d_image" % r].view(np.int32))


def test_view_resolution_rule():
    from gaussianmesh_amd.dataset import view_resolution
    assert view_resolution(800, 600, 1) == (800, 600) and view_resolution(801, 601, 2) == (round(801 / 2), round(601 / 2))
    assert view_resolution(800, 600, 8) == (100, 75) and view_resolution(800, 600, 4, 2.0) == (100, 75)
    assert view_resolution(1600, 1200, -1) == (1600, 1200)
    assert view_resolution(3840, 2160, -1) == (1600, 900)                  # the 1600-pixel default
    assert view_resolution(3840, 2160, 960) == (960, 540)                  # a target width
    assert view_resolution(1000, 700, 3) == (3, 2)                         # 3 is not one of 1/2/4/8: a width, as in the reference


@pytest.mark.parametrize("name", ["blender", "colmap"])
def test_float_target_equals_the_reference_composite(name, exp):
    from gaussianmesh_amd import dataset
    sc = _scene(name, eval=True, is_exist_bg=True)
    for r in (1, 2):
        key = "%s_train_0_r%d_" % (name, r)
        _, gt = dataset.load_view(sc.train_cameras[0], resolution=r, device="cpu")
        got = gt.float_target(torch.from_numpy(exp[key + "bg"]))
        assert got.dtype == torch.float32
        assert np.array_equal(got.numpy().view(np.int32), exp[key + "composite"].view(np.int32)), key
    rgb_only = dataset.GroundTruth(gt.rgb)
    assert np.array_equal(rgb_only.float_target().numpy().view(np.int32), exp[key + "image"].view(np.int32))
    assert gt.nbytes == gt.rgb.numel() + gt.mask.numel()
    with pytest.raises(ValueError):
        gt.float_target(None)


def test_u8_quotients_are_correctly_rounded():
    from gaussianmesh_amd.dataset import _u8_to_unit
    lut = _u8_to_unit().numpy()
    exact = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    assert np.array_equal(lut.view(np.int32), exact.view(np.int32))
    wrong = (np.arange(256, dtype=np.float32) * (np.float32(1.0) / np.float32(255.0)))
    assert int((wrong != exact).sum()) == 126                               # why the kernels divide


def test_blender_frame_cap_and_refusals(tmp_path):
    from gaussianmesh_amd import dataset
    src = os.path.join(_DATA, "blender")
    dst = tmp_path / "many"
    shutil.copytree(src, dst)
    with open(dst / "transforms_train.json") as f:
        tr = json.load(f)
    tr["frames"] = [tr["frames"][k % 4] for k in range(153)]
    with open(dst / "transforms_train.json", "w") as f:
        json.dump(tr, f)
    assert len(dataset.read_blender(str(dst)).train_cameras) == 150        # the reference's cap
    assert len(dataset.read_blender(str(dst), max_frames=7).train_cameras) == 7
    assert len(dataset.read_blender(str(dst), max_frames=None).train_cameras) == 153
    # COLMAP: no masks + is_exist_bg, and a camera model that is not (SIMPLE_)PINHOLE
    col = tmp_path / "colmap"
    shutil.copytree(os.path.join(_DATA, "colmap"), col)
    shutil.rmtree(col / "masks")
    assert all(v.mask_path is None for v in dataset.read_colmap(str(col)).train_cameras)
    with pytest.raises(ValueError, match="You need mask to deform the scene!"):
        dataset.read_colmap(str(col), is_exist_bg=True)
    raw = bytearray(open(col / "sparse/0/cameras.bin", "rb").read())
    import struct
    struct.pack_into("<i", raw, 8 + 4, 2)        # first camera: PINHOLE (4 parameters) -> SIMPLE_RADIAL (4 parameters)
    open(col / "sparse/0/cameras.bin", "wb").write(bytes(raw))
    with pytest.raises(ValueError, match=re.escape("only undistorted datasets (PINHOLE or SIMPLE_PINHOLE cameras) supported!")):
        dataset.read_colmap(str(col))
    with pytest.raises(ValueError, match="Could not recognize scene type!"):
        dataset.load_scene(str(tmp_path))


def test_create_from_mesh_host_tensors_match_create_from_pcd():
    """mesh_init.npz: the tensors the reference's create_from_pcd made of a 41-face mesh whose last face is degenerate, with
    np.random seeded.  Everything but the scales (distCUDA2: GPU) is compared exactly, given the same draw."""
    from gaussianmesh_amd.renderer import MeshBoundGaussians
    fix = np.load(os.path.join(_GOLD, "mesh_init.npz"))
    rs = np.random.RandomState(int(fix["seed"]))
    t = MeshBoundGaussians.mesh_init_tensors(fix["vertices"], fix["faces"], 3, rs)
    assert np.array_equal(np.random.RandomState(int(fix["seed"])).random((fix["faces"].shape[0], 3)), fix["draw"])
    for key in ("bc", "distance", "features_dc", "features_rest", "rotation", "opacity", "vertex1", "vertex2", "vertex3", "normal", "r", "fid",
                "vertex_index", "v"):
        got = t[key].numpy()
        assert got.shape == fix[key].shape, key
        if got.dtype == np.float32:
            assert fix[key].dtype == np.float32 and np.array_equal(got.view(np.int32), fix[key].view(np.int32)), key
        else:
            assert np.array_equal(got, fix[key]), key
    assert np.array_equal(t["normal"][-1].numpy(), [1.0, 0.0, 0.0])        # igl's fallback for the degenerate face
    # the global numpy stream is what the reference draws from
    np.random.seed(int(fix["seed"]))
    t2 = MeshBoundGaussians.mesh_init_tensors(fix["vertices"], fix["faces"], 3)
    assert torch.equal(t2["features_dc"], t["features_dc"])
    with pytest.raises(Exception):               # the scales need the device: no CPU path
        MeshBoundGaussians.create_from_mesh(fix["vertices"], fix["faces"], device="cpu")


def test_save_ply_fills_the_reference_columns(tmp_path):
    """x,y,z = get_xyz, ca,cb,cc = raw _bc, the rest raw: the rows io.save_mesh_gaussians pins against the reference's writer
    (tests/golden/mesh_ply.npz) for the same model."""
    from gaussianmesh_amd import io as gio
    from gaussianmesh_amd.renderer import MeshBoundGaussians
    fix = np.load(os.path.join(_GOLD, "mesh_ply.npz"))
    t = lambda k: torch.tensor(fix[k])
    m = MeshBoundGaussians(t("bc"), t("distance"), t("features_dc"), t("features_rest"), t("scaling"), t("rotation"), t("opacity"), t("v1"), t("v2"),
                           t("v3"), t("normal"), t("radius"), fid=t("fid").to(torch.int32), vertex_index=t("vertex_index").to(torch.int32))
    path = tmp_path / "point_cloud" / "iteration_7" / "point_cloud.ply"
    m.save_ply(str(path))
    names, rows = gio.read_ply(str(path))
    assert names == list(fix["names"])
    xyz = names.index("x")
    assert np.array_equal(np.delete(rows, [xyz, xyz + 1, xyz + 2], axis=1), np.delete(fix["elements"], [xyz, xyz + 1, xyz + 2], axis=1))
    assert np.allclose(rows[:, xyz:xyz + 3], fix["elements"][:, xyz:xyz + 3], rtol=0, atol=4 * ULP * np.abs(fix["xyz"]).max())   # get_xyz: torch vs the shim's sums
    loaded = gio.load_mesh_gaussians(str(path), bc_from_xyz=True)
    assert np.array_equal(loaded["bc"], rows[:, xyz:xyz + 3])              # what the edit tool's loader takes for _bc


def test_u8_loss_entry_points_abi():
    """Header and _lib agree on gm_ssim_fwd_u8 / gm_ssim_bwd_u8; every refusal is decided on the arguments alone (no device)."""
    import ctypes as C
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for name, nargs in (("gm_ssim_fwd_u8", 13), ("gm_ssim_bwd_u8", 15)):
        assert name in _lib.header_symbols() and hasattr(l, name)
        decl = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, hdr, flags=re.S).group(1)
        params = [p.strip() for p in decl.split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.i32 and len(args) == len(params) == nargs
        for p, a in zip(params, args):
            want = _lib.vp if "*" in p else (_lib.i64 if p.startswith("int64_t") else _lib.i32)
            assert a is want, (name, p)
    assert l.gm_abi_version() == 3
    one = 4096
    fwd = lambda rgb=one, mask=one, stride=0, bg=one, planes=3, H=8, W=8, maps=(one, one, one), img=one: l.gm_ssim_fwd_u8(
        img, rgb, mask, stride, bg, planes, H, W, maps[0], maps[1], maps[2], one, None)
    assert fwd(planes=0) == 0 and fwd(H=0) == 0                            # empty: nothing to do
    assert fwd(planes=-1) == 1
    assert fwd(planes=4) == 1 and b"3 planes" in l.gm_last_error()
    assert fwd(rgb=None) == 1 and b"null rgb" in l.gm_last_error()
    assert fwd(bg=None) == 1 and b"background" in l.gm_last_error()
    assert fwd(stride=63) == 1 and b"mask_plane_stride" in l.gm_last_error()
    assert fwd(maps=(one, None, one)) == 1 and b"all three" in l.gm_last_error()
    assert fwd(img=None) == 1
    bwd = lambda rgb=one, mask=one, stride=0, bg=one, planes=3, g=one, out=one: l.gm_ssim_bwd_u8(
        one, rgb, mask, stride, bg, one, one, one, planes, 8, 8, g, None, out, None)
    assert bwd(planes=1) == 1 and bwd(rgb=None) == 1 and bwd(bg=None) == 1 and bwd(g=None) == 1 and bwd(out=None) == 1
    assert bwd(stride=-64) == 1


def test_train_mesh_cli_refusals(tmp_path, capsys):
    from gaussianmesh_amd import train_mesh
    src = os.path.join(_DATA, "blender")
    for argv in (["-m", str(tmp_path / "o"), "--input_mesh", "x.obj"],                                   # no source
                 ["-s", src, "--input_mesh", "x.obj"],                                                   # no output folder
                 ["-s", src, "-m", str(tmp_path / "o")],                                                 # no mesh
                 ["-s", src, "-m", str(tmp_path / "o"), "--input_mesh", "x.obj", "--iterations", "0"],
                 ["-s", src, "-m", str(tmp_path / "o"), "--input_mesh", "x.obj", "--sh_degree", "4"],
                 ["-s", src, "-m", str(tmp_path / "o"), "--input_mesh", str(tmp_path / "missing.obj")],
                 ["-s", str(tmp_path / "nowhere"), "-m", str(tmp_path / "o"), "--input_mesh", os.path.join(src, "transforms_train.json")]):
        with pytest.raises(SystemExit) as e:
            train_mesh.main(argv)
        assert e.value.code == 2, argv
    assert not (tmp_path / "o").exists()                                    # refused before anything is written
