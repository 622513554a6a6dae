"""Generates tests/golden/dataset/ (a tiny Blender set and a tiny COLMAP set), dataset_expected.npz and mesh_init.npz by EXECUTING the
reference's dataset readers, loadCam, Camera and create_from_pcd on this package's torch-backed `jittor` subset
(gaussianmesh_amd.compat), as make_golden_model.py / make_golden_bg_model.py do for the model classes.

Runs only where the reference tree is available, GM_REFERENCE_TREE=<its path> (the fixtures are committed; the tests never read it).
The two image sets are made here (seeded numpy noise + gradients, written through PIL; cameras.bin / images.bin written with struct
from COLMAP's documented binary format); everything in the two .npz files is what the reference's code RETURNED for them.

Stand-ins, and what they do:
  plyfile          not installed; the readers only use it for the point cloud, which this package does not read: PlyElement.describe /
                   PlyData.write do nothing, PlyData.read raises (the readers catch that and carry point_cloud = None).
  igl              not installed: gaussianmesh_amd.compat.igl_subset.  read_triangle_mesh reads the OBJ; per_face_normals implements
                   libigl's documented rule: the unit normal (v1 - v0) x (v2 - v0) / |.| of every face, and the given fallback vector Z
                   for a face whose cross product has zero length (a degenerate face; create_from_pcd passes Z = (1, 0, 0)).
  distCUDA2        CUDA; replaced by oracle.knn_mean_dist2 (the CPU oracle of gm_knn, oracle/oracle.py) - so "scaling" in mesh_init.npz is
                   the oracle's, and the GPU test compares the scales against the HIP operator instead.
  PIL.Image.fromarray   the installed Pillow refuses the int8 array readCamerasFromTransforms (:227) hands it with mode "RGB" (older releases
                   reinterpreted the bytes): inside the readers module `Image.fromarray` first views int8 as uint8 - the same bytes.
  np.random.random seeded (np.random.seed) before create_from_pcd, and its draw recorded ("draw").
The point-cloud files the readers would create next to the images are kept out of the fixture: the readers run on a temporary copy
that already holds empty points3d.ply / points3D.ply files.

Reference code executed (file:line):
  scene/dataset_readers.py:194-272     readCamerasFromTransforms, readNerfSyntheticInfo
  scene/dataset_readers.py:69-118, 145-192   readColmapCameras, readColmapSceneInfo  (scene/colmap_loader.py binary readers, qvec2rotmat)
  scene/dataset_readers.py:46-67       getNerfppNorm
  utils/camera_utils.py:18-55, 63-83   loadCam (PILtoJittor, utils/general_utils.py:21-27), camera_to_JSON
  scene/cameras.py:18-51               Camera
  train_mesh_gaussian.py:89-91         the composite gt * mask + bg * (1 - mask), restated here on the reference Camera's tensors
  scene/mesh_based_gaussian_model.py:183-240   create_from_pcd
"""
import importlib.util
import json
import math
import os
import shutil
import struct
import sys
import tempfile
import types

import numpy as np

REF = os.environ.get("GM_REFERENCE_TREE", "")
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, ROOT)
DATA = os.path.join(OUT, "dataset")


def _load(name, relpath):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _pose(k, n, radius=4.0):
    """camera-to-world of a camera on a circle looking at the origin, OpenGL axes (x right, y up, z back), as Blender writes it"""
    a = 2 * math.pi * k / n + 0.3
    eye = np.array([radius * math.cos(a), radius * math.sin(a), 1.0 + 0.2 * k])
    back = eye / np.linalg.norm(eye)
    right = np.cross(np.array([0.0, 0.0, 1.0]), back); right /= np.linalg.norm(right)
    up = np.cross(back, right)
    M = np.eye(4)
    M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = right, up, back, eye
    return M


def _image(rng, w, h, channels):
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 255 // max(w + h - 2, 1))], -1)
    img = np.clip(base + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)
    if channels == 4:
        d = np.hypot(xx - w / 2, yy - h / 2) / (0.5 * min(w, h))
        alpha = np.clip(255 * (1.3 - d) + rng.integers(-30, 31, (h, w)), 0, 255).astype(np.uint8)
        img = np.concatenate([img, alpha[..., None]], -1)
    return img


def make_blender(rng):
    from PIL import Image
    root = os.path.join(DATA, "blender")
    for split, n in (("train", 4), ("val", 2)):
        os.makedirs(os.path.join(root, split), exist_ok=True)
        frames = []
        for k in range(n):
            Image.fromarray(_image(rng, 24, 16, 4), "RGBA").save(os.path.join(root, split, "r_%d.png" % k))
            frames.append({"file_path": "./%s/r_%d" % (split, k), "transform_matrix": _pose(k + (0 if split == "train" else 4), 6).tolist()})
        with open(os.path.join(root, "transforms_%s.json" % split), "w") as f:
            json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames}, f, indent=1)
    return root


def make_colmap(rng):
    """9 views of two cameras (PINHOLE 26x18, SIMPLE_PINHOLE 22x14): with eval, views 0 and 8 of the sorted list are held out."""
    from PIL import Image
    root = os.path.join(DATA, "colmap")
    for d in ("sparse/0", "images", "masks"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    cams = [(1, 1, 26, 18, (30.5, 29.25, 13.0, 9.0)), (2, 0, 22, 14, (25.75, 11.0, 7.0))]
    with open(os.path.join(root, "sparse/0/cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(cams)))
        for cid, model, w, h, params in cams:
            f.write(struct.pack("<iiQQ", cid, model, w, h) + struct.pack("<%dd" % len(params), *params))
    order = [5, 2, 8, 0, 3, 7, 1, 6, 4]                        # file order differs from name order: the reader sorts by name
    with open(os.path.join(root, "sparse/0/images.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(order)))
        for k in order:
            q = rng.normal(size=4); q /= np.linalg.norm(q)
            if q[0] < 0:
                q = -q
            t = rng.normal(size=3) * 2
            cid, model, w, h, _ = cams[k % 2]
            name = "view_%02d.png" % k
            f.write(struct.pack("<idddddddi", 100 + k, *q, *t, cid) + name.encode() + b"\x00")
            pts = [(1.5 * j, 2.5 * j, -1) for j in range(k % 3)]      # a few 2-D points the reader has to step over
            f.write(struct.pack("<Q", len(pts)))
            for p in pts:
                f.write(struct.pack("<ddq", *p))
            Image.fromarray(_image(rng, w, h, 3), "RGB").save(os.path.join(root, "images", name))
            if k % 2 == 0:                                       # RGB mask with unequal channels
                Image.fromarray(_image(rng, w, h, 3), "RGB").save(os.path.join(root, "masks", "view_%02d.png" % k))
            else:                                                # single-channel mask
                Image.fromarray(_image(rng, w, h, 4)[..., 3], "L").save(os.path.join(root, "masks", "view_%02d.png" % k))
    return root


def main():
    assert os.path.isdir(REF), "set GM_REFERENCE_TREE to the reference checkout; the fixtures can only be regenerated there"
    import gaussianmesh_amd.compat as compat
    from gaussianmesh_amd.compat import igl_subset
    from gaussianmesh_amd import io as gio
    from oracle import oracle as orc
    jt = compat.install(force=True, operators=True)
    import torch

    ply = types.ModuleType("plyfile")

    class _NoPly:
        @staticmethod
        def describe(*a, **k):
            return None

        def __init__(self, *a, **k):
            pass

        def write(self, path):
            pass

        @staticmethod
        def read(path):
            raise IOError("no point cloud in this fixture")
    ply.PlyData = ply.PlyElement = _NoPly
    sys.modules["plyfile"] = ply
    sys.modules["igl"] = igl_subset
    pkg = types.ModuleType("scene"); pkg.__path__ = [os.path.join(REF, "scene")]      # keep scene/__init__.py out
    sys.modules["scene"] = pkg
    knn = types.ModuleType("scene.simple_knn")
    knn.distCUDA2 = lambda pts: jt.array(orc.knn_mean_dist2(pts.detach().cpu().numpy()))
    sys.modules["scene.simple_knn"] = knn
    sys.path.insert(0, REF)
    dr = _load("ref_dataset_readers", "scene/dataset_readers.py")
    cu = _load("ref_camera_utils", "utils/camera_utils.py")
    mm = _load("ref_mesh_model", "scene/mesh_based_gaussian_model.py")
    from PIL import Image as _PILImage
    shim = types.SimpleNamespace(open=_PILImage.open,
                                 fromarray=lambda a, mode=None: _PILImage.fromarray(a.view(np.uint8) if a.dtype == np.int8 else a, mode))
    dr.Image = shim

    if os.path.isdir(DATA):
        shutil.rmtree(DATA)
    rng = np.random.default_rng(20261016)
    make_blender(rng)
    make_colmap(rng)
    tmp = tempfile.mkdtemp()
    out = {}
    t = lambda x: np.ascontiguousarray(x.detach().cpu().numpy())
    try:
        work = os.path.join(tmp, "dataset")
        shutil.copytree(DATA, work)
        open(os.path.join(work, "blender", "points3d.ply"), "wb").close()
        open(os.path.join(work, "colmap", "sparse/0/points3D.ply"), "wb").close()
        scenes_ = {"blender": dr.readNerfSyntheticInfo(os.path.join(work, "blender"), False, True),
                   "colmap": dr.readColmapSceneInfo(os.path.join(work, "colmap"), None, True, True)}
        noeval = {"blender": dr.readNerfSyntheticInfo(os.path.join(work, "blender"), False, False),
                  "colmap": dr.readColmapSceneInfo(os.path.join(work, "colmap"), None, False, False)}
        for name, info in scenes_.items():
            out[name + "_noeval_train_names"] = np.array([c.image_name for c in noeval[name].train_cameras])
            out[name + "_noeval_n_test"] = np.int64(len(noeval[name].test_cameras))
            out[name + "_noeval_radius"] = np.float64(noeval[name].nerf_normalization["radius"])
            out[name + "_translate"] = np.asarray(info.nerf_normalization["translate"])
            out[name + "_radius"] = np.float64(info.nerf_normalization["radius"])
            camlist = list(info.test_cameras) + list(info.train_cameras)           # scene/__init__.py:46-53
            out[name + "_cameras_json"] = np.array(json.dumps([cu.camera_to_JSON(i, c) for i, c in enumerate(camlist)]))
            for split, cams in (("train", info.train_cameras), ("test", info.test_cameras)):
                key = "%s_%s_" % (name, split)
                out[key + "names"] = np.array([c.image_name for c in cams])
                out[key + "uid"] = np.array([c.uid for c in cams], np.int64)
                out[key + "R"] = np.array([c.R for c in cams]); out[key + "T"] = np.array([c.T for c in cams])
                out[key + "FovX"] = np.array([c.FovX for c in cams], np.float64); out[key + "FovY"] = np.array([c.FovY for c in cams], np.float64)
                out[key + "size"] = np.array([(c.width, c.height) for c in cams], np.int64)
                for i, c in enumerate(cams):
                    for r in (1, 2):
                        cam = cu.loadCam(types.SimpleNamespace(resolution=r), i, c, 1.0)
                        k2 = "%s%d_r%d_" % (key, i, r)
                        out[k2 + "image"] = t(cam.original_image)                    # float32 [3,H,W] = bytes / 255
                        out[k2 + "mask"] = t(cam.mask)
                        if r == 1:
                            out[k2 + "view"] = t(cam.world_view_transform); out[k2 + "proj"] = t(cam.full_proj_transform)
                            out[k2 + "projection"] = t(cam.projection_matrix); out[k2 + "center"] = t(cam.camera_center)
                            out[k2 + "fov"] = np.array([cam.FoVx, cam.FoVy], np.float64)
                        if split == "train" and i == 0:
                            bg = jt.array(np.array([0.25, 0.6640625, 0.9]), dtype=jt.float32) if r == 1 else jt.array(rng.random(3), dtype=jt.float32)
                            gt_image = cam.original_image * cam.mask + (jt.unsqueeze(jt.unsqueeze(bg, 1), 1)) * (1 - cam.mask)
                            out[k2 + "bg"] = t(bg); out[k2 + "composite"] = t(gt_image)
        # loadCam's other size rules, on a view of the COLMAP set: the default (-1) and an explicit width
        c = scenes_["colmap"].train_cameras[0]
        for r in (-1, 13):
            cam = cu.loadCam(types.SimpleNamespace(resolution=r), 0, c, 1.0)
            out["colmap_train_0_r%d_image" % r] = t(cam.original_image)
    finally:
        shutil.rmtree(tmp)
    np.savez_compressed(os.path.join(OUT, "dataset_expected.npz"), **out)

    # ---- create_from_pcd on a small mesh with one degenerate face ----------------------------------------------------------------
    from gaussianmesh_amd import scenes
    verts, faces = scenes.torus_mesh(5, 4)
    verts = np.round(verts, 6)
    faces = np.concatenate([faces, np.array([[0, 0, 7]], np.int32)], 0)             # two equal corners: zero-length cross product
    tmp = tempfile.mkdtemp()
    try:
        obj = os.path.join(tmp, "mesh.obj")
        gio.write_obj(obj, verts, faces)
        seed = 424242
        np.random.seed(seed)
        draw = np.random.random((faces.shape[0], 3))
        np.random.seed(seed)
        g = mm.MeshBasedGaussianModel(3, obj)
        g.create_from_pcd(None, 1.0)
        v_read, f_read = igl_subset.read_triangle_mesh(obj)
    finally:
        shutil.rmtree(tmp)
    fix = dict(vertices=v_read, faces=f_read, seed=np.int64(seed), draw=draw, bc=t(g._bc), distance=t(g._distance), features_dc=t(g._features_dc),
               features_rest=t(g._features_rest), scaling=t(g._scaling), rotation=t(g._rotation), opacity=t(g._opacity), vertex1=t(g.vertex1),
               vertex2=t(g.vertex2), vertex3=t(g.vertex3), normal=t(g.normal), r=t(g.r), fid=t(g.fid), vertex_index=t(g.vertex_index), v=t(g.v))
    assert np.array_equal(fix["normal"][-1], [1.0, 0.0, 0.0]), "the degenerate face takes the fallback normal"
    np.savez_compressed(os.path.join(OUT, "mesh_init.npz"), **fix)
    size = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(DATA) for f in fs)
    print("wrote dataset/ (%d bytes), dataset_expected.npz (%d arrays, %d bytes), mesh_init.npz (%d faces, %d bytes)" % (
        size, len(out), os.path.getsize(os.path.join(OUT, "dataset_expected.npz")), faces.shape[0], os.path.getsize(os.path.join(OUT, "mesh_init.npz"))))


if __name__ == "__main__":
    main()
