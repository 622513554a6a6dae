"""Image sets the reference trains on, and their ground truth resident on the device in the 8 bits per sample the files hold.

Mirrors (reference file:line):
  scene/dataset_readers.py:194-262   readCamerasFromTransforms / readNerfSyntheticInfo    -> read_blender
  scene/dataset_readers.py:69-118, 145-192   readColmapCameras / readColmapSceneInfo      -> read_colmap
  scene/colmap_loader.py:43-53, 180-241      qvec2rotmat, read_extrinsics_binary, read_intrinsics_binary (COLMAP's documented
                                             binary model: cameras.bin / images.bin)
  scene/dataset_readers.py:46-67     getNerfppNorm                                        -> nerf_normalization
  scene/__init__.py:35-61            scene type by what the folder holds, cameras.json, cameras_extent   -> load_scene / write_cameras_json
  utils/camera_utils.py:18-55        loadCam: the -r rule, PILtoJittor (utils/general_utils.py:21-27) -> load_view

A view is described by a ViewInfo (paths and pose: nothing is decoded until load_view).  load_view returns a renderer.Camera and a
GroundTruth: rgb uint8 [3,H,W] and mask uint8 [1 or 3,H,W] (or None), resized by PIL on the 8-bit image exactly as PILtoJittor
does - the reference then divides by 255, so 8-bit storage loses nothing against it - 33 MB per 4K view instead of the 133 MB of a
float image plus a float mask.  loss.photometric_loss_u8 composites it inside the loss kernels; GroundTruth.float_target is the
reference's tensor expression, for tests and for callers of the float path.  The point cloud (points3D) is not read: the mesh-bound
model starts from the proxy mesh (MeshBoundGaussians.create_from_mesh).
"""
import json
import math
import os
import struct
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import io as gio
from . import scenes

_LUT = None


def _u8_to_unit():
    """float32 [256]: u / 255 correctly rounded (numpy's float32 division).  torch's `tensor / 255.0` on a GPU multiplies by the
    rounded reciprocal instead, which differs from the quotient for 126 of the 256 values; the reference (and torch on the CPU) divides."""
    global _LUT
    if _LUT is None:
        _LUT = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0))
    return _LUT


class GroundTruth:
    """One view's target as stored: rgb uint8 [3,H,W], mask uint8 [1,H,W] or [3,H,W] or None (contiguous, one device)."""

    def __init__(self, rgb_u8, mask_u8=None):
        if rgb_u8.dtype != torch.uint8 or rgb_u8.dim() != 3 or rgb_u8.shape[0] != 3:
            raise ValueError("GroundTruth: rgb must be uint8 [3,H,W] (got %s %s)" % (rgb_u8.dtype, tuple(rgb_u8.shape)))
        if mask_u8 is not None:
            if mask_u8.dtype != torch.uint8 or mask_u8.dim() != 3 or mask_u8.shape[0] not in (1, 3) or mask_u8.shape[1:] != rgb_u8.shape[1:]:
                raise ValueError("GroundTruth: mask must be uint8 [1,H,W] or [3,H,W] of the image's size (got %s %s)" % (
                    mask_u8.dtype, tuple(mask_u8.shape)))
            if mask_u8.device != rgb_u8.device:
                raise ValueError("GroundTruth: rgb and mask are on different devices")
            mask_u8 = mask_u8.contiguous()
        self.rgb, self.mask = rgb_u8.contiguous(), mask_u8

    @property
    def height(self):
        return int(self.rgb.shape[1])

    @property
    def width(self):
        return int(self.rgb.shape[2])

    @property
    def device(self):
        return self.rgb.device

    @property
    def nbytes(self):
        return self.rgb.numel() + (0 if self.mask is None else self.mask.numel())

    def to(self, device):
        return GroundTruth(self.rgb.to(device), None if self.mask is None else self.mask.to(device))

    def float_target(self, background=None):
        """float32 [3,H,W]: gt * mask + bg * (1 - mask) with gt = rgb/255, mask = mask/255 (train_mesh_gaussian.py:89-91 on what
        PILtoJittor made of the files), as separate tensor operations in that order; without a mask gt itself."""
        lut = _u8_to_unit().to(self.rgb.device)
        g = lut[self.rgb.long()]
        if self.mask is None:
            return g
        if background is None:
            raise ValueError("GroundTruth.float_target: a masked ground truth needs the background colour")
        m = lut[self.mask.long()]
        bg = background.to(device=g.device, dtype=torch.float32).reshape(3, 1, 1)
        return g * m + bg * (1 - m)


class ViewInfo(NamedTuple):
    """CameraInfo of scene/dataset_readers.py:26-37 with the files named instead of opened: mask_path None and alpha_mask False =
    no mask; alpha_mask True = the image's own alpha channel is the mask (Blender sets)."""
    uid: int
    R: np.ndarray
    T: np.ndarray
    FovY: float
    FovX: float
    image_path: str
    image_name: str
    width: int
    height: int
    mask_path: Optional[str] = None
    alpha_mask: bool = False


class SceneInfo(NamedTuple):
    train_cameras: list
    test_cameras: list
    nerf_normalization: dict
    kind: str


def focal2fov(focal, pixels):
    return 2 * math.atan(pixels / (2 * focal))


def fov2focal(fov, pixels):
    return pixels / (2 * math.tan(fov / 2))


def _world2view(R, t):
    """getWorld2View2 with no recentring (utils/graphics_utils.py:38-49), operation for operation - the 4x4 is inverted twice and
    then narrowed to float32 - so that nerf_normalization has the reference's bits."""
    Rt = np.zeros((4, 4))
    Rt[:3, :3] = R.transpose()
    Rt[:3, 3] = t
    Rt[3, 3] = 1.0
    C2W = np.linalg.inv(Rt)
    return np.float32(np.linalg.inv(C2W))


def nerf_normalization(views):
    """getNerfppNorm (:46-67): {"translate": -mean camera centre, "radius": 1.1 x the largest distance of a centre from the mean}."""
    centres = [np.linalg.inv(_world2view(v.R, v.T))[:3, 3:4] for v in views]
    centres = np.hstack(centres)
    centre = np.mean(centres, axis=1, keepdims=True)
    dist = np.linalg.norm(centres - centre, axis=0, keepdims=True)
    return {"translate": -centre.flatten(), "radius": np.max(dist) * 1.1}


def read_blender_transforms(path, transformsfile, extension=".png", max_frames=150):
    """readCamerasFromTransforms (:194-235): at most max_frames frames of one transforms file (the reference stops at 150)."""
    from PIL import Image
    views = []
    with open(os.path.join(path, transformsfile)) as f:
        contents = json.load(f)
    fovx = contents["camera_angle_x"]
    for idx, frame in enumerate(contents["frames"]):
        if max_frames is not None and idx >= max_frames:
            break
        image_path = os.path.join(path, frame["file_path"] + extension)
        c2w = np.array(frame["transform_matrix"])
        c2w[:3, 1:3] *= -1                       # OpenGL / Blender axes (y up, z back) -> COLMAP (y down, z forward)
        w2c = np.linalg.inv(c2w)
        R = np.transpose(w2c[:3, :3])            # stored transposed (the rasterizer's glm convention)
        T = w2c[:3, 3]
        with Image.open(image_path) as im:
            width, height = im.size
        fovy = focal2fov(fov2focal(fovx, width), height)
        views.append(ViewInfo(uid=idx, R=R, T=T, FovY=fovy, FovX=fovx, image_path=image_path,
                              image_name=os.path.splitext(os.path.basename(image_path))[0], width=width, height=height, alpha_mask=True))
    return views


def read_blender(path, eval=False, extension=".png", max_frames=150):
    """readNerfSyntheticInfo (:237-272) without its random point cloud: transforms_train.json, and transforms_val.json with eval."""
    train = read_blender_transforms(path, "transforms_train.json", extension, max_frames)
    test = read_blender_transforms(path, "transforms_val.json", extension, max_frames) if eval else []
    return SceneInfo(train, test, nerf_normalization(train), "Blender")


# COLMAP's camera models by id: (name, number of parameters)
_COLMAP_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8), 5: ("OPENCV_FISHEYE", 8),
                  6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4), 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}


def read_colmap_cameras_bin(path):
    """cameras.bin: uint64 count, then per camera int32 id, int32 model, uint64 width, uint64 height, float64 params[model]."""
    cams = {}
    with open(path, "rb") as f:
        n, = struct.unpack("<Q", f.read(8))
        for _ in range(n):
            cid, model, width, height = struct.unpack("<iiQQ", f.read(24))
            name, npar = _COLMAP_MODELS[model]
            cams[cid] = dict(id=cid, model=name, width=width, height=height, params=np.array(struct.unpack("<%dd" % npar, f.read(8 * npar))))
    return cams


def read_colmap_images_bin(path):
    """images.bin: uint64 count, then per image int32 id, float64 qvec[4], float64 tvec[3], int32 camera id, a zero-terminated
    name, uint64 number of 2-D points and that many (float64 x, float64 y, int64 point3D id), which are skipped."""
    images = {}
    with open(path, "rb") as f:
        n, = struct.unpack("<Q", f.read(8))
        for _ in range(n):
            rec = struct.unpack("<idddddddi", f.read(64))
            name = b""
            while True:
                ch = f.read(1)
                if ch in (b"\x00", b""):
                    break
                name += ch
            n2d, = struct.unpack("<Q", f.read(8))
            f.seek(24 * n2d, os.SEEK_CUR)
            images[rec[0]] = dict(id=rec[0], qvec=np.array(rec[1:5]), tvec=np.array(rec[5:8]), camera_id=rec[8], name=name.decode("utf-8"))
    return images


def qvec2rotmat(q):
    """Rotation matrix of COLMAP's (w, x, y, z) quaternion (scene/colmap_loader.py:43-53, COLMAP's read_write_model.py)."""
    return np.array([
        [1 - 2 * q[2] ** 2 - 2 * q[3] ** 2, 2 * q[1] * q[2] - 2 * q[0] * q[3], 2 * q[3] * q[1] + 2 * q[0] * q[2]],
        [2 * q[1] * q[2] + 2 * q[0] * q[3], 1 - 2 * q[1] ** 2 - 2 * q[3] ** 2, 2 * q[2] * q[3] - 2 * q[0] * q[1]],
        [2 * q[3] * q[1] - 2 * q[0] * q[2], 2 * q[2] * q[3] + 2 * q[0] * q[1], 1 - 2 * q[1] ** 2 - 2 * q[2] ** 2]])


def read_colmap(path, images=None, eval=False, is_exist_bg=False, llffhold=8):
    """readColmapSceneInfo / readColmapCameras (:69-118, 145-192) for the binary model in sparse/0: PINHOLE and SIMPLE_PINHOLE
    cameras, masks/<image_name>.png when the folder exists, views sorted by name, every llffhold-th held out with eval."""
    extr = read_colmap_images_bin(os.path.join(path, "sparse/0", "images.bin"))
    intr = read_colmap_cameras_bin(os.path.join(path, "sparse/0", "cameras.bin"))
    images_folder = os.path.join(path, "images" if images is None else images)
    masks_folder = os.path.join(os.path.dirname(images_folder), "masks")
    have_masks = os.path.exists(masks_folder)
    views = []
    for key in extr:
        e = extr[key]
        c = intr[e["camera_id"]]
        height, width = c["height"], c["width"]
        R = np.transpose(qvec2rotmat(e["qvec"]))
        T = np.array(e["tvec"])
        if c["model"] == "SIMPLE_PINHOLE":
            fovy, fovx = focal2fov(c["params"][0], height), focal2fov(c["params"][0], width)
        elif c["model"] == "PINHOLE":
            fovy, fovx = focal2fov(c["params"][1], height), focal2fov(c["params"][0], width)
        else:
            raise ValueError("Colmap camera model not handled: only undistorted datasets (PINHOLE or SIMPLE_PINHOLE cameras) supported!")
        image_path = os.path.join(images_folder, os.path.basename(e["name"]))
        image_name = os.path.basename(image_path).split(".")[0]
        mask_path = None
        if have_masks:
            mask_path = os.path.join(masks_folder, image_name + ".png")
        elif is_exist_bg:
            raise ValueError("You need mask to deform the scene!")
        views.append(ViewInfo(uid=c["id"], R=R, T=T, FovY=fovy, FovX=fovx, image_path=image_path, image_name=image_name, width=width,
                              height=height, mask_path=mask_path))
    views = sorted(views, key=lambda v: v.image_name)
    if eval:
        train = [v for i, v in enumerate(views) if i % llffhold != 0]
        test = [v for i, v in enumerate(views) if i % llffhold == 0]
    else:
        train, test = views, []
    return SceneInfo(train, test, nerf_normalization(train), "Colmap")


def load_scene(source_path, eval=False, is_exist_bg=False, images=None):
    """scene/__init__.py:35-41: a folder with sparse/ is a COLMAP set, one with transforms_train.json a Blender set."""
    if os.path.exists(os.path.join(source_path, "sparse")):
        return read_colmap(source_path, images, eval, is_exist_bg)
    if os.path.exists(os.path.join(source_path, "transforms_train.json")):
        return read_blender(source_path, eval)
    raise ValueError("Could not recognize scene type!")


def cameras_json_entries(scene):
    """scene/__init__.py:46-53: the test cameras, then the training cameras, numbered in that order."""
    return [gio.camera_to_json(i, v.R, v.T, v.width, v.height, v.FovX, v.FovY, v.image_name)
            for i, v in enumerate(list(scene.test_cameras) + list(scene.train_cameras))]


def write_cameras_json(scene, path):
    with open(path, "w") as f:
        json.dump(cameras_json_entries(scene), f)


def view_resolution(orig_w, orig_h, resolution=-1, resolution_scale=1.0):
    """loadCam's size rule (utils/camera_utils.py:20-39): -r 1/2/4/8 divides (rounded); -1 keeps images up to 1600 pixels wide and
    scales wider ones to 1600; any other value is the target width."""
    if resolution in (1, 2, 4, 8):
        return round(orig_w / (resolution_scale * resolution)), round(orig_h / (resolution_scale * resolution))
    if resolution == -1:
        down = orig_w / 1600 if orig_w > 1600 else 1
    else:
        down = orig_w / resolution
    scale = float(down) * float(resolution_scale)
    return int(orig_w / scale), int(orig_h / scale)


def _planes(pil_image, size):
    """PILtoJittor before its division (utils/general_utils.py:21-27): PIL's resize of the 8-bit image, channels first."""
    a = np.array(pil_image.resize(size))
    if a.dtype != np.uint8:
        raise ValueError("dataset: only 8-bit images and masks are supported (got %s from mode %r)" % (a.dtype, pil_image.mode))
    return a[None] if a.ndim == 2 else np.ascontiguousarray(a.transpose(2, 0, 1))


def load_view_arrays(view, resolution=-1, resolution_scale=1.0):
    """(rgb uint8 [3,H,W], mask uint8 [Cm,H,W] or None) of a view at loadCam's size.  A Blender image's alpha channel is the mask
    (dataset_readers.py:221-227 hands loadCam the alpha repeated on three equal channels, which PIL resizes alike: one plane here);
    a COLMAP mask file keeps the channels it has - an RGB mask three planes, an L mask one."""
    from PIL import Image
    with Image.open(view.image_path) as im:
        im.load()
        size = view_resolution(im.size[0], im.size[1], resolution, resolution_scale)
        mask = None
        if view.alpha_mask:
            alpha = np.array(im.convert("RGBA"))[:, :, 3]
            mask = _planes(Image.fromarray(alpha, "L"), size)
        if im.mode not in ("RGB", "RGBA"):
            im = im.convert("RGB")
        rgb = _planes(im, size)[:3]
    if view.mask_path is not None:
        with Image.open(view.mask_path) as mk:
            mask = _planes(mk, size)
        if mask.shape[0] not in (1, 3):
            raise ValueError("dataset: mask %s has %d channels; 1 or 3 expected" % (view.mask_path, mask.shape[0]))
    return np.ascontiguousarray(rgb), mask


def load_view(view, resolution=-1, resolution_scale=1.0, device="cuda"):
    """loadCam (utils/camera_utils.py:18-55): (renderer.Camera, GroundTruth) of a ViewInfo; the camera also carries image_name, uid,
    R, T as the reference's does."""
    from .renderer import Camera
    rgb, mask = load_view_arrays(view, resolution, resolution_scale)
    H, W = rgb.shape[1], rgb.shape[2]
    cam = Camera(scenes.camera_from_RT(view.R, view.T, view.FovX, view.FovY, W, H), device)
    cam.image_name, cam.uid, cam.R, cam.T = view.image_name, view.uid, view.R, view.T
    gt = GroundTruth(torch.from_numpy(rgb).to(device), None if mask is None else torch.from_numpy(mask).to(device))
    return cam, gt


def load_views(views, resolution=-1, resolution_scale=1.0, device="cuda"):
    """cameraList_from_camInfos (:56-62): [(Camera, GroundTruth)]."""
    return [load_view(v, resolution, resolution_scale, device) for v in views]
