"""Per-Gaussian blend weights: lift the data set's 2-D masks onto a trained cloud, prune a cloud by contribution.

For every Gaussian the blend weight alpha_i T_i - the factor the colour blend multiplies its colour by - is summed over the pixels
inside and outside a mask, over all views (gm_blend_weights: one more walk of the frame's tile lists with the arithmetic of the
GM_FWD_EXACT_EXPONENT blend, scattering per Gaussian).  The ratio inside / total separates THE OBJECT from THE SCENE
(select, split_plain: the two clouds SingleObjectDeform.from_plain / --background_gaussian take); the same sums with an all-ones mask
are the usual importance score for pruning (importance_rows).  The accumulators are integers: a result does not depend on the emission
policy, on the order of the views or on the run.

    python -m gaussianmesh_amd.contribution --gaussian scene.ply -s DATA --out_object obj.ply --out_background bg.ply
"""
import argparse
import json
import os
import sys
import time
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import GmeshError
from ._op import enqueue, need_cuda

WEIGHT_UNIT = 2.0 ** -24          # sums[:, 0] counts weights in this unit, sums[:, 1] in WEIGHT_UNIT / 255 (mask bytes 0..255)


def _check(name, t, dtype, shape, device):
    if not isinstance(t, torch.Tensor):
        raise GmeshError("blend_weights: %s must be a tensor" % name)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise GmeshError("blend_weights: %s must be %s %s (got %s %s)" % (name, dtype, list(shape), t.dtype, list(t.shape)))
    if t.device != device:
        raise GmeshError("blend_weights: %s is on %s, the frame on %s" % (name, t.device, device))
    if not t.is_contiguous():
        raise GmeshError("blend_weights: %s must be contiguous" % name)


def blend_weights(policy, geom, binning, img, P, width, height, mask=None, sums=None, peak=None, stream=None, *, num_rendered):
    """gm_blend_weights on the buffers a completed forward returned (rasterize_forward / PendingForward.finish:
    (num_rendered, color, radii, geom, binning, img); num_rendered as rasterize_backward takes it - of a sync-free frame the capacity).
    mask: uint8 [H,W] on the frame's device, None = 255 everywhere.  sums int64 [P,2] and peak int32 [P] (float bits) are ADDED to;
    zeroed ones are allocated when not given.  stream: the raw stream the forward ran on (default: torch's current one).
    Returns (sums, peak)."""
    P, W, H = int(P), int(width), int(height)
    for name, t in (("geom", geom), ("binning", binning), ("img", img)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_contiguous():
            raise GmeshError("blend_weights: %s must be the contiguous uint8 buffer a forward returned" % name)
    device = geom.device
    need_cuda(device, "blend_weights", "buffers")
    for name, t in (("binning", binning), ("img", img)):
        if t.device != device:
            raise GmeshError("blend_weights: %s is on %s, geom on %s" % (name, t.device, device))
    lib = _lib.lib()
    cap = max(int(num_rendered), 0)
    for name, t, need in (("geom", geom, lib.gm_geom_bytes(P)), ("binning", binning, lib.gm_binning_bytes(cap)), ("img", img, lib.gm_image_bytes(W, H))):
        if P > 0 and t.numel() < need:
            raise GmeshError("blend_weights: %s holds %d bytes, the frame needs %d" % (name, t.numel(), need))
    if mask is not None:
        _check("mask", mask, torch.uint8, (H, W), device)
    if sums is None:
        sums = torch.zeros((P, 2), dtype=torch.int64, device=device)
    if peak is None:
        peak = torch.zeros((P,), dtype=torch.int32, device=device)
    _check("sums", sums, torch.int64, (P, 2), device)
    _check("peak", peak, torch.int32, (P,), device)
    some = lambda t: None if (t is None or t.numel() == 0) else t                  # (an empty tensor goes as NULL)
    enqueue(device, "gm_blend_weights", int(policy), some(geom), some(binning), some(img), P, cap, W, H, some(mask), some(sums), some(peak), 0,
            stream=stream)
    return sums, peak


class Contribution(NamedTuple):
    """total / inside: float64 [P], the summed weight (all pixels / weighted by mask / 255); peak: float32 [P], the largest single weight;
    views: frames accumulated; sums int64 [P,2] and peak_bits int32 [P]: the raw accumulators."""
    total: torch.Tensor
    inside: torch.Tensor
    peak: torch.Tensor
    views: int
    sums: torch.Tensor
    peak_bits: torch.Tensor


def contribution_from_raw(sums, peak_bits, views):
    return Contribution(sums[:, 0].double() * WEIGHT_UNIT, sums[:, 1].double() / 255.0 * WEIGHT_UNIT, peak_bits.view(torch.float32),
                        int(views), sums, peak_bits)


def _mask_of(m, H, W):
    """uint8 [H,W] of a masks entry: a tensor, a GroundTruth (its mask's first plane; none = all inside) or None."""
    if m is None:
        return None
    if hasattr(m, "rgb") and hasattr(m, "mask"):
        m = m.mask
        if m is None:
            return None
        m = m[0]
    if m.dim() == 3 and m.shape[0] in (1, 3):
        m = m[0]
    if tuple(m.shape) != (H, W):
        raise GmeshError("accumulate: a mask of %s for a %dx%d view" % (list(m.shape), H, W))
    return m.contiguous()


def accumulate(pc, cameras, masks=None, scaling_modifier=1.0, emission_policy=None):
    """One forward (no_grad, image only) and one blend_weights per camera, on torch's current stream; nothing waits on the host beyond
    the forward's own read of its instance count.  pc: a model with get_xyz / get_features / get_opacity / get_scaling / get_rotation /
    active_sh_degree (PlainGaussians, MeshBoundGaussians); cameras: renderer.Camera's; masks: per camera a uint8 [H,W] tensor, a
    dataset.GroundTruth or None - or None for no masks at all (inside == total)."""
    import math
    from . import rasterizer as R
    cameras = list(cameras)
    if masks is not None:
        masks = list(masks)
        if len(masks) != len(cameras):
            raise GmeshError("accumulate: %d masks for %d cameras" % (len(masks), len(cameras)))
    with torch.no_grad():
        means = pc.get_xyz.detach().contiguous()
        device = means.device
        P = means.shape[0]
        shs, opacity = pc.get_features.detach().contiguous(), pc.get_opacity.detach().contiguous()
        scales, rots = pc.get_scaling.detach().contiguous(), pc.get_rotation.detach().contiguous()
        sums = torch.zeros((P, 2), dtype=torch.int64, device=device)
        peak = torch.zeros((P,), dtype=torch.int32, device=device)
        bg = torch.zeros(3, device=device)
        for k, cam in enumerate(cameras if P > 0 else ()):
            H, W = int(cam.image_height), int(cam.image_width)
            h = R.rasterize_forward_begin(bg, means, None, opacity, scales, rots, float(scaling_modifier), None, cam.world_view_transform,
                                          cam.full_proj_transform, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), H, W, shs,
                                          int(pc.active_sh_degree), cam.camera_center, emission_policy=emission_policy)
            nr, _, _, geom, binning, img = h.finish(image_only=True)[:6]
            blend_weights(h.policy, geom, binning, img, P, W, H, None if masks is None else _mask_of(masks[k], H, W), sums, peak,
                          h.stream.cuda_stream, num_rendered=nr)
    return contribution_from_raw(sums, peak, len(cameras))


def select(contribution, threshold=0.5, min_total=0.0):
    """bool [P]: inside / total > threshold and total > min_total.  Rows no view ever blended (total == 0) are False."""
    total, inside = contribution.total, contribution.inside
    return (total > 0) & (total > min_total) & (inside > threshold * total)


def importance_rows(contribution, keep_fraction=None, min_peak=None):
    """bool [P] of the rows to keep.  keep_fraction: the round(keep_fraction * P) rows with the largest total (ties: the lower row id
    first).  min_peak: rows whose largest single weight reached it (1/255: exactly the rows some view accepted).  Both: the intersection."""
    P = contribution.total.shape[0]
    keep = torch.ones((P,), dtype=torch.bool, device=contribution.total.device)
    if keep_fraction is not None:
        if not 0.0 <= float(keep_fraction) <= 1.0:
            raise GmeshError("importance_rows: keep_fraction must lie in [0, 1]")
        n = min(P, max(0, int(round(float(keep_fraction) * P))))
        order = torch.sort(contribution.sums[:, 0], descending=True, stable=True).indices      # (the exact integer totals; stable: row id breaks ties)
        keep = torch.zeros_like(keep)
        keep[order[:n]] = True
    if min_peak is not None:
        keep = keep & (contribution.peak >= float(np.float32(min_peak)))          # (the threshold as the float32 the weights are)
    return keep


def split_plain(pc, rows):
    """(selected, rest): two bg_model.PlainGaussians holding the rows of pc's raw parameters (xyz, features, scaling, rotation, opacity)
    where rows is True / False, with pc's SH degrees; no optimizer state."""
    from .bg_model import PlainGaussians
    rows = torch.as_tensor(rows, dtype=torch.bool, device=pc._xyz.device)
    if rows.shape != (pc._xyz.shape[0],):
        raise GmeshError("split_plain: rows must be bool [%d]" % pc._xyz.shape[0])
    out = []
    for sel in (rows, ~rows):
        g = PlainGaussians(getattr(pc, "max_sh_degree", 3), device=pc._xyz.device)
        g._set_params(pc._xyz.detach()[sel], pc._features.detach()[sel], pc._scaling.detach()[sel], pc._rotation.detach()[sel],
                      pc._opacity.detach()[sel])
        g.active_sh_degree = pc.active_sh_degree
        out.append(g)
    return tuple(out)


def plain_columns(pc):
    """The dict io.save_plain_gaussians takes, of a PlainGaussians."""
    c = lambda t: t.detach().cpu().numpy()
    return dict(xyz=c(pc._xyz), features_dc=c(pc._features[:, :1]), features_rest=c(pc._features[:, 1:]), opacity=c(pc._opacity),
                scaling=c(pc._scaling), rotation=c(pc._rotation))


def load_plain(path, sh_degree=3, device="cuda"):
    """A PlainGaussians from a free-standing Gaussian PLY (io.load_plain_gaussians), all SH degrees active."""
    from . import io as gio
    from .bg_model import PlainGaussians
    d = gio.load_plain_gaussians(path, sh_degree)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32)
    g = PlainGaussians(sh_degree, device=device)
    g._set_params(t(d["xyz"]), torch.cat([t(d["features_dc"]), t(d["features_rest"])], dim=1), t(d["scaling"]), t(d["rotation"]), t(d["opacity"]))
    g.active_sh_degree = sh_degree
    return g


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m gaussianmesh_amd.contribution", description=__doc__.split("\n\n")[0])
    p.add_argument("--gaussian", required=True, help="the trained scene: a free-standing Gaussian PLY")
    p.add_argument("-s", "--source_path", required=True, help="the data set (COLMAP or Blender) whose views and masks are used")
    p.add_argument("--images", default=None)
    p.add_argument("-r", "--resolution", type=int, default=-1)
    p.add_argument("--sh_degree", type=int, default=3)
    p.add_argument("--out_object", default=None)
    p.add_argument("--out_background", default=None)
    p.add_argument("--threshold", type=float, default=0.5)
    p.add_argument("--out_pruned", default=None)
    g = p.add_mutually_exclusive_group()
    g.add_argument("--keep_fraction", type=float, default=None)
    g.add_argument("--min_peak", type=float, default=None)
    a = p.parse_args(argv)
    outs = [o for o in (a.out_object, a.out_background, a.out_pruned) if o]
    if not outs:
        p.error("nothing to write: give --out_object / --out_background and / or --out_pruned")
    if a.out_pruned and a.keep_fraction is None and a.min_peak is None:
        p.error("--out_pruned needs --keep_fraction or --min_peak")
    same = lambda x, y: os.path.abspath(x) == os.path.abspath(y) or (os.path.exists(x) and os.path.exists(y) and os.path.samefile(x, y))
    for o in outs:
        if same(o, a.gaussian):
            p.error("refusing to overwrite the input %s" % a.gaussian)
    if len({os.path.abspath(o) for o in outs}) != len(outs):
        p.error("two outputs name the same file")
    return a


def main(argv=None):
    from . import dataset, io as gio
    a = parse_args(argv)
    t0 = time.time()
    pc = load_plain(a.gaussian, a.sh_degree, "cuda")
    scene = dataset.load_scene(a.source_path, images=a.images)
    cams, gts = [], []
    for v in list(scene.train_cameras) + list(scene.test_cameras):
        cam, gt = dataset.load_view(v, a.resolution, device="cuda")
        cams.append(cam); gts.append(gt)
    con = accumulate(pc, cams, gts)
    out = {"rows": int(pc.get_number), "views": con.views, "rows_never_seen": int((con.sums[:, 0] == 0).sum())}
    if a.out_object or a.out_background:
        rows = select(con, a.threshold)
        obj, rest = split_plain(pc, rows)
        out["rows_selected"] = int(rows.sum())
        if a.out_object:
            gio.save_plain_gaussians(a.out_object, plain_columns(obj))
        if a.out_background:
            gio.save_plain_gaussians(a.out_background, plain_columns(rest))
    if a.out_pruned:
        keep = importance_rows(con, a.keep_fraction, a.min_peak)
        out["rows_kept"] = int(keep.sum())
        gio.save_plain_gaussians(a.out_pruned, plain_columns(split_plain(pc, keep)[0]))
    torch.cuda.synchronize()
    out["seconds"] = round(time.time() - t0, 3)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
