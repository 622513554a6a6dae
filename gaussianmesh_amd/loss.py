"""Photometric losses of the training loop, mirroring utils/loss_utils.py of the reference.

  l1_loss(network_output, gt)                       loss_utils.py:17-18
  mesh_restrict_loss(scale, v1, v2, v3, weight)     loss_utils.py:83-108 (torch elementwise; once per iteration on [N,3])
  l2_loss(network_output, gt)                       loss_utils.py:20-21
  ssim(img1, img2, window_size=11, size_average=True)   loss_utils.py:35-81
  photometric_loss(image, gt, lambda_dssim)         train_mesh_gaussian.py:92-94:
                                                    (1 - l) * l1_loss + l * (1 - ssim), one fused pass

  photometric_loss_u8(image, gt, background, lambda_dssim)   the same loss against a dataset.GroundTruth: the 8-bit planes of the
                                                    file, composited gt * mask + bg * (1 - mask) (train_mesh_gaussian.py:89-91) inside
                                                    the kernels' own load (gm_ssim_fwd_u8 / gm_ssim_bwd_u8)

ssim and photometric_loss run csrc/gm_loss.hip (gm_ssim_fwd / gm_ssim_bwd) and are differentiable with respect to
the first image (the rendered one); the ground truth gets no gradient, as in the training loop.  There is no CPU path.
"""
import torch

from . import _lib
from ._op import enqueue, f32, need_cuda


def l1_loss(network_output, gt):
    return (network_output - gt).abs().mean()


def l2_loss(network_output, gt):
    return ((network_output - gt) ** 2).mean()


def _planes(img):
    if img.dim() == 3:
        return img.shape[0], 1
    if img.dim() == 4:
        return img.shape[0] * img.shape[1], img.shape[0]
    raise ValueError("ssim expects [C,H,W] or [B,C,H,W] images")


def _fwd(img1, img2, want_grad):
    need_cuda(img1, "ssim", "tensors")
    if img1.shape != img2.shape:
        raise ValueError("ssim: image shapes differ: %s vs %s" % (tuple(img1.shape), tuple(img2.shape)))
    a, b = f32(img1), f32(img2)
    planes, _ = _planes(a)
    H, W = a.shape[-2], a.shape[-1]
    dev = a.device
    n = int(_lib.lib().gm_ssim_partials(planes, H, W))
    partial = torch.empty((n, 2), dtype=torch.float32, device=dev)
    maps = torch.empty((3,) + tuple(a.shape), dtype=torch.float32, device=dev) if want_grad else None
    mp = maps if want_grad else [None, None, None]
    enqueue(dev, "gm_ssim_fwd", a, b, planes, H, W, mp[0], mp[1], mp[2], partial)
    return a, b, maps, partial.view(planes, -1, 2)


def _bwd(a, b, maps, g_ssim_planes, g_l1):
    planes, _ = _planes(a)
    H, W = a.shape[-2], a.shape[-1]
    grad = torch.empty_like(a)
    g_ssim_planes = g_ssim_planes.contiguous().float()          # views of one small tensor are contiguous already
    g_l1 = None if g_l1 is None else g_l1.reshape(1).contiguous().float()
    enqueue(a.device, "gm_ssim_bwd", a, b, maps[0], maps[1], maps[2], planes, H, W, g_ssim_planes, g_l1, grad)
    return grad


class _Ssim(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2, size_average):
        a, b, maps, partial = _fwd(img1, img2, ctx.needs_input_grad[0])
        planes, batch = _planes(a)
        per_plane = partial[:, :, 0].double().sum(dim=1)                     # [planes]
        count = a.shape[-2] * a.shape[-1]
        ctx.size_average, ctx.shape, ctx.batch = size_average, img1.shape, batch
        if maps is not None:
            ctx.save_for_backward(a, b, maps)
        if size_average or a.dim() == 3:
            out = (per_plane.sum() / (planes * count)).float()
            return out if size_average else out.reshape(1)
        return (per_plane.view(batch, -1).sum(dim=1) / (planes // batch * count)).float()

    @staticmethod
    def backward(ctx, g):
        a, b, maps = ctx.saved_tensors
        planes, batch = _planes(a)
        count = a.shape[-2] * a.shape[-1]
        if ctx.size_average or a.dim() == 3:
            gp = (g.reshape(1) / (planes * count)).expand(planes)
        else:
            gp = (g.reshape(batch, 1) / (planes // batch * count)).expand(batch, planes // batch).reshape(planes)
        return _bwd(a, b, maps, gp, None).view(ctx.shape), None, None


def ssim(img1, img2, window_size=11, size_average=True):
    """Mean structural similarity; size_average=False returns one mean per image of a [B,C,H,W] batch
    (loss_utils.py:78-81).  Only the reference's window (11, sigma 1.5) is built."""
    if window_size != 11:
        raise NotImplementedError("ssim: only window_size=11 (the reference's only use) is implemented")
    return _Ssim.apply(img1, img2, bool(size_average))


_COEF_CACHE = {}


def _coefs(lam, n, planes, device):
    """device constants of the fused loss: value = lam + <coef, (sum ssim, sum |a-b|)>; per-plane / L1 gradient scales"""
    key = (float(lam), int(n), int(planes), device)
    c = _COEF_CACHE.get(key)
    if c is None:
        val = torch.tensor([-lam / n, (1.0 - lam) / n], dtype=torch.float64, device=device)
        grad = torch.tensor([-lam / n] * planes + [(1.0 - lam) / n], dtype=torch.float32, device=device)
        c = _COEF_CACHE[key] = (val, grad)
    return c


class _Photometric(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt, lambda_dssim):
        a, b, maps, partial = _fwd(image, gt, ctx.needs_input_grad[0])
        lam, n = float(lambda_dssim), a.numel()
        planes, _ = _planes(a)
        _, grad = _coefs(lam, n, planes, a.device)
        ctx.shape, ctx.planes = image.shape, planes
        if maps is not None:
            ctx.save_for_backward(a, b, maps, grad)
        out = torch.empty((), dtype=torch.float32, device=a.device)
        flat = partial.reshape(-1, 2)
        # lam + <(-lam/n, (1-lam)/n), (sum ssim, sum |a-b|)>, one launch
        enqueue(a.device, "gm_loss_combine", flat, flat.shape[0], -lam / n, (1.0 - lam) / n, lam, out)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b, maps, grad = ctx.saved_tensors
        gv = grad * g.reshape(1)                                               # [planes] ssim scales | [1] L1 scale
        return _bwd(a, b, maps, gv[:ctx.planes], gv[ctx.planes:]).view(ctx.shape), None, None


def photometric_loss(image, gt, lambda_dssim=0.2):
    """(1 - lambda) * l1_loss(image, gt) + lambda * (1 - ssim(image, gt)) in one forward and one backward kernel."""
    return _Photometric.apply(image, gt, float(lambda_dssim))


def _u8_args(a, gt, background):
    """pointers of a dataset.GroundTruth for gm_ssim_*_u8: (rgb, mask or None, mask plane stride, background or None, keep-alive list)"""
    rgb, mask = gt.rgb, gt.mask
    if rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[0] != 3 or not rgb.is_contiguous():
        raise ValueError("photometric_loss_u8: gt.rgb must be a contiguous uint8 [3,H,W] tensor")
    if a.dim() != 3 or tuple(a.shape) != tuple(rgb.shape):
        raise ValueError("photometric_loss_u8: image %s and ground truth %s differ in shape" % (tuple(a.shape), tuple(rgb.shape)))
    if rgb.device != a.device:
        raise ValueError("photometric_loss_u8: the ground truth is on %s, the image on %s" % (rgb.device, a.device))
    if mask is None:
        return rgb.data_ptr(), None, 0, None, [rgb]
    if mask.dtype != torch.uint8 or mask.dim() != 3 or mask.shape[0] not in (1, 3) or tuple(mask.shape[1:]) != tuple(rgb.shape[1:]) or \
            not mask.is_contiguous() or mask.device != a.device:
        raise ValueError("photometric_loss_u8: gt.mask must be a contiguous uint8 [1,H,W] or [3,H,W] tensor on the image's device")
    if background is None:
        raise ValueError("photometric_loss_u8: a masked ground truth needs the background colour")
    bg = background.detach().to(device=a.device, dtype=torch.float32).reshape(3).contiguous()      # (no copy for a device float32 [3])
    stride = 0 if mask.shape[0] == 1 else mask.shape[1] * mask.shape[2]
    return rgb.data_ptr(), mask.data_ptr(), stride, bg.data_ptr(), [rgb, mask, bg]


class _PhotometricU8(torch.autograd.Function):
    """_Photometric with the target read through gm_ssim_fwd_u8 / gm_ssim_bwd_u8: same partial sums, same derivative maps, same
    combine - bit for bit _Photometric on gt.float_target(background)."""

    @staticmethod
    def forward(ctx, image, gt, background, lambda_dssim):
        need_cuda(image, "photometric_loss_u8", "tensors")
        a = f32(image)
        rgb, mask, stride, bg, keep = _u8_args(a, gt, background)
        H, W = a.shape[-2], a.shape[-1]
        dev = a.device
        want_grad = ctx.needs_input_grad[0]
        n_part = int(_lib.lib().gm_ssim_partials(3, H, W))
        partial = torch.empty((n_part, 2), dtype=torch.float32, device=dev)
        maps = torch.empty((3,) + tuple(a.shape), dtype=torch.float32, device=dev) if want_grad else None
        mp = maps if want_grad else [None, None, None]
        lam, n = float(lambda_dssim), a.numel()
        _, grad = _coefs(lam, n, 3, dev)
        out = torch.empty((), dtype=torch.float32, device=dev)
        enqueue(dev, "gm_ssim_fwd_u8", a, rgb, mask, stride, bg, 3, H, W, mp[0], mp[1], mp[2], partial)
        enqueue(dev, "gm_loss_combine", partial, n_part, -lam / n, (1.0 - lam) / n, lam, out)
        ctx.shape, ctx.u8 = image.shape, (rgb, mask, stride, bg, keep)
        ctx.partial = partial                    # (tests read the partial sums; a small tensor)
        if maps is not None:
            ctx.save_for_backward(a, maps, grad)
        return out

    @staticmethod
    def backward(ctx, g):
        a, maps, grad = ctx.saved_tensors
        rgb, mask, stride, bg, _keep = ctx.u8
        gv = grad * g.reshape(1)
        g_ssim, g_l1 = gv[:3].contiguous(), gv[3:].contiguous()
        out = torch.empty_like(a)
        H, W = a.shape[-2], a.shape[-1]
        enqueue(a.device, "gm_ssim_bwd_u8", a, rgb, mask, stride, bg, maps[0], maps[1], maps[2], 3, H, W, g_ssim, g_l1, out)
        return out.view(ctx.shape), None, None, None


def photometric_loss_u8(image, gt, background=None, lambda_dssim=0.2):
    """photometric_loss(image, gt.float_target(background), lambda_dssim), bit for bit, without the float target: `gt` is a
    dataset.GroundTruth (uint8 rgb [3,H,W] and an optional uint8 mask [1 or 3,H,W] on the device), `background` a float [3] tensor
    (on the device it stays there: a colour drawn per iteration costs no synchronisation).  Gradient to `image` only."""
    return _PhotometricU8.apply(image, gt, background, float(lambda_dssim))


def distance(point1, point2):
    """loss_utils.py:83-84"""
    return torch.linalg.vector_norm(point1 - point2, dim=1)


def circumradius(point1, point2, point3):
    """loss_utils.py:86-101: despite the name, sqrt(|AB x AC|) (the square root of twice the triangle's area) - kept as
    the reference computes it."""
    areas = torch.linalg.vector_norm(torch.cross(point2 - point1, point3 - point1, dim=1), dim=1)
    return torch.sqrt(areas)


def mesh_restrict_loss(scale, point1, point2, point3, weight=10):
    """loss_utils.py:103-108: sum over Gaussians of max(0, max_axis(scale) - weight * circumradius(face)); keeps a bound
    Gaussian from growing past its triangle (train_mesh_gaussian.py:93)."""
    max_s = scale.max(dim=1).values
    return torch.clamp(max_s - weight * circumradius(point1, point2, point3), min=0).sum()
