#!/usr/bin/env python
"""ms per forward + backward of the training loss for three ways of giving it the ground truth, at 3840x2160 and 1920x1080:
  (a) float image + float mask resident, composited with torch per iteration (gt * mask + bg * (1 - mask), bg on the device), then
      photometric_loss - what the training loop had to do before the 8-bit kernels;
  (b) photometric_loss on a precomposed float target: the float kernels alone;
  (c) photometric_loss_u8 on the resident 8-bit planes (gm_ssim_fwd_u8 / gm_ssim_bwd_u8).
Device events; the legs alternate inside one process; median and min..max of REPEATS repeats of ITERS iterations each."""
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianmesh_amd.dataset import GroundTruth
from gaussianmesh_amd.loss import photometric_loss, photometric_loss_u8

REPEATS, ITERS = int(os.environ.get("GT_REPEATS", 5)), int(os.environ.get("GT_ITERS", 300))
for (W, H) in ((3840, 2160), (1920, 1080)):
    g = torch.Generator("cuda").manual_seed(0)
    img = torch.rand((3, H, W), device="cuda", generator=g).requires_grad_(True)
    gt = GroundTruth(torch.randint(0, 256, (3, H, W), device="cuda", generator=g, dtype=torch.uint8),
                     torch.randint(0, 256, (1, H, W), device="cuda", generator=g, dtype=torch.uint8))
    bg = torch.rand(3, device="cuda", generator=g)
    f_img, f_mask = gt.float_target(None) if gt.mask is None else GroundTruth(gt.rgb).float_target(), GroundTruth(gt.mask.expand(3, H, W).contiguous()).float_target()[:1].contiguous()
    target = gt.float_target(bg)

    def leg_a():
        img.grad = None
        photometric_loss(img, f_img * f_mask + bg.reshape(3, 1, 1) * (1 - f_mask), 0.2).backward()

    def leg_b():
        img.grad = None
        photometric_loss(img, target, 0.2).backward()

    def leg_c():
        img.grad = None
        photometric_loss_u8(img, gt, bg, 0.2).backward()

    legs = (("a torch composite + float kernels", leg_a), ("b float kernels, precomposed target", leg_b), ("c 8-bit kernels", leg_c))
    for _, f in legs:
        for _ in range(5):
            f()
    times = {name: [] for name, _ in legs}
    for _ in range(REPEATS):
        for name, f in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(ITERS):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / ITERS)
    print("%dx%d (%d repeats x %d iterations): resident ground truth %.1f MB as 8-bit planes, %.1f MB as float image + float mask" % (
        W, H, REPEATS, ITERS, gt.nbytes / 1e6, 4 * 4 * H * W / 1e6))
    for name, _ in legs:
        t = np.array(times[name])
        print("  (%s)  median %.4f ms   min %.4f   max %.4f" % (name, np.median(t), t.min(), t.max()))
