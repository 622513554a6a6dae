"""The definition of gm_ssim_fwd / gm_ssim_bwd (include/gmesh_hip.h, csrc/gm_loss.hip) in float64, per pixel and per tile, with a
per-pixel bound on what float32 rounding may do to each output.  Plain numpy, no GPU.  The window is oracle.loss_oracle.window_2d():
the float32 outer product of the float32 window_1d() that the kernel's make_window() restates; all arithmetic on it is float64.

The bound is derived by counting roundings, never from what a kernel produces.  u = 2^-24 (unit roundoff of float32).

  A window moment sum_ij w_i w_j q_ij of q in {a, b, aa, bb, ab}, as a separable float32 computation against this file's float64 sum
  with the float32-rounded products fl(w_i w_j), each rounding measured against M = the same moment of |a|, |b| (every partial sum of
  the moment is at most M in magnitude):
      1    the product aa, bb or ab (none for a, b)
      12   horizontal pass: 11 tap products, each rounded once (together at most u*M; none when the compiler fuses them into the add)
           plus 11 additions (the first, to zero, is exact) of partial sums of magnitude <= M
      12   vertical pass, the same
      1    this file's window holds fl(w_i w_j), the separable form multiplies by w_i and w_j exactly: one rounding of difference
      1    the rounding of mu^2 in E - mu^2 acts as a perturbation of E of at most u*mu^2 <= u*M, since (sum w x)^2 <= sum w x^2
           (for E[ab] the rounding of mu1*mu2 is charged to the closing arithmetic below, where |mu1 mu2| is one of the terms)
      --
      27   <= K = 32.
  The closing arithmetic (moments -> S and the three derivatives): every intermediate X carries T(X), the sum of the absolute values
  of the terms it was added up from, propagated through products and quotients as the relative condition T(X)/|X| >= 1 (running
  error analysis).  Roundings charged per unit of T: at most 2 for A1 (mu1 mu2; + C1), 3 for A2, 3 for B1, 4 for B2 (two squares, two
  differences in parallel, two additions), so at most 4 for any factor; the 5 reciprocals and products of S, spread over four
  conditions that are each >= 1, add at most 1.25; one more product for dS/dE11 and dS/dE12; at most 3 more products per term of
  dS/dmu1 and 3 additions of its four terms: 4 + 1.25 + 3 + 3 < 12 roundings in all, fewer than Kc = 16.
  Gradient: three more 11x11 separable sums over the maps (25 roundings as above, the mu^2 one does not occur) and 6 for
  gs * (A + 2 x B + y C) + gl * sign: 31 <= K, measured against the same sums of absolute values; the final addition of the L1 term
  and the product gl * sign round |g_l1| at most twice, bounded by 4u|g_l1|.
  Tile sums: 4 additions per thread, 6 shuffle levels, 3 additions across the waves, and |a - b| itself: 14 <= 16.
"""
import functools
import zlib

import numpy as np

from oracle import loss_oracle as lo

U = 2.0 ** -24
K = 32
KC = 16
C1, C2 = 0.01 ** 2, 0.03 ** 2
TILE = 32
W2 = lo.window_2d().astype(np.float64)
OUTPUTS = ("S", "dmu1", "dE11", "dE12")


def conv(x, w2=None, mode="constant"):
    """[..., H, W] float64 -> the 11x11 window correlation with 5 pixels of padding (zeros unless `mode` says otherwise)"""
    w2 = W2 if w2 is None else w2
    x = np.asarray(x, np.float64)
    H, W = x.shape[-2:]
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(5, 5), (5, 5)], mode=mode)
    return np.tensordot(np.lib.stride_tricks.sliding_window_view(p, (11, 11), axis=(-2, -1)), w2, axes=([-2, -1], [0, 1]))


def moments(a, b, w2=None, mode="constant"):
    """[5, planes, H, W]: mu1, mu2, E11, E22, E12"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.stack([conv(q, w2, mode) for q in (a, b, a * a, b * b, a * b)])


def outputs(m, c1=C1, c2=C2):
    """({name: value}, {name: sum of |terms|}) for S and dS/dmu1, dS/dE11, dS/dE12 as the kernel defines them: S a function of
    (mu1, E11, E12) with mu2, E22 fixed."""
    mu1, mu2, e11, e22, e12 = m
    with np.errstate(all="ignore"):
        mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
        s1, s2, s12 = e11 - mu1_sq, e22 - mu2_sq, e12 - mu12
        A1, A2, B1, B2 = 2 * mu12 + c1, 2 * s12 + c2, mu1_sq + mu2_sq + c1, s1 + s2 + c2
        S = A1 * A2 / (B1 * B2)
        dE11 = -S / B2
        dE12 = 2 * A1 / (B1 * B2)
        t = (2 * mu2 * A2 / (B1 * B2), -2 * mu1 * S / B1, -2 * mu1 * dE11, -mu2 * dE12)
        dmu1 = t[0] + t[1] + t[2] + t[3]
        # relative conditions T(X)/|X| of the four factors.  A difference E - mu^2 rounds relative to its RESULT (what its cancellation
        # does to the moments' own errors is the perturbation part of bound()); the rounding of mu1*mu2 enters A2 absolutely.
        cA1 = (2 * np.abs(mu12) + c1) / np.abs(A1)
        cA2 = (2 * (np.abs(s12) + np.abs(mu12)) + c2) / np.abs(A2)
        cB1 = np.ones_like(B1)                                               # a sum of non-negative terms
        cB2 = (np.abs(s1) + np.abs(s2) + c2) / np.abs(B2)
        cS = cA1 + cA2 + cB1 + cB2
        T = {"S": np.abs(S) * cS,
             "dE11": np.abs(dE11) * (cS + cB2),
             "dE12": np.abs(dE12) * (cA1 + cB1 + cB2),
             "dmu1": np.abs(t[0]) * (1 + cA2 + cB1 + cB2) + np.abs(t[1]) * (1 + cS + cB1) + np.abs(t[2]) * (1 + cS + cB2)
                     + np.abs(t[3]) * (1 + cA1 + cB1 + cB2)}
    return {"S": S, "dmu1": dmu1, "dE11": dE11, "dE12": dE12}, T


def bound(a, b):
    """{name: per-pixel bound on the float32 rounding error of that output} (see the module's docstring)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    m = moments(a, b)
    M = moments(np.abs(a), np.abs(b))
    base, T = outputs(m)
    bd = {k: KC * U * T[k] for k in OUTPUTS}
    with np.errstate(all="ignore"):
        for i in range(5):
            worst = {k: 0.0 for k in OUTPUTS}
            for sgn in (1.0, -1.0):
                mp = m.copy()
                mp[i] = m[i] + sgn * K * U * M[i]
                o, _ = outputs(mp)
                for k in OUTPUTS:
                    worst[k] = np.maximum(worst[k], np.abs(o[k] - base[k]))
            for k in OUTPUTS:
                bd[k] = bd[k] + worst[k]
    return bd


def _per_plane(g, planes):
    return np.asarray(g, np.float64).reshape(-1)[:, None, None] * np.ones((planes, 1, 1))


def grad(a, b, g_ssim, g_l1, out=None, sign0=0.0, e11_factor=2.0):
    """dL/da [planes,H,W] for L = sum_z g_ssim[z] * sum(S_z) + g_l1 * sum|a - b|; `out`: the maps to use (default: this definition's)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if out is None:
        out, _ = outputs(moments(a, b))
    gs = _per_plane(g_ssim, a.shape[0])
    d = a - b
    sgn = np.where(d > 0, 1.0, np.where(d < 0, -1.0, np.where(d == 0, sign0, np.nan)))
    return gs * (conv(out["dmu1"]) + e11_factor * a * conv(out["dE11"]) + b * conv(out["dE12"])) + float(g_l1) * sgn


def grad_bound(a, b, g_ssim, g_l1, out=None, bd=None):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if out is None:
        out, _ = outputs(moments(a, b))
    bd = bound(a, b) if bd is None else bd
    gs = np.abs(_per_plane(g_ssim, a.shape[0]))
    A, B = np.abs(a), np.abs(b)
    return gs * (conv(bd["dmu1"]) + 2 * A * conv(bd["dE11"]) + B * conv(bd["dE12"])
                 + K * U * (conv(np.abs(out["dmu1"])) + 2 * A * conv(np.abs(out["dE11"])) + B * conv(np.abs(out["dE12"])))) \
        + 4 * U * abs(float(g_l1))


def tiles(x, swap=False):
    """[planes,H,W] -> per-tile sums [planes * gy * gx] in the kernel's partial layout ((z * gy + y) * gx + x)"""
    P, H, W = x.shape
    gy, gx = (H + TILE - 1) // TILE, (W + TILE - 1) // TILE
    out = np.zeros((P, gy, gx))
    for y in range(gy):
        for xx in range(gx):
            out[:, y, xx] = x[:, y * TILE:(y + 1) * TILE, xx * TILE:(xx + 1) * TILE].sum(axis=(1, 2))
    return (out.transpose(0, 2, 1) if swap else out).reshape(-1)


def tile_sums(S, l1, bd_S=None, swap=False):
    """(partial [n,2] = (sum S, sum |a-b|) per tile, its bound [n,2]); `l1` = |a - b|"""
    val = np.stack([tiles(S, swap), tiles(l1, swap)], axis=1)
    bd_S = np.zeros_like(S) if bd_S is None else bd_S
    bd = np.stack([tiles(bd_S) + 16 * U * tiles(np.abs(S)), 16 * U * tiles(np.abs(l1))], axis=1)
    return val, bd


# ---- the inputs of tests/test_ssim_ref_host.py and tests/test_gpu_loss_pixels.py ----
# every shape is there for one edge of the 32x32 tile / 5-pixel halo / 4-rows-per-thread layout
SHAPES = [(1, 1), (1, 11), (11, 1),            # smaller than the halo, one row, one column
          (4, 6), (5, 5), (6, 5), (10, 12),    # up to / just past the halo width, H = 0, 1, 2 (mod 4)
          (27, 32), (31, 33), (32, 32),        # H = 3 (mod 4); a second tile of one column; the exact tile
          (32, 37), (33, 31), (34, 38),        # a second tile exactly as wide as the halo; a second tile of one row; H = 2 (mod 4), 6 columns
          (35, 64), (37, 65), (43, 42),        # H = 3 (mod 4) with two full tiles; a third tile of one column; the staged span
          (64, 69), (65, 63)]                  # a third tile as wide as the halo under two full rows; a third tile row of one row
CROSS = [(5, 5), (32, 37), (37, 65), (64, 69)]
CLASSES = ("noise", "planted", "black", "flat_equal", "flat_unequal", "lowcontrast", "signed", "impulse", "ramps", "flat_bright", "ramps_bright")
# Where an image is flat and bright, E[xx] - mu^2 cancels against C2 = 9e-4: a moment error of K u v^2 is K u v^2 / C2 of B2 (6e-4 at
# v = 0.5), the three terms of the gradient are each ~ 1/C2 and cancel to nothing, and no float32 evaluation resolves the gradient to
# 1e-3 of its largest entry.  flat_equal, lowcontrast, flat_bright and ramps_bright are in that regime (the maps carry them, and the
# gradient is still held to its bound); flat_unequal and ramps are the same pictures at v <= 0.05, where K u v^2 / C2 < 6e-6.
NO_GRADIENT_RESOLUTION = ("flat_equal", "lowcontrast", "flat_bright", "ramps_bright")
f32 = np.float32


def _make(cls, planes, H, W):
    rng = np.random.default_rng(zlib.crc32(("%s %d %d %d" % (cls, planes, H, W)).encode()))
    shape = (planes, H, W)
    noise = lambda: rng.random(shape).astype(f32)
    if cls in ("noise", "planted"):
        a = noise()
        b = np.clip(a + 0.15 * rng.standard_normal(shape), 0, 1).astype(f32)
        if cls == "planted":
            flat = rng.choice(H * W, size=min(6, H * W), replace=False)
            for z in range(planes):
                b[z].reshape(-1)[flat] = a[z].reshape(-1)[flat]
            b[:, 0, 0] = a[:, 0, 0]
            b[:, H - 1, W - 1] = a[:, H - 1, W - 1]
    elif cls == "black":
        a, b = np.zeros(shape, f32), noise()
    elif cls == "flat_equal":
        a = b = np.full(shape, 0.5, f32)
    elif cls == "flat_unequal":
        a, b = np.full(shape, 0.02, f32), np.full(shape, 0.05, f32)
    elif cls == "flat_bright":
        a, b = np.full(shape, 0.3, f32), np.full(shape, 0.7, f32)
    elif cls == "lowcontrast":
        a, b = (f32(0.9) + f32(1e-3) * noise()).astype(f32), (f32(0.9) + f32(1e-3) * noise()).astype(f32)
    elif cls == "signed":
        a = (f32(6) * noise() ** 3 - f32(3)).astype(f32)
        b = np.clip(a + 0.45 * rng.standard_normal(shape), -3, 3).astype(f32)
    elif cls == "impulse":
        a, b = np.zeros(shape, f32), np.zeros(shape, f32)
        a[:, H // 2, W // 2] = 1.0
        b[:, H // 2, min(W // 2 + 1, W - 1)] = 0.5
    elif cls in ("ramps", "ramps_bright"):                 # horizontal against vertical: a row/column swap changes every pixel
        a = np.broadcast_to((np.arange(W, dtype=f32) / f32(max(W - 1, 1)))[None, None, :], shape).astype(f32)
        b = np.broadcast_to((np.arange(H, dtype=f32) / f32(max(H - 1, 1)))[None, :, None], shape).astype(f32)
        a = a * np.linspace(1.0, 0.5, planes, dtype=f32)[:, None, None]
        if cls == "ramps":
            a, b = a * f32(0.05), b * f32(0.05)
    else:
        raise KeyError(cls)
    return np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)


class Case:
    def __init__(self, cls, planes, H, W):
        self.cls, self.planes, self.H, self.W = cls, planes, H, W
        self.name = "%s-%dx%dx%d" % (cls, planes, H, W)
        self.a, self.b = _make(cls, planes, H, W)
        for x in (self.a, self.b):
            x.setflags(write=False)

    def __repr__(self):
        return self.name


CASES = [Case("noise", p, H, W) for (H, W) in SHAPES for p in (1, 3)] + \
        [Case(cls, 3, H, W) for cls in CLASSES[1:] for (H, W) in CROSS]
BY_NAME = {c.name: c for c in CASES}
G_L1 = 0.37                                       # the tests' L1 gradient scale is G_L1 / (planes * H * W)


def scales(case):
    """(g_ssim float32 [planes], g_l1 float32): a distinct SSIM scale per plane, both of the size a mean over the image gives"""
    n = f32(case.H * case.W)
    return (np.array([-0.3, 0.7, -1.1][:case.planes], f32) / n).astype(f32), f32(f32(G_L1) / (f32(case.planes) * n))


class Reference:
    """Everything the tests compare against for one case, computed once and left unchanged."""

    def __init__(self, a, b, g_ssim, g_l1):
        self.out, _ = outputs(moments(a, b))
        self.bd = bound(a, b)
        self.grad = grad(a, b, g_ssim, g_l1, self.out)
        self.grad_bd = grad_bound(a, b, g_ssim, g_l1, self.out, self.bd)
        self.l1 = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
        self.partial, self.partial_bd = tile_sums(self.out["S"], self.l1, self.bd["S"])
        for x in list(self.out.values()) + list(self.bd.values()) + [self.grad, self.grad_bd, self.partial, self.partial_bd]:
            x.setflags(write=False)


@functools.lru_cache(maxsize=None)
def reference(name):
    c = BY_NAME[name]
    gs, gl = scales(c)
    return Reference(c.a, c.b, gs, gl)
