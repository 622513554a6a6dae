"""CPU: tests/ssim_ref.py is the definition of the SSIM/L1 loss kernels (against oracle/loss_oracle.py in float64), its rounding bound
covers two float32 evaluations with different association, is small enough to mean something, and is exceeded by every planted fault.

Largest error/bound ratios of the two float32 restatements per class (printed by test_the_bound_covers_float32; S / dS/dmu1 / dS/dE11 /
dS/dE12 / gradient / tile sums, the larger of the separable and the direct form): see the "per-pixel loss tests" entry of NOTEBOOK.md."""
import numpy as np
import pytest
import torch

import ssim_ref as sr
from oracle import loss_oracle as lo

f32 = np.float32
KEYS = sr.OUTPUTS + ("grad", "partial")


# ---- the reference is the definition ----
def _autograd(c):
    gs, gl = sr.scales(c)
    ta = torch.tensor(c.a, dtype=torch.float64, requires_grad=True)
    tb = torch.tensor(c.b, dtype=torch.float64)
    per_plane = lo.ssim_torch(ta[:, None], tb[:, None], size_average=False) * (c.H * c.W)      # planes as a batch: one sum of S per plane
    L = float(gl) * (ta - tb).abs().sum() + (torch.tensor(gs, dtype=torch.float64) * per_plane).sum()
    g, = torch.autograd.grad(L, ta)
    return g.numpy(), float(lo.ssim_torch(ta.detach(), tb))


@pytest.mark.parametrize("cls", sr.CLASSES)
def test_the_reference_is_the_oracles_definition(cls):
    for c in (c for c in sr.CASES if c.cls == cls):
        r = sr.reference(c.name)
        g, mean = _autograd(c)
        assert abs(r.out["S"].mean() - mean) <= 1e-9 * abs(mean), c
        diff = float(np.abs(r.grad - g).max())
        if cls == "flat_equal":
            # the gradient is identically zero: three terms of ~ |g_ssim| / C2 each cancel; relative to those terms
            gs, _ = sr.scales(c)
            terms = np.abs(gs.astype(np.float64))[:, None, None] * (sr.conv(np.abs(r.out["dmu1"])) + 2 * np.abs(c.a) * sr.conv(np.abs(r.out["dE11"]))
                                                                     + np.abs(c.b) * sr.conv(np.abs(r.out["dE12"])))
            assert diff <= 1e-9 * terms.max() and float(np.abs(g).max()) <= 1e-9 * terms.max(), c
        else:
            assert diff <= 1e-9 * float(np.abs(g).max()), (c, diff)
        assert float((np.abs(r.grad - g) / r.grad_bd).max()) < 1e-6, c        # a millionth of what float32 rounding is allowed


def test_the_cases_cover_the_tile_edges():
    shapes = {(c.H, c.W) for c in sr.CASES}
    assert shapes == set(sr.SHAPES) and len(sr.SHAPES) == 18
    assert {c.planes for c in sr.CASES} == {1, 3}
    for cls in sr.CLASSES[1:]:
        assert {(c.H, c.W) for c in sr.CASES if c.cls == cls} == set(sr.CROSS), cls
    assert {H % 4 for H, _ in sr.SHAPES} == {0, 1, 2, 3}
    for c in sr.CASES:
        planted = (c.a == c.b)
        if c.cls == "planted":
            assert 2 <= int(planted[0].sum()) <= 8 and planted[:, 0, 0].all(), c
        if c.cls == "signed":
            assert c.a.min() < -2.5 and c.a.max() > 2.5
    assert len({c.name for c in sr.CASES}) == len(sr.CASES)


# ---- two float32 evaluations with different association ----
def _sep32(x, w):
    """separable: horizontal then vertical, taps added one after the other, every operation rounded to float32"""
    H, W = x.shape[-2:]
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(0, 0), (5, 5)])
    h = np.zeros_like(x)
    for k in range(11):
        h = h + w[k] * p[..., :, k:k + W]
    p = np.pad(h, [(0, 0)] * (x.ndim - 2) + [(5, 5), (0, 0)])
    v = np.zeros_like(x)
    for k in range(11):
        v = v + w[k] * p[..., k:k + H, :]
    assert v.dtype == f32
    return v


def _direct32(x, w2):
    """one 2-D sum of 121 taps in row-major order (120 additions in a row: its worst case is outside the count behind K, its
    typical error is not)"""
    H, W = x.shape[-2:]
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(5, 5), (5, 5)])
    out = np.zeros_like(x)
    for i in range(11):
        for j in range(11):
            out = out + w2[i, j] * p[..., i:i + H, j:j + W]
    assert out.dtype == f32
    return out


def _float32_evaluation(c, form):
    a, b = c.a, c.b
    gs, gl = sr.scales(c)
    gs = gs[:, None, None]
    if form == "separable":
        w = lo.window_1d()
        conv = lambda x: _sep32(x, w)
    else:
        w2 = lo.window_2d()
        conv = lambda x: _direct32(x, w2)
    two, c1, c2 = f32(2), f32(0.01) * f32(0.01), f32(0.03) * f32(0.03)
    with np.errstate(all="ignore"):
        mu1, mu2, e11, e22, e12 = conv(a), conv(b), conv(a * a), conv(b * b), conv(a * b)
        mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
        s1, s2, s12 = e11 - mu1_sq, e22 - mu2_sq, e12 - mu12
        A1, A2, B1, B2 = two * mu12 + c1, two * s12 + c2, mu1_sq + mu2_sq + c1, s1 + s2 + c2
        if form == "separable":                                              # reciprocals, as the kernel writes it
            ib1, ib2 = f32(1) / B1, f32(1) / B2
            S = (A1 * A2) * (ib1 * ib2)
            dE11 = -S * ib2
            dE12 = two * A1 * (ib1 * ib2)
            dmu1 = two * mu2 * A2 * (ib1 * ib2) - two * mu1 * S * ib1 - two * mu1 * dE11 - mu2 * dE12
        else:                                                                # quotients, terms added from the other end
            S = (A1 * A2) / (B1 * B2)
            dE11 = -(S / B2)
            dE12 = (two * A1) / (B1 * B2)
            dmu1 = (two * mu2 * A2) / (B1 * B2) + (-(two * mu1 * S) / B1 + (-(two * mu1) * dE11 + -(mu2 * dE12)))
        d = a - b
        sgn = np.sign(d).astype(f32)
        if form == "separable":
            g = gs * (conv(dmu1) + two * a * conv(dE11) + b * conv(dE12)) + gl * sgn
        else:
            g = gl * sgn + (gs * conv(dmu1) + (gs * (two * a)) * conv(dE11) + (gs * b) * conv(dE12))
        l1 = np.abs(d)
        P, H, W = a.shape
        gy, gx = (H + 31) // 32, (W + 31) // 32
        part = np.zeros((P, gy, gx, 2), f32)
        for y in range(gy):
            for x in range(gx):
                for k, q in enumerate((S, l1)):
                    t = q[:, y * 32:(y + 1) * 32, x * 32:(x + 1) * 32]
                    if form == "separable":
                        part[:, y, x, k] = t.reshape(P, -1).sum(axis=1, dtype=f32)
                    else:                                                    # rows first, then the row sums (pairwise: depth 7 + 7)
                        part[:, y, x, k] = np.ascontiguousarray(t).sum(axis=2, dtype=f32).sum(axis=1, dtype=f32)
    out = {"S": S, "dmu1": dmu1, "dE11": dE11, "dE12": dE12, "grad": g, "partial": part.reshape(-1, 2)}
    assert all(v.dtype == f32 for v in out.values())
    return out


def _ratios(got, r):
    """{output: largest |got - reference| / bound}; a difference where the bound is zero counts as infinite"""
    ref = dict(r.out, grad=r.grad, partial=r.partial)
    bd = dict(r.bd, grad=r.grad_bd, partial=r.partial_bd)
    res = {}
    for k in KEYS:
        err = np.abs(np.asarray(got[k], np.float64) - ref[k])
        with np.errstate(all="ignore"):
            q = np.where(err == 0, 0.0, err / bd[k])
        res[k] = float(np.max(q)) if q.size else 0.0
    return res


def test_the_bound_covers_float32():
    worst = {cls: {form: dict.fromkeys(KEYS, 0.0) for form in ("separable", "direct")} for cls in sr.CLASSES}
    for c in sr.CASES:
        r = sr.reference(c.name)
        for form in ("separable", "direct"):
            q = _ratios(_float32_evaluation(c, form), r)
            for k in KEYS:
                assert q[k] < 0.5, "%s, %s form: %s is %.3f of its bound" % (c, form, k, q[k])
                worst[c.cls][form][k] = max(worst[c.cls][form][k], q[k])
    print("\nlargest |float32 - float64| / bound per class (separable | direct)")
    print("%-14s" % "class" + "".join("%16s" % k for k in KEYS))
    for cls in sr.CLASSES:
        print("%-14s" % cls + "".join("   %.3f | %.3f" % (worst[cls]["separable"][k], worst[cls]["direct"][k]) for k in KEYS))


# ---- the bound is not vacuous ----
def test_the_bound_is_not_vacuous():
    for c in sr.CASES:
        r = sr.reference(c.name)
        top = float(r.bd["S"].max())
        if c.cls in ("noise", "planted", "black", "signed", "impulse", "flat_unequal", "ramps"):
            assert top < 1e-4, (c, top)
        else:
            assert c.cls in sr.NO_GRADIENT_RESOLUTION and top < 1e-2, (c, top)
        if c.cls not in sr.NO_GRADIENT_RESOLUTION:
            # at least as tight at every pixel as the max-norm bar of tests/test_gpu_loss.py
            assert float(r.grad_bd.max()) < 1e-3 * float(np.abs(r.grad).max()), (c, float(r.grad_bd.max()), float(np.abs(r.grad).max()))


# ---- the bound has teeth: faults planted into the float64 definition ----
def _with_moments(c, m=None, c2=sr.C2, **grad_kw):
    gs, gl = sr.scales(c)
    out, _ = sr.outputs(sr.moments(c.a, c.b) if m is None else m, c2=c2)
    l1 = np.abs(c.a.astype(np.float64) - c.b)
    return dict(out, grad=sr.grad(c.a, c.b, gs, gl, out, **grad_kw), partial=sr.tile_sums(out["S"], l1)[0])


def _shifted(c):
    w = np.zeros_like(sr.W2)
    w[:, 1:] = sr.W2[:, :-1]
    return _with_moments(c, sr.moments(c.a, c.b, w))


def _tap0_dropped(c):
    w = sr.W2.copy()
    w[0, :] = 0
    w[:, 0] = 0
    return _with_moments(c, sr.moments(c.a, c.b, w))


def _seam_halo_of_four(c):
    """tap 0 missing only for the output column x = 32 and the output row y = 32: a tile staged with a 4-pixel halo on its low side"""
    m = sr.moments(c.a, c.b)
    wc, wr = sr.W2.copy(), sr.W2.copy()
    wc[:, 0] = 0
    wr[0, :] = 0
    if c.W > 32:
        m[..., :, 32] = sr.moments(c.a, c.b, wc)[..., :, 32]
    if c.H > 32:
        m[..., 32, :] = sr.moments(c.a, c.b, wr)[..., 32, :]
    return _with_moments(c, m)


def _swapped_g(c):
    gs, gl = sr.scales(c)
    gs = gs.copy()
    gs[0] = gs[1]
    return dict(_with_moments(c), grad=sr.grad(c.a, c.b, gs, gl))


def _swapped_tiles(c):
    out = _with_moments(c)
    l1 = np.abs(c.a.astype(np.float64) - c.b)
    return dict(out, partial=sr.tile_sums(out["S"], l1, swap=True)[0])


# fault -> (how to evaluate it, the output that must leave its bound, the case on which it must)
FAULTS = {
    "window shifted by one tap": (_shifted, "S", "noise-3x37x65"),
    "tap 0 dropped everywhere": (_tap0_dropped, "dE12", "noise-3x37x65"),
    "tap 0 dropped at the tile seam x = 32, y = 32": (_seam_halo_of_four, "dmu1", "noise-3x37x65"),
    "clamp-to-edge padding": (lambda c: _with_moments(c, sr.moments(c.a, c.b, mode="edge")), "S", "noise-3x5x5"),
    "C2 off by 1%": (lambda c: _with_moments(c, c2=1.01 * sr.C2), "dE12", "noise-3x37x65"),
    "sign(0) = +1": (lambda c: _with_moments(c, sign0=1.0), "grad", "planted-3x37x65"),
    "2a dropped to a": (lambda c: _with_moments(c, e11_factor=1.0), "grad", "noise-3x37x65"),
    "tile sums with x and y swapped": (_swapped_tiles, "partial", "noise-3x37x65"),
    "plane 0 scaled by plane 1's g_ssim": (_swapped_g, "grad", "noise-3x37x65"),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_a_planted_fault_exceeds_the_bound(fault):
    make, key, name = FAULTS[fault]
    c = sr.BY_NAME[name]
    q = _ratios(make(c), sr.reference(name))
    print("\n%s on %s: error/bound " % (fault, name) + ", ".join("%s %.3g" % (k, q[k]) for k in KEYS))
    assert q[key] > 1.0, "%s stays within the bound of %s on %s (%.3g of it)" % (fault, key, name, q[key])
