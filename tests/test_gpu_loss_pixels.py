"""-m gpu: gm_ssim_fwd / gm_ssim_bwd / gm_loss_combine and the _u8 variants through the C ABI, per pixel and per tile, against the float64
definition of tests/ssim_ref.py within its derived float32 rounding bound (K = 32, Kc = 16: counted there, not measured here), on
every case of ssim_ref.CASES: shapes at each edge of the 32x32 tile / 5-pixel halo / 4-rows-per-thread layout, and the input classes
of the workload.  Every output buffer is pre-filled with a sentinel and sits between two sentinel guard regions.

The tests print the largest error/bound ratio the kernels reach per output and class; the figures of an MI355X are in NOTEBOOK.md
("per-pixel loss tests")."""
import math

import numpy as np
import pytest
import torch

import ssim_ref as sr

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = f32(-7777.25)
GUARD = 64                       # floats of guard in front of and behind every output buffer
MAPS = ("dmu1", "dE11", "dE12")


def _lib():
    from gaussianmesh_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(x, dtype=torch.float32):
    return torch.as_tensor(np.array(x), dtype=dtype, device="cuda")          # (a copy: the cases' arrays are read-only)


def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


class Guarded:
    """n floats on the device between two guard regions, everything pre-filled with the sentinel"""

    def __init__(self, n):
        self.n = int(n)
        self.t = torch.full((self.n + 2 * GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * GUARD

    def read(self, what):
        torch.cuda.synchronize()
        h = self.t.cpu().numpy()
        assert (_bits(h[:GUARD]) == _bits(SENTINEL)).all(), "%s: the guard in front of the buffer was written" % what
        assert (_bits(h[GUARD + self.n:]) == _bits(SENTINEL)).all(), "%s: the guard behind the buffer was written" % what
        return h[GUARD:GUARD + self.n].copy()


def _forward(a, b, planes, H, W, maps=True):
    """gm_ssim_fwd on device images: ({name: [planes,H,W]} or None, partial [n,2])"""
    L, lib = _lib()
    n = int(lib.gm_ssim_partials(planes, H, W))
    part = Guarded(2 * n)
    bufs = [Guarded(planes * H * W) for _ in MAPS] if maps else None
    ptrs = [g.ptr for g in bufs] if maps else [None, None, None]
    L.check(lib.gm_ssim_fwd(a.data_ptr(), b.data_ptr(), planes, H, W, ptrs[0], ptrs[1], ptrs[2], part.ptr, _stream()))
    out = {k: g.read(k).reshape(planes, H, W) for k, g in zip(MAPS, bufs)} if maps else None
    return out, part.read("partial").reshape(n, 2)


def _backward(a, b, maps, planes, H, W, g_ssim, g_l1):
    """gm_ssim_bwd on device images and host maps; g_l1 None: the NULL pointer"""
    L, lib = _lib()
    dm = [_dev(maps[k]) for k in MAPS]
    gs = _dev(g_ssim)
    gl = None if g_l1 is None else _dev(np.array([g_l1], f32))
    out = Guarded(planes * H * W)
    L.check(lib.gm_ssim_bwd(a.data_ptr(), b.data_ptr(), dm[0].data_ptr(), dm[1].data_ptr(), dm[2].data_ptr(), planes, H, W, gs.data_ptr(),
                            None if gl is None else gl.data_ptr(), out.ptr, _stream()))
    return out.read("dL_dimg1").reshape(planes, H, W)


def _ratio(got, ref, bd, what):
    """largest |got - ref| / bd over the entries where the reference is a number; the kernel's NaNs must be the reference's"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "%s: NaNs at %s, the reference has them at %s" % (
        what, np.argwhere(np.isnan(got))[:4].tolist(), np.argwhere(np.isnan(ref))[:4].tolist())
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
        q = np.where(np.isnan(ref) | (err == 0), 0.0, err / bd)
    if q.size == 0:
        return 0.0
    i = np.unravel_index(int(np.argmax(q)), q.shape)
    assert q[i] <= 1.0, "%s: entry %s is %.9g, the definition %.9g: off by %.3g, %.3g times the bound" % (
        what, tuple(int(v) for v in i), got[i], ref[i], err[i], q[i])
    return float(q[i])


def _report(title, worst):
    print("\n%s: largest error/bound" % title)
    for name, q in worst.items():
        print("  %-10s %.3f" % (name, q))


def _cases(cls):
    return [c for c in sr.CASES if c.cls == cls]


# ---- forward ----
@pytest.mark.parametrize("cls", sr.CLASSES)
def test_forward_maps_and_partials_per_pixel(cls):
    _, lib = _lib()
    worst = dict.fromkeys(MAPS + ("sum S", "sum |a-b|"), 0.0)
    for c in _cases(cls):
        r = sr.reference(c.name)
        a, b = _dev(c.a), _dev(c.b)
        gy, gx = (c.H + 31) // 32, (c.W + 31) // 32
        assert int(lib.gm_ssim_partials(c.planes, c.H, c.W)) == c.planes * gy * gx == len(r.partial), c
        maps, part = _forward(a, b, c.planes, c.H, c.W)
        for k in MAPS:
            assert not (_bits(maps[k]) == _bits(SENTINEL)).any(), "%s: %s has pixels that were not written" % (c, k)
            worst[k] = max(worst[k], _ratio(maps[k], r.out[k], r.bd[k], "%s %s" % (c, k)))
        assert not (_bits(part) == _bits(SENTINEL)).any(), "%s: partial sums that were not written" % c
        # layout ((z * gy + y) * gx + x), pairs (sum S, sum |a - b|)
        worst["sum S"] = max(worst["sum S"], _ratio(part[:, 0], r.partial[:, 0], r.partial_bd[:, 0], "%s sum S of tile" % c))
        worst["sum |a-b|"] = max(worst["sum |a-b|"], _ratio(part[:, 1], r.partial[:, 1], r.partial_bd[:, 1], "%s sum |a-b| of tile" % c))
        # without the maps: the same partial sums, bit for bit; and the same bits from a second call
        _, part_only = _forward(a, b, c.planes, c.H, c.W, maps=False)
        assert np.array_equal(_bits(part_only), _bits(part)), "%s: the partial sums differ when no maps are written" % c
        maps2, part2 = _forward(a, b, c.planes, c.H, c.W)
        assert np.array_equal(_bits(part2), _bits(part)) and all(np.array_equal(_bits(maps2[k]), _bits(maps[k])) for k in MAPS), \
            "%s: two calls give different bits" % c
    _report("forward, %s" % cls, worst)


# ---- backward ----
@pytest.mark.parametrize("cls", sr.CLASSES)
def test_backward_per_pixel(cls):
    worst = {"grad": 0.0}
    for c in _cases(cls):
        r = sr.reference(c.name)
        gs, gl = sr.scales(c)
        a, b = _dev(c.a), _dev(c.b)
        maps, _ = _forward(a, b, c.planes, c.H, c.W)                          # the kernel's own maps: their error is inside the bound
        g = _backward(a, b, maps, c.planes, c.H, c.W, gs, gl)
        worst["grad"] = max(worst["grad"], _ratio(g, r.grad, r.grad_bd, "%s dL/dimage" % c))
        g0 = _backward(a, b, maps, c.planes, c.H, c.W, gs, 0.0)
        gn = _backward(a, b, maps, c.planes, c.H, c.W, gs, None)
        assert np.array_equal(_bits(gn), _bits(g0)), "%s: g_l1 NULL differs from g_l1 = 0" % c
        same = c.a == c.b
        if same.any():                                                        # sign(0) = 0: no L1 gradient where the images agree
            assert np.array_equal(_bits(g[same]), _bits(g0[same])), "%s: an L1 gradient where image and target are equal" % c
        if cls in ("planted", "flat_equal"):
            assert same.any()
        assert not np.array_equal(_bits(g[~same]), _bits(g0[~same])) or not (~same).any()
    _report("backward, %s" % cls, worst)


# ---- the Python surface, with the gradient scales the module documents ----
def test_ssim_per_image_and_photometric_loss_per_pixel():
    from gaussianmesh_amd import loss
    rng = np.random.default_rng(11)
    a = rng.random((2, 3, 33, 37)).astype(f32)
    b = np.clip(a + 0.15 * rng.standard_normal(a.shape), 0, 1).astype(f32)
    ta = _dev(a).requires_grad_(True)
    s = loss.ssim(ta, _dev(b), size_average=False)
    w = np.array([1.0, -2.0], f32)
    (s * _dev(w)).sum().backward()
    count = 33 * 37
    gs = np.repeat(w / f32(3 * count), 3)                                    # loss._Ssim.backward: g / (planes per image * H * W), in float32
    r = sr.Reference(a.reshape(6, 33, 37), b.reshape(6, 33, 37), gs, 0.0)
    q_ssim = _ratio(ta.grad.cpu().numpy().reshape(6, 33, 37), r.grad, r.grad_bd, "loss.ssim gradient")
    mean = r.out["S"].reshape(2, -1).mean(axis=1)
    mean_bd = r.partial_bd[:, 0].reshape(2, -1).sum(axis=1) / (3 * count) + sr.U * np.abs(mean)          # tile sums in double, one cast
    q_mean = _ratio(s.detach().cpu().numpy(), mean, mean_bd, "loss.ssim per-image mean")

    H, W, lam = 37, 65, 0.2
    c = sr.BY_NAME["noise-3x37x65"]
    n = 3 * H * W
    tc = _dev(c.a).requires_grad_(True)
    L = loss.photometric_loss(tc, _dev(c.b), lam)
    L.backward()
    gs, gl = np.full(3, f32(-lam / n), f32), f32((1.0 - lam) / n)           # loss._coefs
    r = sr.Reference(c.a, c.b, gs, gl)
    q_photo = _ratio(tc.grad.cpu().numpy(), r.grad, r.grad_bd, "loss.photometric_loss gradient")
    value = lam - lam / n * r.partial[:, 0].sum() + (1.0 - lam) / n * r.partial[:, 1].sum()
    value_bd = lam / n * r.partial_bd[:, 0].sum() + (1.0 - lam) / n * r.partial_bd[:, 1].sum() + sr.U * abs(value)
    q_value = _ratio(np.array([float(L.detach())]), np.array([value]), np.array([value_bd]), "loss.photometric_loss value")
    _report("python surface", {"ssim grad": q_ssim, "ssim mean": q_mean, "photo grad": q_photo, "photo value": q_value})


# ---- a NaN stays in its neighbourhood ----
def test_a_nan_pixel_reaches_its_window_and_nothing_else():
    c = sr.BY_NAME["noise-3x64x69"]
    a = c.a.copy()
    a[0, 16, 16] = np.nan
    gs, gl = sr.scales(c)
    with np.errstate(all="ignore"):
        r = sr.Reference(a, c.b, gs, gl)
    hood = np.zeros(a.shape, bool)
    hood[0, 11:22, 11:22] = True
    assert all(np.array_equal(np.isnan(r.out[k]), hood) for k in MAPS)
    assert np.isnan(r.partial).sum() == 2 and np.isnan(r.partial[0]).all()       # tile (0, 0) of plane 0: both sums
    maps, part = _forward(_dev(a), _dev(c.b), 3, c.H, c.W)
    worst = {k: _ratio(maps[k], r.out[k], r.bd[k], "NaN case %s" % k) for k in MAPS}     # (also: the NaN sets are equal)
    worst["sum S"] = _ratio(part[:, 0], r.partial[:, 0], r.partial_bd[:, 0], "NaN case sum S")
    worst["sum |a-b|"] = _ratio(part[:, 1], r.partial[:, 1], r.partial_bd[:, 1], "NaN case sum |a-b|")
    _report("one NaN pixel", worst)


# ---- the 8-bit target at the new edges ----
@pytest.mark.parametrize("shape", [(1, 1), (5, 5), (32, 37), (33, 31), (37, 65)], ids=lambda s: "%dx%d" % s)
def test_u8_kernels_give_the_float_kernels_bits(shape):
    from gaussianmesh_amd import loss
    from gaussianmesh_amd.dataset import GroundTruth
    L, lib = _lib()
    H, W = shape
    rng = np.random.default_rng(100 * H + W)
    gt = GroundTruth(_dev(rng.integers(0, 256, (3, H, W), dtype=np.uint8), torch.uint8), _dev(rng.integers(0, 256, (3, H, W), dtype=np.uint8), torch.uint8))
    bg = _dev(np.array([0.1, 0.7283951, 1.0 / 3.0], f32))
    a = _dev(rng.random((3, H, W)).astype(f32))
    target = gt.float_target(bg).contiguous()
    maps_f, part_f = _forward(a, target, 3, H, W)
    rgb, mask, stride, bgp, keep = loss._u8_args(a, gt, bg)
    assert mask is not None and stride == H * W
    n = int(lib.gm_ssim_partials(3, H, W))
    part, bufs = Guarded(2 * n), [Guarded(3 * H * W) for _ in MAPS]
    L.check(lib.gm_ssim_fwd_u8(a.data_ptr(), rgb, mask, stride, bgp, 3, H, W, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, part.ptr, _stream()))
    assert np.array_equal(_bits(part.read("u8 partial").reshape(n, 2)), _bits(part_f)), "partial sums"
    for k, g in zip(MAPS, bufs):
        assert np.array_equal(_bits(g.read("u8 " + k).reshape(3, H, W)), _bits(maps_f[k])), k
    gs, gl = np.array([-0.3, 0.7, -1.1], f32) / f32(H * W), f32(0.37) / f32(3 * H * W)
    g_f = _backward(a, target, maps_f, 3, H, W, gs, gl)
    dm, dgs, dgl, out = [_dev(maps_f[k]) for k in MAPS], _dev(gs), _dev(np.array([gl], f32)), Guarded(3 * H * W)
    L.check(lib.gm_ssim_bwd_u8(a.data_ptr(), rgb, mask, stride, bgp, dm[0].data_ptr(), dm[1].data_ptr(), dm[2].data_ptr(), 3, H, W,
                               dgs.data_ptr(), dgl.data_ptr(), out.ptr, _stream()))
    assert np.array_equal(_bits(out.read("u8 dL_dimg1").reshape(3, H, W)), _bits(g_f)), "gradient"


# ---- gm_loss_combine ----
@pytest.mark.parametrize("n", [0, 1, 63, 1023, 1024, 1025, 6120])
def test_loss_combine_is_the_rounded_exact_sum(n):
    """offset + c_ssim * sum a + c_l1 * sum b accumulated in double, against math.fsum: one float32 ulp (double accumulation leaves at
    most a straddle of a rounding boundary)"""
    L, lib = _lib()
    rng = np.random.default_rng(n)
    p = (1000.0 * rng.standard_normal((n, 2))).astype(f32)
    c_ssim, c_l1, offset = -0.2 / 12345.0, 0.8 / 12345.0, 0.2
    expect = f32(offset + c_ssim * math.fsum(p[:, 0].astype(np.float64)) + c_l1 * math.fsum(p[:, 1].astype(np.float64)))
    out = Guarded(1)
    dp = _dev(p) if n else None
    L.check(lib.gm_loss_combine(None if dp is None else dp.data_ptr(), n, c_ssim, c_l1, offset, out.ptr, _stream()))
    got = out.read("combine")[0]
    if n == 0:
        assert got == f32(offset)
    assert abs(float(got) - float(expect)) <= float(np.spacing(np.abs(expect))), (n, got, expect)


def test_refusals_and_empty_sizes():
    L, lib = _lib()
    c = sr.BY_NAME["noise-1x5x5"]
    a, b = _dev(c.a), _dev(c.b)
    part, maps, out = Guarded(2), [Guarded(25) for _ in MAPS], Guarded(25)
    gs = _dev(np.array([1.0], f32))
    fwd = lambda planes, H, W, m: lib.gm_ssim_fwd(a.data_ptr(), b.data_ptr(), planes, H, W, m[0], m[1], m[2], part.ptr, _stream())
    bwd = lambda planes, H, W: lib.gm_ssim_bwd(a.data_ptr(), b.data_ptr(), maps[0].ptr, maps[1].ptr, maps[2].ptr, planes, H, W, gs.data_ptr(), None,
                                               out.ptr, _stream())
    full = [g.ptr for g in maps]
    for some in ([full[0], None, None], [None, full[1], None], [None, None, full[2]], [full[0], full[1], None], [None, full[1], full[2]],
                 [full[0], None, full[2]]):
        assert fwd(1, 5, 5, some) != 0, "one or two map pointers must be refused"
        with pytest.raises(L.GmeshError, match="three"):
            L.check(fwd(1, 5, 5, some))
    for size in ((-1, 5, 5), (1, -5, 5), (1, 5, -5)):
        assert fwd(*size, full) != 0 and bwd(*size) != 0, size
        assert int(lib.gm_ssim_partials(*size)) == 0
    for size in ((0, 5, 5), (1, 0, 5), (1, 5, 0)):
        assert fwd(*size, full) == 0 and bwd(*size) == 0, size
        assert int(lib.gm_ssim_partials(*size)) == 0
    one = Guarded(1)
    assert lib.gm_loss_combine(part.ptr, -1, 1.0, 1.0, 0.0, one.ptr, _stream()) != 0
    assert lib.gm_loss_combine(part.ptr, 1, 1.0, 1.0, 0.0, None, _stream()) != 0
    assert lib.gm_loss_combine(None, 1, 1.0, 1.0, 0.0, one.ptr, _stream()) != 0
    # nothing above wrote anything
    for g, what in [(part, "partial"), (out, "dL_dimg1"), (one, "combine")] + [(m, k) for m, k in zip(maps, MAPS)]:
        assert (_bits(g.read(what)) == _bits(SENTINEL)).all(), "%s was written by a refused or empty call" % what
