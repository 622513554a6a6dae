"""-m gpu: every storage layout of the SH operand against the CPU oracle, forward and backward.

The layout of `shs` ([P,M,3], and whether its base is 16-byte aligned) picks the kernel (gm_preprocess.hip launch_preprocess /
launch_preprocess_bwd, gm_deform.hip launch_deform_shade):
  forward   M == 16 aligned -> rows staged through LDS by DMA; M in {1, 4, 12} aligned -> dense rows, 16-byte loads (load_sh);
            anything else (M = 9, M = 20, any unaligned operand) -> the generic 256-thread kernel (load_sh)
  backward  M == 16 with shs and dL_dsh aligned -> staged rows; otherwise the generic kernel, which stores dL/dSH 16 bytes at a time
            when 3M % 4 == 0, M <= 16 and dL_dsh is aligned, and one float at a time else (zeroing coefficients 16..M-1)
  colour    deform_shade: M == 16 and aligned -> the fused kernel; otherwise deform + sh_colors
An unaligned operand here is a contiguous view at a 4-byte offset into a NaN-filled buffer: its pointer reaches the library unchanged,
and a read past a row picks up NaN.  The oracle indexes rows with stride M (oracle/gm_oracle.c), so each case is checked against it.

Bars (BASELINE.json north_star, as test_gpu_parity.py): radii, tiles, instance lists, ranges and the per-Gaussian geometry (rgb, clamp
bits included) bit-exact; the image within 1e-4 (assert_forward_gate); every gradient within 1e-3 relative (and element-wise).
"""
import numpy as np
import pytest
import torch

from helpers import _check_geometry, assert_forward_gate, small_scene
from test_gpu_parity import _grad_gate

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-4
ATOMIC_RTOL = 2e-5           # two backward passes differ by float-atomic summation order (test_gpu_train.py, dense leaf vs rows)
W, H = 70, 50
# every (M, D) with (D+1)^2 <= M
CASES = [(M, D) for M in (1, 4, 9, 12, 16, 20) for D in range(4) if (D + 1) ** 2 <= M]
# ragged last workgroup for both block widths: 293 = 4 * 64 + 37 = 256 + 37, 513 = 8 * 64 + 1 = 2 * 256 + 1
SIZES = (293, 513)


@pytest.fixture(autouse=True)
def _default_emission_policy():
    from gaussianmesh_amd import rasterizer
    rasterizer.set_default_emission_policy(2)
    yield
    rasterizer.set_default_emission_policy(2)


def _scene(P, seed=0):
    """make_cloud(D=3) with some Gaussians behind the camera (culled: their dL/dSH rows must be written too)."""
    sc, cam = small_scene(P=P, W=W, H=H, seed=seed, D=3)
    bg = np.array([0.2, 0.5, 0.7], np.float32)
    return sc, cam, bg


def _rows(shs16, M, seed=0):
    """[P,16,3] -> [P,M,3]: the leading M coefficients, or for M > 16 the 16 followed by random coefficients that no degree reads."""
    if M <= 16:
        return np.ascontiguousarray(shs16[:, :M])
    junk = np.random.default_rng(seed + 1000).normal(size=(shs16.shape[0], M - 16, 3)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([shs16, junk], 1))


def _operand(rows, aligned):
    """rows as a contiguous float32 device tensor whose base is 16-byte aligned, or 4 bytes past a 16-byte boundary inside a
    NaN-filled buffer"""
    P, M, _ = rows.shape
    n = P * M * 3
    buf = torch.full((n + 8,), float("nan"), dtype=torch.float32, device="cuda")
    t = buf[0:n] if aligned else buf[1:1 + n]
    t = t.view(P, M, 3)
    t.copy_(torch.from_numpy(rows))
    assert t.is_contiguous() and t.data_ptr() % 16 == (0 if aligned else 4)
    return t


def _grads(sc, cam, bg, dpix, D, shs):
    """autograd through GaussianRasterizer with `shs` (a device tensor of any layout) as the SH leaf"""
    from gpu_utils import T, settings
    from gaussianmesh_amd import GaussianRasterizer
    shs = shs.detach().requires_grad_(True)
    means = T(sc["means"], True); opac = T(sc["opac"], True); scales = T(sc["scales"], True); rots = T(sc["rots"], True)
    m2d = torch.zeros_like(means, requires_grad=True)
    color, radii = GaussianRasterizer(settings(cam, bg, D))(means, m2d, opac, shs=shs, scales=scales, rotations=rots)
    (color * T(dpix)).sum().backward()
    torch.cuda.synchronize()
    g = dict(means=means.grad, m2d=m2d.grad, opac=opac.grad, scales=scales.grad, rots=rots.grad, shs=shs.grad)
    return color.detach().cpu().numpy(), radii.cpu().numpy(), {k: v.cpu().numpy() for k, v in g.items()}


@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset4"])
@pytest.mark.parametrize("M,D", CASES)
def test_forward_every_layout_matches_the_oracle(oracle, M, D, aligned, P):
    from gpu_utils import forward_state
    sc, cam, bg = _scene(P, seed=M + 7 * D)
    sc["shs"] = _rows(sc["shs"], M)
    fw = oracle.forward_full(sc, cam, bg, D=D)
    st = forward_state(sc, cam, bg, D=D, shs=_operand(sc["shs"], aligned))
    _check_geometry(oracle, st, fw, sc, False)
    assert_forward_gate(fw, st["color"], W, H, FWD_TOL, "M=%d D=%d aligned=%s" % (M, D, aligned))


@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset4"])
@pytest.mark.parametrize("M,D", CASES)
def test_backward_every_layout_matches_the_oracle(oracle, M, D, aligned, P):
    sc, cam, bg = _scene(P, seed=M + 7 * D + 1)
    sc["shs"] = _rows(sc["shs"], M)
    dpix = np.random.default_rng(M + D).normal(size=(3, H, W)).astype(np.float32)
    fw = oracle.forward_full(sc, cam, bg, D=D)
    bw = oracle.backward_full(sc, cam, bg, fw, dpix, D=D)
    color, radii, g = _grads(sc, cam, bg, dpix, D, _operand(sc["shs"], aligned))
    what = "M=%d D=%d aligned=%s" % (M, D, aligned)
    assert np.array_equal(radii, fw["geo"]["radii"]), what
    assert_forward_gate(fw, color, W, H, FWD_TOL, what)
    nc = (D + 1) ** 2
    assert g["shs"].shape == (P, M, 3), what
    for k, v in g.items():                          # the gradient outputs come from torch.empty: every row must be written
        assert np.isfinite(v).all(), (what, k)
    assert (g["shs"][:, nc:] == 0).all(), what      # including 16..M-1 for M = 20
    assert np.abs(g["shs"][:, :nc]).max() > 0, what
    culled = fw["geo"]["radii"] == 0
    assert culled.any() and (g["shs"][culled] == 0).all(), what
    _grad_gate(g["shs"][:, :nc], bw["dsh"].reshape(P, M, 3)[:, :nc], what + " d/dshs")
    for name, ref in (("means", bw["dmean3D"]), ("opac", bw["dopacity"]), ("scales", bw["dscale"]), ("rots", bw["drot"])):
        _grad_gate(g[name].reshape(ref.shape), ref, "%s d/d%s" % (what, name))


def _abi_backward(sc, cam, bg, st, shs, D, dpix, dsh_offset, keep=None):
    """gm_backward_p through the C ABI on the forward state `st` (policy 0), every output pre-filled with NaN; dL_dsh is a view at
    `dsh_offset` floats into a NaN buffer with slack on both sides.  Returns (outputs as numpy, the whole dL_dsh buffer); `keep` (a list)
    receives the device outputs before the call."""
    from gpu_utils import T
    from gaussianmesh_amd import _lib
    lib = _lib.lib()
    P, M = shs.shape[0], shs.shape[1]
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")
    o = dict(dmean2D=nan(P, 3), dconic=nan(P, 4), dopac=nan(P), dcolor=nan(P, 3), dmean3D=nan(P, 3), dcov3D=nan(P, 6),
             dscale=nan(P, 3), drot=nan(P, 4))
    dbuf = nan(P * M * 3 + 8)
    dsh = dbuf[dsh_offset:dsh_offset + P * M * 3]
    ins = [T(x) for x in (bg, sc["means"], sc["scales"], sc["rots"], cam["view"], cam["proj"], cam["campos"], dpix)]
    bg_t, means, scales, rots, view, proj, campos, dpix_t = ins
    p = lambda t: t.data_ptr()
    if keep is not None:
        keep.extend(list(o.values()) + [dbuf])
    _lib.check(lib.gm_backward_p(0, P, D, M, int(st["R"]), p(bg_t), W, H, p(means), p(shs), None, p(scales), 1.0, p(rots), None,
                                 p(view), p(proj), p(campos), float(cam["tanx"]), float(cam["tany"]), p(st["radii_t"]), p(st["geom"]),
                                 p(st["binning"]), p(st["img"]), p(dpix_t), p(o["dmean2D"]), p(o["dconic"]), p(o["dopac"]),
                                 p(o["dcolor"]), p(o["dmean3D"]), p(o["dcov3D"]), p(dsh), p(o["dscale"]), p(o["drot"]), 0,
                                 torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out["dsh"] = dsh.reshape(P, M, 3).cpu().numpy()
    return out, dbuf.cpu().numpy()


def _two_pixel_gradient(seed, W=W, H=H):
    """dL/dpix non-zero on two pixels only: every accumulator then sums at most two non-zero terms (and exact zeros), so its value is the
    same in every summation order and two backward passes give the same bits"""
    dpix = np.zeros((3, H, W), np.float32)
    rng = np.random.default_rng(seed)
    dpix[:, H // 2, W // 2] = rng.normal(size=3)
    dpix[:, H // 3, W // 4] = rng.normal(size=3)
    return dpix


@pytest.mark.parametrize("M,D", [(4, 1), (12, 2), (12, 0), (16, 3), (16, 1)])
def test_backward_store_routes_agree_bit_for_bit(oracle, M, D):
    """The generic backward's two dL/dSH store routes on the same forward: an aligned dL_dsh (16-byte stores) and one at a 4-byte offset
    (scalar stores) give the same bits in every output; every output row is written (NaN pre-fill), nothing outside the dL_dsh view is;
    dL/dSH agrees with the oracle.  M = 16 takes the generic kernel through an unaligned shs operand."""
    from gpu_utils import forward_state
    P = 513
    sc, cam, bg = _scene(P, seed=40 + M + D)
    sc["shs"] = _rows(sc["shs"], M)
    shs = _operand(sc["shs"], aligned=M != 16)
    st = forward_state(sc, cam, bg, D=D, shs=shs)
    dpix = _two_pixel_gradient(M + D)
    n = P * M * 3
    a, abuf = _abi_backward(sc, cam, bg, st, shs, D, dpix, 0)           # 16-byte stores
    u, ubuf = _abi_backward(sc, cam, bg, st, shs, D, dpix, 1)           # scalar stores
    assert np.isnan(abuf[n:]).all() and np.isnan(ubuf[:1]).all() and np.isnan(ubuf[1 + n:]).all()
    for k in a:
        assert np.isfinite(a[k]).all() and np.isfinite(u[k]).all(), k
        assert np.array_equal(a[k].view(np.uint32), u[k].view(np.uint32)), k
    nc = (D + 1) ** 2
    assert (a["dsh"][:, nc:] == 0).all() and np.abs(a["dsh"]).max() > 0
    fw = oracle.forward_full(sc, cam, bg, D=D)
    bw = oracle.backward_full(sc, cam, bg, fw, dpix, D=D)
    _grad_gate(a["dsh"][:, :nc], bw["dsh"].reshape(P, M, 3)[:, :nc], "M=%d D=%d d/dshs" % (M, D))


@pytest.mark.parametrize("D", [0, 1, 2, 3])
def test_routes_agree_with_each_other(D):
    """Staged M = 16, generic M = 16 (unaligned), M = (D+1)^2 (dense at D = 0, 1; generic M = 9 at D = 2) and dense M = 12 (D <= 2) on one
    scene: image, radii, per-Gaussian rgb and clamp bits identical; gradients (on the coefficients they share) to float-atomic order."""
    from gpu_utils import forward_state
    P = 1061                                        # 16 * 64 + 37
    sc, cam, bg = _scene(P, seed=60 + D)
    shs16 = sc["shs"]
    dpix = np.random.default_rng(D).normal(size=(3, H, W)).astype(np.float32)
    nc = (D + 1) ** 2
    layouts = [(16, True), (16, False), (nc, True)] + ([(12, True)] if D <= 2 else [])
    ref = None
    for M, aligned in layouts:
        rows = _rows(shs16, M)
        st = forward_state(sc, cam, bg, D=D, shs=_operand(rows, aligned))
        color, radii, g = _grads(sc, cam, bg, dpix, D, _operand(rows, aligned))
        g["shs"] = g["shs"][:, :nc]
        cur = dict(st=st, color=color, radii=radii, g=g)
        if ref is None:
            ref = cur
            continue
        what = "D=%d M=%d aligned=%s" % (D, M, aligned)
        vis = st["radii"] > 0                       # (the preprocess writes no splat record / clamp bits for a culled Gaussian)
        assert np.array_equal(st["radii"], ref["st"]["radii"]), what
        for k in ("color", "point_list", "ranges"):
            assert np.array_equal(st[k].view(np.uint8), ref["st"][k].view(np.uint8)), (what, k)
        for k in ("splat", "clamped"):
            assert np.array_equal(st[k][vis].view(np.uint8), ref["st"][k][vis].view(np.uint8)), (what, k)
        assert np.array_equal(radii, ref["radii"]) and np.array_equal(color.view(np.uint32), ref["color"].view(np.uint32)), what
        for k, v in g.items():
            r = ref["g"][k]
            assert np.abs(v - r).max() <= ATOMIC_RTOL * np.abs(r).max(), (what, k)


def _rot_frames(N, seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(N, 3, 3)))
    return q.astype(np.float32)


@pytest.mark.parametrize("with_rot", [False, True], ids=["dir", "rot"])
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_sh_colors_every_layout(oracle, deg, with_rot):
    """deform.sh_colors (the deform fallback's colour kernel) over the M grid and both alignments against oracle.sh_colors_rotated (no
    rotation = the identity frame), and bit-identical across layouts (the layout changes the data movement only)"""
    from gpu_utils import T
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.deform import sh_colors
    N = 1061
    sc = scenes.make_cloud(N, seed=80 + deg, D=3)
    campos = np.array([4.0, 1.0, -3.0], np.float32)
    rot = _rot_frames(N, deg) if with_rot else np.broadcast_to(np.eye(3, dtype=np.float32), (N, 3, 3)).copy()
    first = None
    for M in (1, 4, 9, 12, 16, 20):
        if M < (deg + 1) ** 2:
            continue
        rows = _rows(sc["shs"], M)
        ref = oracle.sh_colors_rotated(sc["means"], campos, rot, rows, deg=deg)
        for aligned in (True, False):
            rgb = sh_colors(T(sc["means"]), T(campos), _operand(rows, aligned), rot=T(rot) if with_rot else None, deg=deg).cpu().numpy()
            what = "deg=%d M=%d aligned=%s" % (deg, M, aligned)
            assert np.isfinite(rgb).all() and np.abs(rgb - ref).max() <= 1e-5, what
            if first is None:
                first = rgb
            assert np.array_equal(rgb.view(np.uint32), first.view(np.uint32)), what


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_deform_shade_fallback_equals_the_fused_kernel(deg):
    """deform_shade(want_cov_rot=True) for M != 16 and for an unaligned M = 16 operand (deform + sh_colors) against the fused M = 16
    kernel on aligned rows: every output bit-identical"""
    from gpu_utils import T
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.deform import deform_shade
    verts, faces = scenes.torus_mesh(40, 30)
    N = 2 * 1024 + 37
    cl = scenes.bind_cloud_to_mesh(N, verts, faces, seed=5 + deg)
    V1, Rv, Sv = scenes.twist_bend_frame(verts, t=7)
    cov = scenes.cov3d_from_scale_rot(cl["scales"], cl["rots"]).astype(np.float32)
    dV = (V1 - verts).astype(np.float32)
    campos = np.array([4.0, 1.0, -3.0], np.float32)
    args = (T(cl["tri"], dtype=torch.int32), T(cl["weights"]), T(dV), T(Rv), T(Sv), T(cov), T(cl["means"]))
    fused = [x.cpu().numpy() for x in deform_shade(*args, _operand(cl["shs"], True), T(campos), deg=deg, want_cov_rot=True)]
    for M, aligned in sorted({((deg + 1) ** 2, True), (12, True), (20, True), (16, False), (9, False)}):
        if M < (deg + 1) ** 2:
            continue
        out = deform_shade(*args, _operand(_rows(cl["shs"], M), aligned), T(campos), deg=deg, want_cov_rot=True)
        for k, (x, y) in enumerate(zip(out, fused)):
            x = x.cpu().numpy()
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), ("M=%d aligned=%s output %d" % (M, aligned, k))


def test_too_few_coefficients_are_refused_before_any_launch(oracle):
    """M < (D+1)^2 is an argument error (gm_api.hip check_raster_args): the forward raises GmeshError with the library's message, and a
    backward given the same shapes returns the error without writing any of its (NaN pre-filled) outputs"""
    from gpu_utils import forward_state
    from gaussianmesh_amd import _lib
    P = 293
    sc, cam, bg = _scene(P, seed=3)
    for M, D in ((1, 1), (4, 2), (12, 3), (9, 3)):
        rows = _rows(sc["shs"], M)
        with pytest.raises(_lib.GmeshError, match=r"SH degree %d needs M >= %d coefficients \(got %d\); degree must be 0\.\.3" % (
                D, (D + 1) ** 2, M)):
            forward_state(dict(sc, shs=rows), cam, bg, D=D, shs=_operand(rows, True))
    sc["shs"] = _rows(sc["shs"], 4)
    shs = _operand(sc["shs"], True)
    st = forward_state(sc, cam, bg, D=1, shs=shs)
    outs = []
    with pytest.raises(_lib.GmeshError, match=r"SH degree 2 needs M >= 9 coefficients \(got 4\)"):
        _abi_backward(sc, cam, bg, st, shs, 2, _two_pixel_gradient(0), 0, keep=outs)
    torch.cuda.synchronize()
    assert len(outs) == 9 and all(bool(t.isnan().all()) for t in outs)
