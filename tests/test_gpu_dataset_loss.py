"""GPU: the loss kernels on an 8-bit ground truth (gm_ssim_fwd_u8 / gm_ssim_bwd_u8, loss.photometric_loss_u8) against the float
kernels on GroundTruth.float_target - BIT FOR BIT: the target's bits are equal by construction (correctly rounded u/255, the
composite's four operations rounded one by one in the reference's order) and every later instruction is the same kernel body.
Also the first model from a proxy mesh on the device, and Trainer.step with a GroundTruth."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(64, 64), (37, 45), (130, 97), (5, 7), (1080, 1920)]
MASKS = ["none", "c1", "c3", "zeros", "full"]


def _ground_truth(seed, H, W, variant):
    from gaussianmesh_amd.dataset import GroundTruth
    rng = np.random.default_rng(seed)
    rgb = torch.tensor(rng.integers(0, 256, (3, H, W), dtype=np.uint8), device="cuda")
    mask = {"none": None,
            "c1": lambda: rng.integers(0, 256, (1, H, W), dtype=np.uint8),
            "c3": lambda: rng.integers(0, 256, (3, H, W), dtype=np.uint8),
            "zeros": lambda: np.zeros((1, H, W), np.uint8),
            "full": lambda: np.full((3, H, W), 255, np.uint8)}[variant]
    mask = None if mask is None else torch.tensor(mask(), device="cuda")
    image = torch.tensor(rng.random((3, H, W)).astype(np.float32), device="cuda")
    return GroundTruth(rgb, mask), image


def _u8_forward(image, gt, bg):
    """gm_ssim_fwd_u8 called as loss._fwd calls gm_ssim_fwd: (maps [3,3,H,W], partial [n,2])"""
    from gaussianmesh_amd import _lib, loss
    lib = _lib.lib()
    a = image.detach().contiguous()
    H, W = a.shape[-2:]
    rgb, mask, stride, bgp, keep = loss._u8_args(a, gt, bg)
    partial = torch.empty((int(lib.gm_ssim_partials(3, H, W)), 2), dtype=torch.float32, device="cuda")
    maps = torch.empty((3, 3, H, W), dtype=torch.float32, device="cuda")
    _lib.check(lib.gm_ssim_fwd_u8(a.data_ptr(), rgb, mask, stride, bgp, 3, H, W, maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr(),
                                  partial.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return maps, partial


def _assert_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    same = torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)
    if not same:
        d = (a.double() - b.double()).abs()
        print("%s: %d of %d entries differ, largest difference %.3e" % (what, int((d > 0).sum()), d.numel(), float(d.max())))
    assert same, what


@pytest.mark.parametrize("variant", MASKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_u8_loss_is_bit_identical_to_the_float_loss_on_the_composited_target(shape, variant):
    from gaussianmesh_amd import loss
    H, W = shape
    gt, image = _ground_truth(1000 * H + W, H, W, variant)
    bg = torch.rand(3, device="cuda", generator=torch.Generator("cuda").manual_seed(H + W))      # a device-side random background
    target = gt.float_target(bg)
    assert target.dtype == torch.float32 and target.shape == (3, H, W)
    _, _, maps_f, partial_f = loss._fwd(image, target, True)
    maps_u, partial_u = _u8_forward(image, gt, bg)
    _assert_bits(partial_u, partial_f.reshape(-1, 2), "partial sums")
    for k, name in enumerate(("dS/dmu1", "dS/dE11", "dS/dE12")):
        _assert_bits(maps_u[k], maps_f[k], name)
    for lam in (0.2, 0.0, 1.0):
        xf = image.clone().requires_grad_(True)
        xu = image.clone().requires_grad_(True)
        Lf = loss.photometric_loss(xf, target, lam)
        Lu = loss.photometric_loss_u8(xu, gt, bg, lam)
        _assert_bits(Lu.detach().reshape(1), Lf.detach().reshape(1), "loss value, lambda %g" % lam)
        (3.0 * Lf).backward()
        (3.0 * Lu).backward()
        _assert_bits(xu.grad, xf.grad, "dL/dimage, lambda %g" % lam)


def test_every_pair_of_byte_values_composites_to_the_tensor_expressions_bits():
    """All 256 x 256 (rgb, mask) byte pairs against three backgrounds: with lambda = 0 and a zero image the L1 gradient's sign and the
    partial L1 sums see every target value; the derivative maps (functions of the target's window sums) see them too."""
    from gaussianmesh_amd import loss
    from gaussianmesh_amd.dataset import GroundTruth
    i = torch.arange(256, dtype=torch.uint8, device="cuda")
    rgb = i.reshape(1, 256, 1).expand(3, 256, 256).contiguous()
    mask = i.reshape(1, 1, 256).expand(1, 256, 256).contiguous()
    gt = GroundTruth(rgb, mask)
    bg = torch.tensor([0.1, 0.7283951, 1.0 / 3.0], device="cuda")
    target = gt.float_target(bg)
    lut = np.arange(256, dtype=np.float32) / np.float32(255.0)                   # float32 division: correctly rounded
    g, m = lut[:, None], lut[None, :]
    for c in range(3):                                                           # float_target itself against numpy, operation by operation
        b = np.float32(bg[c].item())
        expect = (g * m).astype(np.float32) + (b * (np.float32(1.0) - m)).astype(np.float32)
        assert np.array_equal(target[c].cpu().numpy().view(np.int32), expect.astype(np.float32).view(np.int32)), c
    image = torch.full((3, 256, 256), 0.5, device="cuda")
    _, _, maps_f, partial_f = loss._fwd(image, target, True)
    maps_u, partial_u = _u8_forward(image, gt, bg)
    _assert_bits(partial_u, partial_f.reshape(-1, 2), "partial sums")
    _assert_bits(maps_u, maps_f, "derivative maps")
    # image == target exactly where the kernels composite the same bits: the L1 sum of the u8 path on image = float target is 0
    _, partial_0 = _u8_forward(target, gt, bg)
    assert float(partial_0[:, 1].abs().max()) == 0.0


def test_u8_loss_argument_errors():
    from gaussianmesh_amd import loss
    from gaussianmesh_amd.dataset import GroundTruth
    gt, image = _ground_truth(5, 16, 24, "c1")
    with pytest.raises(ValueError, match="background"):
        loss.photometric_loss_u8(image, gt, None)
    with pytest.raises(ValueError, match="shape"):
        loss.photometric_loss_u8(image[:, :-1], gt, torch.zeros(3, device="cuda"))
    with pytest.raises(ValueError):
        GroundTruth(gt.rgb.float())
    with pytest.raises(ValueError):
        GroundTruth(gt.rgb, gt.mask[:, :-1])
    # no gradient asked for: the forward writes no maps and returns the same value
    bg = torch.rand(3, device="cuda")
    a = loss.photometric_loss_u8(image, gt, bg, 0.2)
    b = loss.photometric_loss_u8(image.clone().requires_grad_(True), gt, bg, 0.2)
    _assert_bits(a.reshape(1), b.detach().reshape(1), "loss without / with maps")


def test_create_from_mesh_on_the_device():
    """The scales are log(sqrt(clamp(distCUDA2(face centres), 1e-7))) of the existing operator, bit for bit, on all three axes; every
    other tensor is the fixture's (tests/golden/mesh_init.npz: create_from_pcd executed on the reference's code, with a degenerate face)."""
    from gaussianmesh_amd import distCUDA2
    from gaussianmesh_amd.renderer import MeshBoundGaussians
    fix = np.load(os.path.join(_GOLD, "mesh_init.npz"))
    rs = np.random.RandomState(int(fix["seed"]))
    m = MeshBoundGaussians.create_from_mesh(fix["vertices"], fix["faces"], sh_degree=3, generator=rs)
    centres = ((m.vertex1.cpu() + m.vertex2.cpu() + m.vertex3.cpu()) / 3).cuda()      # the host's sum and true division, as create_from_mesh forms them
    expect = torch.log(torch.sqrt(torch.clamp(distCUDA2(centres), min=0.0000001)))[..., None].repeat(1, 3)
    _assert_bits(m._scaling.detach(), expect, "scales")
    assert m.active_sh_degree == 0 and m.max_sh_degree == 3
    for key, t in (("bc", m._bc), ("distance", m._distance), ("features_dc", m._features_dc), ("features_rest", m._features_rest),
                   ("rotation", m._rotation), ("opacity", m._opacity), ("vertex1", m.vertex1), ("vertex2", m.vertex2), ("vertex3", m.vertex3),
                   ("normal", m.normal), ("r", m.r), ("fid", m.fid), ("vertex_index", m.vertex_index), ("v", m.v)):
        got = t.detach().cpu().numpy()
        assert got.shape == fix[key].shape, key
        assert np.array_equal(got, fix[key].astype(got.dtype)), key
    # the CPU oracle's distances (what the fixture's scales were made from) agree to float32 rounding of the log / sqrt
    assert np.allclose(m._scaling.detach().cpu().numpy(), fix["scaling"], rtol=0, atol=2e-6)


def _trainer_pair():
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.dataset import GroundTruth
    from gaussianmesh_amd.renderer import Camera, MeshBoundGaussians
    verts, faces = scenes.torus_mesh(40, 24)
    build = lambda: MeshBoundGaussians.create_from_mesh(verts, faces, generator=np.random.RandomState(3))
    cam = Camera(scenes.orbit_camera(1, 5, 160, 96, radius=6.5), "cuda")
    rng = np.random.default_rng(8)
    gt = GroundTruth(torch.tensor(rng.integers(0, 256, (3, 96, 160), dtype=np.uint8), device="cuda"),
                     torch.tensor(rng.integers(0, 256, (1, 96, 160), dtype=np.uint8), device="cuda"))
    return build, cam, gt


# Run-to-run spread of ONE path's gradients in this iteration, as a fraction of the parameter group's largest gradient entry: the float
# path run six times on an MI355X gave at most 5.8e-7 (bc), 1.7e-7 (scaling), 1.3e-7 (SH), 1.2e-7 (view-space probe), 1.1e-7 (distance),
# 4.9e-8 (opacity); the rotation gradient is exactly zero (isotropic first model).  The bound is twice the maximum.
GRAD_SPREAD_MEASURED = 5.8e-7


def test_trainer_step_takes_a_ground_truth():
    """One iteration from identical states with keep_grads: Trainer.step(camera, GroundTruth, bg) against
    Trainer.step(camera, gt.float_target(bg), bg).  Same loss bits.  The gradients pass through the backward blend's float atomics,
    so two runs of ONE path already differ: measured spread of the float path GRAD_SPREAD_MEASURED (above) of a group's largest
    entry; the 8-bit path against the float path, same measurement: the same figures (5.8e-7 bc ... 4.9e-8 opacity).
    Bound: 2 x GRAD_SPREAD_MEASURED x the group's largest gradient entry.  The spread of this run is printed next to it."""
    from gaussianmesh_amd.train import Trainer
    build, cam, gt = _trainer_pair()
    bg = torch.tensor([0.2, 0.5, 0.9], device="cuda")
    target = gt.float_target(bg)

    def run(gt_arg):
        tr = Trainer(build())
        tr.keep_grads = True
        loss, _ = tr.step(cam, gt_arg, bg)
        torch.cuda.synchronize()
        return loss, {k: v.detach().clone() for k, v in tr.last_grads.items() if v is not None}

    loss_f1, g_f1 = run(target)
    loss_f2, g_f2 = run(target)
    loss_u, g_u = run(gt)
    _assert_bits(loss_u.reshape(1), loss_f1.reshape(1), "loss of the iteration")
    assert set(g_u) == set(g_f1)
    for name in sorted(g_f1):
        top = float(g_f1[name].abs().max())
        spread = float((g_f1[name] - g_f2[name]).abs().max())
        diff = float((g_u[name] - g_f1[name]).abs().max())
        print("%-12s largest |g| %.3e   float path twice: %.3e   u8 against float: %.3e" % (name, top, spread, diff))
        assert diff <= 2.0 * GRAD_SPREAD_MEASURED * top, (name, diff, top)
    assert sum(float(v.abs().max()) > 0 for v in g_u.values()) >= 6
