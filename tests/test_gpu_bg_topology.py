"""GPU: the topology edits of bg_model.PlainGaussians on the device - densify_and_prune, prune_points, reset_opacity, with and without kept
gradients - with the SH rows shared with the joint buffer of renderer.bg_render.  The CPU model is the definition (test_bg_model_host.py
ties it to the reference's recorded states, tests/golden/bg_densify.npz): every copied quantity equals the CPU model's bit for bit, every
computed one is held per element to 8 x 2^-24 x its absolute sum against the float64 restatement of bg_topology_ref.py, the joint buffers
and the optimizer are wired to the new rows, the optimizer still steps them, a render after an edit matches the generic route, and
BgTrainer.neighbor_mask equals the float32 brute force."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bg_topology_ref as topo
import poison
from test_gpu_bg_train import PIPE, _brute_np, _camera, _clone_plain, _mesh_model, _plain, _rel

pytestmark = pytest.mark.gpu

PARAMS = ("_xyz", "_features", "_scaling", "_rotation", "_opacity")
STATS = ("max_radii2D", "xyz_gradient_accum", "denom")
NMESH = 50


def _opt_args():
    from gaussianmesh_amd.bg_train import BG_DEFAULT_OPT
    return SimpleNamespace(**BG_DEFAULT_OPT)


def _seeded_grads(model, seed):
    """the same non-zero float32 gradients for a CPU and a device model of the same row count"""
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(getattr(model, k).shape, generator=g) for k in PARAMS}


def _set_grads(model, grads):
    for k, v in grads.items():
        getattr(model, k).grad = v.to(model.device).clone()


def _pair(d, prefix, mesh, seed=11):
    cpu = topo.model_from(d, prefix, "cpu")
    dev = topo.model_from(d, prefix, "cuda")
    dev.share_feature_storage(mesh)
    grads = _seeded_grads(cpu, seed)
    _set_grads(cpu, grads)
    _set_grads(dev, grads)
    return cpu, dev


def _groups(model):
    return {g["name"]: g for g in model.optimizer.param_groups}


def _np(t):
    return t.detach().cpu().numpy()


def _assert_rows(dev, cpu, computed=(), grads=False):
    """row count and order, every copied quantity bit for bit the CPU model's.  computed: {attribute: bool mask [n] or [n,1..]} of the
    elements that are computed, not copied (checked by the caller against float64)"""
    n = cpu._xyz.shape[0]
    computed = dict(computed)
    gd, gc = _groups(dev), _groups(cpu)
    assert [g["name"] for g in dev.optimizer.param_groups] == [g["name"] for g in cpu.optimizer.param_groups]
    for name, attr in dev._PARAM_OF_GROUP.items():
        a, b = _np(getattr(dev, attr)), _np(getattr(cpu, attr))
        assert a.shape == b.shape and a.shape[0] == n, (attr, a.shape, b.shape)
        copied = ~np.broadcast_to(computed.get(attr, np.zeros(1, bool)).reshape((-1,) + (1,) * (a.ndim - 1)), a.shape)
        assert np.array_equal(a.view(np.uint32)[copied], b.view(np.uint32)[copied]), attr
        for slot in ("m", "values"):                              # both Adam moments of all five groups
            assert poison.same_bits(gd[name][slot][0].cpu(), gc[name][slot][0]), (name, slot)
        assert gd[name]["params"][0] is getattr(dev, attr), name
        if grads:
            assert getattr(cpu, attr).grad is not None and getattr(dev, attr).grad is not None, attr
            assert poison.same_bits(getattr(dev, attr).grad.cpu(), getattr(cpu, attr).grad), attr
    for s in STATS:
        assert poison.same_bits(getattr(dev, s).cpu(), getattr(cpu, s)), s


def _assert_wiring(dev, mesh):
    from gaussianmesh_amd.bg_model import PlainGaussians
    n = dev._xyz.shape[0]
    jb = dev._plain_joint
    assert dev._features.data_ptr() == jb["shs"].data_ptr()
    assert _groups(dev)[PlainGaussians.SH_GROUP]["params"][0] is dev._features
    assert jb["N"] == n and jb["Nm"] == NMESH
    with torch.no_grad():
        tails = {"xyz": mesh.get_xyz, "scales": mesh.get_scaling, "rots": mesh.get_rotation, "opac": mesh.get_opacity.reshape(-1, 1),
                 "shs": mesh.get_features[:, :jb["K"]]}
        for k, want in tails.items():
            assert jb[k].shape[0] == n + NMESH and poison.same_bits(jb[k][n:], want.detach()), k
    assert dev.screenspace_points.shape == (n, 3) and dev.screenspace_points.is_cuda and jb["ss"].shape == (n + NMESH, 3)
    for s in STATS:
        assert getattr(dev, s).shape[0] == n and getattr(dev, s).is_cuda


def _assert_optimizer_steps(dev, mesh, seed=23):
    """the model against a twin restored from its own capture(): same gradients, one step each, every bit equal - and the step moved the
    model's own tensors, `_features` (the head of the joint SH buffer) included, and nothing behind them"""
    from gaussianmesh_amd.bg_model import PlainGaussians
    twin = PlainGaussians(dev.max_sh_degree, device="cuda")
    twin.restore(dev.capture(), _opt_args())
    assert twin.optimizer.n_step == dev.optimizer.n_step
    gt, gd = _groups(twin), _groups(dev)
    for k in PARAMS:
        assert poison.same_bits(getattr(twin, k), getattr(dev, k)), k
    for name in gd:
        assert twin.optimizer is not dev.optimizer and gt[name]["params"][0].data_ptr() != gd[name]["params"][0].data_ptr()
        assert poison.same_bits(gt[name]["m"][0], gd[name]["m"][0]) and poison.same_bits(gt[name]["values"][0], gd[name]["values"][0])
        assert gt[name]["lr"] == gd[name]["lr"] and gt[name].get("lr_rest") == gd[name].get("lr_rest")
    for s in STATS:
        assert poison.same_bits(getattr(twin, s), getattr(dev, s)), s
    grads = _seeded_grads(dev, seed)
    before = {k: getattr(dev, k).detach().clone() for k in PARAMS}
    for m in (twin, dev):
        _set_grads(m, grads)
        m.optimizer.step()
    torch.cuda.synchronize()
    for k in PARAMS:
        assert poison.same_bits(getattr(twin, k), getattr(dev, k)), k
        changed = getattr(dev, k).detach() != before[k]
        assert changed.float().mean().item() > 0.9, (k, changed.float().mean().item())
    assert (dev._features[:, :1].detach() != before["_features"][:, :1]).any() and (dev._features[:, 1:].detach() != before["_features"][:, 1:]).any()
    for name in gd:
        assert poison.same_bits(gt[name]["m"][0], gd[name]["m"][0]) and poison.same_bits(gt[name]["values"][0], gd[name]["values"][0]), name
    _assert_wiring(dev, mesh)                                     # (the tails still hold the mesh model's rows)
    dev.optimizer.zero_grad()


@pytest.fixture(scope="module")
def gold():
    return np.load(topo.GOLD)


@pytest.fixture(scope="module")
def mesh():
    return _mesh_model(n=NMESH)


# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["A", "B"])
def test_densify_and_prune(case, gold, mesh):
    d = gold
    plan = topo.densify_plan(d, case)
    assert plan["margin"] >= topo.MARGIN                          # an exp that is an ulp off cannot change a selection
    cpu, dev = _pair(d, case + "0", mesh)
    _assert_rows(dev, cpu, grads=True)
    _assert_wiring(dev, mesh)
    for m in (cpu, dev):
        m.densify_and_prune(float(d[case + "_threshold"]), topo.MIN_OPACITY, topo.EXTENT, None, samples=torch.as_tensor(d[case + "_Z"]))
    split = plan["kind"] == "split"
    assert cpu._xyz.shape[0] == dev._xyz.shape[0] == plan["src"].size and 0 < split.sum() < split.size
    _assert_rows(dev, cpu, computed={"_xyz": split, "_scaling": split})
    assert all(getattr(dev, k).grad is None for k in PARAMS)      # (no kept gradients on this path)
    for attr, name in (("_xyz", "xyz"), ("_scaling", "scaling")):
        r = topo.ratio(_np(getattr(dev, attr))[split], plan[name][split], plan[name + "_abs"][split])
        print("case %s, split rows' %s on the device: worst %.3f units of 2^-24 S_abs (bound %g)" % (case, name, r.max(), topo.FACTOR))
        assert (r <= topo.FACTOR).all(), (attr, float(r.max()))
    _assert_wiring(dev, mesh)
    _assert_optimizer_steps(dev, mesh)


def test_prune_then_reset_opacity(gold, mesh):
    d = gold
    cpu, dev = _pair(d, "C0", mesh)
    mask = torch.as_tensor(d["C_mask"])
    cpu.prune_points(mask)
    dev.prune_points(mask.cuda())
    assert dev._xyz.shape[0] == int((~mask).sum()) < mask.numel()
    _assert_rows(dev, cpu)
    assert all(getattr(dev, k).grad is None for k in PARAMS)
    _assert_wiring(dev, mesh)
    x = _np(cpu._opacity).copy()
    cpu.reset_opacity()
    dev.reset_opacity()
    _assert_rows(dev, cpu, computed={"_opacity": np.ones(x.shape[0], bool)})
    assert not _groups(dev)["opacity"]["m"][0].any() and not _groups(dev)["opacity"]["values"][0].any()
    want, s_abs = topo.reset_opacity_ref(x)
    r = topo.ratio(_np(dev._opacity), want, s_abs)
    print("reset opacities on the device: worst %.3f units of 2^-24 S_abs (bound %g)" % (r.max(), topo.FACTOR))
    assert (r <= topo.FACTOR).all()
    assert dev._opacity.grad is None
    _assert_wiring(dev, mesh)
    _assert_optimizer_steps(dev, mesh)


def test_prune_with_kept_gradients(gold, mesh):
    """the path BgTrainer.remove_neighbors takes: the surviving rows carry their gradients to this iteration's step"""
    d = gold
    cpu, dev = _pair(d, "B0", mesh)
    n = cpu._xyz.shape[0]
    mask = torch.rand(n, generator=torch.Generator().manual_seed(4)) < 0.4
    mask[0], mask[n - 1], mask[1] = True, True, False             # the first and the last row go, the second stays
    old = {k: getattr(cpu, k).grad.clone() for k in PARAMS}
    cpu.prune_points(mask, keep_grads=True)
    dev.prune_points(mask.cuda(), keep_grads=True)
    assert dev._xyz.shape[0] == int((~mask).sum())
    _assert_rows(dev, cpu, grads=True)
    for k in PARAMS:                                              # ... the gradients of the rows that stayed, in their order
        assert poison.same_bits(getattr(dev, k).grad.cpu(), old[k][~mask]), k
    _assert_wiring(dev, mesh)
    _assert_optimizer_steps(dev, mesh)


def test_reset_opacity_with_kept_gradient(gold, mesh):
    d = gold
    cpu, dev = _pair(d, "A0", mesh)
    old = {k: getattr(cpu, k).grad.clone() for k in PARAMS}
    x = _np(cpu._opacity).copy()
    cpu.reset_opacity(keep_grad=True)
    dev.reset_opacity(keep_grad=True)
    _assert_rows(dev, cpu, computed={"_opacity": np.ones(x.shape[0], bool)}, grads=True)
    for k in PARAMS:
        assert poison.same_bits(getattr(dev, k).grad.cpu(), old[k]), k
    want, s_abs = topo.reset_opacity_ref(x)
    assert (topo.ratio(_np(dev._opacity), want, s_abs) <= topo.FACTOR).all()
    _assert_wiring(dev, mesh)
    _assert_optimizer_steps(dev, mesh)


# ---------------------------------------------------------------------------------------------------------------------------------------
def _render_both(a, mesh, cam, up):
    """bg_render on the fused route of `a` and on the generic route of a clone; the gates of test_bg_render_fused_route_matches_generic_route"""
    from gaussianmesh_amd.renderer import bg_render
    b = _clone_plain(a, fused=False)
    bg = torch.tensor([0.1, 0.2, 0.3], device="cuda")
    pk = []
    for m in (a, b):
        for k in PARAMS:
            getattr(m, k).grad = None
        pkg = bg_render(cam, m, PIPE, bg, mesh_gaussians=mesh)
        (pkg["render"] * up).sum().backward()
        pk.append(pkg)
    pa, pb = pk
    n = a._xyz.shape[0]
    assert pa["radii"].shape[0] == n + NMESH and torch.equal(pa["radii"], pb["radii"])
    assert int((pa["radii"][:n] > 0).sum()) >= 30                # the rows are in view
    assert (pa["render"] - pb["render"]).abs().max().item() <= 1e-5
    for k in PARAMS:
        ga, gb = getattr(a, k).grad, getattr(b, k).grad
        assert ga is not None and ga.shape == gb.shape and gb.abs().max().item() > 0, k
        assert _rel(ga.cpu(), gb.cpu()) <= 1e-4, (k, _rel(ga.cpu(), gb.cpu()))
    assert a.screenspace_points.grad is not None and a.screenspace_points.grad.shape == (n, 3)
    assert _rel(a.screenspace_points.grad.cpu(), b.screenspace_points.grad.cpu()) <= 1e-4
    a.optimizer.zero_grad()


def test_a_render_after_an_edit_matches_the_generic_route(mesh):
    a = _plain(n=300)
    a.spatial_lr_scale = 1.0
    a.share_feature_storage(mesh)
    a.training_setup(_opt_args())
    cam = _camera(1, 6, w=64, h=48)
    up = torch.randn((3, 48, 64), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    _render_both(a, mesh, cam, up)
    g = torch.Generator().manual_seed(6)
    a.xyz_gradient_accum = torch.rand((300, 1), generator=g).cuda()
    a.denom = torch.ones((300, 1), device="cuda")
    # scales are 0.05 .. 0.3: with an extent of 15 the rows fall on both sides of percent_dense * extent = 0.15
    a.densify_and_prune(0.5, 0.005, 15.0, None, generator=torch.Generator(device="cuda").manual_seed(1))
    n1 = a._xyz.shape[0]
    assert n1 > 300
    _assert_wiring(a, mesh)
    _render_both(a, mesh, cam, up)
    # back to an earlier row count: plain_joint_buffers keys its cache on the row count
    mask = torch.zeros(n1, dtype=torch.bool, device="cuda")
    mask[torch.randperm(n1, generator=g)[:n1 - 300].cuda()] = True
    a.prune_points(mask)
    assert a._xyz.shape[0] == 300
    _assert_wiring(a, mesh)
    _render_both(a, mesh, cam, up)


@pytest.mark.parametrize("squared", [True, False])
def test_neighbor_mask_equals_the_brute_force(squared, mesh):
    from gaussianmesh_amd.bg_train import BgTrainer
    obj = mesh.get_xyz.detach()
    n = 90
    model = _plain(n=n)
    g = torch.Generator().manual_seed(8)
    direction = torch.nn.functional.normalize(torch.randn(n, 3, generator=g)).cuda()
    # rows ON the object, near it on either side of the threshold (0.1 squared, 0.01 not), and far from it
    offsets = {True: (0.0, 0.03, 0.08, 0.097, 0.103, 0.15, 0.5, 3.0), False: (0.0, 0.003, 0.008, 0.0097, 0.0103, 0.015, 0.5, 3.0)}[squared]
    off = torch.tensor(offsets, device="cuda").repeat_interleave(10)
    with torch.no_grad():
        model._xyz[:80].copy_(obj[torch.arange(80) % NMESH] + off[:, None] * direction[:80])
    tr = BgTrainer(model, mesh, remove_neighbor_iterations=(), squared=squared)
    mask = tr.neighbor_mask()
    d2, _ = _brute_np(_np(model._xyz), _np(obj))
    dist = d2 if squared else np.sqrt(d2)
    thr = np.float32(tr.min_distance)
    assert (np.abs(dist.astype(np.float64) - float(thr)) > 1e-4 * float(thr)).all()       # no row within 1e-4 of the threshold
    want = dist < thr
    assert mask.shape == (n,) and mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), want)
    assert 10 <= want.sum() <= n - 10 and want[:10].all() and not want[80:].any()
    kept = _np(model._xyz)[~want]
    tr.remove_neighbors(keep_grads=False)
    assert tr.pruned_neighbors == int(want.sum()) and np.array_equal(_np(model._xyz), kept)
    _assert_wiring(model, mesh)
