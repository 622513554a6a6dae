"""-m gpu: gm_deform_shade_bwd (csrc/gm_deform_bwd.hip) on the cases of deform_bwd_cases.py, and deform.deform_shade_differentiable on top.

a. Every element of g_dV / g_Rv / g_Sv and of the optional g_shs / g_cov / g_rest_pos against the float64 definition (deform_bwd_ref.py):
   |got - ref| <= 2 r_f32 2^-24 S_abs, r_f32 what the float32 emulation with sequential vertex sums reaches (measured on the CPU,
   test_deform_bwd_ref_host.py, which also shows that this gate rejects wrong backwards).  All five kinds, degrees 0..3, N in (1, 63, 64, 65,
   257), both colour cameras, the inactive SH coefficients NaN.  The clamp gate and the view direction's positions are the device forward's
   own (rgb > 0, pos'), as deform_bwd_ref.py explains.
b. The rewired bindings: lists of 0, 1, 63, 64, 65, 129 and 600 entries, an unused last vertex; empty lists give +0.0 exactly.
c. The mandatory outputs' bits do not depend on which optional outputs are asked for, nor on NULL against all-zero g_rgb / g_cov6.
d. The same bits on two runs and under every fill of poison.run_under_fills, guard bands intact (outputs and workspace).
e. Wiring: autograd through deform_shade_differentiable and GaussianRasterizer equals, bit for bit, one gm_deform_shade_bwd on the three
   gradients the rasterizer delivered in that backward; None for inputs that do not require grad; the forward's bits are deform_shade's.
   The chain by hand from leaf copies runs the rasterizer's backward a second time, and that backward sums with float atomics: measured
   on the MI355X it does not repeat its bits and the tables then differ by 2e-7 of their max-norm.  That route is asserted bit for bit
   whenever the rasterizer repeats itself and to 1e-3 of the max-norm otherwise (the reasoning stands at the assertion).
f. Rows of M != 16 coefficients (other load and store routes) give the bits of the M = 16 call."""
import numpy as np
import pytest
import torch

import deform_bwd_cases as bc
import deform_bwd_ref as bref
import deform_cases as dc
import poison

pytestmark = pytest.mark.gpu

OPTIONAL = ("g_shs", "g_cov", "g_rest_pos")


def _inputs(kind, deg, n):
    from gpu_utils import T
    from gaussianmesh_amd.deform import DeformBinding
    c, u = bc.case(kind), bc.upstream(kind)
    g = dict(cov=T(c["cov"][:n]), pos=T(c["pos"][:n]), shs=T(bc.shs(kind, deg)[:n]), dV=T(c["dV"]), Rv=T(c["Rv"]), Sv=T(c["Sv"]),
             g_pos=T(u["g_pos"][:n]), g_cov6=T(u["g_cov6"][:n]), g_rgb=T(u["g_rgb"][:n]))
    g["binding"] = DeformBinding(T(c["tri"][:n], dtype=torch.int32), T(c["w"][:n]), c["Vm"])
    return g


def _forward(g, deg, campos):
    from gaussianmesh_amd.deform import deform_shade
    b = g["binding"]
    return deform_shade(b.tri, b.w, g["dV"], g["Rv"], g["Sv"], g["cov"], g["pos"], g["shs"], campos, deg=deg)


def _backward(g, deg, campos, optional=OPTIONAL, g_cov6="given", g_rgb="given", keep_workspace=False):
    """one gm_deform_shade_bwd on fresh torch.empty buffers: dict of the outputs (and the workspace)"""
    from gaussianmesh_amd._op import enqueue, workspace
    b = g["binding"]
    dev = g["pos"].device
    N, M, Vm = g["pos"].shape[0], g["shs"].shape[1], b.Vm
    f = dict(dtype=torch.float32, device=dev)
    out = dict(g_dV=torch.empty((Vm, 3), **f), g_Rv=torch.empty((Vm, 9), **f), g_Sv=torch.empty((Vm, 9), **f))
    shapes = dict(g_shs=(N, M, 3), g_cov=(N, 9), g_rest_pos=(N, 3))
    for k in OPTIONAL:
        out[k] = torch.empty(shapes[k], **f) if k in optional else None
    up = {"g_cov6": g_cov6, "g_rgb": g_rgb}
    for k, v in up.items():
        up[k] = g[k] if v == "given" else (torch.zeros_like(g[k]) if v == "zeros" else None)
    ws = workspace(dev, "gm_deform_shade_bwd_workspace_bytes", N, Vm)
    enqueue(dev, "gm_deform_shade_bwd", N, deg, M, Vm, b.tri, b.w, g["dV"], g["Rv"], g["Sv"], g["cov"], g["pos"], g["shs"], campos, b.inc_offsets,
            b.inc_entries, g["g_pos"], up["g_cov6"], up["g_rgb"], out["g_dV"], out["g_Rv"], out["g_Sv"], out["g_shs"], out["g_cov"],
            out["g_rest_pos"], workspace=ws)
    if keep_workspace:
        out["workspace"] = ws[:N * 21 * 4]                  # (the bytes the call defines; the size is rounded up)
    return out


def _check_against_float64(kind, deg, n, cam_name, campos, worst, problems):
    from gpu_utils import T
    g = _inputs(kind, deg, n)
    cam = T(campos)
    pos1, _, rgb = _forward(g, deg, cam)
    got = {k: v.cpu().numpy() for k, v in _backward(g, deg, cam).items()}
    assert all(np.isfinite(v).all() for v in got.values()), (kind, deg, n, cam_name)            # NaN beyond the degree is never read
    assert not got["g_shs"][:, (deg + 1) ** 2:].any(), (kind, deg, n)
    gate, npos32 = rgb.cpu().numpy() > 0, pos1.cpu().numpy()
    a = bc.args(kind, deg, campos, n)
    want = bref.backward(*a, gate, np.float64, npos_dir=npos32)
    s_abs = bref.backward_abs(*a, gate, npos_dir=npos32)
    for t, r in bref.ratios(got, want, s_abs).items():
        bar = 2.0 * bref.R_F32[kind][t]
        i = int(np.argmax(r))
        worst[t] = max(worst[t], float(r.reshape(-1)[i]) / bar)
        if not r.max() <= bar:
            problems.append("N = %d, %s camera: %s element %d at %.3g (bar %.3g); %d elements over" % (n, cam_name, t, i, r.reshape(-1)[i], bar, int((r > bar).sum())))
    return got


@pytest.mark.parametrize("kind,deg", [(kind, deg) for kind in dc.KINDS for deg in range(4)])
def test_every_element_against_float64(kind, deg):
    worst, problems = dict.fromkeys(bref.TENSORS, 0.0), []
    for n in bc.NS:
        for cam_name, campos in bc.cameras(kind):
            _check_against_float64(kind, deg, n, cam_name, campos, worst, problems)
    print("deform backward, per element: %s degree %d: worst ratio / (2 r_f32): " % (kind, deg) + "  ".join("%s %.3f" % (t, worst[t]) for t in bref.TENSORS))
    assert not problems, "%s, degree %d:\n" % (kind, deg) + "\n".join(problems[:20])


@pytest.mark.parametrize("kind", bc.REWIRED)
def test_accumulation_edges(kind):
    worst, problems = dict.fromkeys(bref.TENSORS, 0.0), []
    lengths = bc.list_lengths(kind)
    empty = np.where(lengths == 0)[0]
    assert len(empty) and lengths[-1] == 0 if kind != "hub" else lengths.max() > 256
    for deg in (0, 3):
        for cam_name, campos in bc.cameras(kind):
            got = _check_against_float64(kind, deg, dc.NMAX, cam_name, campos, worst, problems)
            for t in bref.VERTEX_TENSORS:                   # an empty list: +0.0, every bit
                assert not got[t][empty].view(np.uint32).any(), (kind, deg, t)
                assert np.abs(got[t][lengths > 0]).max() > 0
    print("deform backward, %s (lists of up to %d entries, %d empty): worst ratio / (2 r_f32): " % (kind, lengths.max(), len(empty)) +
          "  ".join("%s %.3f" % (t, worst[t]) for t in bref.TENSORS))
    assert not problems, "%s:\n" % kind + "\n".join(problems[:20])


@pytest.mark.parametrize("kind,deg,n", [("twist", 3, 257), ("clamp", 2, 65), ("hub", 1, 257), ("needle", 0, 64)])
def test_mandatory_bits_do_not_depend_on_the_options(kind, deg, n):
    from gpu_utils import T
    g, cam = _inputs(kind, deg, n), T(dc.CAMPOS)
    full = _backward(g, deg, cam)
    tables = lambda o: {t: o[t] for t in bref.VERTEX_TENSORS}
    assert poison.same_bits(tables(_backward(g, deg, cam, optional=())), tables(full))
    for only in OPTIONAL:
        one = _backward(g, deg, cam, optional=(only,))
        assert poison.same_bits(tables(one), tables(full)) and poison.same_bits(one[only], full[only]), only
    for name in ("g_rgb", "g_cov6"):
        null, zeros = _backward(g, deg, cam, **{name: None}), _backward(g, deg, cam, **{name: "zeros"})
        assert poison.same_bits(null, zeros), name
        if deg > 0 or name == "g_cov6":                     # (at degree 0 the colour does not depend on the pose)
            assert not poison.same_bits(tables(null), tables(full)), name + " contributes"
    null = _backward(g, deg, cam, optional=("g_cov", "g_rest_pos"), g_rgb=None, g_cov6=None)      # positions alone
    zeros = _backward(g, deg, cam, optional=("g_cov", "g_rest_pos"), g_rgb="zeros", g_cov6="zeros")
    assert poison.same_bits(null, zeros)
    assert torch.equal(null["g_rest_pos"], g["g_pos"])


@pytest.mark.parametrize("kind,deg,n", [("twist", 3, 257), ("hub", 3, 257), ("edges", 2, 65), ("outside", 1, 1)])
def test_same_bits_every_run_and_under_every_fill(kind, deg, n):
    from gpu_utils import T
    g, cam = _inputs(kind, deg, n), T(dc.CAMPOS)
    route = lambda: _backward(g, deg, cam, keep_workspace=True)
    first, second = route(), route()
    assert poison.same_bits(first, second)
    runs = poison.run_under_fills(route)
    assert all(p.handed_out == 7 for p, _ in runs), [p.handed_out for p, _ in runs]               # three tables, three optional outputs, the workspace
    assert poison.differing(runs) == []
    assert poison.same_bits(runs[0][1], first)


@pytest.mark.parametrize("deg,M", [(0, 1), (1, 4), (2, 9), (3, 20)])
def test_other_row_strides_give_the_same_bits(deg, M):
    """rows of M != 16 coefficients (load_sh's float-at-a-time route, a g_shs row of another stride; M > 16: the tail is written as 0)
    against the M = 16 call on the same values: every shared element bit for bit.  Through the op as well: its forward takes the
    unfused route there."""
    from gpu_utils import T
    from gaussianmesh_amd.deform import deform_shade_differentiable
    n = 65
    g, cam = _inputs("twist", deg, n), T(dc.CAMPOS)
    want = _backward(g, deg, cam)
    h = dict(g)
    h["shs"] = torch.full((n, M, 3), float("nan"), device=cam.device)
    k = min(M, 16)
    h["shs"][:, :k] = g["shs"][:, :k]
    got = _backward(h, deg, cam)
    assert got["g_shs"].shape == (n, M, 3) and poison.same_bits(got["g_shs"][:, :k].contiguous(), want["g_shs"][:, :k].contiguous())
    assert not got["g_shs"][:, (deg + 1) ** 2:].view(torch.int32).any()
    for t in bref.VERTEX_TENSORS + ("g_cov", "g_rest_pos"):
        assert poison.same_bits(got[t], want[t]), t
    dV = g["dV"].clone().requires_grad_(True)
    out = deform_shade_differentiable(g["binding"], dV, g["Rv"], g["Sv"], g["cov"], g["pos"], h["shs"], cam, deg=deg)
    assert poison.same_bits(tuple(t.detach() for t in out), _forward(g, deg, cam))
    torch.autograd.backward(out, (g["g_pos"], g["g_cov6"], g["g_rgb"]))
    assert poison.same_bits(dV.grad, want["g_dV"])


def test_wiring_through_the_rasterizer():
    """loss = (image * dpix).sum() through deform_shade_differentiable and GaussianRasterizer against the chain by hand"""
    from gpu_utils import T, settings
    from gaussianmesh_amd import GaussianRasterizer
    from gaussianmesh_amd.deform import deform_shade_differentiable
    kind, deg, n = "twist", 3, dc.NMAX
    c = bc.case(kind)
    cam = dc.frame_camera(1)
    g = _inputs(kind, deg, n)
    g["shs"] = T(c["shs"][:n])
    opac, campos = T(c["opac"][:n]), T(cam["campos"])
    dpix = T(np.random.default_rng(3).normal(size=(3, dc.H, dc.W)).astype(np.float32))
    rast = GaussianRasterizer(settings(cam, np.array([0.1, 0.5, 0.9], np.float32), deg))

    def render(pos1, cov6, rgb):
        image, radii = rast(pos1, torch.zeros_like(pos1), opac, colors_precomp=rgb, cov3D_precomp=cov6)
        assert int((radii > 0).sum()) > n // 4
        return (image * dpix).sum()

    # autograd: gradients to the tables and the SH rows, not to cov and pos
    leaves = {k: g[k].clone().requires_grad_(True) for k in ("dV", "Rv", "Sv", "shs")}
    out = deform_shade_differentiable(g["binding"], leaves["dV"], leaves["Rv"].reshape(-1, 3, 3), leaves["Sv"], g["cov"], g["pos"], leaves["shs"], campos, deg=deg)
    assert poison.same_bits(tuple(t.detach() for t in out), _forward(g, deg, campos))
    for t in out:
        t.retain_grad()                                     # what the rasterizer hands to the Function in THIS backward
    render(*out).backward()
    # by hand: those three gradients into gm_deform_shade_bwd - bit for bit what autograd delivered
    up = dict(g, g_pos=out[0].grad, g_cov6=out[1].grad, g_rgb=out[2].grad)
    want = _backward(up, deg, campos, optional=("g_shs",))
    assert all(float(want[t].abs().max()) > 0 for t in ("g_dV", "g_Rv", "g_Sv", "g_shs"))
    names = (("dV", "g_dV"), ("Rv", "g_Rv"), ("Sv", "g_Sv"), ("shs", "g_shs"))
    for name, t in names:
        assert leaves[name].grad.shape == leaves[name].shape
        assert poison.same_bits(leaves[name].grad.reshape(want[t].shape), want[t]), name
    # by hand from scratch: the rasterizer on leaf copies of the forward's outputs.  Its backward sums with float atomics (the
    # summation order varies from run to run), so this second backward need not repeat the first one's bits: where it does, the tables must
    # too; where it does not, they differ by the linear image of that difference - held to 1e-3 of each tensor's max-norm, the bar the
    # rasterizer's own gradients are held to (DESIGN.md "Gradients"; reordering a sum of n <= W H = 6144 pixel terms moves it by at most
    # 2 n 2^-24 = 7e-4 of the terms' absolute sum).
    hand = [t.detach().clone().requires_grad_(True) for t in out]
    render(*hand).backward()
    repeated = poison.same_bits([h.grad for h in hand], [t.grad for t in out])
    up2 = dict(g, g_pos=hand[0].grad, g_cov6=hand[1].grad, g_rgb=hand[2].grad)
    want2 = _backward(up2, deg, campos, optional=("g_shs",))
    worst = max(float((want2[t] - want[t]).abs().max() / want[t].abs().max()) for _, t in names)
    print("wiring: the rasterizer's second backward %s the first one's bits; by-hand tables differ by %.3g of their max-norm" % (
        "repeated" if repeated else "did not repeat", worst))
    for name, t in names:
        if repeated:
            assert poison.same_bits(leaves[name].grad.reshape(want2[t].shape), want2[t]), name
    assert worst <= 1e-3
    up = up2
    # None for the inputs that do not require grad; cov and pos when they do
    cov, pos = g["cov"].clone().requires_grad_(True), g["pos"].clone().requires_grad_(True)
    out = deform_shade_differentiable(g["binding"], g["dV"], g["Rv"], g["Sv"], cov, pos, g["shs"], campos, deg=deg)
    from gaussianmesh_amd.deform import _DeformShade
    # the Function's own answer, per input (binding, deg, dV, Rv, Sv, cov, pos, shs, campos): the node is its context
    res = _DeformShade.backward(out[0].grad_fn, hand[0].grad, hand[1].grad, hand[2].grad)
    assert [r is None for r in res] == [True, True, True, True, True, False, False, True, True], [r is None for r in res]
    want = _backward(up, deg, campos, optional=("g_cov", "g_rest_pos"))
    assert res[5].shape == cov.shape and poison.same_bits(res[5].reshape(n, 9), want["g_cov"]) and poison.same_bits(res[6], want["g_rest_pos"])
    for t in out:
        t.retain_grad()
    render(*out).backward()                                 # (a third backward of the rasterizer: its own upstream gradients)
    want = _backward(dict(g, g_pos=out[0].grad, g_cov6=out[1].grad, g_rgb=out[2].grad), deg, campos, optional=("g_cov", "g_rest_pos"))
    assert poison.same_bits(cov.grad.reshape(n, 9), want["g_cov"]) and poison.same_bits(pos.grad, want["g_rest_pos"])
    assert all(g[k].grad is None for k in ("dV", "Rv", "Sv", "shs"))
