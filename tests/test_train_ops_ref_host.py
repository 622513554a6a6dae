"""Host checks of tests/train_ops_ref.py, the numpy reference the GPU tests of csrc/gm_train.hip compare with: its float64 adjoints equal
torch.autograd on the float64 torch composition of the reference's formulas (scene/mesh_based_gaussian_model.py:122-152, 172-174,
scene/gaussian_model.py:26-43, utils/loss_utils.py:86-108); adam_ref32 equals float32 torch.optim.Adam and the float64 rule; and the
float32 torch composition of every activation stays inside the GPU tests' tolerances on the GPU tests' inputs - the tolerances are ones a
correct float32 implementation meets there."""
import numpy as np
import pytest
import torch

import train_ops_ref as R

f64 = np.float64


def _torch_mesh(ins, dtype, mr_weight=None):
    """the torch composition; leaves bc, dist, scaling, rot, opac require a gradient"""
    t = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in ins.items()}
    leaves = [t[k].requires_grad_(True) for k in ("bc", "dist", "scaling", "rot", "opac")]
    w = torch.softmax(t["bc"], dim=1)
    xyz = w[:, 0:1] * t["v1"] + w[:, 1:2] * t["v2"] + w[:, 2:3] * t["v3"]
    xyz = xyz + 4.0 * t["r"] * (torch.sigmoid(t["dist"]) - 0.5) * t["normal"]
    sc = torch.exp(t["scaling"])
    out = [xyz, sc, torch.nn.functional.normalize(t["rot"]), torch.sigmoid(t["opac"])]
    if mr_weight is not None:
        wt = float(np.float32(mr_weight))
        radius = torch.sqrt(torch.norm(torch.cross(t["v2"] - t["v1"], t["v3"] - t["v1"], dim=1), dim=1))
        out.append(torch.clamp(sc.max(dim=1).values - wt * radius, min=0).sum())
    return leaves, out


def _grads(leaves, out, ups, g_mr=None):
    loss = sum((o * torch.tensor(u, dtype=o.dtype)).sum() for o, u in zip(out[:4], ups) if u is not None)
    if g_mr is not None:
        loss = loss + float(g_mr) * out[4]
    gs = torch.autograd.grad(loss, leaves, allow_unused=True)
    return {k: (np.zeros(tuple(l.shape)) if g is None else g.numpy()) for k, l, g in zip(("bc", "dist", "scaling", "rot", "opac"), leaves, gs)}


@pytest.mark.parametrize("N,which", [(1, 15), (257, 15), (4000, 15), (4000, 1), (4000, 2), (4000, 4), (4000, 8), (4000, 10)])
@pytest.mark.parametrize("mr", [False, True])
def test_mesh_adjoint_equals_float64_autograd(N, which, mr):
    """... to 1e-12 of the per-element scale, on the edge inputs of the GPU tests (clamp-active quaternions, the tied largest scale axis,
    hinge rows, saturated softmax and sigmoids included)"""
    ins, labels = R.mesh_edge_inputs(N, seed=N, shift=3 * N)
    ups = R.upstream(N, N, [bool(which >> b & 1) for b in range(4)])
    wt, g_mr = (R.MR_WEIGHT, 2.5) if mr else (None, None)
    leaves, out = _torch_mesh(ins, torch.float64, wt)
    want = _grads(leaves, out, ups, g_mr)
    fw = R.mesh_activate_ref(**ins, mr_weight=wt)
    for k, o in zip(("xyz", "scales", "rots", "opac"), out):
        msg = R.report("forward " + k, fw["out"][k], o.detach().numpy(), 1e-12 * fw["scale"][k] + 1e-300, labels, fw["scale"][k], cols=o.shape[1])
        assert not msg, msg
    if mr:
        assert abs(fw["out"]["mr"] - float(out[4].detach())) <= 1e-12 * fw["scale"]["mr"]
        tied = np.array(["same-bits" in l for l in labels])
        assert N < 100 or (tied & (fw["term"] > 0)).sum() > 10                         # tied axes with a live term are in the set
    grad, scale = R.mesh_activate_adjoint(ins["bc"], ins["dist"], ins["scaling"], ins["rot"], ins["opac"], ins["v1"], ins["v2"], ins["v3"],
                                          ins["normal"], ins["r"], *ups, mr_weight=wt, g_mr=g_mr)
    for k in grad:
        msg = R.report("d_" + k, grad[k], want[k], 1e-12 * scale[k] + 1e-300, labels, scale[k], cols=grad[k].shape[1])
        assert not msg, msg
    # the clamp-active rows: g / eps
    if ups[2] is not None:
        q = np.linalg.norm(ins["rot"].astype(f64), axis=1)
        act = q <= 1e-12
        assert N < 100 or (act & (q > 0)).sum() > 10
        assert np.allclose(grad["rot"][act], ups[2][act].astype(f64) * 1e12, rtol=1e-15, atol=0)


def test_the_issue_s_clamp_example():
    """q = (3e-13, 0, -4e-13, 0), g = (1, 2, 3, 4): autograd gives g 1e12; the projection formula would give (1.27, 2, 2.64, 4) 1e12"""
    q = np.array([[3e-13, 0, -4e-13, 0]]); g = np.array([[1.0, 2, 3, 4]])
    d, _ = R._normalize_adjoint(q, g)
    t = torch.tensor(q, requires_grad=True)
    (torch.nn.functional.normalize(t) * torch.tensor(g)).sum().backward()
    assert np.allclose(d, g * 1e12, rtol=1e-15) and np.allclose(t.grad.numpy(), d, rtol=1e-12)
    y = q / 1e-12
    assert abs(((g - y * (y * g).sum()) / 1e-12)[0, 0] / 1e12 - 1.27) < 0.005


def test_plain_adjoint_equals_float64_autograd():
    N = 3000
    ins, labels = R.mesh_edge_inputs(N, seed=5)
    ups = R.upstream(N, 5)
    xyz = ins["v1"]
    t = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (xyz, ins["scaling"], ins["rot"], ins["opac"])]
    out = (t[0] * 1.0, torch.exp(t[1]), torch.nn.functional.normalize(t[2]), torch.sigmoid(t[3]))
    ref_out, ref_scale, _ = R.plain_activate_ref(xyz, ins["scaling"], ins["rot"], ins["opac"])
    for k, o in zip(("xyz", "scales", "rots", "opac"), out):
        assert not R.report(k, ref_out[k], o.detach().numpy(), 1e-12 * ref_scale[k] + 1e-300, labels, cols=o.shape[1])
    gs = torch.autograd.grad(sum((o * torch.tensor(u, dtype=torch.float64)).sum() for o, u in zip(out, ups)), t)
    grad, scale = R.plain_activate_adjoint(xyz, ins["scaling"], ins["rot"], ins["opac"], *ups)
    for k, g in zip(("xyz", "scaling", "rot", "opac"), gs):
        msg = R.report("d_" + k, grad[k], g.numpy(), 1e-12 * scale[k] + 1e-300, labels, scale[k], cols=g.shape[1])
        assert not msg, msg


# ------------------------------------------------------------------------------------------------------------ Adam
def test_adam_ref32_equals_float32_torch_adam_two_rate_layout():
    """eps = 1e-15, the SH tensor [n,16,3] as one two-rate tensor against torch's f_dc / f_rest groups, six steps: within 2 ulp of each
    parameter.  (Equal bits are not required: torch groups the step-size arithmetic differently.)
    The ulp is that of the largest magnitude the parameter has had so far, and the two implementations' STEPS may differ on top of it: a
    parameter that a step carries through zero is the small difference of two numbers, and 2 ulp of ITSELF is then not a statement about
    rounding (measured: up to 79 of its own ulp, 7e-11 absolute, on a parameter of 4e-6).  Per step t both sides round the moments
    (2 roundings each on the magnitudes b1 |m| + c1 |g| that are added, 4 U; v: 4 U on sqrt(v), i.e. 2 U) and the step itself
    (4 roundings each, 8 U): 16 U of st (b1 |m| + c1 |g|) / (sqrt(v') + eps), and the moments' own differences persist from the earlier
    steps, hence the factor t."""
    rng = np.random.default_rng(0)
    n, lr, steps = 1000, 0.005, 6
    p = rng.standard_normal((n, 16, 3)).astype(np.float32)
    m = np.zeros_like(p); v = np.zeros_like(p)
    q_dc = torch.tensor(p[:, :1].copy(), requires_grad=True); q_rest = torch.tensor(p[:, 1:].copy(), requires_grad=True)
    opt = torch.optim.Adam([{"params": [q_dc], "lr": lr}, {"params": [q_rest], "lr": lr / 20}], lr=0.0, eps=1e-15)
    rate = np.full((1, 16, 1), lr / 20); rate[:, 0] = lr
    pmax, allow, worst = np.abs(p).astype(f64), np.zeros(p.shape), 0.0
    for t in range(1, steps + 1):
        g = rng.standard_normal(p.shape).astype(np.float32)
        q_dc.grad, q_rest.grad = torch.tensor(g[:, :1].copy()), torch.tensor(g[:, 1:].copy())
        opt.step()
        mag = 0.9 * np.abs(m.astype(f64)) + 0.1 * np.abs(g.astype(f64))
        pf, mf, vf = R.adam_ref32(p, m, v, g, t, lr, eps=1e-15, lr_rest=lr / 20, period=48, split=3)
        p, m, v = pf.reshape(p.shape), mf.reshape(p.shape), vf.reshape(p.shape)
        st = rate * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        allow += 16 * R.U * t * st * mag / (np.sqrt(v.astype(f64)) + 1e-15)
        want = np.concatenate([q_dc.detach().numpy(), q_rest.detach().numpy()], axis=1)
        pmax = np.maximum(pmax, np.abs(want))
        d = np.abs(p.astype(f64) - want)
        bound = 2 * R.ulp32(pmax) + allow
        worst = max(worst, float((d / bound).max()))
        assert (d <= bound).all(), (t, float((d / bound).max()))
    assert float(np.median(allow / R.ulp32(pmax))) < 0.25       # for the typical parameter the allowance is a detail beside its 2 ulp
    print("adam_ref32 vs torch float32 Adam: worst error / bound %.2f over %d steps" % (worst, steps))


@pytest.mark.parametrize("t", [1, 2, 7, 1000, 30000])
@pytest.mark.parametrize("eps", [1e-15, 1e-8])
def test_adam_ref32_equals_the_float64_rule(t, eps):
    """moments: 3 (m) and 4 (v) roundings of the magnitudes added - c1 g, the fma, and the float32 of 1 - beta (v: one more product);
    parameter: the GPU tests' bound, 2e-6 |step| + 1.3e-7 |p| + 1e-12, for the float64 rule applied to adam_ref32's own moments"""
    p, m, v, g = adam_state(5000, seed=t, t=t)
    kw = dict(lr=0.0025, eps=eps, lr_rest=0.0025 / 20, period=48, split=3)
    p1, m1, v1 = R.adam_ref32(p, m, v, g, t, **kw)
    _, m64, v64, _ = R.adam_ref64(p, m, v, g, t, **kw)
    m_, v_, g_ = m.astype(f64), v.astype(f64), g.astype(f64)
    assert (np.abs(m1 - m64) <= 3 * R.U * (0.9 * np.abs(m_) + 0.1 * np.abs(g_)) + R.TINY32).all()
    assert (np.abs(v1 - v64) <= 4 * R.U * (0.999 * v_ + 0.001 * g_ * g_) + R.TINY32).all()
    want, step = R.adam_param_from_moments(p, m1, v1, t, **kw)
    err = np.abs(p1.astype(f64) - want)
    assert (err <= 2e-6 * np.abs(step) + 1.3e-7 * np.abs(p.astype(f64)) + 1e-12).all(), float(err.max())
    assert np.abs(step).max() > 0


def adam_state(n, seed, t):
    """non-trivial state: gradients over the decades 1e-20 .. 1e3, m != 0 and v > 0 consistent with gradients of that size"""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-20, 3, n)
    g = (mag * rng.standard_normal(n)).astype(np.float32)
    m = (mag * rng.standard_normal(n) * 0.5).astype(np.float32)
    v = ((mag * rng.uniform(0.3, 2.0, n)) ** 2).astype(np.float32)
    p = rng.standard_normal(n).astype(np.float32)
    return p, m, v, g


def test_adam_ref32_active_and_rates():
    n, period = 48 * 7, 48
    p, m, v, g = adam_state(n, 1, 3)
    for active in (1, 3, 4, 5, 27, 47):
        ga = 4 * ((active + 3) // 4)
        p1, m1, v1 = R.adam_ref32(p, m, v, g, 3, 0.01, lr_rest=0.0005, period=period, split=3, active=active)
        dead = (np.arange(n) % period) >= ga
        assert np.array_equal(p1[dead], p[dead]) and np.array_equal(m1[dead], m[dead]) and np.array_equal(v1[dead], v[dead])
        pf, mf, vf = R.adam_ref32(p, m, v, g, 3, 0.01, lr_rest=0.0005, period=period, split=3)
        assert np.array_equal(p1[~dead], pf[~dead]) and np.array_equal(m1[~dead], mf[~dead])
    full = R.adam_ref32(p, m, v, g, 3, 0.01, lr_rest=0.0005, period=period, split=3, active=48)
    assert np.array_equal(full[0], pf)                                                  # active >= period: everything


# ------------------------------------------------------------------------------------------------------------ the tolerances are attainable
@pytest.mark.parametrize("N", [1, 257, 65537])
def test_float32_torch_composition_of_mesh_activate_stays_inside_the_gpu_bounds(N):
    ins, labels = R.mesh_edge_inputs(N, seed=N, shift=N)
    ups = R.upstream(N, N)
    leaves, out = _torch_mesh(ins, torch.float32, R.MR_WEIGHT)
    fw = R.mesh_activate_ref(**ins, mr_weight=R.MR_WEIGHT)
    got = {k: o.detach().numpy() for k, o in zip(("xyz", "scales", "rots", "opac"), out)}
    got["mr"] = float(out[4].detach())
    msg = R.check_mesh_forward(got, fw, labels, N)
    assert not msg, msg
    hinge = np.array(["hinge" in l for l in labels])
    exempt = (fw["margin"] < 2.0 ** -18) & ~hinge
    assert exempt.sum() <= max(1, N // 1000)
    g = _grads(leaves, out, ups, 2.5)
    msg = R.check_mesh_backward(g, ins, ups, labels, mr_weight=R.MR_WEIGHT, g_mr=2.5, hinge_exempt=exempt)
    assert not msg, msg


def test_float32_torch_composition_of_plain_activate_stays_inside_the_bounds():
    N = 20000
    ins, labels = R.mesh_edge_inputs(N, seed=2)
    ups = R.upstream(N, 2)
    t = [torch.tensor(a, requires_grad=True) for a in (ins["v1"], ins["scaling"], ins["rot"], ins["opac"])]
    out = (t[0] * 1.0, torch.exp(t[1]), torch.nn.functional.normalize(t[2]), torch.sigmoid(t[3]))
    ref_out, ref_scale, ref_exp = R.plain_activate_ref(ins["v1"], ins["scaling"], ins["rot"], ins["opac"])
    K = dict(xyz=0, scales=R.K_FWD["scales"], rots=R.K_FWD["rots"], opac=R.K_FWD["opac"])
    for k, o in zip(("xyz", "scales", "rots", "opac"), out):
        bound = np.minimum(K[k] * R.U * ref_scale[k] + 2.0 ** -23 * ref_exp[k], R.FWD_FIGURE * np.maximum(1.0, np.abs(ref_out[k]))) + R.TINY32
        msg = R.report(k, o.detach().numpy(), ref_out[k], bound if K[k] else 0.0 * bound, labels, ref_scale[k], cols=o.shape[1])
        assert not msg, msg
    gs = torch.autograd.grad(sum((o * torch.tensor(u)).sum() for o, u in zip(out, ups)), t)
    grad, scale = R.plain_activate_adjoint(ins["v1"], ins["scaling"], ins["rot"], ins["opac"], *ups)
    x = ins["opac"].astype(f64)
    for k, g in zip(("xyz", "scaling", "rot", "opac"), gs):
        want, bound = grad[k], R.BWD_FIGURE * scale[k] + R.TINY32
        if k == "opac":
            hi, band = x >= R.BAND[1], (x > R.BAND[0]) & (x < R.BAND[1])
            want = np.where(hi | band, 0.0, want)
            bound = np.where(hi, 0.0, np.where(band, R.BAND_FIGURE * np.abs(ups[3].astype(f64)), bound))
        msg = R.report("d_" + k, g.numpy(), want, bound, labels, scale[k], cols=g.shape[1])
        assert not msg, msg


def test_densify_reference_statements():
    radii = np.array([0, -3, 1, 5, 2 ** 24 + 1, 2 ** 30 + 65], np.int32)
    grad = np.array([[1, 1, 9], [1, 1, 9], [3, 4, 9], [1e-20, 0, 9], [1e15, 1e15, 9], [3e19, 4e19, 9]], np.float32)
    mr = np.array([7, 7, 0.5, 9, 1, 1], np.float32); acc = np.ones(6, np.float32); den = np.arange(6, dtype=np.float32)
    d = R.densify_stats_ref(radii, grad, mr, acc, den)
    assert list(d["vis"]) == [False, False, True, True, True, True]
    assert list(d["max_radii2D"]) == [7, 7, 1, 9, 2.0 ** 24, float(np.float32(2 ** 30 + 65))] and list(d["denom"]) == [0, 1, 3, 4, 5, 6]
    assert d["accum64"][2] == 6.0 and d["accum32"][2] == 6.0 and d["accum64"][0] == 1.0
    assert list(d["safe"]) == [True, True, True, False, True, False]
    assert d["accum32"][3] == 1.0 and np.isinf(d["accum32"][5]) and abs(d["accum64"][5] - 5e19) < 1e13
