"""GPU parity of the fused training-loop operators (csrc/gm_train.hip) against the plain torch composition of the
reference's formulas (scene/mesh_based_gaussian_model.py:122-152, 172-174) and against torch.optim.Adam."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_ops_ref as R

pytestmark = pytest.mark.gpu


def _inputs(N, seed):
    rng = np.random.default_rng(seed)
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float32), device="cuda", requires_grad=g)
    n = rng.standard_normal((N, 3)); n /= np.linalg.norm(n, axis=1, keepdims=True)
    return dict(bc=t(rng.standard_normal((N, 3)) * 2, True), dist=t(rng.standard_normal((N, 1)), True),
                scaling=t(rng.standard_normal((N, 3)) - 2, True), rot=t(rng.standard_normal((N, 4)), True),
                opac=t(rng.standard_normal((N, 1)) * 2, True), v1=t(rng.standard_normal((N, 3))), v2=t(rng.standard_normal((N, 3))),
                v3=t(rng.standard_normal((N, 3))), n=t(n), r=t(rng.random((N, 1)) + 0.1))


def _torch_ref(d):
    w = torch.softmax(d["bc"].double(), dim=1)
    xyz = w[:, 0:1] * d["v1"].double() + w[:, 1:2] * d["v2"].double() + w[:, 2:3] * d["v3"].double()
    xyz = xyz + 4 * d["r"].double() * (torch.sigmoid(d["dist"].double()) - 0.5) * d["n"].double()
    return xyz, torch.exp(d["scaling"].double()), torch.nn.functional.normalize(d["rot"].double()), torch.sigmoid(d["opac"].double())


@pytest.mark.parametrize("N", [1, 257, 10000])
def test_mesh_activate_forward_and_backward(N):
    from gaussianmesh_amd.model_ops import mesh_activate
    d = _inputs(N, N)
    out = mesh_activate(d["bc"], d["dist"], d["scaling"], d["rot"], d["opac"], d["v1"], d["v2"], d["v3"], d["n"], d["r"], 4.0)
    ref = _torch_ref(d)
    for o, r_ in zip(out, ref):
        assert o.shape == r_.shape and float((o.double() - r_).abs().max()) <= 2e-6 * max(1.0, float(r_.abs().max()))
    ws = [torch.randn_like(o) for o in out]
    leaves = [d[k] for k in ("bc", "dist", "scaling", "rot", "opac")]
    g = torch.autograd.grad(sum((o * w).sum() for o, w in zip(out, ws)), leaves, retain_graph=True)
    gr = torch.autograd.grad(sum((r_ * w.double()).sum() for r_, w in zip(ref, ws)), leaves)
    for a, b, k in zip(g, gr, ("bc", "dist", "scaling", "rot", "opac")):
        assert float((a.double() - b).abs().max()) <= 1e-5 * max(1e-6, float(b.abs().max())), k
    # a missing upstream gradient is a zero gradient
    g2 = torch.autograd.grad((out[0] * ws[0]).sum(), leaves, allow_unused=True)
    assert float(g2[2].abs().max()) == 0.0 and float(g2[0].abs().max()) > 0


def test_mesh_restrict_term_fused_into_the_activation():
    """5th output of mesh_activate == loss.mesh_restrict_loss on the activated scales (value and gradient)."""
    from gaussianmesh_amd.model_ops import mesh_activate
    from gaussianmesh_amd.loss import mesh_restrict_loss
    d = _inputs(5000, 7)
    with torch.no_grad():
        d["scaling"] += 2.0                                            # make a good share of the terms positive
    args = (d["bc"], d["dist"], d["scaling"], d["rot"], d["opac"], d["v1"], d["v2"], d["v3"], d["n"], d["r"], 4.0)
    xyz, sc, rt, op, mr = mesh_activate(*args, mr_weight=0.7)
    ref = mesh_restrict_loss(torch.exp(d["scaling"].double()), d["v1"].double(), d["v2"].double(), d["v3"].double(), weight=0.7)
    assert float(ref) > 0 and abs(float(mr) - float(ref)) <= 1e-5 * float(ref)
    w = torch.randn_like(sc)
    g, = torch.autograd.grad(2.5 * mr + (sc * w).sum(), [d["scaling"]])
    gr, = torch.autograd.grad(2.5 * ref + (torch.exp(d["scaling"].double()) * w.double()).sum(), [d["scaling"]])
    assert float((g.double() - gr).abs().max()) <= 1e-5 * float(gr.abs().max())
    assert len(mesh_activate(*args)) == 4


def test_fused_adam_matches_torch_adam_and_two_rate_tensor():
    from gaussianmesh_amd.model_ops import FusedAdam
    rng = np.random.default_rng(0)
    shapes = [(1000, 3), (1000, 1), (1000, 16, 3), (37,), (5, 4)]
    ps = [torch.tensor(rng.standard_normal(s).astype(np.float32), device="cuda", requires_grad=True) for s in shapes]
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    q_dc = qs[2].detach()[:, :1].clone().requires_grad_(True); q_rest = qs[2].detach()[:, 1:].clone().requires_grad_(True)
    lrs = [0.01, 0.02, 0.005, 0.1, 0.03]
    groups = [{"params": [p], "lr": lr, "name": str(i)} for i, (p, lr) in enumerate(zip(ps, lrs))]
    groups[2].update(lr_rest=0.005 / 20, period=48, split=3)
    opt = FusedAdam(groups, eps=1e-15)
    ref = torch.optim.Adam([{"params": [qs[0]], "lr": lrs[0]}, {"params": [qs[1]], "lr": lrs[1]}, {"params": [q_dc], "lr": lrs[2]},
                            {"params": [q_rest], "lr": lrs[2] / 20}, {"params": [qs[3]], "lr": lrs[3]}, {"params": [qs[4]], "lr": lrs[4]}],
                           lr=0.0, eps=1e-15)
    for it in range(6):
        for p in ps:
            p.grad = torch.tensor(rng.standard_normal(tuple(p.shape)).astype(np.float32), device="cuda")
        qs[0].grad, qs[1].grad, qs[3].grad, qs[4].grad = ps[0].grad.clone(), ps[1].grad.clone(), ps[3].grad.clone(), ps[4].grad.clone()
        q_dc.grad, q_rest.grad = ps[2].grad[:, :1].clone(), ps[2].grad[:, 1:].clone()
        opt.step(); ref.step()
    chk = lambda a, b: float((a.detach() - b.detach()).abs().max()) <= 2e-6
    assert chk(ps[0], qs[0]) and chk(ps[1], qs[1]) and chk(ps[3], qs[3]) and chk(ps[4], qs[4])
    assert chk(ps[2][:, :1], q_dc) and chk(ps[2][:, 1:], q_rest)
    opt.zero_grad()
    assert all(p.grad is None for p in ps)
    ps[0].grad = None
    opt.step()                                             # nothing to do: no gradients


@pytest.mark.parametrize("deg", [0, 1, 2])
def test_fused_adam_active_coefficients_only(deg):
    """gm_adam_step_active: while only the coefficients of SH degrees <= deg have ever had a gradient, an optimizer that skips the
    rest gives, bit for bit, what the full update gives on zero gradients - parameters, both moments - also across the step at
    which the degree goes up."""
    from gaussianmesh_amd.model_ops import FusedAdam
    g = torch.Generator(device="cuda").manual_seed(deg)
    N = 1537
    p0 = torch.randn((N, 16, 3), device="cuda", generator=g)
    other0 = torch.randn((N, 3), device="cuda", generator=g)

    def make():
        p, o = p0.clone().requires_grad_(True), other0.clone().requires_grad_(True)
        return p, o, FusedAdam([{"params": [p], "lr": 0.0025, "lr_rest": 0.0025 / 20, "period": 48, "split": 3, "name": "f"},
                                {"params": [o], "lr": 0.01, "name": "o"}], eps=1e-15)
    pa, oa, full = make()
    pb, ob, lim = make()
    for it in range(7):
        d = deg if it < 4 else deg + 1                                   # the degree goes up before the fifth step
        nc = (d + 1) ** 2
        grad = torch.zeros((N, 16, 3), device="cuda")
        grad[:, :nc] = torch.randn((N, nc, 3), device="cuda", generator=g)
        go = torch.randn((N, 3), device="cuda", generator=g)
        pa.grad, oa.grad, pb.grad, ob.grad = grad.clone(), go.clone(), grad.clone(), go.clone()
        lim.param_groups[0]["active"] = 3 * nc if d < 3 else 0
        full.step(); lim.step()
        assert torch.equal(pa, pb) and torch.equal(oa, ob), it
        for k in ("m", "values"):
            assert torch.equal(full.param_groups[0][k][0], lim.param_groups[0][k][0]), (it, k)
    assert torch.equal(pa.detach()[:, (deg + 2) ** 2:], p0[:, (deg + 2) ** 2:]) or deg == 2       # never-active coefficients never moved
    assert not torch.equal(pa.detach()[:, :1], p0[:, :1])


# =====================================================================================================================================
# Every element against float64 (tests/train_ops_ref.py), at the edges.  The tolerances multiply a PER-ELEMENT scale - the sum of the
# magnitudes of the terms added to form the element - so that one wrong row among 65537 fails and a small value is not hidden behind the
# tensor's largest; their constants and derivations are in train_ops_ref (K_FWD, k_mr, check_mesh_forward, check_mesh_backward), which
# tests/test_train_ops_ref_host.py validates on the host and shows to be attainable by a float32 evaluation on these very inputs.
# =====================================================================================================================================
SIZES = [1, 63, 64, 255, 256, 257, 1000, 65537]       # straddle the wave (64), the workgroup (256) and the mr_partial boundaries
_LEAVES = ("bc", "dist", "scaling", "rot", "opac")
_ORDER = ("bc", "dist", "scaling", "rot", "opac", "v1", "v2", "v3", "normal", "r")


def _cu(a, grad=False):
    return torch.tensor(np.ascontiguousarray(a), device="cuda", requires_grad=grad)


def _mesh_run(ins, ups, mr_weight=None, g_mr=None, joint=None):
    """mesh_activate through autograd: (forward dict of numpy, gradient dict of numpy)"""
    from gaussianmesh_amd.model_ops import mesh_activate
    d = {k: _cu(v, k in _LEAVES) for k, v in ins.items()}
    out = mesh_activate(*[d[k] for k in _ORDER], 4.0, mr_weight=mr_weight, joint=joint)
    N = ins["bc"].shape[0]
    fw = {k: o.detach()[:N].cpu().numpy() for k, o in zip(("xyz", "scales", "rots", "opac"), out)}
    if mr_weight is not None:
        fw["mr"] = float(out[4].detach())
    outs = [o for o, u in zip(out[:4], ups) if u is not None]
    gos = [_cu(u) for u in ups if u is not None]
    if g_mr is not None:
        outs.append(out[4]); gos.append(torch.tensor(float(g_mr), device="cuda"))
    g = torch.autograd.grad(outs, [d[k] for k in _LEAVES], gos, allow_unused=True)
    return fw, {k: (np.zeros(ins[k].shape, np.float32) if t is None else t.cpu().numpy()) for k, t in zip(_LEAVES, g)}, out


def _hinge_exempt(fw64, labels, N):
    """rows whose mesh-restrict term lies within 2^-18 of the hinge (relative to smax + w R) WITHOUT having been built there - the kernel's
    float32 term may take either sign; at most one row in a thousand, so the exemption cannot hide a wrong kernel"""
    hinge = np.array(["hinge" in l for l in labels])
    exempt = (fw64["margin"] < 2.0 ** -18) & ~hinge
    assert exempt.sum() <= max(1, N // 1000)
    return exempt


@pytest.mark.parametrize("N", SIZES)
def test_mesh_activate_every_element_against_float64(N):
    """forward (with the fused mesh-restrict value) and backward of mesh_activate on the named classes of train_ops_ref.mesh_edge_inputs:
    saturated and tied softmax, distance and opacity through +-100 and the 16.6 .. 16.7 band, scaling over [-12, 4] with tied axes,
    quaternions from norm 1e3 down to the clamp and zero, degenerate faces, hinge rows 8 ulp either side, r = 0.
    Measured on the MI355X, worst error / bound over all N: scales 0.62, rots 0.64, opac 0.57, xyz 0.56, mr 0.07 (printed with -s)."""
    ins, labels = R.mesh_edge_inputs(N, seed=N, shift=N)
    ups = R.upstream(N, N)
    fw64 = R.mesh_activate_ref(**ins, mr_weight=R.MR_WEIGHT)
    got, grads, _ = _mesh_run(ins, ups, R.MR_WEIGHT, 2.5)
    b = R.forward_bounds(fw64, N)
    for k in R.K_FWD:
        print("N=%d forward %-6s worst err/bound %.3f" % (N, k, float((np.abs(got[k] - fw64["out"][k]) / b[k]).max())))
    print("N=%d forward mr     err/bound %.3f (got %.9g want %.9g)" % (N, abs(got["mr"] - fw64["out"]["mr"]) / b["mr"], got["mr"], fw64["out"]["mr"]))
    msg = R.check_mesh_forward(got, fw64, labels, N)
    assert not msg, msg
    msg = R.check_mesh_backward(grads, ins, ups, labels, mr_weight=R.MR_WEIGHT, g_mr=2.5, hinge_exempt=_hinge_exempt(fw64, labels, N))
    assert not msg, msg
    # without the mesh-restrict output the four tensors are the same bits (mr_partial == null is the other branch of the kernel)
    plain, grads2, _ = _mesh_run(ins, ups)
    for k in R.K_FWD:
        assert np.array_equal(plain[k].view(np.int32), got[k].view(np.int32)), k
    msg = R.check_mesh_backward(grads2, ins, ups, labels)
    assert not msg, msg
    if N >= 1000:                                                 # the classes the exact statements are about are in the set
        for k in ("dist", "opac"):
            assert (ins[k] >= R.BAND[1]).sum() > 5 and ((ins[k] > R.BAND[0]) & (ins[k] < R.BAND[1])).sum() > 5, k


def test_mesh_activate_clamp_active_quaternion_gradient():
    """0 < |q| <= 1e-12: jt.normalize is x / maximum(|x|, eps), whose gradient there is g / eps (the maximum passes nothing to |x|) - the
    projection (g - y (y.g)) / eps that holds above the clamp gives (1.27, 2, 2.64, 4) 1e12 for q = (3e-13, 0, -4e-13, 0), g = (1, 2, 3, 4)
    where autograd gives (1, 2, 3, 4) 1e12.  plain_activate_bwd_kernel has the branch; mesh_activate_bwd_kernel had not."""
    N = 300
    ins, labels = R.mesh_edge_inputs(N, seed=9)
    ins["rot"][0] = (3e-13, 0, -4e-13, 0)
    ins["rot"][1] = 0.0
    ups = R.upstream(N, 9)
    ups[2][0] = (1, 2, 3, 4); ups[2][1] = (1, 2, 3, 4)
    _, grads, _ = _mesh_run(ins, ups)
    want = np.array([1, 2, 3, 4], np.float64) * 1e12
    assert np.abs(grads["rot"][0] - want).max() <= 1e-5 * want.min(), grads["rot"][0]
    assert np.abs(grads["rot"][1] - want).max() <= 1e-5 * want.min(), grads["rot"][1]           # the zero quaternion: g 1e12
    msg = R.check_mesh_backward(grads, ins, ups, labels)
    assert not msg, msg


def test_mesh_activate_nan_rotation_component_makes_its_row_nan():
    """one NaN component: |q| is NaN, and torch's F.normalize (clamp_min keeps a NaN) makes the whole row NaN, forward and backward - what
    Jittor's maximum(|x|, eps) returns for a NaN was not checked.  fmaxf(|q|, eps) returned eps instead: three finite rots of ~1e12 beside the NaN and a finite gradient g / eps - found on plain_activate by
    test_gpu_plain_activate.py::test_the_rows_kept_out_of_the_gate.  No other row and no other tensor of the row is touched."""
    N = 300
    ins, labels = R.mesh_edge_inputs(N, seed=9)
    clean, clean_grads, _ = _mesh_run(ins, R.upstream(N, 9))
    ins["rot"][5, 2] = np.nan
    ins["rot"][256, 0] = np.nan
    got, grads, _ = _mesh_run(ins, R.upstream(N, 9))
    rows = np.zeros(N, bool)
    rows[[5, 256]] = True
    assert np.isnan(got["rots"][rows]).all() and np.isnan(grads["rot"][rows]).all()
    for k in got:
        keep = slice(None) if k != "rots" else ~rows
        assert np.array_equal(got[k][keep].view(np.int32), clean[k][keep].view(np.int32)), k
    for k in grads:
        keep = slice(None) if k != "rot" else ~rows
        assert np.array_equal(grads[k][keep].view(np.int32), clean_grads[k][keep].view(np.int32)), k


def _abi_bwd(ins, ups, mr_weight=None, g_mr=None):
    """gm_mesh_activate_bwd at the C ABI: a missing upstream gradient is a NULL pointer (autograd materialises zeros instead, so the
    kernel's null branches are only reached from here).  The outputs start as NaN."""
    from gaussianmesh_amd import _lib
    N = ins["bc"].shape[0]
    d = [_cu(ins[k]) for k in _ORDER]
    g = [None if u is None else _cu(u) for u in ups]
    gm = None if g_mr is None else torch.tensor([float(g_mr)], device="cuda")
    outs = [torch.full((N, k), float("nan"), device="cuda") for k in (3, 1, 3, 4, 1)]
    _lib.check(_lib.lib().gm_mesh_activate_bwd(N, 4.0, *[t.data_ptr() for t in d], *[None if t is None else t.data_ptr() for t in g],
                                               *[t.data_ptr() for t in outs], float(mr_weight or 0.0), None if gm is None else gm.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in zip(_LEAVES, outs)}


@pytest.mark.parametrize("which", range(16))
@pytest.mark.parametrize("mr", [False, True])
def test_mesh_activate_backward_missing_upstream_gradients(which, mr):
    """every subset of the four upstream gradients as NULL pointers, with and without the gradient of the mesh-restrict output: exact zeros
    where nothing arrives, the float64 adjoint elsewhere; with nothing but d_mr, the whole of it lands on the FIRST largest axis of a row
    with a positive term and nowhere else"""
    N = 1000
    ins, labels = R.mesh_edge_inputs(N, seed=40, shift=7)
    ups = R.upstream(N, 40, [bool(which >> b & 1) for b in range(4)])
    wt, g_mr = (R.MR_WEIGHT, -1.75) if mr else (None, None)
    got = _abi_bwd(ins, ups, wt, g_mr)
    fw64 = R.mesh_activate_ref(**ins, mr_weight=R.MR_WEIGHT)
    exempt = _hinge_exempt(fw64, labels, N)
    msg = R.check_mesh_backward(got, ins, ups, labels, mr_weight=wt, g_mr=g_mr, hinge_exempt=exempt)
    assert not msg, msg
    if mr and ups[1] is None:
        on = np.zeros((N, 3), bool); on[np.arange(N), fw64["axis"]] = fw64["term"] > 0
        tied = np.array(["same-bits" in l for l in labels]) & (fw64["term"] > 0)
        assert tied.sum() > 50 and (got["scaling"][on & ~exempt[:, None]] != 0).all()
        off = got["scaling"][~on & ~exempt[:, None]]
        assert not off.any(), "d_mr leaked to %d elements off the first largest axis" % int((off != 0).sum())


# ---------------------------------------------------------------------------------------------------------------- the joint= route
def test_mesh_activate_joint_route():
    """joint= (so far reached only through the renderer): the leading N rows are the plain route's bits, the Nb tail rows keep a sentinel
    bit for bit, the gradient of the tail rows is dropped, and the backward of an EARLIER forward after a second forward raises autograd's
    in-place-modification error, as the contract comment in model_ops.py promises."""
    from gaussianmesh_amd.model_ops import mesh_activate
    N, Nb = 1000, 37
    ins, labels = R.mesh_edge_inputs(N, seed=21, shift=2)
    ups = R.upstream(N, 21)
    plain, gplain, _ = _mesh_run(ins, ups, R.MR_WEIGHT, 2.5)
    f = dict(dtype=torch.float32, device="cuda")
    sent = -123.456
    jb = {k: torch.full((N + Nb, c), sent, **f) for k, c in (("xyz", 3), ("scales", 3), ("rots", 4), ("opac", 1))}
    d = {k: _cu(v, k in _LEAVES) for k, v in ins.items()}
    out = mesh_activate(*[d[k] for k in _ORDER], 4.0, mr_weight=R.MR_WEIGHT, joint=jb)
    for k, o in zip(("xyz", "scales", "rots", "opac"), out):
        assert o.shape[0] == N + Nb and o.data_ptr() == jb[k].data_ptr()
        assert np.array_equal(o.detach()[:N].cpu().numpy().view(np.int32), plain[k].view(np.int32)), k
        assert torch.equal(o.detach()[N:], torch.full_like(o.detach()[N:], sent)), k
    assert float(out[4].detach()) == plain["mr"]
    big = [torch.cat([_cu(u), torch.randn((Nb, u.shape[1]), device="cuda") * 100]) for u in ups]      # tail gradients: dropped
    g = torch.autograd.grad(list(out), [d[k] for k in _LEAVES], big + [torch.tensor(2.5, device="cuda")])
    for k, t in zip(_LEAVES, g):
        assert np.array_equal(t.cpu().numpy().view(np.int32), gplain[k].view(np.int32)), k
    # one forward per backward: an op downstream saved the outputs of forward 1; forward 2 rewrites the buffers under it
    d1 = {k: _cu(v, k in _LEAVES) for k, v in ins.items()}
    o1 = mesh_activate(*[d1[k] for k in _ORDER], 4.0, joint=jb)
    loss1 = sum((o * o).sum() for o in o1)
    d2 = {k: _cu(v, k in _LEAVES) for k, v in ins.items()}
    o2 = mesh_activate(*[d2[k] for k in _ORDER], 4.0, joint=jb)
    with pytest.raises(RuntimeError, match="modified (by an )?inplace"):      # autograd's in-place-modification error
        loss1.backward()
    sum((o * o).sum() for o in o2).backward()                     # the latest forward's backward is fine
    assert all(torch.isfinite(d2[k].grad).all() for k in ("scaling", "rot"))


# =====================================================================================================================================
# FusedAdam / gm_adam_step_active, every element
# =====================================================================================================================================
_PAD = 32                                  # guard elements on either side of a tensor: 128 bytes, so the slice stays 16-byte aligned
_SENT = 0x7FC0BEEF                         # a NaN with a payload: a stray float write or a stray read-modify-write changes its bits


class _Guarded:
    """a float32 tensor that is a 16-byte-aligned slice of a larger buffer filled with a sentinel pattern"""

    def __init__(self, values, offset=0):
        values = np.ascontiguousarray(values, np.float32).reshape(-1)
        self.n = values.size
        self.lo = _PAD + offset
        self.buf = torch.full((self.n + 2 * _PAD + 4,), _SENT, dtype=torch.int32, device="cuda")
        self.buf += torch.arange(self.buf.numel(), dtype=torch.int32, device="cuda") % 7
        self.t = self.buf.view(torch.float32)[self.lo:self.lo + self.n]
        self.t.copy_(torch.from_numpy(values))
        self.before = self.buf.clone()

    def bits(self):
        return self.buf[self.lo:self.lo + self.n].cpu().numpy()

    def value(self):
        return self.t.cpu().numpy()

    def guards_unchanged(self):
        return torch.equal(self.buf[:self.lo], self.before[:self.lo]) and torch.equal(self.buf[self.lo + self.n:], self.before[self.lo + self.n:])

    def unchanged(self):
        return torch.equal(self.buf, self.before)


def _adam_data(n, seed, kind="normal"):
    """(p, m, v, g) float32 with a non-trivial state, m != 0 and v > 0.  'range': gradients over the decades 1e-20 .. 1e3 and moments
    consistent with them;  'aligned': m and g of one sign per element and small parameters, so that every step is far above an ulp of
    its parameter (the rate-recovery check needs that)"""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-20, 3, n) if kind == "range" else np.ones(n)
    sgn = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    if kind == "aligned":
        g, m = sgn * rng.uniform(0.2, 2.0, n), sgn * rng.uniform(0.2, 2.0, n)
        p = 0.01 * rng.standard_normal(n)
    else:
        g, m = mag * rng.standard_normal(n), mag * 0.5 * rng.standard_normal(n)
        p = rng.standard_normal(n)
    v = (mag * rng.uniform(0.3, 2.0, n)) ** 2
    f = lambda a: a.astype(np.float32)
    m = f(m); m[m == 0] = np.float32(1e-30)
    return f(p), m, f(v), f(g)


def _fused_step(tensors, t, eps, betas=(0.9, 0.999)):
    """one FusedAdam.step() at step count t over `tensors`: dicts with Guarded p, m, v, g (g None: no gradient) and lr, optional lr_rest,
    period, split, active.  Parameters, moments and gradients are the guarded slices themselves."""
    from gaussianmesh_amd.model_ops import FusedAdam
    groups = []
    for i, d in enumerate(tensors):
        grp = {"params": [d["p"].t], "lr": d["lr"], "name": "t%d" % i}
        grp.update({k: d[k] for k in ("lr_rest", "period", "split", "active") if k in d})
        groups.append(grp)
    opt = FusedAdam(groups, eps=eps, betas=betas)
    for grp, d in zip(opt.param_groups, tensors):
        grp["m"][0], grp["values"][0] = d["m"].t, d["v"].t
        grp["params"][0].grad = None if d.get("g") is None else d["g"].t
    opt.n_step = t - 1
    opt.step()
    torch.cuda.synchronize()
    return opt


def _adam_gates(d, host, t, eps, what="", rate_check=False):
    """The gates of one tensor after one step.  host = (p, m, v, g) before the step.
      m', v' against adam_ref32: within 1 ulp, plus float32's smallest normal (values that are subnormal in float32);
      p' against the float64 rule applied to the float64 value of the moments the device wrote: |err| <= 2e-6 |step| + 1.3e-7 |p| + 1e-12
         (tests/test_gpu_sh_step.py's bound for the same rule);
      untouched elements (at or past the granule 4 ceil(active / 4) of their period) keep their bits in p, m, v;
      the gradient buffer and the guard elements around p, m, v are unchanged."""
    p0, m0, v0, g = host
    kw = dict(lr=d["lr"], eps=eps, lr_rest=d.get("lr_rest"), period=d.get("period", 0), split=d.get("split", 0))
    active = d.get("active", 0)
    n = p0.size
    live = R._live(n, kw["period"], active)
    p1, m1, v1 = d["p"].value(), d["m"].value(), d["v"].value()
    _, mr, vr = R.adam_ref32(p0, m0, v0, g, t, active=active, **kw)
    lab = None
    for name, got, ref in (("m'", m1, mr), ("v'", v1, vr)):
        msg = R.report("%s %s vs adam_ref32" % (what, name), got[live], ref[live], R.ulp32(ref[live]) + R.TINY32, lab)
        assert not msg, msg
    want, step = R.adam_param_from_moments(p0, m1, v1, t, **kw)
    bound = 2e-6 * np.abs(step) + 1.3e-7 * np.abs(p0.astype(np.float64)) + 1e-12
    msg = R.report("%s p'" % what, p1[live], want[live], bound[live], lab, np.abs(step[live]))
    assert not msg, msg
    for name, x, x0 in (("p", d["p"], p0), ("m", d["m"], m0), ("v", d["v"], v0)):
        assert np.array_equal(x.bits()[~live], x0.view(np.int32)[~live]), "%s %s: an untouched element changed" % (what, name)
        assert x.guards_unchanged(), "%s %s: bytes outside the tensor changed" % (what, name)
    assert d["g"].unchanged(), "%s: the gradient buffer changed" % what
    if rate_check:
        # which rate did every element receive?  rate = dp (sqrt(v') + eps) / m' / corr; lr and lr_rest are a factor of 20 apart
        corr = np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        dp = p0.astype(np.float64) - p1.astype(np.float64)
        rate = dp * (np.sqrt(v1.astype(np.float64)) + eps) / m1.astype(np.float64) / corr
        expect, _ = R._rates(n, kw["lr"], kw["lr_rest"], kw["period"], kw["split"])
        lo, hi = min(kw["lr"], kw["lr_rest"]), max(kw["lr"], kw["lr_rest"])
        assert (np.abs(dp[live]) >= 64 * R.ulp32(p0[live])).all()                  # every step is far above its parameter's rounding
        took = np.where(rate > np.sqrt(lo * hi), hi, lo)
        bad = np.flatnonzero(live & (took != expect))
        assert bad.size == 0, "%s: %d elements took the other rate, first at index %d (in-period %d): rate %.4g, expected %.4g" % (
            what, bad.size, bad[0], bad[0] % max(kw["period"], 1), rate[bad[0]], expect[bad[0]])
        assert (np.abs(rate[live] / expect[live] - 1) < 0.02).all()


def _one(n, seed, kind, offset=0, nan_dead=None, **cfg):
    p, m, v, g = _adam_data(n, seed, kind)
    if nan_dead is not None:                                      # the region the step must not touch holds NaN in p, m, v and g
        for a in (p, m, v, g):
            a[nan_dead] = np.nan
    d = dict(p=_Guarded(p, offset), m=_Guarded(m), v=_Guarded(v, offset), g=_Guarded(g), **cfg)
    return d, (p, m, v, g)


@pytest.mark.parametrize("t", [1, 2, 7, 1000, 30000])
@pytest.mark.parametrize("eps", [1e-15, 1e-8])
def test_fused_adam_every_element_all_shapes(t, eps):
    """period = 0, n across the float4 body / scalar tail split and the workgroup boundary; both ends of a 30,000-iteration schedule's
    bias correction"""
    for n in (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 262145):
        for kind in ("normal", "range"):
            d, host = _one(n, 1000 * t + n, kind, offset=4 * (n % 3), lr=0.0025)
            _fused_step([d], t, eps)
            _adam_gates(d, host, t, eps, "n=%d %s t=%d" % (n, kind, t))


def test_fused_adam_eight_tensors_of_very_different_sizes():
    """one call: the grid is sized by the largest tensor, the small tensors' scalar tails run in workgroup 0 while the other workgroups
    idle; groups without a gradient stay untouched bit for bit while n_step advances for all (the step count is global, as Jittor's)"""
    sizes = [262145 * 3, 1, 5, 48 * 300, 1023, 7, 4096, 3]
    eps, t = 1e-15, 7
    ds, hosts = [], []
    for i, n in enumerate(sizes):
        cfg = dict(lr=0.001 * (i + 1))
        if i == 3:
            cfg.update(lr_rest=0.004 / 20, period=48, split=3)
        d, h = _one(n, 70 + i, "normal", **cfg)
        ds.append(d); hosts.append(h)
    skipped = (2, 6)
    gs = {i: ds[i]["g"] for i in skipped}
    for i in skipped:
        ds[i]["g"] = None
    opt = _fused_step(ds, t, eps)
    assert opt.n_step == t
    for i, (d, h) in enumerate(zip(ds, hosts)):
        if i in skipped:
            assert d["p"].unchanged() and d["m"].unchanged() and d["v"].unchanged() and gs[i].unchanged(), i
        else:
            _adam_gates(d, h, t, eps, "tensor %d (n=%d)" % (i, d["p"].n))
    # the next step counts on for every group, also those that sat the last one out
    for i in skipped:
        ds[i]["g"] = gs[i]
    before = [tuple(x.value() for x in (d["p"], d["m"], d["v"])) + (d["g"].value(),) for d in ds]
    for grp, d in zip(opt.param_groups, ds):
        grp["params"][0].grad = d["g"].t
    opt.step(); torch.cuda.synchronize()
    assert opt.n_step == t + 1
    for i, (d, h) in enumerate(zip(ds, before)):
        _adam_gates(d, h, t + 1, eps, "second step, tensor %d" % i)


@pytest.mark.parametrize("period", [4, 8, 48])
def test_fused_adam_two_rates_every_element_gets_its_rate(period):
    """split in {0, 1, 3, 4, 5, period - 1, period}; n a multiple of the period and not, with a tail of 1 to 3 elements: which rate an
    element received is recovered from dp (sqrt(v') + eps) / m' - the rates are a factor of 20 apart, so this does not hang on a tolerance"""
    eps, t = 1e-15, 7
    for split in sorted({0, 1, 3, 4, 5, period - 1, period}):
        if split > period:
            continue
        for n in (period * 257, period * 257 + 1, period * 5 + period // 2 + 2, period * 3 + 3, period):
            d, host = _one(n, period * 100 + split, "aligned", lr=0.02, lr_rest=0.001, period=period, split=split)
            _fused_step([d], t, eps)
            _adam_gates(d, host, t, eps, "period=%d split=%d n=%d" % (period, split, n), rate_check=True)


@pytest.mark.parametrize("rows", [1, 2, 1537])
def test_fused_adam_active_every_element(rows):
    """period = 48: the untouched region starts at 4 ceil(active / 4) of every period, holds NaN in p, m, v and g and keeps its bits in all
    four; the live region meets the gates; the elements between `active` and the granule end are updated by the ordinary rule with
    whatever gradient they hold (non-zero here); active >= 48 means everything"""
    eps, t, period = 1e-15, 7, 48
    for active in (1, 3, 4, 5, 12, 27, 28, 44, 45, 47, 48, 60):
        n = rows * period
        ga = 4 * ((active + 3) // 4)
        dead = (np.arange(n) % period) >= ga if active < period else np.zeros(n, bool)
        d, host = _one(n, 7 * active + rows, "aligned", nan_dead=dead, lr=0.02, lr_rest=0.001, period=period, split=3, active=active)
        _fused_step([d], t, eps)
        what = "rows=%d active=%d" % (rows, active)
        _adam_gates(d, host, t, eps, what, rate_check=True)
        assert np.array_equal(d["g"].bits()[dead], host[3].view(np.int32)[dead])
        between = ((np.arange(n) % period) >= active) & ~dead       # past `active`, inside the granule: updated like any other
        if between.any():
            assert (d["p"].value()[between] != host[0][between]).all(), what


@pytest.mark.parametrize("eps", [1e-15, 1e-8])
def test_fused_adam_at_rest_stays_at_rest(eps):
    """g = 0 with m = v = 0: all three tensors keep their bits (m' = v' = 0 and p - st 0 / (0 + eps) = p), whatever p holds"""
    n = 48 * 100 + 3
    rng = np.random.default_rng(3)
    p = (10.0 ** rng.uniform(-30, 10, n) * rng.standard_normal(n)).astype(np.float32)
    z = np.zeros(n, np.float32)
    d = dict(p=_Guarded(p), m=_Guarded(z), v=_Guarded(z), g=_Guarded(z), lr=0.02, lr_rest=0.001, period=48, split=3)
    _fused_step([d], 5, eps)
    assert d["p"].unchanged() and d["m"].unchanged() and d["v"].unchanged() and d["g"].unchanged()


def test_adam_refusals_at_the_c_abi():
    """period not a multiple of 4, a pointer off by 4 bytes, `active` with n not a whole number of periods, count = 9, step = 0: each
    returns GM_ERR_INVALID_ARG (1) with a message and, after a synchronize, every buffer keeps its bits.  Through FusedAdam a .grad
    that is a contiguous but misaligned slice raises GmeshError."""
    from gaussianmesh_amd import _lib
    from gaussianmesh_amd.model_ops import FusedAdam
    lib = _lib.lib()
    n = 48 * 20
    p, m, v, g = _adam_data(n, 1)
    G = [_Guarded(a) for a in (p, m, v, g)]

    def call(count=1, ptrs=None, size=n, period=48, split=3, active=0, step=3):
        ptrs = ptrs or [x.t.data_ptr() for x in G]
        arr = lambda ty, val: (ty * count)(*([val] * count))
        return lib.gm_adam_step_active(count, arr(C.c_void_p, ptrs[0]), arr(C.c_void_p, ptrs[3]), arr(C.c_void_p, ptrs[1]), arr(C.c_void_p, ptrs[2]),
                                       arr(C.c_uint64, size), arr(C.c_float, 0.01), arr(C.c_float, 0.001), arr(C.c_uint32, period),
                                       arr(C.c_uint32, split), arr(C.c_uint32, active), 0.9, 0.999, 1e-15, step,
                                       torch.cuda.current_stream().cuda_stream)

    base = [x.t.data_ptr() for x in G]
    cases = {"period not a multiple of 4": dict(period=6), "count = 9": dict(count=9), "step = 0": dict(step=0),
             "active with a partial period": dict(size=n - 8, active=12)}
    for k in range(4):
        cases["pointer %d off by 4 bytes" % k] = dict(ptrs=[b + (4 if i == k else 0) for i, b in enumerate(base)], size=n - 4)
    for name, kw in cases.items():
        rc = call(**kw)
        msg = lib.gm_last_error().decode()
        torch.cuda.synchronize()
        assert rc == 1 and len(msg) > 0, (name, rc, msg)
        assert all(x.unchanged() for x in G), name
    assert call() == 0                                            # the same call without the defect is accepted ...
    torch.cuda.synchronize()
    assert not G[0].unchanged() and G[0].guards_unchanged() and G[3].unchanged()           # ... and steps
    q = torch.zeros(64, device="cuda")
    opt = FusedAdam([{"params": [q], "lr": 0.01, "name": "q"}])
    q.grad = torch.ones(65, device="cuda")[1:]
    assert q.grad.is_contiguous() and q.grad.data_ptr() % 16 == 4
    with pytest.raises(_lib.GmeshError):
        opt.step()
    torch.cuda.synchronize()
    assert not q.any()


# =====================================================================================================================================
# densify_stats
# =====================================================================================================================================
@pytest.mark.parametrize("N", [1, 255, 256, 257, 100003])
def test_densify_stats_every_row(N):
    """radii include 0, negatives, 1 and values above 2^24 (whose float conversion rounds, as the reference's radii.float() does); gradient
    components span 1e-20 .. 1e15 (and a few 3e19, whose squares overflow).  Visible rows (radii > 0): max_radii2D and denom bit-equal
    to the reference statements, grad_accum within 2 ulp of the float64 acc + hypot(gx, gy).  Where gx^2 + gy^2 overflows or underflows
    in float32 the reference's own float32 torch.norm does the same: those rows are compared with the float32 statement
    acc + sqrt(gx gx + gy gy) instead, to 2 ulp plus what one spacing of the subnormal sum of squares (2^-149, a contracted
    multiply-add rounds it once, numpy twice) moves its root by.  Invisible rows hold NaN in the three accumulators and in the gradient
    and keep their bits."""
    from gaussianmesh_amd.model_ops import densify_stats
    rng = np.random.default_rng(N)
    j = np.arange(N)
    radii = rng.integers(1, 40, N)
    radii = np.where(j % 5 == 0, 0, radii); radii = np.where(j % 5 == 1, -rng.integers(1, 2 ** 30, N), radii)
    radii = np.where(j % 7 == 3, 1, radii); radii = np.where(j % 11 == 4, 2 ** 24 + rng.integers(1, 2 ** 30, N), radii)
    radii = radii.astype(np.int32)
    grad = (10.0 ** rng.uniform(-20, 15, (N, 3)) * rng.standard_normal((N, 3))).astype(np.float32)
    grad[j % 97 == 13, 0] = 3e19
    grad[j % 13 == 6, 1] = 0.0
    grad[j % 17 == 2, :2] = 0.0
    mr = (rng.random(N) * 30).astype(np.float32); mr[j % 3 == 0] = 2.0 ** 31
    acc = (10.0 ** rng.uniform(-20, 15, N)).astype(np.float32); acc[j % 4 == 1] = 0.0
    den = rng.integers(0, 30000, N).astype(np.float32)
    vis = radii > 0
    for a in (mr, acc, den):
        a[~vis] = np.nan
    grad[~vis] = np.nan
    ref = R.densify_stats_ref(radii, grad, mr, acc, den)
    t = [torch.tensor(a, device="cuda") for a in (radii, grad, mr, acc.reshape(N, 1), den.reshape(N, 1))]
    g0 = t[1].clone()
    densify_stats(*t)
    torch.cuda.synchronize()
    got_mr, got_acc, got_den = (x.cpu().numpy().reshape(-1) for x in t[2:])
    assert torch.equal(t[1].view(torch.int32), g0.view(torch.int32))
    for name, got, before in (("max_radii2D", got_mr, mr), ("grad_accum", got_acc, acc), ("denom", got_den, den)):
        assert np.array_equal(got.view(np.int32)[~vis], before.view(np.int32)[~vis]), name + ": an invisible row changed"
    assert np.array_equal(got_mr.view(np.int32)[vis], ref["max_radii2D"].view(np.int32)[vis])
    assert np.array_equal(got_den.view(np.int32)[vis], ref["denom"].view(np.int32)[vis])
    safe = vis & ref["safe"]
    msg = R.report("grad_accum vs float64", got_acc[safe], ref["accum64"][safe], 2 * R.ulp32(ref["accum64"][safe]), None)
    assert not msg, msg
    rest = vis & ~ref["safe"]
    if rest.any():
        a32 = ref["accum32"][rest].astype(np.float64)
        gx, gy = grad[rest, 0].astype(np.float64), grad[rest, 1].astype(np.float64)
        root = np.sqrt(gx * gx + gy * gy)
        fin = np.isfinite(a32)
        assert np.array_equal(np.isinf(got_acc[rest]), ~fin)
        bound = 2 * R.ulp32(a32[fin]) + 2.0 ** -149 / np.maximum(root[fin], 2.0 ** -75)
        msg = R.report("grad_accum vs the float32 statement", got_acc[rest][fin], a32[fin], bound, None)
        assert not msg, msg
    assert N < 1000 or (rest.sum() > 50 and (radii[vis] > 2 ** 24).sum() > 50)
