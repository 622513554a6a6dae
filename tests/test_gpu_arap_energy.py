"""-m gpu: gm_arap_energy_grad and gm_mesh_smooth_rows against their float64 restatement (tests/arap_energy_ref.py, established by
tests/test_arap_energy_ref_host.py), arap.ArapEnergy's autograd node, the refusals of the two entry points, and a pose fit that uses both.

Bars.  Energy and gradient: |g - g_ref| <= 1e-9 max(1, max|g_ref|) per element and |E - E_ref| <= 1e-9 max(E_ref, 1e-9 scale).  A row is a
few hundred float64 roundings; perturbing the reference's inputs by 1e-13 relative moves g by at most 2.8e-11 and E by 1.3e-12 relative
on the twelve case poses (the worst rotation conditioning among them, (s2 +- s3) / s1 = 0.05, is one_handle's start), so 1e-9 is more than
30 times the effect of a perturbation far above float64 rounding, while a wrong factor, neighbour or sign errs at order 1.
Smoothing: |y - y_ref| <= 1e-11 max|g|: a sweep is a convex combination, so errors do not grow; at most 50 roundings a row a sweep, 64
sweeps: <= 4e-13.  The worst measured ratios are printed (NOTEBOOK.md "Pose fitting")."""
import functools

import numpy as np
import pytest
import torch

import arap_cases as ac
import arap_energy_ref as er
import arap_ref
import poison

pytestmark = pytest.mark.gpu

MESHES = ("t256", "t257", "pinned", "torus_c", "fan")


@functools.lru_cache(maxsize=None)
def mesh(key):
    """(V0 float32, faces, Reference, ArapEnergy) of a case of arap_cases or one of the extra meshes; shared, do not modify"""
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.arap import ArapEnergy
    if key in ac.NAMES:
        V0, faces, ref = ac.case(key)["V0"], ac.case(key)["faces"], ac.reference(key)
    else:
        if key in ("t256", "t257"):
            verts, faces = scenes.torus_mesh(16, 16)                  # Vm = 256: exactly one full workgroup
            V0 = verts.astype(np.float32)
            if key == "t257":                                         # + one vertex no face names: a second workgroup of one, pinned, row
                V0 = np.concatenate([V0, [[0.25, 2.5, -0.5]]], 0).astype(np.float32)
        else:
            V0, faces = ac.pinned_mesh()
        faces = np.asarray(faces, np.int32)
        ref = arap_ref.Reference(V0, faces, [])
    return V0, faces, ref, ArapEnergy(V0, faces, device="cuda:0")


def bent(V0, seed):
    """a pose of the mesh for which nothing is special: a twist about y, a shear and noise of 0.02, float32"""
    rng = np.random.default_rng(seed)
    X = V0.astype(np.float64)
    a = 0.35 * X[:, 1]
    Y = np.stack([np.cos(a) * X[:, 0] + np.sin(a) * X[:, 2], X[:, 1] + 0.2 * X[:, 0], -np.sin(a) * X[:, 0] + np.cos(a) * X[:, 2]], -1)
    return (Y + 0.02 * rng.normal(size=Y.shape)).astype(np.float32)


def poses():
    out = []
    for name in ac.NAMES:
        out += [(name, "start"), (name, "iter2")]
    return out + [(m, "bent") for m in MESHES]


def pose_of(key, which):
    if which == "start":
        return ac.start(ac.case(key))
    if which == "iter2":
        return ac.reference_run(key)[0][1].astype(np.float32)
    return bent(mesh(key)[0], 11)


def device_pose(X):
    from gpu_utils import T
    return T(X)


def check_energy(key, X, label):
    V0, faces, ref, energy = mesh(key)
    E_ref, g_ref = er.value_and_grad(ref, X.astype(np.float64))
    E, g = energy.value_and_grad(device_pose(X))
    E, g = float(E.cpu()), g.cpu().numpy()
    g_bar, E_bar = 1e-9 * max(1.0, np.abs(g_ref).max()), 1e-9 * max(E_ref, 1e-9 * ref.scale)
    g_err, E_err = np.abs(g - g_ref).max(), abs(E - E_ref)
    print("%s %s (Vm %d): E %.6g, max|g| %.3g; |g - ref| / bar = %.3g, |E - ref| / bar = %.3g" % (key, label, len(V0), E_ref, np.abs(g_ref).max(),
                                                                                             g_err / g_bar, E_err / E_bar))
    assert abs(energy.scale - ref.scale) <= 1e-12 * ref.scale
    assert g.shape == g_ref.shape and g_err <= g_bar
    assert E_err <= E_bar
    return g


@pytest.mark.parametrize("key,which", poses(), ids=lambda v: v)
def test_energy_and_gradient_against_reference(key, which):
    g = check_energy(key, pose_of(key, which), which)
    ref = mesh(key)[2]
    assert not g[ref.pinned].any()                                      # pinned rows (t257: the only row of the second workgroup): 0 exactly


@pytest.mark.parametrize("key", ("torus_a", "flat_patch", "one_handle") + MESHES)
def test_rest_pose_is_exactly_zero(key):
    V0, faces, ref, energy = mesh(key)
    E, g = energy.value_and_grad(device_pose(V0))
    assert float(E.cpu()) == 0.0 and not g.cpu().numpy().any()
    # and a fold of the flat patch, which changes no edge length, is seen
    if key == "flat_patch":
        idx = ac.flat_patch_mesh()[2]
        check_energy(key, er.fold(V0, idx, 5, 0.7).astype(np.float32), "fold")


@pytest.mark.parametrize("key", ("t257", "torus_c", "fan"))
def test_same_bits_on_every_call_and_fill_and_without_the_gradient(key):
    V0, faces, ref, energy = mesh(key)
    V1 = device_pose(bent(V0, 3))
    route = lambda: energy.value_and_grad(V1)
    runs = poison.run_under_fills(route)                                # a damaged band around E or grad raises GuardViolation
    assert all(p.handed_out == 2 for p, _ in runs)
    assert poison.differing(runs) == []
    again = route()
    assert poison.same_bits(runs[0][1], again)
    with poison.poisoned(0xFF) as p:
        E_only, none = energy.value_and_grad(V1, want_grad=False)
    assert none is None and p.handed_out == 1 and poison.same_bits(E_only, again[0])
    g = device_pose(np.random.default_rng(2).normal(size=V0.shape))
    runs = poison.run_under_fills(lambda: energy.smooth_rows(g.double(), 4.0, 3))
    assert poison.differing(runs) == []


def test_autograd_node():
    V0, faces, ref, energy = mesh("torus_a")
    X = bent(V0, 5)
    E64, g64 = energy.value_and_grad(device_pose(X))
    V1 = device_pose(X).requires_grad_(True)
    E = energy(V1)
    assert E.dim() == 0 and E.dtype is torch.float32 and torch.equal(E.detach(), (E64 / energy.scale).float())
    E.backward()
    assert V1.grad.dtype is torch.float32 and torch.equal(V1.grad, (g64 / energy.scale).float())
    V1.grad = None
    (3.0 * energy(V1)).backward()                                       # the upstream factor
    assert torch.equal(V1.grad, (3.0 * g64 / energy.scale).float())
    Vd = device_pose(X).double().requires_grad_(True)                   # a float64 pose: read as float32, answered in float64
    Ed = energy(Vd)
    Ed.backward()
    assert Ed.dtype is torch.float64 and Vd.grad.dtype is torch.float64 and torch.equal(Vd.grad, g64 / energy.scale)
    (first,) = torch.autograd.grad(energy(V1), V1, create_graph=True)
    with pytest.raises(RuntimeError):                                   # once_differentiable: no second derivative
        first.sum().backward()
    from gaussianmesh_amd._lib import GmeshError
    with pytest.raises(GmeshError):
        energy(torch.tensor(X, requires_grad=True))                     # a CPU tensor


def smooth_in_place(energy, g, lam, sweeps):
    """gm_mesh_smooth_rows with out == g_in, on a copy of g"""
    from gaussianmesh_amd._op import enqueue, workspace
    buf = g.clone()
    ws = workspace(buf.device, "gm_mesh_smooth_workspace_bytes", energy.Vm)
    enqueue(buf.device, "gm_mesh_smooth_rows", energy.Vm, energy._off, energy._cols, energy._w, buf, float(lam), int(sweeps), buf, workspace=ws)
    return buf


@pytest.mark.parametrize("key", ("torus_a", "t257", "fan"))
def test_smoothing_against_reference(key):
    V0, faces, ref, energy = mesh(key)
    g = np.random.default_rng(9).normal(size=V0.shape) * np.array([1.0, 3.0, 0.2])
    dg = device_pose(g).double()
    dg.copy_(torch.tensor(g))                                           # the float64 values themselves
    bar, worst = 1e-11 * np.abs(g).max(), 0.0
    for lam in (0.0, 0.5, 4.0):
        for T in (0, 1, 2, 64):
            want = er.smooth(ref, g, lam, T)
            out = energy.smooth_rows(dg, lam, T)
            there = smooth_in_place(energy, dg, lam, T)
            assert out.dtype is torch.float64 and out.data_ptr() != dg.data_ptr() and torch.equal(dg.cpu(), torch.tensor(g))
            assert torch.equal(out, there), (lam, T)                    # in place and out of place: the same bits
            err = np.abs(out.cpu().numpy() - want).max()
            worst = max(worst, err)
            assert err <= bar, (lam, T, err)
            if T == 0 or lam == 0.0:
                assert torch.equal(out, dg)
            assert np.array_equal(out.cpu().numpy()[ref.pinned], g[ref.pinned])     # d_i = 0 keeps g_i
    print("%s: smoothing, worst |y - ref| / bar = %.3g" % (key, worst / bar))
    const = torch.tensor([[0.7, -2.5, 3.0]], dtype=torch.float64, device=dg.device).repeat(len(V0), 1)
    assert float((energy.smooth_rows(const, 4.0, 16) - const).abs().max()) <= 1e-14 * 3.0
    f32 = energy.smooth_rows(dg.float(), 0.5, 2)                        # float32 rows: float64 arithmetic, float32 answer
    assert f32.dtype is torch.float32 and torch.equal(f32, energy.smooth_rows(dg.float().double(), 0.5, 2).float())


def test_refusals_launch_nothing():
    """every refusal is decided on the arguments alone (the pointers below are not memory) and leaves its text in gm_last_error()"""
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    Vm = 300
    we, ws = l.gm_arap_energy_workspace_bytes(Vm), l.gm_mesh_smooth_workspace_bytes(Vm)
    assert we >= 72 * Vm and ws >= 56 * Vm and l.gm_arap_energy_workspace_bytes(2 * Vm) > we and l.gm_mesh_smooth_workspace_bytes(2 * Vm) > ws
    P = [k << 20 for k in range(1, 9)]                                  # eight ranges 1 MiB apart
    eg = lambda Vm=Vm, V1=P[4], E=P[5], g=P[6], w=P[7], nb=we: l.gm_arap_energy_grad(Vm, P[0], P[1], P[2], P[3], V1, E, g, w, nb, None)
    sm = lambda Vm=Vm, g=P[3], lam=1.0, T=2, out=P[4], w=P[5], nb=ws: l.gm_mesh_smooth_rows(Vm, P[0], P[1], P[2], g, lam, T, out, w, nb, None)
    for call, text in ((lambda: eg(Vm=0), b"Vm = 0"), (lambda: eg(Vm=-3), b"Vm = -3"), (lambda: eg(V1=None), b"null pointer"),
                       (lambda: eg(E=None), b"null pointer"), (lambda: eg(w=None), b"null pointer"),
                       (lambda: eg(g=P[5] + 4), b"energy_out overlaps grad_out"), (lambda: eg(g=P[4]), b"V1 overlaps grad_out"),
                       (lambda: eg(w=P[6] + 64), b"grad_out overlaps workspace"),
                       (lambda: sm(Vm=0), b"Vm = 0"), (lambda: sm(T=-1), b"sweeps = -1"), (lambda: sm(lam=-0.5), b"lambda"),
                       (lambda: sm(lam=float("nan")), b"lambda"), (lambda: sm(lam=float("inf")), b"lambda"), (lambda: sm(g=None), b"null pointer"),
                       (lambda: sm(out=None), b"null pointer"), (lambda: sm(out=P[3] + 24), b"g_in overlaps out"),
                       (lambda: sm(w=P[4] + 8), b"out overlaps workspace")):
        assert call() == 1                                              # GM_ERR_INVALID_ARG
        assert text in l.gm_last_error(), (text, l.gm_last_error())
    for call in (lambda: eg(nb=we - 1), lambda: sm(nb=ws - 1), lambda: eg(nb=0)):
        assert call() == 3 and b"workspace too small" in l.gm_last_error()   # GM_ERR_BUFFER
    from gaussianmesh_amd._lib import GmeshError
    V0, faces, ref, energy = mesh("torus_a")
    rows = device_pose(V0)
    for lam, T in ((-1.0, 2), (1.0, -2), (float("nan"), 1)):
        with pytest.raises(GmeshError):
            energy.smooth_rows(rows, lam, T)
    with pytest.raises(ValueError):
        energy.smooth_rows(rows[:5], 1.0, 1)
    with pytest.raises(ValueError):
        energy.value_and_grad(rows[:5])


def test_fit_with_the_arap_term_and_a_smoothed_gradient():
    """the scene of test_gpu_pose_fit.py; 20 steps at the default lr with regularizer="arap" and smooth_sweeps=4: no refusal, finite
    losses, each of the last three steps below the first step of the same view (a sanity condition, not a tuned number: the plain fitter
    already falls at this lr), and the gradient Adam saw is the smoothed one"""
    from gpu_utils import T
    from gaussianmesh_amd import GaussianRasterizer, scenes
    from gaussianmesh_amd.deform import SingleObjectDeform
    from gaussianmesh_amd.pose_fit import PoseFitter
    from gaussianmesh_amd.renderer import Camera, _settings
    W, H, steps = 96, 64, 20
    verts, faces = scenes.torus_mesh(24, 16)
    cl = scenes.bind_cloud_to_mesh(4000, verts, faces, seed=5)
    cov = scenes.cov3d_from_scale_rot(cl["scales"], cl["rots"]).astype(np.float32)
    obj = SingleObjectDeform(T(cl["means"]), T(cov), T(cl["opac"]), T(cl["shs"]), T(cl["tri"], dtype=torch.int32), T(cl["weights"]), T(verts))
    dev = obj.vertex.device
    cams = [Camera(scenes.orbit_camera(k, 3, W, H, radius=6.0), dev) for k in range(3)]
    V1, R, S = (T(a) for a in scenes.twist_bend_frame(verts, t=4))
    bg = torch.ones(3, device=dev)
    views = []
    with torch.no_grad():
        for cam in cams:
            pos, rgb, cov6 = obj.deform_and_shade(V1, R, S, cam.camera_center)
            image, radii = GaussianRasterizer(_settings(cam, bg, 1.0, 3, False))(pos, torch.zeros_like(pos), obj.gaussian_o, colors_precomp=rgb,
                                                                                 cov3D_precomp=cov6)
            views.append((cam, image.clone()))
    obj.deform_state = None                                             # every fit below starts at rest
    f = T(faces, dtype=torch.int32)
    plain = PoseFitter(obj, f, regularizer="arap")
    smooth = PoseFitter(obj, f, regularizer="arap", smooth_sweeps=4)
    assert plain.arap is not None and PoseFitter(obj, f).arap is None
    plain.step(*views[0]); smooth.step(*views[0])
    raw, seen = plain.pose.V1.grad, smooth.pose.V1.grad
    top = float(raw.abs().max())
    assert top > 0 and float((seen - raw).abs().max()) > 1e-2 * top    # not the raw gradient ...
    want = smooth.arap.smooth_rows(raw, 1.0, 4)                         # ... but its smoothed rows (the rasterizer's backward sums with
    assert float((seen - want).abs().max()) <= 1e-4 * top              # float atomics: 2e-7 of the max-norm from run to run)
    fitter = obj.fit_pose(views, steps, faces=f, regularizer="arap", smooth_sweeps=4, smooth_lambda=1.0)
    assert fitter.regularizer == "arap" and fitter.smooth_sweeps == 4
    losses = torch.stack(fitter.losses).cpu().numpy()
    assert losses.shape == (steps,) and np.isfinite(losses).all()
    rms = lambda a: float(((a - V1) ** 2).sum(1).mean().sqrt())
    print("pose fit, arap + 4 sweeps, %d steps: loss %s; vertex RMS error %.4f -> %.4f" % (
        steps, ", ".join("%.4f -> %.4f" % (losses[s % 3], losses[s]) for s in range(steps - 3, steps)), rms(obj.vertex), rms(fitter.pose.V1.detach())))
    for s in range(steps - 3, steps):                                   # steps s % 3 and s saw the same view
        assert losses[s] < losses[s % 3], s
