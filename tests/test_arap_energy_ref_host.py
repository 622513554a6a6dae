"""CPU: the float64 restatement of the pose energy, its gradient and the smoothing sweep (tests/arap_energy_ref.py) is itself right -
the gradient against central differences of the energy, the step that cannot raise the energy, what the energy sees (a fold) and does
not see (a rigid motion), the exact zeros of the rest pose, the sweep's invariants - and the Python entry points refuse what they must
without a device.  tests/test_gpu_arap_energy.py then holds the kernels to this restatement."""
import numpy as np
import pytest
import torch

import arap_cases as ac
import arap_energy_ref as er


def perturbed_start(name, amount=0.01):
    """the case's starting pose (handles at their targets) with every coordinate moved by N(0, amount), as float64"""
    c = ac.case(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    return ac.start(c).astype(np.float64) + amount * rng.normal(size=c["V0"].shape)


@pytest.mark.parametrize("name", ac.NAMES)
def test_gradient_against_central_differences(name):
    """40 random coordinates, h = 1e-6, the rotations re-minimised at both ends (the total derivative).  Bar 1e-6 max(1, max|g|): the
    difference quotient carries the rounding of E, a float64 sum of up to 6.4 k terms (n eps E at worst, about 1e-12 E) over 2h, with E
    up to a few units here - some 1e-6 at the very worst, a few 1e-9 as observed; the truncation term h^2 E'''/6 is below 1e-10.  A wrong
    factor, sign or neighbour errs at the order of |g|."""
    ref, X = ac.reference(name), perturbed_start(name)
    g = er.gradient(ref, X)
    rng = np.random.default_rng(7)
    h, worst = 1e-6, 0.0
    for i, c in zip(rng.integers(0, len(X), 40), rng.integers(0, 3, 40)):
        Xp, Xm = X.copy(), X.copy()
        Xp[i, c] += h; Xm[i, c] -= h
        fd = (er.energy(ref, Xp) - er.energy(ref, Xm)) / (2 * h)
        worst = max(worst, abs(fd - g[i, c]))
    bar = 1e-6 * max(1.0, np.abs(g).max())
    print("%s: central differences against the formula, worst |diff| %.3g, max|g| %.3g (bar %.3g)" % (name, worst, np.abs(g).max(), bar))
    assert worst <= bar
    # the edge-by-edge sum is the residual of the global step's equation, times 4
    R = er.rotations(ref, X)
    assert np.abs(g - 4.0 * (ref.L @ X - ref.rhs(R))).max() <= 1e-12 * max(1.0, np.abs(g).max())


@pytest.mark.parametrize("name", ac.NAMES)
def test_step_of_one_over_8_max_degree_never_raises_the_energy(name):
    """for fixed R, E is quadratic in x with Hessian 4 L and lambda_max(L) <= 2 max d, so x - g / (8 max d) cannot raise E(., R), and
    re-minimising R cannot either.  30 steps; every E at most its predecessor (to the rounding of the sum, 1e-12 relative)."""
    ref, X = ac.reference(name), perturbed_start(name)
    step = 1.0 / (8.0 * ref.deg.max())
    E, g = er.value_and_grad(ref, X)
    first = E
    for _ in range(30):
        X = X - step * g
        E_next, g = er.value_and_grad(ref, X)
        assert E_next <= E * (1 + 1e-12), (E, E_next)
        E = E_next
    print("%s: E %.4g -> %.4g in 30 steps of 1 / (8 max d)" % (name, first, E))
    assert E < first


def test_a_fold_changes_no_edge_length_and_has_energy():
    """the 12 x 9 flat patch folded by 0.7 rad along the vertex line i = 5: the bending the edge-length term cannot see"""
    flat, faces, idx = ac.flat_patch_mesh()
    ref = ac.reference("flat_patch")
    X = er.fold(ref.V0, idx, 5, 0.7)
    length = lambda P: np.linalg.norm(P[ref.I] - P[ref.J], axis=1)
    change = np.abs(length(X) - length(ref.V0)).max()
    E = er.energy(ref, X)
    print("fold: worst edge-length change %.3g, E %.4g, E / scale %.3g" % (change, E, E / ref.scale))
    assert change <= 1e-12
    assert E / ref.scale > 1e-3


@pytest.mark.parametrize("name", ac.NAMES)
def test_rigid_motion_and_rest_pose(name):
    ref = ac.reference(name)
    X = ref.V0 @ ac.rotation((1, 2, -0.5), 0.9).T + np.array([0.3, -1.0, 0.2])
    E, g = er.value_and_grad(ref, X)
    print("%s: rigid motion E / scale %.3g, max|g| %.3g" % (name, E / ref.scale, np.abs(g).max()))
    assert E <= 1e-20 * ref.scale
    E, g = er.value_and_grad(ref, ref.V0)
    assert E == 0.0 and not g.any()
    assert np.array_equal(er.rotations(ref, ref.V0), np.tile(np.eye(3), (len(ref.V0), 1, 1)))


@pytest.mark.parametrize("name", ("torus_a", "fan"))
def test_sweep_keeps_constants_and_grows_nothing(name):
    """Every sweep is a convex combination of g_i and the neighbours' current values, and y starts at g: by induction max|y^t| <=
    max|g| for every t (to one rounding per sweep).  (From one sweep to the next the maximum CAN rise - a single spike first spreads to
    its neighbours and then receives some of it back - so the bound that holds is the one against g.)"""
    ref = ac.reference(name)
    const = np.tile([[0.7, -2.5, 3.0]], (len(ref.V0), 1))
    for lam in (0.0, 0.5, 4.0):
        assert np.abs(er.smooth(ref, const, lam, 16) - const).max() <= 1e-14 * 3.0
    rng = np.random.default_rng(3)
    spike = np.zeros_like(ref.V0); spike[1] = (1.0, -2.0, 0.5)
    for g in (rng.normal(size=ref.V0.shape), spike):
        top = np.abs(g).max()
        for lam in (0.5, 4.0):
            for T in (1, 2, 3, 8, 64):
                assert np.abs(er.smooth(ref, g, lam, T)).max() <= top * (1 + 1e-14)
        assert np.array_equal(er.smooth(ref, g, 4.0, 0), g) and np.array_equal(er.smooth(ref, g, 0.0, 5), g)


def test_pinned_rows_keep_their_value_under_the_sweep():
    import arap_ref
    V0, faces = ac.pinned_mesh()
    ref = arap_ref.Reference(V0, faces, [])
    g = np.random.default_rng(5).normal(size=V0.shape)
    y = er.smooth(ref, g, 4.0, 7)
    assert ref.pinned.sum() == 2 and np.array_equal(y[ref.pinned], g[ref.pinned])
    E, gr = er.value_and_grad(ref, V0.astype(np.float64) + 0.01 * g)
    assert not gr[ref.pinned].any()


def test_python_entry_points_refuse_without_a_device():
    from gaussianmesh_amd._lib import GmeshError
    from gaussianmesh_amd.arap import ArapEnergy
    from gaussianmesh_amd.pose_fit import PoseFitter
    c = ac.case("torus_a")
    energy = ArapEnergy(c["V0"], c["faces"], device="cpu")
    ref = ac.reference("torus_a")
    assert abs(energy.scale - ref.scale) <= 1e-12 * ref.scale
    V1 = torch.tensor(c["V0"], requires_grad=True)
    with pytest.raises(GmeshError):
        energy(V1)
    with pytest.raises(GmeshError):
        energy.value_and_grad(V1)
    with pytest.raises(GmeshError):
        energy.smooth_rows(torch.zeros(len(c["V0"]), 3), 1.0, 2)
    with pytest.raises(ValueError, match="regularizer"):
        PoseFitter(None, c["faces"], regularizer="bogus")
