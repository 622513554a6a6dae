"""-m gpu: gm_sh_rotate (deform.rotate_sh) against the float64 definition of tests/sh_rotate_ref.py, per coefficient; what it must leave
untouched; determinism; and the claim it exists for: SH at the unrotated direction of the re-expressed row is the edit path's colour."""
import functools

import numpy as np
import pytest
import torch

import sh_rotate_ref as ref

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257, 1000)               # the one-wave edges, more than one 256-thread block, a partial last block
KINDS = ("identity", "rotation", "blend", "real", "2R", "zero")


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")            # (a copy: the shared cases are read-only arrays)


@functools.lru_cache(maxsize=None)
def _real_rot():
    """rot_out of deform_tensors for scenes' analytic twist (t = 9: 0.39 rad per unit height) on torus_mesh(24, 16), 1000 bound Gaussians"""
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.deform import deform_tensors
    verts, faces = scenes.torus_mesh(24, 16)
    cl = scenes.bind_cloud_to_mesh(1000, verts, faces, seed=4)
    V1, R, S = scenes.twist_bend_frame(verts, t=9)
    cov = scenes.cov3d_from_scale_rot(cl["scales"], cl["rots"])
    pos, _, rot, _ = deform_tensors(_dev(cl["tri"], torch.int32), _dev(cl["weights"]), _dev(V1 - verts), _dev(R), _dev(S), _dev(cov), _dev(cl["means"]))
    return pos.cpu().numpy(), rot.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(kind, N, deg):
    """(A float32 [N,3,3], c float32 [N,16,3], the float64 reference of its first (deg+1)^2 coefficients): computed once, never written"""
    rng = np.random.default_rng(1000 * KINDS.index(kind) + 10 * N + deg)
    if kind == "identity":
        A = np.tile(np.eye(3), (N, 1, 1))
    elif kind == "rotation":
        A = ref.random_rotations(N, rng)
    elif kind == "blend":
        A = ref.blended_matrices(N, rng)
    elif kind == "real":
        A = _real_rot()[1][:N]
    elif kind == "2R":
        A = 2.0 * ref.random_rotations(N, rng)
    else:
        A = np.zeros((N, 3, 3))
    A = A.astype(np.float32)
    c = ref.random_coefficients(N, rng).astype(np.float32)
    exp = ref.rotate_sh_ref(c, A, deg)[:, :(deg + 1) ** 2]
    for a in (A, c, exp):
        a.setflags(write=False)
    return A, c, exp


def _ratio(got, A, c, exp, deg):
    """worst |got - exp| over the bar 1e-5 max(1, |A|_F)^deg max_k |c_k| (the row's largest coefficient)"""
    n = (deg + 1) ** 2
    bar = 1e-5 * np.maximum(1.0, np.linalg.norm(A.astype(np.float64), axis=(1, 2))) ** deg * np.abs(c[:, :n]).max(axis=(1, 2))
    return float((np.abs(got[:, :n].astype(np.float64) - exp).max(axis=(1, 2)) / bar).max())


@pytest.mark.parametrize("full_rows", [False, True])
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
@pytest.mark.parametrize("N", SIZES)
def test_coefficients_untouched_data_and_determinism(N, deg, full_rows):
    from gaussianmesh_amd.deform import rotate_sh
    n = (deg + 1) ** 2
    M = 16 if full_rows else n
    worst = 0.0
    for kind in KINDS:
        A, c16, exp = _case(kind, N, deg)
        c = np.ascontiguousarray(c16[:, :M])
        shs, rot = _dev(c), _dev(A)
        out = rotate_sh(shs, rot, deg)
        got = out.cpu().numpy()
        assert torch.equal(shs, _dev(c)), "the input was written"
        # 2. untouched data: the coefficients beyond the degree, and every row at degree 0, bit for bit
        assert np.array_equal(got[:, n:].view(np.uint32), c[:, n:].view(np.uint32)), kind
        if deg == 0:
            assert np.array_equal(got.view(np.uint32), c.view(np.uint32)), kind
        # 1. coefficients
        worst = max(worst, _ratio(got, A, c, exp, deg))
        # 3. determinism: twice equals once, in place equals out of place
        assert torch.equal(rotate_sh(shs, rot, deg), out), kind
        inplace = shs.clone()
        assert rotate_sh(inplace, rot, deg, out=inplace) is inplace and torch.equal(inplace, out), kind
    print("N %d deg %d M %d: worst error / bar = %.3g" % (N, deg, M, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("deg, M", [(3, 16), (2, 16), (2, 9), (1, 7)])
@pytest.mark.parametrize("off_in, off_out", [(1, 1), (1, 0), (0, 1)])
def test_bases_offset_by_one_float_take_the_scalar_route(deg, M, off_in, off_out):
    """a base pointer 4 bytes past a 16-byte boundary (load_sh's scalar loads, scalar stores), on either side or both, and row strides
    that are no whole number of 16-byte granules (M = 9, 7): the same bits as the aligned call, and nothing written outside the rows"""
    from gaussianmesh_amd.deform import rotate_sh
    N = 257
    A, c16, exp = _case("blend", N, deg)
    c = np.ascontiguousarray(c16[:, :M])
    aligned = rotate_sh(_dev(c), _dev(A), deg) if (M * 3) % 4 == 0 else None
    src = torch.zeros(N * M * 3 + 2, device="cuda")
    dst = torch.full((N * M * 3 + 2,), 7.0, device="cuda")
    shs = src[off_in:off_in + N * M * 3].view(N, M, 3)
    out = dst[off_out:off_out + N * M * 3].view(N, M, 3)
    shs.copy_(_dev(c))
    assert shs.data_ptr() % 16 == 4 * off_in and out.data_ptr() % 16 == 4 * off_out
    assert rotate_sh(shs, _dev(A), deg, out=out) is out
    got = out.cpu().numpy()
    assert _ratio(got, A, c, exp, deg) <= 1.0
    assert np.array_equal(got[:, (deg + 1) ** 2:], c[:, (deg + 1) ** 2:])
    if aligned is not None:
        assert torch.equal(out, aligned)
    assert bool((dst[:off_out] == 7.0).all()) and bool((dst[off_out + N * M * 3:] == 7.0).all())
    inplace = shs.clone() if off_in == 0 else shs
    rotate_sh(inplace, _dev(A), deg, out=inplace)
    assert torch.equal(inplace, out)
    assert bool((src[:off_in] == 0).all()) and bool((src[off_in + N * M * 3:] == 0).all())


def test_non_finite_entries_stay_in_their_row():
    from gaussianmesh_amd.deform import rotate_sh
    A, c, _ = _case("blend", 257, 3)
    clean = rotate_sh(_dev(c), _dev(A), 3)
    A2, c2 = A.copy(), c.copy()
    A2[70, 1, 2] = np.nan; c2[130, 5, 1] = np.inf
    got = rotate_sh(_dev(c2), _dev(A2), 3)
    keep = np.ones(257, bool); keep[[70, 130]] = False
    assert torch.equal(got[_dev(keep, torch.bool)], clean[_dev(keep, torch.bool)])
    assert not bool(torch.isfinite(got[70]).all()) and not bool(torch.isfinite(got[130, :, 1]).all())
    assert bool(torch.isfinite(got[130, :, 0]).all() and torch.isfinite(got[130, :, 2]).all())     # (the channels do not mix either)


@pytest.mark.parametrize("deg", [1, 2, 3])
@pytest.mark.parametrize("kind", ["blend", "real"])
def test_unrotated_sh_of_the_rotated_row_is_the_edit_paths_colour(kind, deg):
    """4. sh_colors(pos, campos, rotate_sh(shs, A), rot=None) is within 1e-5 of sh_colors(pos, campos, shs, rot=A), per Gaussian"""
    from gaussianmesh_amd.deform import rotate_sh, sh_colors
    N = 1000
    A, c, _ = _case(kind, N, deg)
    rng = np.random.default_rng(deg)
    pos = _real_rot()[0] if kind == "real" else rng.uniform(-3, 3, size=(N, 3))
    worst = 0.0
    for campos in ((4.0, 3.0, 5.0), (-6.5, 1.5, 0.2), (0.1, -7.0, 0.3)):
        p, cam, shs, rot = _dev(pos), _dev(campos), _dev(c), _dev(A)
        exp = sh_colors(p, cam, shs, rot=rot, deg=deg)
        got = sh_colors(p, cam, rotate_sh(shs, rot, deg), rot=None, deg=deg)
        worst = max(worst, float((got - exp).abs().max()))
        plain = sh_colors(p, cam, shs, rot=None, deg=deg)
        assert float((plain - exp).abs().max()) > 3e-3                 # (the rotation matters on these inputs: the unrotated rows miss)
    print("%s deg %d: max colour difference %.3g" % (kind, deg, worst))
    assert worst <= 1e-5
