"""Host side of the sampled signed-distance grid (gm_sdf_grid_prepare / gm_sdf_grid_sample, dynamics.SdfGrid): the numpy restatement of
tests/sdf_grid_ref.py is established before the device is held to it - an affine field comes back exactly, a sphere converges as voxel^2,
the gradients over known neighbours by hand - then the declaration and typing of the two entry points, their refusals that need no
device, and SdfGrid's own.  No device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dynamics_field_cases as fc
import sdf_grid_ref as sg
from gaussianmesh_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_an_affine_field_is_reproduced_and_its_normal_is_the_planes():
    """samples at multiples of 1/8 and the plane 2 x + y + 2 z = 0.75 (every sample value exact in float32, scale 1/4): trilinear
    interpolation reproduces an affine function, so phi = (2 x + y + 2 z - 0.75) / 4 and n = (2, 1, 2) / 3 within 1e-12, at cell centres,
    on faces, on corners and in the first and last cell; one-sided differences at the border give the same gradient"""
    dims, origin, voxel = (9, 7, 8), (-1.0, -0.75, -1.125), 0.25
    a = np.array([2.0, 1.0, 2.0])
    values = (fc.centres(dims, origin, voxel) @ a - 0.75).astype(F)
    grid = sg.prepare(values, voxel, scale=0.25)
    assert grid.dtype == F and grid.shape == (8, 7, 9, 4) and not np.isnan(grid).any()
    assert np.array_equal(grid[..., 1:], np.broadcast_to((a / 4.0).astype(F), grid[..., 1:].shape))           # border samples included
    rng = np.random.default_rng(0)
    lo, hi = np.asarray(origin) + 0.5 * voxel, np.asarray(origin) + (np.asarray(dims) - 0.5) * voxel
    P = np.concatenate([rng.uniform(lo, hi - 1e-9, size=(300, 3)), fc.centres(dims, origin, voxel)[:-1, :-1, :-1].reshape(-1, 3),
                        lo[None], lo[None] + [0.125, 0.25, 0.0], hi[None] - 1e-7])
    phi, n = sg.sample(grid, origin, voxel, P)
    assert not np.isnan(phi).any()
    assert float(np.abs(phi - (P @ a - 0.75) / 4.0).max()) <= 1e-12 and float(np.abs(n - a / 3.0).max()) <= 1e-12


def test_a_sphere_converges_as_the_square_of_the_voxel():
    """|p| - 1 sampled at voxel 0.2, 0.1, 0.05: the largest error of phi over points between 0.6 and 1.4 from the centre falls by a
    factor of 4 per halving (trilinear interpolation is second order), and so does the normal's"""
    rng = np.random.default_rng(1)
    d = rng.normal(size=(400, 3))
    P = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.6, 1.4, size=(400, 1))
    errs, nerrs = [], []
    for voxel in (0.2, 0.1, 0.05):
        n = int(round(4.0 / voxel))
        origin = (-2.0 + 0.013, -2.0 + 0.007, -2.0 - 0.011)
        values = fc.sphere_values((n, n, n), origin, voxel, (0.0, 0.0, 0.0), 1.0)
        phi, nor = sg.sample(sg.prepare(values, voxel), origin, voxel, P)
        assert not np.isnan(phi).any()
        errs.append(float(np.abs(phi - (np.linalg.norm(P, axis=1) - 1.0)).max()))
        nerrs.append(float(np.abs(nor - P / np.linalg.norm(P, axis=1, keepdims=True)).max()))
    print("sphere: phi errors %s, normal errors %s" % (errs, nerrs))
    for e in (errs, nerrs):
        assert 3.0 <= e[0] / e[1] <= 5.5 and 3.0 <= e[1] / e[2] <= 5.5
    assert errs[2] < 2e-3


def test_prepare_takes_its_gradients_over_the_known_neighbours():
    v = np.arange(27, dtype=F).reshape(3, 3, 3) ** 2                   # value = (9 z + 3 y + x)^2
    w = np.ones((3, 3, 3), F)
    v[1, 1, 2] = np.nan                                                # unknown by value
    w[1, 0, 1] = 0.5                                                   # unknown by weight
    g = sg.prepare(v, 0.5, w, 1.0, 2.0)
    assert np.isnan(g[1, 1, 2]).all() and np.isnan(g[1, 0, 1]).all() and np.isnan(g[..., 0]).sum() == 2
    c = g[1, 1, 1]                                                     # the centre: x has only its lower neighbour, y only its upper, z both
    assert c[0] == F(2 * 13 ** 2)
    assert c[1] == F((2 * 13 ** 2 - 2 * 12 ** 2) / 0.5) and c[2] == F((2 * 16 ** 2 - 2 * 13 ** 2) / 0.5) and c[3] == F((2 * 22 ** 2 - 2 * 4 ** 2) / 1.0)
    alone = np.full((3, 3, 3), np.nan, F)
    alone[1, 1, 1] = 3.0
    g = sg.prepare(alone, 0.5)
    assert np.array_equal(g[1, 1, 1], np.array([3.0, 0.0, 0.0, 0.0], F)) and np.isnan(g[..., 0]).sum() == 26
    phi, n = sg.sample(g, (0, 0, 0), 0.5, np.array([[0.6, 0.6, 0.6]]))
    assert np.isnan(phi).all() and np.isnan(n).all()                   # next to unknown samples
    flat = sg.prepare(np.full((3, 3, 3), 0.25, F), 0.5)                # a constant region: a gradient without a direction
    phi, n = sg.sample(flat, (0, 0, 0), 0.5, np.array([[0.6, 0.6, 0.6], [0.2, 0.6, 0.6], [np.nan, 0.6, 0.6], [np.inf, 0.6, 0.6]]))
    assert np.isnan(phi).all() and np.isnan(n).all()
    w2 = np.full((3, 3, 3), np.nan, F)                                 # a NaN weight fails the test; without weights every sample passes it
    assert np.isnan(sg.prepare(np.ones((3, 3, 3), F), 0.5, w2)).all() and not np.isnan(sg.prepare(np.ones((3, 3, 3), F), 0.5)).any()


def test_outside_is_decided_per_axis_on_the_grid_coordinate():
    dims, origin, voxel = (4, 3, 5), (0.0, 0.0, 0.0), 0.5
    grid = sg.prepare(fc.plane_values(dims, origin, voxel, (1.0, 2.0, 3.0), 0.1), voxel)
    first, last = 0.25, np.array([1.75, 1.25, 2.25])                   # g = 0 and g = n - 1
    inside = np.array([[first, first, first], [1.0, 1.0, 1.0], np.nextafter(last, 0.0)])
    outside = np.array([[np.nextafter(first, -1.0), 1.0, 1.0], [1.0, last[1], 1.0], [1.0, 1.0, last[2]], [last[0], 1.0, 1.0], [-5.0, 1.0, 1.0], [1.0, 1e30, 1.0]])
    assert not np.isnan(sg.sample(grid, origin, voxel, inside)[0]).any() and np.isnan(sg.sample(grid, origin, voxel, outside)[0]).all()


# ---- the entry points ----
@pytest.mark.parametrize("name, n", [("gm_sdf_grid_prepare", 10), ("gm_sdf_grid_sample", 11), ("gm_mesh_dynamics_field", 41)])
def test_header_declares_and_lib_types_the_entry_points(name, n):
    text = open(os.path.join(ROOT, "include", "gmesh_hip.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m and len(m.group(1).split(",")) == n
    assert name in _lib.header_symbols() and len(_lib.SIGNATURES[name][1]) == n and hasattr(_lib.lib(), name)
    assert "#define GM_ABI_VERSION 3" in text and _lib.lib().gm_abi_version() == 3


def test_the_field_entry_is_the_contact_entry_plus_the_grid():
    a, b = _lib.SIGNATURES["gm_mesh_dynamics_field"][1], _lib.SIGNATURES["gm_mesh_dynamics_contact"][1]
    assert a[:27] == b[:27] and a[34:] == b[27:] and len(a) == len(b) + 7


def test_prepare_and_sample_refuse_before_any_gpu_work():
    """bogus non-null "pointers", never dereferenced: every refusal is decided on the arguments alone"""
    l = _lib.lib()
    M = 1 << 24
    org = (C.c_float * 3)(0.0, 0.0, 0.0)

    def prep(n=(4, 5, 6), values=1 * M, weight=2 * M, min_weight=1.0, scale=1.0, voxel=0.1, out=3 * M):
        return l.gm_sdf_grid_prepare(n[0], n[1], n[2], values, weight, min_weight, scale, voxel, out, None)

    def samp(N=10, points=1 * M, n=(4, 5, 6), origin=org, voxel=0.1, grid=2 * M, phi=3 * M, nor=4 * M):
        return l.gm_sdf_grid_sample(N, points, n[0], n[1], n[2], origin, voxel, grid, phi, nor, None)
    nan, inf = float("nan"), float("inf")
    for call, fn in ((prep, b"gm_sdf_grid_prepare"), (samp, b"gm_sdf_grid_sample")):
        def refused(what, **kw):
            assert call(**kw) == 1 and fn in l.gm_last_error() and what in l.gm_last_error(), (kw, l.gm_last_error())
        for n in ((1, 5, 6), (4, 1, 6), (4, 5, 1), (0, 5, 6), (-2, 5, 6)):
            refused(b"at least 2", n=n)
        for n in ((1 << 15, 1 << 14, 2), (1 << 10, 1 << 10, (1 << 8) + 1)):
            refused(b"2^28", n=n)
        for voxel in (0.0, -0.1, nan, inf):
            refused(b"voxel", voxel=voxel)
    def refused(call, fn, what, **kw):
        assert call(**kw) == 1 and fn in l.gm_last_error() and what in l.gm_last_error(), (kw, l.gm_last_error())
    for scale in (nan, inf, -inf):
        refused(prep, b"prepare", b"scale", scale=scale)
    for k in ("values", "out"):
        refused(prep, b"prepare", b"null", **{k: None})
    refused(prep, b"prepare", b"aligned", out=3 * M + 4)
    refused(prep, b"prepare", b"overlaps", out=1 * M + 16)
    refused(prep, b"prepare", b"overlaps", out=2 * M - 16 * 119)
    refused(prep, b"prepare", b"overlaps", weight=3 * M + 16 * 119)
    for N in (0, -1):
        refused(samp, b"sample", b"N =", N=N)
    for bad in ((nan, 0.0, 0.0), (0.0, inf, 0.0), (0.0, 0.0, -inf)):
        refused(samp, b"sample", b"origin", origin=(C.c_float * 3)(*bad))
    for k in ("points", "origin", "grid", "phi", "nor"):
        refused(samp, b"sample", b"null", **{k: None})
    refused(samp, b"sample", b"aligned", grid=2 * M + 8)
    refused(samp, b"sample", b"overlaps", phi=2 * M + 16)
    refused(samp, b"sample", b"overlaps", nor=1 * M + 12)
    refused(samp, b"sample", b"overlaps", nor=3 * M + 72)


def test_sdf_grid_refuses_on_the_host():
    from gaussianmesh_amd._lib import GmeshError
    from gaussianmesh_amd.dynamics import SdfGrid
    v = np.zeros((3, 4, 5), F)
    for kw in (dict(values=np.zeros((4, 5), F)), dict(values=np.zeros((1, 4, 5), F)), dict(values=[[0.0]]), dict(origin=(0.0, 0.0)), dict(origin=(0.0, np.nan, 0.0)),
               dict(origin=(0.0, np.inf, 0.0)), dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=np.nan), dict(voxel=np.inf), dict(voxel="1"), dict(scale=np.nan),
               dict(scale=np.inf), dict(weight=np.zeros((3, 4, 4), F)), dict(weight=np.zeros((60,), F)), dict(min_weight=np.nan)):
        with pytest.raises(ValueError):
            SdfGrid(**dict(dict(values=v, origin=(0.0, 0.0, 0.0), voxel=0.1, device="cpu"), **kw))
    with pytest.raises(GmeshError):                                    # everything in order but the device: there is no CPU path
        SdfGrid(v, (0.0, 0.0, 0.0), 0.1, device="cpu")
