"""-m gpu: gm_sdf_grid_prepare against its definition - the numpy float32 restatement of tests/sdf_grid_ref.py, bit for bit, on grids whose
last block is partly empty, with and without weights, with unknown samples of every kind, on poisoned guard-banded buffers - and
gm_sdf_grid_sample (dynamics.SdfGrid.sample) against the float64 restatement at every edge of a cell and of the grid."""
import numpy as np
import pytest
import torch

import dynamics_field_cases as fc
import sdf_grid_ref as sg
from poison import differing, run_under_fills, same_bits

pytestmark = pytest.mark.gpu
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _volume(dims, seed, holes=True):
    """(values, weight, voxel): a smooth field plus noise; NaN samples, weights just below min_weight = 2, a valid sample with no valid
    neighbour (its six neighbours made NaN) and one with a single valid neighbour"""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    origin, voxel = (-0.37, 0.21, -1.13), 0.173
    v = (fc.sphere_values(dims, origin, voxel, (0.1, 0.6, -0.7), 0.4) + 0.05 * rng.normal(size=(nz, ny, nx))).astype(F)
    w = rng.integers(2, 5, size=(nz, ny, nx)).astype(F)
    if holes:
        v[rng.random(v.shape) < 0.08] = np.nan
        w[rng.random(v.shape) < 0.08] = np.nextafter(F(2.0), F(0.0))   # just below min_weight
        w[rng.random(v.shape) < 0.03] = np.nan
        if min(dims) >= 3:
            z, y, x = nz // 2, ny // 2, nx // 2
            v[z, y, x], w[z, y, x] = 0.3, 4.0                          # alone among six unknown neighbours ...
            for dz, dy, dx in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
                v[z + dz, y + dy, x + dx] = np.nan
            if nx >= 9:
                v[z, y, x + 3], w[z, y, x + 3] = -0.2, 4.0             # ... and one whose only valid neighbour is its upper x one
                for dz, dy, dx in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, -1)):
                    v[z + dz, y + dy, x + 3 + dx] = np.nan
                v[z, y, x + 4], w[z, y, x + 4] = 0.1, 3.0
    return v, w, voxel


GRIDS = [(2, 2, 2), (3, 5, 7), (33, 9, 5), (7, 5, 3)]                  # 8, 105, 1485 (five full blocks of 256 and 205 samples) and 105 samples


@pytest.mark.parametrize("dims", GRIDS, ids=lambda n: "%dx%dx%d" % n)
def test_prepare_bit_for_bit(dims):
    from gaussianmesh_amd.dynamics import SdfGrid
    v, w, voxel = _volume(dims, sum(dims))
    seen = 0
    for weight, min_weight, scale in ((w, 2.0, 0.519), (None, 1.0, 1.0), (w, 2.0, 1.0), (None, 7.0, -2.5)):
        want = sg.prepare(v, voxel, weight, min_weight, scale)

        def route():
            return SdfGrid(v, (0.0, 0.0, 0.0), voxel, weight=weight, min_weight=min_weight, scale=scale).grid
        runs = run_under_fills(route)
        assert differing(runs) == [] and all(p.handed_out >= 1 for p, _ in runs)
        got = runs[0][1].cpu().numpy()
        assert got.shape == want.shape == (dims[2], dims[1], dims[0], 4) and got.dtype == F
        assert np.array_equal(_bits(got), _bits(want)), "%s weights %s: %d samples differ" % (dims, weight is not None, int((_bits(got) != _bits(want)).any(-1).sum()))
        seen += int(np.isnan(want[..., 0]).sum())
        if weight is None and min(dims) >= 3:
            z, y, x = dims[2] // 2, dims[1] // 2, dims[0] // 2
            assert np.array_equal(got[z, y, x], np.array([F(0.3) * F(scale), 0.0, 0.0, 0.0], F))                # the isolated sample
    assert seen > 0 or dims == (2, 2, 2)
    one = sg.prepare(v, voxel, w, 2.0, 1.0)
    if dims[0] >= 9:
        z, y, x = dims[2] // 2, dims[1] // 2, dims[0] // 2 + 3
        assert one[z, y, x, 1] == F((F(0.1) - F(-0.2)) / F(voxel)) and one[z, y, x, 2] == 0.0 and one[z, y, x, 3] == 0.0


def test_prepare_of_a_volume_without_holes_has_no_nan():
    from gaussianmesh_amd.dynamics import SdfGrid
    v, w, voxel = _volume((33, 9, 5), 3, holes=False)
    got = SdfGrid(v, (0.0, 0.0, 0.0), voxel, weight=w, min_weight=2).grid.cpu().numpy()
    assert not np.isnan(got).any() and np.array_equal(_bits(got), _bits(sg.prepare(v, voxel, w, 2.0)))


def _points(grid, dims, origin, voxel, rng):
    """every kind of point the definition distinguishes, float32 [N,3]"""
    o, h = np.asarray(origin, F).astype(np.float64), float(F(voxel))
    n = np.asarray(dims)
    centres = fc.centres(dims, origin, voxel).reshape(-1, 3)           # sample centres: cell corners, f = 0 (the last ones: outside)
    lo, hi = o + 0.5 * h, o + (n - 0.5) * h                            # g = 0 and g = n - 1
    inside = rng.uniform(lo, hi, size=(200, 3))
    faces = inside.copy()
    faces[:, 0] = o[0] + (np.floor((faces[:, 0] - o[0]) / h - 0.5) + 0.5) * h          # on a cell face across x
    first, last = lo + 0.25 * h, hi - 0.25 * h                         # the first and the last cell of every axis
    ends = []
    for a in range(3):
        for edge in (lo[a], hi[a]):                                    # g_a one float32 step inside and outside both ends
            for step in (-np.inf, np.inf):
                p = (0.5 * (lo + hi)).astype(F)
                p[a] = np.nextafter(F(edge), F(step))
                ends.append(p.astype(np.float64))
            p = (0.5 * (lo + hi)).astype(F)
            p[a] = F(edge)
            ends.append(p.astype(np.float64))
    odd = np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf], [1e30, 0.0, 0.0], [-1e30, 0.0, 0.0]]) + 0.5 * (lo + hi)
    return np.concatenate([centres, inside, faces, first[None], last[None], np.array(ends), odd]).astype(F)


@pytest.mark.parametrize("holes", [False, True], ids=["whole", "holes"])
def test_sample_against_the_float64_restatement(holes):
    """phi and each normal component within 1e-12 on a field of order 1 (about twenty float64 roundings, 4e-15, and numpy has no fma; five
    orders under any float32 effect), the NaN pattern identical: outside, next to an unknown sample, on a gradient without a direction"""
    from gaussianmesh_amd.dynamics import SdfGrid
    dims, origin = (9, 7, 8), (-0.37, 0.21, -1.13)
    v, w, voxel = _volume(dims, 11, holes=holes)
    v[0:3, 0:3, 0:3] = 0.25                                            # a constant region: zero gradient in the cell in its middle
    if holes:
        v[5, 4, 6] = np.nan
    grid = SdfGrid(v, origin, voxel, weight=w if holes else None, min_weight=2)
    ref = sg.prepare(v, voxel, w if holes else None, 2.0)
    assert np.array_equal(_bits(grid.grid.cpu().numpy()), _bits(ref))
    P = _points(ref, dims, origin, voxel, np.random.default_rng(5))
    want_phi, want_n = sg.sample(ref, origin, voxel, P.astype(np.float64))
    phi, n = grid.sample(torch.as_tensor(P, device="cuda"))
    assert phi.dtype == torch.float64 and n.dtype == torch.float64 and phi.shape == (len(P),) and n.shape == (len(P), 3)
    phi, n = phi.cpu().numpy(), n.cpu().numpy()
    nan = np.isnan(want_phi)
    assert np.array_equal(np.isnan(phi), nan) and np.array_equal(np.isnan(n), np.broadcast_to(nan[:, None], n.shape))
    assert nan.sum() > 20 and (~nan).sum() >= 50
    ep, en = float(np.abs(phi - want_phi)[~nan].max()), float(np.abs(n - want_n)[~nan].max())
    print("sample (%s): phi %.3g, normal %.3g over %d rows, %d NaN" % ("holes" if holes else "whole", ep, en, len(P), int(nan.sum())))
    assert ep <= 1e-12 and en <= 1e-12 and float(np.abs(np.linalg.norm(n[~nan], axis=1) - 1.0).max()) <= 1e-12
    mid = (np.asarray(origin, np.float64) + 0.8 * voxel)[None].astype(F)       # in the cell of samples 0 and 1, whose gradients are all 0
    assert np.isnan(grid.sample(mid)[0].cpu().numpy()).all() and np.isnan(sg.sample(ref, origin, voxel, mid)[0]).all()      # the constant cell
    if holes:                                                          # a cell with exactly one NaN corner
        corner = np.isnan(ref[..., 0])
        cells = sum(corner[dz:dims[2] - 1 + dz, dy:dims[1] - 1 + dy, dx:dims[0] - 1 + dx].astype(int) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1))
        z, y, x = np.argwhere(cells == 1)[0]
        p = (np.asarray(origin, np.float64) + (np.array([x, y, z]) + 1.0) * voxel)[None].astype(F)
        assert np.isnan(grid.sample(p)[0].cpu().numpy()).all()


@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_sample_row_counts_on_poisoned_memory(N):
    from gaussianmesh_amd.dynamics import SdfGrid
    dims, origin, voxel = (6, 5, 4), (0.1, -0.2, 0.3), 0.25
    v = fc.plane_values(dims, origin, voxel, (0.3, 1.0, -0.2), 0.1)
    grid = SdfGrid(v, origin, voxel)
    ref = sg.prepare(v, voxel)
    P = np.random.default_rng(N).uniform(0.0, 1.6, size=(N, 3)).astype(F)
    pts = torch.as_tensor(P, device="cuda")
    runs = run_under_fills(lambda: grid.sample(pts))
    assert differing(runs) == [] and all(p.handed_out >= 2 for p, _ in runs)
    phi, n = (t.cpu().numpy() for t in runs[0][1])
    want_phi, want_n = sg.sample(ref, origin, voxel, P.astype(np.float64))
    nan = np.isnan(want_phi)
    assert np.array_equal(np.isnan(phi), nan) and phi.shape == (N,) and n.shape == (N, 3)
    if (~nan).any():
        assert float(np.abs(phi - want_phi)[~nan].max()) <= 1e-12 and float(np.abs(n - want_n)[~nan].max()) <= 1e-12
    assert same_bits(grid.sample(pts), runs[0][1])
    e_phi, e_n = grid.sample(torch.empty((0, 3), device="cuda"))
    assert e_phi.shape == (0,) and e_n.shape == (0, 3)


def test_from_tsdf_takes_the_fill_when_there_is_one():
    from gaussianmesh_amd.dynamics import SdfGrid
    from gaussianmesh_amd.proxy_mesh import TsdfVolume
    vol = TsdfVolume((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), resolution=8, trunc=0.5)
    dims = (vol.nx, vol.ny, vol.nz)
    t = np.clip(fc.plane_values(dims, vol.origin, vol.voxel, (0.0, 1.0, 0.0), 0.1) / F(0.5), -1.0, 1.0).astype(F)
    w = np.ones_like(t)
    w[:, :, :3] = 0.0                                                  # nobody saw x below -0.25
    vol.tsdf.copy_(torch.as_tensor(t, device="cuda"))
    vol.weight.copy_(torch.as_tensor(w, device="cuda"))
    plain = SdfGrid.from_tsdf(vol)
    assert np.array_equal(_bits(plain.grid.cpu().numpy()), _bits(sg.prepare(t, vol.voxel, w, 1.0, vol.trunc))) and plain.scale == vol.trunc
    vol.fill_holes(4)
    filled = SdfGrid.from_tsdf(vol)
    ft, fw = vol.filled_tsdf.cpu().numpy(), vol.filled_weight.cpu().numpy()
    assert np.array_equal(_bits(filled.grid.cpu().numpy()), _bits(sg.prepare(ft, vol.voxel, fw, 1.0, vol.trunc)))
    assert int(torch.isnan(plain.grid[..., 0]).sum()) > int(torch.isnan(filled.grid[..., 0]).sum())
    assert same_bits(SdfGrid.from_tsdf(vol, use_fill=False).grid, plain.grid)
    assert bool(torch.isnan(SdfGrid.from_tsdf(vol, min_weight=2, use_fill=False).grid).all())
