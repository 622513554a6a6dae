"""Hole filling on the host: gm_tsdf_fill's two entry points are exported, in sync with the header, and refuse bad arguments before any
GPU work; the numpy definition (tests/tsdf_fill_ref.py) keeps its sources, reaches exactly as far as its iteration count, and closes
the two holes cut into the analytic sphere - border edges, closedness, Euler characteristic, components, volume, all through
tsdf_ref.surface_nets_ref; the Python surface has no CPU path."""
import functools
import os
import re

import numpy as np
import pytest

import tsdf_fill_ref as fr
import tsdf_ref as tr

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- 1. the ABI ----
def test_entry_points_are_declared_typed_and_in_sync():
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    names = _lib.header_symbols()
    txt = open(_lib.HEADER).read()
    for name, ret, n in (("gm_tsdf_fill_workspace_bytes", "size_t", 3), ("gm_tsdf_fill", "int", 15)):
        assert name in names and name in _lib.SIGNATURES and hasattr(l, name), name
        m = re.search(r"\b%s\s+%s\(([^)]*)\);" % (ret, name), txt)
        assert m and len(m.group(1).split(",")) == n == len(_lib.SIGNATURES[name][1]), name
    assert set(names) == set(_lib.SIGNATURES)
    assert l.gm_abi_version() == 3 and "#define GM_ABI_VERSION 3" in txt
    assert "gm_tsdf_fill.hip" in open(os.path.join(_lib.CSRC, "Makefile")).read()


def test_unit_neither_waits_nor_allocates():
    from gaussianmesh_amd import _lib
    src = open(os.path.join(_lib.CSRC, "gm_tsdf_fill.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("hipMalloc", "hipFree", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy", "while (atomic", "__threadfence"):
        assert word not in code, word
    assert "#pragma clang fp contract(off)" in code


def test_workspace_query_is_monotonic_and_positive():
    from gaussianmesh_amd import _lib
    q = _lib.lib().gm_tsdf_fill_workspace_bytes
    assert q(2, 2, 2) > 0 and q(0, 0, 0) == q(2, 2, 2) and q(-5, 2, 2) == q(2, 2, 2)
    sizes = [2, 3, 5, 16, 17, 31, 32, 33, 64, 65, 128, 300]
    for a, b in zip(sizes, sizes[1:]):
        assert q(a, a, a) <= q(b, b, b) and q(a, 7, 9) <= q(b, 7, 9) and q(7, a, 9) <= q(7, b, 9) and q(7, 9, a) <= q(7, 9, b)
    assert 6 * 128 ** 3 < q(128, 128, 128) < 6.1 * 128 ** 3          # a second value array, two state bytes a sample, a byte a brick


def test_fill_refuses_before_any_gpu_work():
    """bogus non-null "pointers": every refusal is decided on the arguments alone - nothing is dereferenced, no device is touched"""
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    M = 1 << 24
    need = l.gm_tsdf_fill_workspace_bytes(4, 4, 4)
    def call(n=(4, 4, 4), tsdf=1 * M, weight=2 * M, min_weight=1.0, iterations=3, free=0, fill_weight=1.0, out_t=3 * M, out_w=4 * M, counts=5 * M,
             ws=6 * M, ws_bytes=need):
        return l.gm_tsdf_fill(n[0], n[1], n[2], tsdf, weight, min_weight, iterations, free, fill_weight, out_t, out_w, counts, ws, ws_bytes, None)
    err = lambda: l.gm_last_error()
    for n in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4), (4, -2, 4)):
        assert call(n=n) == 1 and b"at least 2" in err(), n
    assert call(n=(1 << 10, 1 << 10, 1 << 9)) == 1 and b"2^28" in err()
    assert call(n=(1 << 16, 1 << 16, 1 << 16)) == 1 and b"2^28" in err()
    assert call(iterations=-1) == 1 and b"iterations" in err()
    assert call(min_weight=float("nan")) == 1 and b"NaN" in err()
    assert call(fill_weight=float("nan")) == 1 and b"NaN" in err()
    for k in ("tsdf", "weight", "out_t", "out_w", "ws"):
        assert call(**{k: None}) == 1 and b"null pointer" in err(), k
    # an output is neither input, nor the other output (equal, or sharing a sample)
    assert call(out_t=1 * M) == 1 and b"tsdf_in overlaps tsdf_out" in err()
    assert call(out_w=1 * M) == 1 and b"tsdf_in overlaps weight_out" in err()
    assert call(out_t=2 * M) == 1 and b"weight_in overlaps tsdf_out" in err()
    assert call(out_w=2 * M) == 1 and b"weight_in overlaps weight_out" in err()
    assert call(out_w=3 * M) == 1 and b"tsdf_out overlaps weight_out" in err()
    assert call(out_t=1 * M + 4 * 63) == 1 and b"tsdf_in overlaps tsdf_out" in err()        # the last sample of the input
    assert call(out_w=3 * M - 4 * 63) == 1 and b"tsdf_out overlaps weight_out" in err()
    assert call(counts=4 * M + 4 * 63) == 1 and b"weight_out overlaps out_counts" in err()
    assert call(ws=2 * M - need + 1) == 1 and b"weight_in overlaps workspace" in err()
    assert call(ws=5 * M + 7) == 1 and b"out_counts overlaps workspace" in err()
    # an undersized workspace: GM_ERR_BUFFER, still before any GPU work
    assert call(ws_bytes=need - 1) == 3 and b"workspace too small" in err()
    assert call(ws_bytes=0) == 3
    assert call(counts=None, ws_bytes=need - 1) == 3                                        # out_counts may be NULL: this got past the pointer checks
    assert call(weight=1 * M, ws_bytes=need - 1) == 3                                       # the inputs may be one buffer


# ---- 2. the reference ----
def test_sources_keep_their_bits_at_any_iteration_count():
    tsdf, w, _, _ = tr.noise_field((9, 8, 7), seed=3, observed=0.5)
    tsdf[1, 2, 3], tsdf[4, 4, 4] = f32(-0.0), f32(np.inf)
    src = w >= 1
    for free in (False, True):
        for n in (0, 1, 2, 5, 12):
            D, W, counts = fr.fill_ref(tsdf, w, 1.0, n, free, 2.5)
            assert np.array_equal(_bits(D[src]), _bits(tsdf[src])) and np.array_equal(_bits(W[src]), _bits(w[src])), (free, n)
            assert set(np.unique(W[~src])) <= {f32(0), f32(2.5)} and counts.tolist() == [int((W[~src] == 2.5).sum()), int((W == 0).sum())]
            if n == 0:
                assert (D[~src] == 0).all() and not np.signbit(D[~src]).any() and counts.tolist() == [0, int((~src).sum())]
    assert counts[1] == 0                                             # twelve steps reach every sample of this grid


def test_reach_is_the_l1_ball():
    n = (9, 7, 6)
    tsdf, w = np.zeros(n[::-1], f32), np.zeros(n[::-1], f32)
    tsdf[0, 0, 0], w[0, 0, 0] = f32(-0.375), 1
    iz, iy, ix = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    for r in (0, 1, 2, 3, 7, 19, 20):
        D, W, counts = fr.fill_ref(tsdf, w, 1.0, r, False)
        ball = ix + iy + iz <= r
        assert np.array_equal(W == 1, ball), r
        assert counts.tolist() == [int(ball.sum()) - 1, int((~ball).sum())]
        assert (D[ball] < 0).all() and (D[~ball] == 0).all()         # averages of one negative number; the rest still +0
    assert counts[1] == 0 and 8 + 6 + 5 == 19                        # the far corner is 19 steps away


def test_all_unknown_and_all_known_volumes():
    n = (7, 5, 4)
    zero = np.zeros(n[::-1], f32)
    tsdf = np.random.default_rng(1).uniform(-1, 1, size=n[::-1]).astype(f32)
    # nothing known, free space outside: the boundary's ones diffuse inwards, and k ones sum to k exactly - 1.0f everywhere
    D, W, counts = fr.fill_ref(tsdf, zero, 1.0, 4, True, 3.0)
    assert np.array_equal(_bits(D), _bits(np.ones_like(zero))) and (W == 3).all() and counts.tolist() == [7 * 5 * 4, 0]
    D, W, counts = fr.fill_ref(tsdf, zero, 1.0, 1, True)
    assert counts.tolist() == [7 * 5 * 4 - 5 * 3 * 2, 5 * 3 * 2]      # one step: the outer layer
    # without it the volume stays unknown: +0, weight 0
    D, W, counts = fr.fill_ref(tsdf, zero, 1.0, 9, False)
    assert np.array_equal(_bits(D), _bits(zero)) and np.array_equal(_bits(W), _bits(zero)) and counts.tolist() == [0, 7 * 5 * 4]
    # everything known: returned bit for bit, whatever the mode
    w = np.full(n[::-1], f32(2))
    for free in (False, True):
        D, W, counts = fr.fill_ref(tsdf, w, 1.0, 5, free, 7.0)
        assert np.array_equal(_bits(D), _bits(tsdf)) and np.array_equal(_bits(W), _bits(w)) and counts.tolist() == [0, 0]
    # min_weight is a threshold on the weight itself, and a NaN weight is no source
    w[1, 2, 3], w[2, 2, 2] = np.nan, 1
    D, W, counts = fr.fill_ref(tsdf, w, 2.0, 1, False)
    assert counts.tolist() == [2, 0] and W[1, 2, 3] == 2 and W[2, 2, 2] == 2 and D[1, 2, 3] != tsdf[1, 2, 3]


@functools.lru_cache(maxsize=None)
def _facts(hole, iterations, free):
    fld = {"A": fr.hole_a, "A+": lambda: fr.hole_a(interior=True), "B": fr.hole_b, "full": lambda: tr.sphere_field((24, 24, 24))}[hole]()
    D, W, counts = fr.fill_ref(fld[0], fld[1], 1.0, iterations, free)
    return dict(fr.mesh_facts(D, W, fld[2], fld[3]), counts=counts.tolist(), weight=fld[1])


def test_hole_a_closes_without_the_boundary():
    """a box around the south cap: 80 border edges without a fill; four steps reach every sample of it and the mesh is closed; at the
    pinned eight the cap has settled further (the volume still grows towards the full sphere's)"""
    full, open_ = _facts("full", 0, False), _facts("A", 0, False)
    assert full["border"] == 0 and full["closed"] and full["chi"] == 2 and abs(full["volume"] - 1.476) < 5e-4
    assert open_["border"] == 80 and not open_["closed"] and open_["chi"] == 1 and open_["components"] == 1 and abs(open_["volume"] - 1.105) < 5e-4
    assert open_["counts"] == [0, 7 * 12 * 12]
    assert [_facts("A", n, False)["border"] for n in (1, 2, 3)] == [64, 44, 32]          # closing in, one layer a step
    assert fr.HOLE_A_ITERATIONS == 8
    for n in (4, 8):
        m = _facts("A", n, False)
        assert m["border"] == 0 and m["closed"] and m["chi"] == 2 and m["components"] == 1 and m["counts"] == [7 * 12 * 12, 0], n
        assert open_["volume"] < m["volume"] < full["volume"], n
    assert abs(_facts("A", 8, False)["volume"] - 1.411) < 5e-4 and _facts("A", 4, False)["volume"] < _facts("A", 8, False)["volume"]
    # the boundary mode changes nothing about a hole that does not reach the grid's sides ... but the samples known beside it
    assert _facts("A", 8, True)["closed"]


def test_hole_a_closes_with_the_interior_unobserved_too():
    """what a real fusion leaves: no view sees further than trunc behind the surface"""
    w = _facts("A+", 0, False)["weight"]
    assert (w == 0).sum() == 1650 > 7 * 12 * 12
    assert _facts("A+", 0, False)["border"] == 80
    assert _facts("A+", 4, False)["border"] == 24 and _facts("A+", 4, False)["counts"] == [1577, 73]      # four steps do not reach the middle
    m = _facts("A+", 8, False)
    assert m["border"] == 0 and m["closed"] and m["chi"] == 2 and m["components"] == 1 and m["counts"] == [1650, 0]
    assert abs(m["volume"] - 1.350) < 5e-4 and _facts("A", 0, False)["volume"] < m["volume"] < _facts("full", 0, False)["volume"]


def test_hole_b_needs_free_space_beyond_the_grid():
    """a slab that reaches the grid's bottom: diffusion alone carries the inside values down to the side and the mesh stays open there;
    with the samples beyond the grid as free space it closes inside the grid"""
    assert fr.HOLE_B_ITERATIONS == 32
    open_ = _facts("B", 0, False)
    assert open_["border"] == 60 and not open_["closed"] and open_["counts"] == [0, 8 * 24 * 24]
    absent = _facts("B", 32, False)
    assert absent["border"] == 56 and not absent["closed"] and absent["counts"] == [8 * 24 * 24, 0]
    free = _facts("B", 32, True)
    assert free["border"] == 0 and free["closed"] and free["chi"] == 2 and free["components"] == 1 and free["counts"] == [8 * 24 * 24, 0]
    assert abs(free["volume"] - 1.489) < 5e-4


# ---- 3. the Python surface ----
def test_no_cpu_path_and_bad_boundaries():
    from gaussianmesh_amd._lib import GmeshError
    from gaussianmesh_amd import proxy_mesh as pm
    vol = object.__new__(pm.TsdfVolume)                              # the methods' own checks, on a volume that could not be built here
    with pytest.raises(GmeshError):
        pm.TsdfVolume.fill_holes(vol)
    with pytest.raises(GmeshError):
        pm.TsdfVolume.fill_holes(vol, iterations=4, boundary="free")
    with pytest.raises(GmeshError):
        pm.TsdfVolume.extract(vol, fill_holes=8)
    with pytest.raises(GmeshError):
        pm.TsdfVolume.extract(vol, fill_holes=True, fill_boundary="free")
    with pytest.raises(ValueError):
        pm.TsdfVolume.fill_holes(vol, boundary="open")
    with pytest.raises(ValueError):
        pm.TsdfVolume.extract(vol, fill_holes=8, fill_boundary="closed")
