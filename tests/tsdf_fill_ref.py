"""The definition of gm_tsdf_fill restated in numpy (include/gmesh_hip.h): volumetric diffusion of a signed distance volume into its
unobserved samples (Davis, Marschner, Garr, Levoy 2002).  Every sum and quotient is written out on np.float32 arrays in the header's
order - the centre, then the face neighbours -x, +x, -y, +y, -z, +z, each added only where it counts -, so the arrays below are, bit
for bit, what the device must produce.  Also here: the two holes cut into tsdf_ref.sphere_field that the tests close."""
import numpy as np

import tsdf_ref as tr

f32 = np.float32
ZERO, ONE = f32(0.0), f32(1.0)


def _neighbour(A, axis, step, fill):
    """(A at g + step e_axis, inside): axis 0 = x is the array's last axis; `fill` where the grid has no such sample"""
    ax = 2 - axis
    out = np.full_like(A, fill)
    inside = np.zeros(A.shape, bool)
    dst = [slice(None)] * 3
    src = [slice(None)] * 3
    if step < 0:
        dst[ax], src[ax] = slice(1, None), slice(0, -1)
    else:
        dst[ax], src[ax] = slice(0, -1), slice(1, None)
    out[tuple(dst)] = A[tuple(src)]
    inside[tuple(dst)] = True
    return out, inside


def fill_step(val, known, src, boundary_free):
    """one Jacobi step: (val_{t+1}, known_{t+1}) from (val_t, known_t)"""
    s = np.where(known, val, ZERO)
    c = known.astype(np.int32)
    with np.errstate(all="ignore"):
        for axis in range(3):
            for step in (-1, 1):
                nv, inside = _neighbour(val, axis, step, ZERO)
                nk, _ = _neighbour(known, axis, step, False)
                s = np.where(nk, s + nv, s)
                c = c + nk
                if boundary_free:
                    s = np.where(inside, s, s + ONE)
                    c = c + ~inside
        upd = ~src & (c > 0)
        q = s / np.maximum(c, 1).astype(f32)
    assert s.dtype == f32 and q.dtype == f32
    return np.where(upd, q, val), known | upd


def fill_ref(tsdf, weight, min_weight=1.0, iterations=0, boundary_free=False, fill_weight=None):
    """(tsdf_out, weight_out float32 [nz,ny,nx], counts [filled, still unknown]) of gm_tsdf_fill"""
    D, W = np.asarray(tsdf, f32), np.asarray(weight, f32)
    fill_weight = f32(min_weight if fill_weight is None else fill_weight)
    with np.errstate(invalid="ignore"):
        src = W >= f32(min_weight)                                   # a NaN weight: false
    val, known = np.where(src, D, ZERO), src.copy()
    for _ in range(int(iterations)):
        val, known = fill_step(val, known, src, bool(boundary_free))
    weight_out = np.where(src, W, np.where(known, fill_weight, ZERO))
    counts = np.array([int((known & ~src).sum()), int((~known).sum())], np.int32)
    return val, weight_out, counts


# ---- the holes of the tests: tsdf_ref.sphere_field((24, 24, 24)) with samples set back to unobserved (indices [z, y, x]) ----
HOLE_A_ITERATIONS = 8
HOLE_B_ITERATIONS = 32


def hole_a(interior=False):
    """a box around the south cap that does not reach the grid's sides; interior: the samples deep inside (D < -1) are unobserved too, as
    a real fusion leaves them"""
    tsdf, w, origin, voxel = tr.sphere_field((24, 24, 24))
    w[2:9, 6:18, 6:18] = 0
    if interior:
        w[tsdf < -1] = 0
    return tsdf, w, origin, voxel


def hole_b():
    """a slab that reaches the grid's bottom: it closes only when the samples beyond the grid count as free space"""
    tsdf, w, origin, voxel = tr.sphere_field((24, 24, 24))
    w[:8] = 0
    return tsdf, w, origin, voxel


def mesh_facts(tsdf, weight, origin, voxel, min_weight=1.0):
    """what the closure tests look at: surface_nets_ref's mesh and its border edges, closedness, Euler characteristic, components, volume"""
    V, F = tr.surface_nets_ref(tsdf, weight, origin, voxel, min_weight)
    return dict(V=V, F=F, border=tr.boundary_edges(F), closed=tr.is_closed(F), chi=tr.euler_characteristic(len(V), F),
                components=tr.n_components(len(V), F), volume=tr.signed_volume(V, F))
