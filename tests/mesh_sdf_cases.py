"""The meshes, points and lattices of test_gpu_mesh_sdf.py, and their references (mesh_sdf_ref.py), each computed once.  The inputs are
chosen so that no sample lies on a surface: condition() is asserted on the reference alone before anything is compared."""
import functools

import numpy as np

from mesh_sdf_ref import cube, lattice_points_ref, merged, signed_distance_ref, tetrahedron

SIZES = (1, 63, 64, 65, 256, 257)             # a lane, a wave minus / exactly / plus one, a workgroup, a workgroup plus one
LATTICE = (5, 7, 9)                           # (nz, ny, nx)


def _torus():
    from gaussianmesh_amd.scenes import torus_mesh
    v, f = torus_mesh(32, 16, R=1.0, r=0.35)
    return v.astype(np.float32), f


def _torus_minus_one():
    v, f = _torus()
    return v, np.delete(f, 517, axis=0)


def _torus_plus_flat():
    v, f = _torus()
    return v, np.concatenate([f, np.array([[3, 40, 40]], np.int32)])


def _two_cubes():
    return merged(cube(), cube((1.0, -0.25, -0.5), (1.75, 0.5, 0.25)))


def _two_tori_and_a_triangle():
    """2049 faces: past the second chunk boundary; the last face is a free-standing triangle, where w is no integer"""
    v, f = _torus()
    w = (v * np.float32(0.4) + np.array([0.0, 1.5, 0.0], np.float32)).astype(np.float32)
    tri = (np.array([[2.0, 0.0, 0.0], [2.0, 1.0, 0.0], [2.0, 0.0, 1.0]], np.float32), np.array([[0, 1, 2]], np.int32))
    return merged((v, f), (w, f), tri)


MESHES = {
    "tetrahedron": tetrahedron,
    "cube": cube,
    "cube_inwards": lambda: (cube()[0], cube()[1][:, ::-1].copy()),
    "cube_open": lambda: (cube()[0], cube()[1][2:]),                  # the -x side removed
    "two_cubes": _two_cubes,
    "torus_1024": _torus,
    "torus_1023": _torus_minus_one,
    "torus_1025": _torus_plus_flat,
    "faces_2049": _two_tori_and_a_triangle,
}
FACES = {"tetrahedron": 4, "cube": 12, "cube_inwards": 12, "cube_open": 10, "two_cubes": 24, "torus_1024": 1024, "torus_1023": 1023,
         "torus_1025": 1025, "faces_2049": 2049}


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(v, f, points float32 [257,3] in a box 1.5 times the mesh's, origin / voxel of the 9 x 7 x 5 lattice over that box,
    ref = (phi, face, closest, w) of the points, lattice_ref = the same of the lattice's samples); read-only arrays"""
    v, f = MESHES[name]()
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    assert len(f) == FACES[name]
    rng = np.random.default_rng(100 + sorted(MESHES).index(name))
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    mid, half = 0.5 * (lo + hi), 0.75 * (hi - lo)
    points = (mid + half * rng.uniform(-1.0, 1.0, size=(max(SIZES), 3))).astype(np.float32)
    nz, ny, nx = LATTICE
    voxel = float(np.float32((2.0 * half / np.array([nx, ny, nz])).max()))
    origin = mid - 0.5 * voxel * np.array([nx, ny, nz]) + 0.0137 * voxel
    c = dict(v=v, f=f, points=points, origin=origin, voxel=voxel, ref=signed_distance_ref(points, v, f),
             lattice_points=lattice_points_ref(origin, voxel, LATTICE))
    c["lattice_ref"] = signed_distance_ref(c["lattice_points"], v, f)
    for a in [c["v"], c["f"], c["points"], c["lattice_points"], *c["ref"], *c["lattice_ref"]]:
        a.setflags(write=False)
    return c


def condition(c):
    """no sample of the case on a surface, none where the sign is undecided: a condition on the inputs, not a tolerance"""
    for phi, face, close, w in (c["ref"], c["lattice_ref"]):
        assert np.isfinite(w).all() and (np.abs(np.abs(w) - 0.5) > 1e-6).all()
        assert (face >= 0).all() and np.isfinite(phi).all() and (phi != 0).all()
