"""gm_mesh_winding / gm_mesh_signed_distance and mesh_sdf on the device against the numpy restatement (mesh_sdf_ref.py), on the cases of
mesh_sdf_cases.py: 4 .. 2049 faces (below, at and past the 1024-face chunk boundaries, closed, open, wound inwards, with a face
without area), 1 .. 257 points (a lane, around a wave, around a workgroup) and one 9 x 7 x 5 lattice.

w: within 1e-10 of the reference.  Both sides evaluate the same float64 formula on the same float32 inputs and differ in atan2 alone, a
few ulp of pi (about 1e-15) per face, F <= 2049.  The sign, and with it phi, face and closest: bit for bit - after condition() has
shown, on the reference alone, that no sample has |w| within 1e-6 of 0.5 or lies on the surface."""
import numpy as np
import pytest
import torch

from gpu_utils import T, dev
from mesh_sdf_cases import LATTICE, MESHES, SIZES, case, condition
from poison import FILLS, run_under_fills, same_bits

pytestmark = pytest.mark.gpu

W_TOL = 1e-10


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _check(got, ref, n=None):
    """(phi, face, closest, w) from the device against the reference's first n rows"""
    phi, face, close, w = (x.cpu().numpy() for x in got)
    rphi, rface, rclose, rw = (x[:n] for x in ref)
    err = np.abs(w - rw).max()
    print("max |w - w_ref| = %.3g" % err)
    assert w.dtype == np.float64 and err <= W_TOL
    assert np.array_equal(np.abs(w) > 0.5, np.abs(rw) > 0.5)
    assert phi.dtype == np.float32 and np.array_equal(_bits(phi), _bits(rphi))
    assert np.array_equal(face, rface)
    assert np.array_equal(_bits(close), _bits(rclose))


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("name", sorted(MESHES))
def test_points_against_the_reference(name, N):
    from gaussianmesh_amd import mesh_sdf
    from gaussianmesh_amd.mesh_bind import closest_faces
    c = case(name)
    condition(c)
    p = T(c["points"][:N])
    got = mesh_sdf.signed_distances(p, c["v"], c["f"], want_face=True, want_closest=True, want_winding=True)
    _check(got, c["ref"], N)
    d2, face, close = closest_faces(p, c["v"], c["f"], want_closest=True)
    assert same_bits(got[1], face) and same_bits(got[2], close)
    again = mesh_sdf.signed_distances(p, c["v"], c["f"], want_face=True, want_closest=True, want_winding=True)
    assert same_bits(got, again)                                              # two runs: identical bits, w included
    w = mesh_sdf.winding_numbers(p, c["v"], c["f"])
    assert same_bits(w, got[3])                                               # gm_mesh_winding alone: the same chain
    # however the points are batched: a point's w and phi do not depend on its neighbours
    if N > 1:
        k = N // 2 + 1
        parts = [mesh_sdf.signed_distances(q, c["v"], c["f"], want_winding=True) for q in (p[:k], p[k:])]
        assert same_bits(torch.cat([parts[0][0], parts[1][0]]), got[0]) and same_bits(torch.cat([parts[0][1], parts[1][1]]), got[3])
    assert same_bits(mesh_sdf.inside(p, c["v"], c["f"]), got[3].abs() > 0.5)
    assert same_bits(mesh_sdf.signed_distances(p, c["v"], c["f"]), got[0])    # nothing asked for: phi alone, the same bits


@pytest.mark.parametrize("name", sorted(MESHES))
def test_lattice_against_the_reference_and_the_slabs(name):
    from gaussianmesh_amd import mesh_sdf
    c = case(name)
    condition(c)
    nz, ny, nx = LATTICE
    vals = mesh_sdf.grid_values(c["v"], c["f"], c["origin"], c["voxel"], LATTICE, device=dev())
    assert vals.shape == LATTICE and vals.dtype == torch.float32
    pts = mesh_sdf.lattice_points(c["origin"], c["voxel"], LATTICE, 0, nx * ny * nz, dev())
    assert np.array_equal(_bits(pts.cpu().numpy()), _bits(c["lattice_points"]))           # the positions the docstring states
    got = mesh_sdf.signed_distances(pts, c["v"], c["f"], want_face=True, want_closest=True, want_winding=True)
    _check(got, c["lattice_ref"])
    assert same_bits(vals.reshape(-1), got[0])
    for slab in (nx * ny, 64, 1000):                                          # one z-layer a slab; a wave a slab; one slab
        assert same_bits(mesh_sdf.grid_values(c["v"], c["f"], c["origin"], c["voxel"], LATTICE, device=dev(), slab_points=slab), vals), slab


@pytest.mark.parametrize("name,N", [("cube_open", 65), ("torus_1025", 257), ("faces_2049", 256)])
def test_outputs_do_not_depend_on_what_the_buffers_held(name, N):
    from gaussianmesh_amd import mesh_sdf
    c = case(name)
    p, v, f = T(c["points"][:N]), T(c["v"]), T(c["f"], dtype=torch.int32)

    def route():
        return (mesh_sdf.signed_distances(p, v, f, want_face=True, want_closest=True, want_winding=True), mesh_sdf.signed_distances(p, v, f),
                mesh_sdf.winding_numbers(p, v, f), mesh_sdf.grid_values(v, f, c["origin"], c["voxel"], LATTICE, device=dev(), slab_points=100))
    runs = run_under_fills(route)                                             # (a damaged guard band raises out of the run that did it)
    for block, _ in runs:
        assert block.handed_out >= 8, block.handed_out
    for (block, out), fill in zip(runs[1:], FILLS[1:]):
        assert same_bits(runs[0][1], out), "0x%02X" % fill
    _check(runs[0][1][0], c["ref"], N)


def test_no_points_enqueue_nothing():
    from gaussianmesh_amd import _lib, mesh_sdf
    from poison import poisoned
    c = case("cube")
    l = _lib.lib()
    assert l.gm_mesh_winding(0, None, 8, None, 12, None, None, None, 0, None) == 0
    assert l.gm_mesh_signed_distance(0, None, 8, None, 12, None, None, None, None, None, None, 0, None) == 0
    assert l.gm_mesh_winding(0, None, 0, None, 0, None, None, None, 0, None) == 0                  # an empty mesh is no refusal without points
    p = torch.zeros((0, 3), device=dev())
    with poisoned(0xFF) as block:
        got = mesh_sdf.signed_distances(p, c["v"], c["f"], want_face=True, want_closest=True, want_winding=True)
        w, inside = mesh_sdf.winding_numbers(p, c["v"], c["f"]), mesh_sdf.inside(p, c["v"], c["f"])
    assert block.handed_out == 0                                              # no workspace, no output of a positive size
    assert [tuple(x.shape) for x in got] == [(0,), (0,), (0, 3), (0,)] and [x.dtype for x in got] == [torch.float32, torch.int64, torch.float32, torch.float64]
    assert tuple(w.shape) == (0,) and w.dtype == torch.float64 and tuple(inside.shape) == (0,) and inside.dtype == torch.bool
    assert tuple(mesh_sdf.signed_distances(p, c["v"], c["f"][:0]).shape) == (0,)                   # nor is it one in Python


def test_c_refusals():
    """every refusal of the two entry points: GM_ERR_INVALID_ARG and its message, decided on the arguments alone (the pointers are never
    dereferenced: most of them are no pointers)"""
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    N, Vm, F = 100, 8, 12
    one = 1 << 20                                                             # bogus, far apart "pointers"
    base = dict(N=N, points=one, Vm=Vm, vertices=2 * one, F=F, faces=3 * one, out_w=4 * one, workspace=8 * one)

    def winding(**kw):
        a = dict(base, **kw)
        a.setdefault("bytes", l.gm_mesh_winding_workspace_bytes(a["N"], a["F"]))
        return l.gm_mesh_winding(a["N"], a["points"], a["Vm"], a["vertices"], a["F"], a["faces"], a["out_w"], a["workspace"], a["bytes"], None)

    def signed(**kw):
        a = dict(dict(base, out_phi=5 * one, out_face=6 * one, out_closest=7 * one), **kw)
        a.setdefault("bytes", l.gm_mesh_signed_distance_workspace_bytes(a["N"], a["F"]))
        return l.gm_mesh_signed_distance(a["N"], a["points"], a["Vm"], a["vertices"], a["F"], a["faces"], a["out_phi"], a["out_face"], a["out_closest"],
                                         a["out_w"], a["workspace"], a["bytes"], None)

    def refused(fn, who, msg, **kw):
        assert fn(**kw) == 1, (who, kw)                                       # GM_ERR_INVALID_ARG
        err = l.gm_last_error().decode()
        assert err.startswith(who + ": ") and msg in err, (kw, err)

    for fn, who, out in ((winding, "gm_mesh_winding", "out_w"), (signed, "gm_mesh_signed_distance", "out_phi")):
        for bad in (dict(N=-1), dict(Vm=-1), dict(F=-1)):
            refused(fn, who, "negative size", **bad)
        refused(fn, who, "empty mesh", F=0)
        refused(fn, who, "empty mesh", Vm=0)
        refused(fn, who, "too large for one launch", N=2**31 - 1, F=2**20, bytes=0)
        for name in ("points", "vertices", "faces", out, "workspace"):
            refused(fn, who, "null pointer", **{name: None})
        need = (l.gm_mesh_winding_workspace_bytes if fn is winding else l.gm_mesh_signed_distance_workspace_bytes)(N, F)
        refused(fn, who, "workspace too small", bytes=need - 1)
        refused(fn, who, "workspace too small", bytes=0)
        refused(fn, who, out + " overlaps points", **{out: base["points"] + 12 * N - 4})
        refused(fn, who, out + " overlaps workspace", **{out: base["workspace"] + need - 4})
        refused(fn, who, "workspace overlaps vertices", vertices=base["workspace"] + 256)
    refused(signed, "gm_mesh_signed_distance", "out_face overlaps out_closest", out_face=7 * one)
    refused(signed, "gm_mesh_signed_distance", "out_phi overlaps out_w", out_w=5 * one)
    assert signed(out_face=None, out_closest=None, out_w=None, workspace=None) == 1                 # the optional outputs may be NULL, the workspace not
    assert "null pointer" in l.gm_last_error().decode()
    # the sizes: monotonic in both, positive at (0, 0), the signed distance's above the sum of its parts
    wb, sb, cb = l.gm_mesh_winding_workspace_bytes, l.gm_mesh_signed_distance_workspace_bytes, l.gm_closest_face_workspace_bytes
    assert wb(0, 0) > 0 and sb(0, 0) > 0
    assert wb(1000, 1024) >= 48 * 1024 + 8 * 1000 and wb(1000, 1025) >= 48 * 1025 + 16 * 1000 and wb(1000, 1025) - wb(1000, 1024) >= 8000
    for n, f in ((1, 1), (1000, 12), (1000, 5000), (10**6, 120000)):
        assert wb(n + 1, f) >= wb(n, f) and wb(n, f + 1) >= wb(n, f) and sb(n, f) >= wb(n, f) + cb(n, f) + 16 * n
