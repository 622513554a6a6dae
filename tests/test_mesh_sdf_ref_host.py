"""The numpy restatement of the winding number and the signed distance (mesh_sdf_ref.py) against closed forms, and every refusal of
mesh_sdf, SdfGrid.from_mesh and the edit_sequence obstacle flags that is decided before a device is needed.  No GPU."""
import numpy as np
import pytest
import torch

from mesh_sdf_ref import cube, face_omega, signed_distance_ref, tetrahedron, winding_ref

INSIDE_CUBE = np.array([[0.0, 0.0, 0.0], [0.3, -0.2, 0.1], [-0.45, 0.45, 0.4], [0.49, 0.0, 0.0]], np.float32)
OUTSIDE_CUBE = np.array([[0.0, 0.0, 0.6], [2.0, 1.0, -3.0], [-0.51, 0.0, 0.0], [0.7, 0.7, 0.7], [0.0, 0.0, 100.0]], np.float32)


def test_closed_cube_and_tetrahedron_are_one_inside_and_zero_outside():
    v, f = cube()
    assert np.abs(winding_ref(INSIDE_CUBE, v, f) - 1.0).max() < 1e-12
    assert np.abs(winding_ref(OUTSIDE_CUBE, v, f)).max() < 1e-12
    v, f = tetrahedron()
    inside = np.array([[0.1, 0.1, 0.1], [0.25, 0.25, 0.25], [0.01, 0.9, 0.01]], np.float32)
    outside = np.array([[0.4, 0.4, 0.4], [-0.1, 0.2, 0.2], [1.0, 1.0, 1.0], [0.2, 0.2, -5.0]], np.float32)
    assert np.abs(winding_ref(inside, v, f) - 1.0).max() < 1e-12
    assert np.abs(winding_ref(outside, v, f)).max() < 1e-12


def test_one_side_of_a_cube_subtends_a_sixth_from_the_centre():
    v, f = cube()
    for side in range(6):
        w = winding_ref(np.zeros((1, 3), np.float32), v, f[2 * side:2 * side + 2])
        assert abs(w[0] - 1.0 / 6.0) < 1e-12, (side, w)


def test_a_cube_wound_inwards_is_minus_one_and_as_solid():
    v, f = cube()
    g = f[:, ::-1].copy()
    pts = np.concatenate([INSIDE_CUBE, OUTSIDE_CUBE])
    assert np.abs(winding_ref(INSIDE_CUBE, v, g) + 1.0).max() < 1e-12
    assert np.abs(winding_ref(OUTSIDE_CUBE, v, g)).max() < 1e-12
    phi, phi_in = signed_distance_ref(pts, v, f)[0], signed_distance_ref(pts, v, g)[0]
    assert phi.dtype == np.float32 and np.array_equal(phi.view(np.uint32), phi_in.view(np.uint32))
    assert (phi[:len(INSIDE_CUBE)] < 0).all() and (phi[len(INSIDE_CUBE):] > 0).all()
    assert phi[0] == np.float32(-0.5) and abs(phi[len(INSIDE_CUBE)] - 0.1) < 1e-6 and abs(phi[3] + 0.01) < 1e-6


def test_a_point_on_a_vertex_and_a_face_without_area_contribute_nothing():
    v, f = cube()
    p = v[5:6]                                                  # a corner of the cube: zero for the six faces at it
    at = [k for k in range(len(f)) if 5 in f[k]]
    om = face_omega(p[:, None, :], v[f[at, 0]][None], v[f[at, 1]][None], v[f[at, 2]][None])
    assert om.shape == (1, len(at)) and (om == 0.0).all()
    flat = np.array([[0, 3, 3], [6, 6, 6], [2, 2, 5]], np.int32)           # two or three equal corners
    pts = np.concatenate([INSIDE_CUBE, OUTSIDE_CUBE])
    A, B, C = v[flat[:, 0]][None], v[flat[:, 1]][None], v[flat[:, 2]][None]
    assert (face_omega(pts[:, None, :], A, B, C)[:, :2] == 0.0).all()       # b == c: b cross c is exactly zero
    assert np.abs(face_omega(pts[:, None, :], A, B, C)).max() < 1e-12
    w0, w1 = winding_ref(pts, v, f), winding_ref(pts, v, np.concatenate([f, flat]))
    assert np.abs(w0 - w1).max() < 1e-12
    phi0, phi1 = signed_distance_ref(pts, v, f)[0], signed_distance_ref(pts, v, np.concatenate([f, flat]))[0]
    assert np.array_equal(phi0.view(np.uint32), phi1.view(np.uint32))


def test_the_chunked_order_is_the_definition():
    """1025 faces: the last one is a chunk of its own; the sum is not simply left to right"""
    rng = np.random.default_rng(3)
    v = rng.normal(size=(200, 3)).astype(np.float32)
    f = rng.integers(0, 200, size=(1025, 3)).astype(np.int32)
    p = rng.normal(size=(5, 3)).astype(np.float32) * 3
    om = face_omega(p[:, None, :], v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None])
    want = np.zeros(5)
    for j in range(1024):
        want = want + om[:, j]
    want = (0.0 + want) + (0.0 + om[:, 1024])
    assert np.array_equal(winding_ref(p, v, f), want / (4.0 * np.pi))
    assert np.array_equal(winding_ref(p, v, f, rows=2), winding_ref(p, v, f, rows=5))


def test_python_refusals_fire_before_a_device_is_needed():
    from gaussianmesh_amd import mesh_sdf
    from gaussianmesh_amd._lib import GmeshError
    from gaussianmesh_amd.dynamics import SdfGrid
    v, f = cube()
    p = torch.zeros(4, 3)
    for fn in (mesh_sdf.winding_numbers, mesh_sdf.signed_distances, mesh_sdf.inside):
        with pytest.raises(ValueError, match="points must be a \\[N,3\\] tensor"):
            fn(np.zeros((4, 3), np.float32), v, f)
        with pytest.raises(ValueError, match="points must be a \\[N,3\\] tensor"):
            fn(torch.zeros(4, 2), v, f)
        with pytest.raises(ValueError, match="vertices must be \\[Vm,3\\] and faces \\[F,3\\]"):
            fn(p, v[:, :2], f)
        with pytest.raises(ValueError, match="integer vertex ids"):
            fn(p, v, f.astype(np.float32))
        with pytest.raises(ValueError, match="face index outside"):
            fn(p, v, f + 1)
        with pytest.raises(ValueError, match="the mesh is empty"):
            fn(p, v, f[:0])
        with pytest.raises(GmeshError, match="no CPU path"):                 # everything else is in order: only the device is missing
            fn(p, v, f)
    grid = lambda **kw: mesh_sdf.grid_values(**dict(dict(vertices=v, faces=f, origin=(-1.0, -1.0, -1.0), voxel=0.25, shape=(8, 8, 8), device="cpu"), **kw))
    for bad, match in ((dict(faces=f + 1), "face index outside"), (dict(faces=f[:0]), "the mesh is empty"), (dict(shape=(8, 8)), "shape must be"),
                       (dict(shape=(8, 0, 8)), "shape must be"), (dict(shape=(8, 8.0, 8)), "shape must be"), (dict(shape=(1024, 1024, 1024)), "2\\^28"),
                       (dict(origin=(0.0, 0.0)), "origin must be"), (dict(origin=(0.0, np.nan, 0.0)), "origin must be"), (dict(voxel=0.0), "voxel ="),
                       (dict(voxel=-1.0), "voxel ="), (dict(voxel=float("inf")), "voxel ="), (dict(voxel=1e-60), "voxel ="), (dict(voxel="1"), "voxel ="),
                       (dict(slab_points=0), "slab_points ="), (dict(slab_points=2.5), "slab_points =")):
        with pytest.raises(ValueError, match=match):
            grid(**bad)
    with pytest.raises(GmeshError, match="no CPU path"):
        grid()
    mesh = lambda **kw: SdfGrid.from_mesh(**dict(dict(vertices=v, faces=f, resolution=8, device="cpu"), **kw))
    for bad, match in ((dict(faces=f + 1), "face index outside"), (dict(faces=f[:0]), "the mesh is empty"), (dict(vertices=v * np.float32(np.nan)), "finite"),
                       (dict(resolution=1), "resolution ="), (dict(resolution=8.0), "resolution ="), (dict(resolution=True), "resolution ="),
                       (dict(margin=-0.1), "margin ="), (dict(margin=float("inf")), "margin ="), (dict(margin="a"), "margin ="),
                       (dict(bounds=((0, 0, 0), (1, 1, 0))), "bounds must be"), (dict(bounds=((0, 0, 0),)), "bounds must be"),
                       (dict(bounds=((0, 0, 0), (1, np.inf, 1))), "bounds must be"), (dict(bounds=((0, 0), (1, 1))), "bounds must be")):
        with pytest.raises(ValueError, match=match):
            mesh(**bad)
    with pytest.raises(GmeshError, match="no CPU path"):
        mesh()


def test_box_lattice_follows_background_fields_rules():
    from gaussianmesh_amd.mesh_sdf import box_lattice
    origin, voxel, shape = box_lattice("t", [0.0, 0.0, 0.0], [2.0, 1.0, 0.5], 16, None, 0.5)
    assert np.array_equal(origin, [-1.0, -1.0, -1.0]) and voxel == 4.0 / 16 and shape == (10, 12, 16)       # sides 4, 3, 2.5 -> 16, 12, 10 voxels
    origin, voxel, shape = box_lattice("t", None, None, 10, ((0.0, 0.0, 0.0), (1.0, 0.05, 0.5)), 0.5)
    assert np.array_equal(origin, [0.0, 0.0, 0.0]) and voxel == 0.1 and shape == (5, 2, 10)                  # at least two samples a side


CLI = ["--object_gaussian", "g.ply", "--object_origin_mesh", "m.obj", "--handle_sequence", "h.npz", "--camera_path", "c", "--render_path", "r"]


@pytest.mark.parametrize("extra,match", [
    (["--obstacle_mesh", "o.obj"], "--obstacle_mesh sets what the simulated mesh collides with and needs --dynamics"),
    (["--dynamics", "--obstacle_mesh", "o.obj", "--background_gaussian", "b.ply", "--background_contact"], "a simulation takes one volume"),
    (["--dynamics", "--obstacle_resolution", "32"], "--obstacle_resolution shapes the volume of --obstacle_mesh"),
    (["--dynamics", "--obstacle_margin", "0.25"], "--obstacle_margin shapes the volume of --obstacle_mesh"),
    (["--dynamics", "--obstacle_mesh", __file__, "--obstacle_resolution", "1"], "--obstacle_resolution 1"),
    (["--dynamics", "--obstacle_mesh", __file__, "--obstacle_margin", "-1"], "--obstacle_margin -1.0"),
    (["--dynamics", "--obstacle_mesh", "/nowhere/o.obj"], "no such file"),
    (["--dynamics", "--friction", "0.5"], "--friction is the friction of"),                       # as before: friction still needs a collider
])
def test_cli_refusals(extra, match):
    from gaussianmesh_amd import edit_sequence
    with pytest.raises(SystemExit, match=match):
        edit_sequence.main(CLI + extra)
