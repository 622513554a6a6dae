"""-m gpu: a triangle mesh as the field of MeshDynamics (dynamics.SdfGrid.from_mesh over mesh_sdf.grid_values): the grid against the numpy
restatement's (mesh_sdf_ref.py) bit for bit, a sheet on a box's top against the closed forms of dynamics_contact_cases, a torus dropped
onto a box against the float64 reference of dynamics_field_ref.py fed the restatement's grid, and the edit surface on top of it
(SceneVisualTool.object_field, edit_sequence --obstacle_mesh)."""
import functools
import os

import numpy as np
import pytest
import torch

import dynamics_cases as dc
import dynamics_contact_cases as cc
import dynamics_field_cases as fc
import dynamics_field_ref as fr
import mesh_sdf_ref as mr
import sdf_grid_ref as sg
from poison import same_bits
from test_gpu_arap import _drags, _scene64
from test_gpu_dynamics import _cli
from test_gpu_edittool import _write_scene

pytestmark = pytest.mark.gpu
TIGHT = dict(cg_iterations=fc.TIGHT[0], cg_tolerance=fc.TIGHT[1])


def _dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


def _bounds(grid):
    """(min, max) of a lattice given as dynamics_field_cases gives it: ((nx, ny, nz), origin, voxel)"""
    dims, origin, voxel = grid
    lo = np.asarray(origin, np.float64)
    return lo, lo + np.asarray(dims, np.float64) * voxel


# a box under the free torus of dynamics_cases, its top at dynamics_field_cases' ground, on that file's lattice for the torus; and a wide
# box whose top is the plane y = 0 under the 25-vertex sheet, on that file's lattice for the sheets
TORUS_BOX = mr.cube((-3.2, -2.0, -3.2), (3.2, fc.GROUND, 3.2))
SHEET_BOX = mr.cube((-2.0, -1.0, -2.0), (2.0, 0.0, 2.0))


@functools.lru_cache(maxsize=None)
def _reference_values(which):
    """(values float32 [nz,ny,nx] of the numpy restatement, origin float32 [3], voxel as float32) on the lattice from_mesh derives from the
    bounds - after the condition of test_gpu_mesh_sdf.py: no sample on the surface, none with |w| within 1e-6 of 0.5"""
    from gaussianmesh_amd.mesh_sdf import box_lattice
    (v, f), grid = {"torus": (TORUS_BOX, fc.TORUS_GRID), "sheet": (SHEET_BOX, fc.SHEET_GRID)}[which]
    origin, voxel, shape = box_lattice("test", None, None, max(grid[0]), _bounds(grid), 0.5)
    assert shape == grid[0][::-1] and float(np.float32(voxel)) == float(np.float32(grid[2])) and np.array_equal(origin.astype(np.float32), np.asarray(grid[1], np.float32))
    phi, face, _, w = mr.signed_distance_ref(mr.lattice_points_ref(origin, voxel, shape), v, f)
    assert (np.abs(np.abs(w) - 0.5) > 1e-6).all() and (phi != 0).all() and (face >= 0).all()
    assert (phi < 0).sum() > 100 and (phi > 0).sum() > 100
    return phi.reshape(shape), origin.astype(np.float32), float(np.float32(voxel))


def _from_mesh(which):
    from gaussianmesh_amd.dynamics import SdfGrid
    (v, f), grid = {"torus": (TORUS_BOX, fc.TORUS_GRID), "sheet": (SHEET_BOX, fc.SHEET_GRID)}[which]
    return SdfGrid.from_mesh(v, f, resolution=max(grid[0]), bounds=_bounds(grid))


def _torus_dynamics(field, friction=0.3, material=(50.0, dc.GRAVITY, 0.2)):
    from gaussianmesh_amd.dynamics import MeshDynamics
    c = dc.case("free_torus")
    k, g, d = material
    return MeshDynamics(c["V0"], c["faces"], mass=c["mass"], stiffness=k, gravity=g, damping=d, dt=fc.DT, iterations=fc.ITERATIONS, contact_stiffness=fc.KC,
                        field=field, field_friction=friction, **TIGHT)


def test_from_mesh_is_the_restatements_grid_and_so_is_the_motion():
    """SdfGrid.from_mesh(box) holds, bit for bit, what SdfGrid(values of the numpy restatement) holds - and what sdf_grid_ref.prepare makes
    of them - so MeshDynamics(field=) moves the torus to the same bits over either"""
    from gaussianmesh_amd.dynamics import SdfGrid
    values, origin, voxel = _reference_values("torus")
    a, b = _from_mesh("torus"), SdfGrid(values, origin, voxel)
    assert (a.nx, a.ny, a.nz) == (b.nx, b.ny, b.nz) == fc.TORUS_GRID[0] and a.voxel == b.voxel and np.array_equal(a.origin, b.origin)
    assert same_bits(a.grid, b.grid) and np.array_equal(a.grid.cpu().numpy().view(np.uint32), sg.prepare(values, voxel).view(np.uint32))
    assert not bool(torch.isnan(a.grid).any())                                # every sample of a mesh's grid is known
    ma, mb = _torus_dynamics(a), _torus_dynamics(b)
    got, want = ma.run(fc.STEPS, want_contacts=True, want_stats=True), mb.run(fc.STEPS, want_contacts=True, want_stats=True)
    assert same_bits(got, want) and same_bits(ma.velocities, mb.velocities) and int((got[1] == 1).sum()) > 50


def test_a_torus_dropped_onto_a_box_against_the_reference():
    """the stiff torus of dynamics_cases dropped onto the box against dynamics_field_ref.FieldDynamics over the restatement's grid:
    section AA's bounds, max |X - X_ref| <= 1e-6 and max |v - v_ref| <= 1e-6 / dt, and contact_out equal to the reference's active set on
    the rows test_gpu_dynamics_field.py holds a device to (all but those within 1e-5 of the surface or of where the field stops being
    known, where the last bit of an iterate decides)"""
    values, origin, voxel = _reference_values("torus")
    c = dc.case("free_torus")
    k, g, d = material = (50.0, dc.GRAVITY, 0.2)
    m = _torus_dynamics(_from_mesh("torus"), 0.3, material)
    X, contact = m.run(fc.STEPS, want_contacts=True)
    r = fr.FieldDynamics(c["V0"], c["faces"], c["mass"], dt=fc.DT, stiffness=k, damping=d, gravity=g, iterations=fc.ITERATIONS, contact_stiffness=fc.KC,
                         field=(sg.prepare(values, voxel), origin, voxel), field_friction=0.3)
    wX, wv, _ = r.run(c["V0"], np.zeros_like(c["V0"]), fc.STEPS)
    ex = float(np.abs(X.cpu().numpy().astype(np.float64) - wX).max())
    ev = float(np.abs(m.velocities.cpu().numpy().astype(np.float64) - wv).max())
    compare = ~((np.abs(r.phi_star) < fc.NEAR) | r.fringe)
    contact = contact.cpu().numpy()
    print("torus on a box: positions %.3g, velocities %.3g, %d rows x steps in contact, %d compared rows differ, %d of the %d rows left out differ"
          % (ex, ev, int((contact > 0).sum()), int((contact != r.contact)[compare].sum()), int((contact != r.contact)[~compare].sum()), int((~compare).sum())))
    assert ex <= 1e-6 and ev <= 1e-6 / fc.DT
    assert np.array_equal(contact[compare], r.contact[compare]) and int((contact[-1] == 1).sum()) >= 8 and compare.mean() > 0.98
    assert abs(float(X[-1][:, 1].min()) - fc.GROUND) <= voxel


def _sheet_run(material, v0, steps, height):
    from gaussianmesh_amd.dynamics import MeshDynamics
    V0, faces = cc.sheet(5, 5, height=height)
    k, g, d = material
    m = MeshDynamics(V0, faces, stiffness=k, gravity=g, damping=d, dt=cc.DT, iterations=cc.ITERATIONS, field=_from_mesh("sheet"), field_friction=0.0,
                     contact_stiffness=cc.KC, **TIGHT)
    m.reset(velocities=_dev(np.tile(np.asarray(v0, np.float32), (len(V0), 1))))
    X, contact = m.run(steps, want_contacts=True)
    return X.cpu().numpy().astype(np.float64), contact.cpu().numpy(), V0.astype(np.float64)


@pytest.mark.parametrize("damping", [0.0, 0.02])
def test_a_flat_sheet_on_a_box_follows_the_scalar_recursion(damping):
    """the 25-vertex sheet dropped flat onto the middle of a 4 x 4 box's top: dynamics_contact_cases.sheet_recursion to 1e-7, as over the
    analytic floor (test_gpu_dynamics_contact.py).  Above the top face, 1.5 away from its edges, a sample's value is the float32 root of
    the float32 square of its height: the plane's distance to within a float32 rounding of a number below 0.5 (3e-8), and a sample's
    computed position is as close to where the sampler takes it to be; nothing moves sideways but by the gradient's noise times the depth."""
    _reference_values("sheet")                                               # the lattice is dynamics_field_cases' for the sheets
    X, contact, V0 = _sheet_run((10.0, dc.GRAVITY, damping), (0.0, -0.5, 0.0), 24, 0.1)
    want = cc.sheet_recursion(0.1, -0.5, 24, damping=damping)
    err = float(np.abs(X[:, :, 1] - want[:, None]).max())
    side = float(np.abs(X[:, :, [0, 2]] - V0[None][:, :, [0, 2]]).max())
    print("sheet on a box, damping %g: recursion %.3g, sideways %.3g" % (damping, err, side))
    assert err <= 1e-7 and side <= 1e-7
    assert ((contact == 0).all(1) | (contact == 1).all(1)).all() and (contact[0] == 0).all() and (contact == 1).any()


def test_a_damped_sheet_on_a_box_comes_to_rest_at_a_over_kc():
    X, contact, _ = _sheet_run((10.0, dc.GRAVITY, 0.2), (0.0, 0.0, 0.0), 200, 0.01)
    depth = float(np.abs(X[-1, :, 1] - dc.GRAVITY[1] / cc.KC).max())
    print("sheet at rest on a box: |y - a / kc| %.3g, last step %.3g" % (depth, float(np.abs(X[-1] - X[-2]).max())))
    assert depth <= 1e-7 and float(np.abs(X[-1] - X[-2]).max()) <= 1e-8
    assert (contact[-1] == 1).all()


def test_object_field_merges_the_current_meshes_and_holds_a_falling_object(tmp_path):
    """two copies of test_gpu_edittool's object, the second moved 1.6 down by deform_vertices: object_field of both is from_mesh of the
    merged CURRENT meshes; and the first, dropped onto object_field of the second, ends no deeper inside it than |g| / kc + one voxel"""
    from gaussianmesh_amd import mesh_sdf
    from gaussianmesh_amd.dynamics import SdfGrid
    from gaussianmesh_amd.edittool import SceneVisualTool
    d = str(tmp_path)
    _write_scene(d)
    tool = SceneVisualTool(os.path.join(d, "background.ply"))
    for name in ("Top", "Bottom"):
        tool.add_gaussian(os.path.join(d, "object.ply"), os.path.join(d, "rest.obj"), name)
    top, bottom = tool.gaussians_list
    bottom.deform_vertices(bottom.vertex + _dev([0.0, -1.6, 0.0]))
    low = bottom.mesh_vertex_current.cpu().numpy()
    faces = bottom.faces.cpu().numpy()
    both = tool.object_field(["Top", "Bottom"], resolution=32)
    merged = SdfGrid.from_mesh(*mr.merged((top.vertex.cpu().numpy(), faces), (low, faces)), resolution=32)
    assert (both.nx, both.ny, both.nz) == (merged.nx, merged.ny, merged.nz) and max(both.nx, both.ny, both.nz) == 32 and both.voxel == merged.voxel
    rng = np.random.default_rng(5)
    pts = _dev(rng.uniform([-2.5, -2.2, -2.5], [2.5, 0.6, 2.5], size=(64, 3)))
    assert same_bits(both.sample(pts), merged.sample(pts)) and same_bits(both.grid, merged.grid)
    phi = both.sample(pts)[0]
    assert not bool(torch.isnan(phi).any()) and int((phi < 0).sum()) >= 3 and int((phi > 0).sum()) >= 3
    field = tool.object_field("Bottom", resolution=32)
    assert same_bits(field.grid, SdfGrid.from_mesh(low, faces, resolution=32).grid) and not same_bits(field.grid, SdfGrid.from_mesh(bottom.vertex, faces, resolution=32).grid)
    kc = 1.0e4
    X = top.simulate(40, gravity=dc.GRAVITY, damping=0.2, stiffness=50.0, field=field, field_friction=0.3, contact_stiffness=kc)
    assert same_bits(top.mesh_vertex_current, X[-1]) and float(X[-1][:, 1].mean()) < -0.1          # it fell
    deepest = float(mesh_sdf.signed_distances(X[-1].contiguous(), low, faces).min())
    print("a torus resting on a torus: deepest vertex %.4f inside, voxel %.4f, |g| / kc %.4g" % (-deepest, field.voxel, 9.8 / kc))
    assert deepest >= -(9.8 / kc + field.voxel)
    free = top.vertex.cpu().numpy()[:, 1].mean() - 0.5 * 9.8 * (40 * fc.DT) ** 2                    # where free fall would have taken it
    assert float(X[-1][:, 1].mean()) > free + 1.0                                                  # the obstacle held it
    for bad in ([], ["Nobody"]):
        with pytest.raises(ValueError):
            tool.object_field(bad)


def test_cli_obstacle_mesh_changes_the_frames(tmp_path):
    """--dynamics --obstacle_mesh BOX.obj over four frames of the 64-pixel scene: the meshes and the frames differ from the run without
    the obstacle, and no free vertex ends deeper inside the box than a voxel"""
    from gaussianmesh_amd import io as gio
    d = str(tmp_path)
    _scene64(d)
    verts, faces = gio.read_obj(os.path.join(d, "rest.obj"))
    ids, pos = _drags(verts, T=4)
    np.savez(os.path.join(d, "handles.npz"), handles=ids, positions=pos)
    low = float(verts[:, 1].min())
    bv, bf = mr.cube((-3.5, low - 1.0, -3.5), (3.5, low + 0.1, 3.5))          # its top 0.1 above the torus's lowest vertices
    gio.write_obj(os.path.join(d, "box.obj"), bv, bf)
    plain, held = os.path.join(d, "plain"), os.path.join(d, "held")
    common = ("--dynamics", "--gravity", "0", "-9.8", "0")
    _cli(d, plain, *common)
    _cli(d, held, *common, "--obstacle_mesh", os.path.join(d, "box.obj"), "--obstacle_resolution", "32", "--obstacle_margin", "0.25", "--friction", "0.3")
    names = ["%05d.%s" % (k, e) for k in range(4) for e in ("obj", "png")]
    assert sorted(os.listdir(plain)) == names and sorted(os.listdir(held)) == names
    read = lambda folder, n: open(os.path.join(folder, n), "rb").read()
    assert all(read(plain, n) != read(held, n) for n in names)
    last_plain, last_held = (np.asarray(gio.read_obj(os.path.join(f, "00003.obj"))[0]) for f in (plain, held))
    free = np.setdiff1d(np.arange(len(verts)), ids)
    voxel = 7.0 * 1.5 / 32
    assert last_plain[free, 1].min() < low + 0.05 and last_held[free, 1].min() > low + 0.1 - voxel and np.isfinite(last_held).all()
