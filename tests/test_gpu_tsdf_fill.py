"""-m gpu: gm_tsdf_fill against its definition - the numpy float32 restatement of tests/tsdf_fill_ref.py, bit for bit in tsdf_out,
weight_out and out_counts - on every grid size where a brick edge can go wrong, for both parities of the iteration count, both boundary
modes and volumes from almost observed to almost empty; on guard-banded, poisoned buffers; then the surface above it:
TsdfVolume.fill_holes / extract(fill_holes=), from_cloud on a torus cloud seen only from above, and the CLI."""
import functools
import itertools
import json

import numpy as np
import pytest
import torch

import poison
import test_gpu_tsdf as base
import tsdf_fill_ref as fr
import tsdf_ref as tr

pytestmark = pytest.mark.gpu
f32 = np.float32
BRICK = (32, 4, 2)              # TF_BX, TF_BY, TF_BZ of csrc/gm_tsdf_fill.hip: samples of one workgroup
FILL = -7

_bits, _dev = base._bits, base._dev


def _device_fill(tsdf, weight, min_weight=1.0, iterations=0, free=False, fill_weight=1.0, want_counts=True):
    """gm_tsdf_fill through ctypes: (tsdf_out, weight_out, counts or None, tsdf_in and weight_in as they are afterwards); the outputs
    pre-filled with FILL, the workspace at an odd address"""
    from gaussianmesh_amd import _lib
    lib = _lib.lib()
    nz, ny, nx = tsdf.shape
    d, w = _dev(np.array(tsdf, f32)), _dev(np.array(weight, f32))          # (copies: the shared references are read-only)
    D, W = torch.full_like(d, float(FILL)), torch.full_like(d, float(FILL))
    counts = torch.full((2,), FILL, dtype=torch.int32, device="cuda")
    nbytes = lib.gm_tsdf_fill_workspace_bytes(nx, ny, nz)
    ws = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    _lib.check(lib.gm_tsdf_fill(nx, ny, nz, d.data_ptr(), w.data_ptr(), float(min_weight), int(iterations), int(free), float(fill_weight),
                                D.data_ptr(), W.data_ptr(), counts.data_ptr() if want_counts else None, ws.data_ptr() + 4, nbytes,
                                torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return D.cpu().numpy(), W.cpu().numpy(), counts.cpu().numpy() if want_counts else None, (d.cpu().numpy(), w.cpu().numpy())


def _same_fill(got, ref, what):
    assert got[2].tolist() == ref[2].tolist(), "%s: counts %s, reference %s" % (what, got[2].tolist(), ref[2].tolist())
    assert np.array_equal(_bits(got[1]), _bits(ref[1])), "%s: %d weights differ" % (what, (_bits(got[1]) != _bits(ref[1])).sum())
    bad = np.nonzero(_bits(got[0]) != _bits(ref[0]))
    assert len(bad[0]) == 0, "%s: %d values differ, first at %s: device %r reference %r" % (
        what, len(bad[0]), [int(b[0]) for b in bad], got[0][bad][0], ref[0][bad][0])


# (2,2,2) (5,4,3) (9,8,7): inside one brick; (33,9,8) and (31,5,3): beside a brick edge; (33,9,9) and (31,7,3): one past / one short of
# THIS kernel's brick edge on every axis; (64,8,4): whole bricks; (41,39,40): several bricks meet in every direction
GRIDS = [(2, 2, 2), (5, 4, 3), (9, 8, 7), (33, 9, 8), (31, 5, 3), (33, 9, 9), (31, 7, 3), (64, 8, 4), (41, 39, 40)]
ITERATIONS = (0, 1, 2, 3, 7)


@pytest.mark.parametrize("n", GRIDS, ids=lambda n: "%dx%dx%d" % n)
def test_fill_bit_for_bit(n):
    assert all((GRIDS[5][a] - 1) % BRICK[a] == 0 and (GRIDS[6][a] + 1) % BRICK[a] == 0 and GRIDS[7][a] % BRICK[a] == 0 for a in range(3))
    filled = left = 0
    for observed in (0.9, 0.5, 0.1):
        tsdf, w, _, _ = tr.noise_field(n, seed=n[0] + 7 * n[1] + int(10 * observed), observed=observed)
        assert set(np.unique(w)) <= {f32(0), f32(2)}
        for iterations, free, fill_weight, min_weight in itertools.product(ITERATIONS, (False, True), (1.0, 2.5), (1.0, 3.0)):
            what = "%s observed %g iterations %d free %s fill_weight %g min_weight %g" % (n, observed, iterations, free, fill_weight, min_weight)
            ref = fr.fill_ref(tsdf, w, min_weight, iterations, free, fill_weight)
            got = _device_fill(tsdf, w, min_weight, iterations, free, fill_weight)
            _same_fill(got, ref, what)
            assert np.array_equal(_bits(got[3][0]), _bits(tsdf)) and np.array_equal(_bits(got[3][1]), _bits(w)), what + ": the inputs changed"
            if min_weight == 3.0:                                      # nothing weighs 3: every sample is to be filled
                assert ref[2].sum() == tsdf.size and (free or ref[2][0] == 0)
            filled, left = filled + int(ref[2][0]), left + int(ref[2][1])
    assert filled > 0 and left > 0                                     # samples filled, samples not reached


def test_nan_weight_and_nan_source_value():
    tsdf, w, _, _ = tr.noise_field((9, 8, 7), seed=4, observed=0.5)
    w[3, 4, 5], w[0, 0, 0] = np.nan, np.nan                            # no sources: they are filled
    w[2, 2, 2], tsdf[2, 2, 2] = 2, np.nan                              # a source that is NaN: it stays, and spreads
    w[2, 2, 3] = 0
    w[3, 4, 4], w[0, 0, 1] = 2, 2                                      # (and the two have an observed neighbour each)
    for iterations, free in itertools.product((0, 1, 4), (False, True)):
        ref = fr.fill_ref(tsdf, w, 1.0, iterations, free, 1.5)
        got = _device_fill(tsdf, w, 1.0, iterations, free, 1.5)
        _same_fill(got, ref, "NaN case, %d iterations, free %s" % (iterations, free))
        assert _bits(got[0])[2, 2, 2] == _bits(tsdf)[2, 2, 2] and got[1][2, 2, 2] == 2
        assert np.array_equal(_bits(got[3][1]), _bits(w))              # the NaN weights are still in the input
        if iterations:
            assert np.isnan(got[0][2, 2, 3]) and got[1][3, 4, 5] == 1.5 and got[1][0, 0, 0] == 1.5 and not np.isnan(got[0][0, 0, 0])


@functools.lru_cache(maxsize=None)
def _hole(name):
    """(field, iterations, boundary, the reference's filled volume): computed once, shared, never written"""
    fld, n, free = {"A": (fr.hole_a(), fr.HOLE_A_ITERATIONS, False), "A+": (fr.hole_a(interior=True), fr.HOLE_A_ITERATIONS, False),
                    "B": (fr.hole_b(), fr.HOLE_B_ITERATIONS, True)}[name]
    ref = fr.fill_ref(fld[0], fld[1], 1.0, n, free)
    for a in fld[:2] + ref:
        a.setflags(write=False)
    return fld, n, free, ref


@pytest.mark.parametrize("name", ["A", "A+", "B"])
def test_holes_of_the_sphere_at_their_pinned_iteration_counts(name):
    fld, n, free, ref = _hole(name)
    got = _device_fill(fld[0], fld[1], 1.0, n, free)
    _same_fill(got, ref, "hole %s" % name)
    assert got[2].tolist() == [int((fld[1] == 0).sum()), 0]
    m = fr.mesh_facts(got[0], got[1], fld[2], fld[3])                  # and what the fill is for
    assert m["border"] == 0 and m["closed"] and m["chi"] == 2 and m["components"] == 1
    if name == "B":                                                    # without free space beyond the grid it stays open, on the device too
        absent = _device_fill(fld[0], fld[1], 1.0, n, False)
        _same_fill(absent, fr.fill_ref(fld[0], fld[1], 1.0, n, False), "hole B, boundary absent")
        assert tr.boundary_edges(tr.surface_nets_ref(absent[0], absent[1], fld[2], fld[3])[1]) == 56


def test_fill_gives_the_same_bits_twice():
    tsdf, w, _, _ = tr.noise_field((41, 39, 40), seed=9, observed=0.3)
    one, two = _device_fill(tsdf, w, 1.0, 7, True, 2.5), _device_fill(tsdf, w, 1.0, 7, True, 2.5)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(one[:2], two[:2])) and one[2].tolist() == two[2].tolist()
    assert one[2][0] > 1000


# ---- guard bands ----
@pytest.mark.parametrize("want_counts", [True, False], ids=["counts", "no-counts"])
def test_fill_stays_inside_guard_banded_buffers_and_writes_all_it_returns(want_counts):
    """both outputs, out_counts and the workspace AT ITS EXACT QUERIED SIZE between poisoned guard bands (tests/poison.py): the bands are
    intact afterwards, and the result does not depend on what the buffers held"""
    from gaussianmesh_amd import _lib
    lib = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    cases = [((33, 9, 8), 3, True, 0.5), ((31, 5, 3), 4, False, 0.5), ((41, 39, 40), 2, True, 0.1), ((2, 2, 2), 1, True, 0.5), ((64, 8, 4), 0, False, 0.9)]
    for n, iterations, free, observed in cases:
        tsdf, w, _, _ = tr.noise_field(n, seed=n[0], observed=observed)
        d, wt = _dev(tsdf), _dev(w)
        nbytes = lib.gm_tsdf_fill_workspace_bytes(*n)

        def route():
            D, W = torch.empty_like(d), torch.empty_like(wt)
            counts = torch.empty((2,), dtype=torch.int32, device="cuda")
            ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
            _lib.check(lib.gm_tsdf_fill(n[0], n[1], n[2], d.data_ptr(), wt.data_ptr(), 1.0, iterations, int(free), 2.5, D.data_ptr(), W.data_ptr(),
                                        counts.data_ptr() if want_counts else None, ws.data_ptr(), nbytes, stream))
            return (D, W, counts) if want_counts else (D, W)

        runs = poison.run_under_fills(route)                           # a damaged band raises GuardViolation
        assert all(p.handed_out == 4 and p.unguarded == 0 for p, _ in runs)
        assert poison.differing(runs) == [], "%s: the result depends on the buffers' old contents" % (n,)
        ref = fr.fill_ref(tsdf, w, 1.0, iterations, free, 2.5)
        out = [x.cpu().numpy() for x in runs[-1][1]]
        _same_fill((out[0], out[1], out[2] if want_counts else ref[2]), ref, "guard-banded %s" % (n,))
        assert np.array_equal(_bits(d.cpu().numpy()), _bits(tsdf)) and np.array_equal(_bits(wt.cpu().numpy()), _bits(w))


# ---- the Python surface ----
def _volume(fld):
    from gaussianmesh_amd.proxy_mesh import TsdfVolume
    tsdf, w, origin, voxel = fld
    nz, ny, nx = tsdf.shape
    vol = TsdfVolume(origin, origin.astype(np.float64) + np.array([nx, ny, nz]) * float(voxel), voxel_size=float(voxel))
    assert (vol.nx, vol.ny, vol.nz) == (nx, ny, nz)
    vol.tsdf.copy_(_dev(np.array(tsdf, f32))); vol.weight.copy_(_dev(np.array(w, f32)))
    return vol


def test_extract_with_fill_holes_equals_the_reference_and_leaves_the_volume_alone():
    fld, n, free, ref = _hole("A")
    assert n == 8 and not free
    vol = _volume(fld)
    before = [x.cpu().numpy() for x in vol.extract(keep="all")]
    keys = set(vol.stats)
    assert keys == {"vertices", "faces", "components", "components_dropped"} and vol.filled_tsdf is None and vol.fill_stats is None
    assert tr.boundary_edges(before[1]) == 80
    V, F = vol.extract(keep="all", fill_holes=8)
    rV, rF = tr.surface_nets_ref(ref[0], ref[1], fld[2], vol.voxel, 1.0)
    assert V.is_cuda and np.array_equal(_bits(V.cpu().numpy()), _bits(rV)) and np.array_equal(F.cpu().numpy(), rF)
    assert tr.boundary_edges(F.cpu().numpy()) == 0
    assert set(vol.stats) == keys | {"fill_iterations", "filled_voxels", "unreached_voxels", "seconds_fill"}
    assert [vol.stats[k] for k in ("fill_iterations", "filled_voxels", "unreached_voxels")] == [8] + ref[2].tolist() and vol.stats["seconds_fill"] > 0
    assert vol.fill_stats == dict(iterations=8, filled_voxels=int(ref[2][0]), unreached_voxels=int(ref[2][1]))
    assert np.array_equal(_bits(vol.filled_tsdf.cpu().numpy()), _bits(ref[0])) and np.array_equal(_bits(vol.filled_weight.cpu().numpy()), _bits(ref[1]))
    assert np.array_equal(_bits(vol.tsdf.cpu().numpy()), _bits(fld[0])) and np.array_equal(_bits(vol.weight.cpu().numpy()), _bits(fld[1]))
    # no argument, afterwards: the fused volume's own surface again, with the keys it had
    after = [x.cpu().numpy() for x in vol.extract(keep="all")]
    assert np.array_equal(_bits(after[0]), _bits(before[0])) and np.array_equal(after[1], before[1]) and set(vol.stats) == keys
    # keep="largest" on the filled volume: one closed component
    Vl, Fl = vol.extract(fill_holes=8)
    assert vol.stats["components"] == 1 and np.array_equal(Fl.cpu().numpy(), rF)


def test_fill_holes_method_defaults_modes_and_integrate_drops_the_fill():
    fld, n, free, ref = _hole("B")
    vol = _volume(fld)
    assert vol.fill_holes(boundary="free") is vol                      # the default reach: max(nx, ny, nz) = 24 iterations
    r24 = fr.fill_ref(fld[0], fld[1], 1.0, 24, True)
    assert vol.fill_stats == dict(iterations=24, filled_voxels=int(r24[2][0]), unreached_voxels=0)
    assert np.array_equal(_bits(vol.filled_tsdf.cpu().numpy()), _bits(r24[0])) and np.array_equal(_bits(vol.filled_weight.cpu().numpy()), _bits(r24[1]))
    vol.fill_holes(32, min_weight=1, boundary="free", fill_weight=0.25)
    r = fr.fill_ref(fld[0], fld[1], 1.0, 32, True, 0.25)
    assert np.array_equal(_bits(vol.filled_tsdf.cpu().numpy()), _bits(ref[0])) and np.array_equal(_bits(vol.filled_weight.cpu().numpy()), _bits(r[1]))
    V, F = vol.extract(keep="all", fill_holes=True, fill_boundary="free")      # True: the default count; extract's min_weight is the fill's
    rV, rF = tr.surface_nets_ref(r24[0], r24[1], fld[2], vol.voxel, 1.0)
    assert np.array_equal(_bits(V.cpu().numpy()), _bits(rV)) and np.array_equal(F.cpu().numpy(), rF) and vol.stats["fill_iterations"] == 24
    assert tr.boundary_edges(rF) == 0
    with pytest.raises(ValueError):
        vol.fill_holes(boundary="open")
    with pytest.raises(ValueError):
        vol.fill_holes(-1)
    # more views: the fill was of the volume as it was
    case = base._orbit_case((24, 24, 24), 23, 37, 1, seed=1)
    from gaussianmesh_amd import scenes
    cam = scenes.orbit_camera(0, 1, 37, 23, radius=2.6, height=1.2, fovx_deg=60.0)
    assert vol.filled_tsdf is not None
    vol.integrate([cam], [_dev(case[2][0])], [_dev(case[3][0])])
    assert vol.filled_tsdf is None and vol.filled_weight is None and vol.fill_stats is None and vol.views == 1


# ---- end to end: a torus cloud seen only from above -> a closed proxy mesh ----
@functools.lru_cache(maxsize=None)
def _from_above():
    from gaussianmesh_amd import proxy_mesh as pm
    E = base.E2E
    model, cl, verts, faces = base._torus_cloud(E["P"], E["nu"], E["nv"])
    cams = [c for c in base._orbit(E["K"], E["W"], E["H"]) if c["campos"][1] > 0]            # above the torus's equator plane y = 0
    assert len(cams) == E["K"] // 2
    lo, hi, _ = pm.default_bounds(model, E["resolution"])
    V0, F0 = pm.from_cloud(model, cams, resolution=E["resolution"], bounds=(lo, hi))
    V1, F1 = pm.from_cloud(model, cams, resolution=E["resolution"], bounds=(lo, hi), fill_holes=True, fill_boundary="free")
    return dict(model=model, cams=cams, bounds=(lo, hi), open=(V0, F0), filled=(V1, F1))


def test_end_to_end_the_unseen_underside_is_closed_and_the_mesh_is_usable():
    from gaussianmesh_amd.arap import ArapSolver
    from gaussianmesh_amd.mesh_simplify import simplify
    r = _from_above()
    f0 = r["open"][1].cpu().numpy()
    V, F = r["filled"]
    v, f = V.cpu().numpy(), F.cpu().numpy()
    print("from above: open %d faces, %d border edges; filled %d faces, %d border edges" % (len(f0), tr.boundary_edges(f0), len(f), tr.boundary_edges(f)))
    assert tr.boundary_edges(f0) > 0
    assert tr.boundary_edges(f) == 0 and tr.n_components(len(v), f) == 1 and len(f) > len(f0) > 1000
    # one handle is enough: there is one component, and nothing is left hanging on a rim
    top = int(np.argmax(v[:, 1]))
    solver = ArapSolver(V, F, [top])
    moved = solver.solve(_dev(v[[top]] + f32(0.25)))
    torch.cuda.synchronize()
    m = moved.cpu().numpy()
    assert np.isfinite(m).all() and np.array_equal(m[top], v[top] + f32(0.25))
    # and it simplifies to a target: no border vertices to lock
    s = simplify(V, F, target_faces=len(f) // 2)
    print("simplified to half:", s.stats)
    sf = s.faces.cpu().numpy()
    assert 0 < len(sf) < len(f) and sf.min() >= 0 and sf.max() < s.vertices.shape[0] and "reached" in s.stats


def test_cli_with_and_without_fill_holes(tmp_path, capsys):
    from gaussianmesh_amd import io as gio
    from gaussianmesh_amd import proxy_mesh as pm
    r = _from_above()
    ply, cj, obj = str(tmp_path / "cloud.ply"), str(tmp_path / "cameras.json"), str(tmp_path / "proxy.obj")
    r["model"].save_ply(ply)
    entries = []
    for k, c in enumerate(r["cams"]):
        Rt = c["view"].T.astype(np.float64)
        entries.append(gio.camera_to_json(k, Rt[:3, :3].T, Rt[:3, 3], c["W"], c["H"], c["fovx"], c["fovy"], "v%d" % k))
    with open(cj, "w") as fh:
        json.dump(entries, fh)
    lo, hi = r["bounds"]
    args = ["--gaussian", ply, "--cameras", cj, "--out", obj, "--resolution", "48", "--bounds"] + [repr(float(x)) for x in (*lo, *hi)]
    assert pm.main(args) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(plain) == {"vertices", "faces", "components_dropped", "boundary_edges", "grid", "views", "seconds"}
    assert set(plain["seconds"]) == {"load", "render_fuse", "extract", "write"} and plain["boundary_edges"] > 0
    assert pm.main(args + ["--fill_holes", "48", "--fill_boundary", "free"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    v, f = gio.read_obj(obj)
    assert set(line) == set(plain) | {"fill_iterations", "filled_voxels", "unreached_voxels"}
    assert set(line["seconds"]) == {"load", "render_fuse", "extract", "write", "fill"} and line["seconds"]["fill"] > 0
    assert line["boundary_edges"] == 0 and tr.boundary_edges(f) == 0 and line["faces"] == len(f) and line["vertices"] == len(v)
    assert line["fill_iterations"] == 48 and line["filled_voxels"] > 0 and line["unreached_voxels"] == 0
