"""-m gpu: gm_pose_interp (pose_interp.PoseInterpolator) against the float64 reference of tests/pose_interp_ref.py on the cases of
tests/pose_interp_cases.py in both held-row modes, its batches, repeatability on poisoned memory, sequence, robustness, refusals, and
the edit surface on top of it (SingleObjectDeform.interpolate_to, ObjectVisualTool.interpolate_one_gaussian, render_sequence over the
in-betweens, edit_sequence --inbetweens)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pose_interp_cases as pc
from poison import differing, run_under_fills, same_bits
from test_gpu_arap import _drags, _scene64, _tool
from test_gpu_edit_sequence import _gate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIGHT = dict(cg_iterations=2000, cg_tolerance=1e-10)
_made = {}


def _interp(mesh, mode="centroid", fresh=False):
    from gaussianmesh_amd.pose_interp import PoseInterpolator
    if fresh or (mesh, mode) not in _made:
        V0, faces = pc.mesh(mesh)
        p = PoseInterpolator(V0, faces, anchors=None if mode == "centroid" else pc.anchors(mesh))
        if fresh:
            return p
        _made[(mesh, mode)] = p
    return _made[(mesh, mode)]


def _dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


def _keys(mesh, a, b):
    return _dev(pc.key(mesh, a)), _dev(pc.key(mesh, b))


# ---- 1. against the reference ----
@pytest.mark.parametrize("mesh, a, b, mode", pc.ALL, ids=["%s-%s-%s-%s" % c for c in pc.ALL])
def test_against_the_reference(mesh, a, b, mode):
    """max |V_hip - V_ref| <= 1e-6 at t in {0, 1e-9, 0.25, 0.5, 1}: coordinates are below 4, so the float32 rounding of the output is at
    most 2.4e-7, and PCG converged to 1e-10 stays within about 1e-9 of the dense solve."""
    want = pc.reference_run(mesh, a, b, mode)
    A, B = _keys(mesh, a, b)
    V, stats = _interp(mesh, mode).between(A, B, pc.TS, want_stats=True, **TIGHT)
    V, stats = V.cpu().numpy().astype(np.float64), stats.cpu().numpy()
    assert V.shape == want.shape and stats.shape == (len(pc.TS), 6)
    err = np.abs(V - want).reshape(len(pc.TS), -1).max(axis=1)
    print("%s %s -> %s (%s): max |V_hip - V_ref| per t = %s, CG steps at most %d, residual at most %.3g"
          % (mesh, a, b, mode, " ".join("%.3g" % e for e in err), int(stats[:, :3].max()), stats[:, 3:].max()))
    assert np.isfinite(V).all() and float(err.max()) <= 1e-6
    assert (stats[:, 3:] <= 1e-10).all() and (stats[:, :3] <= 2000).all() and (stats[:, :3] == np.round(stats[:, :3])).all()
    if mode == "anchors":
        # the anchors sit on their linear path's float32 rounding: exactly where t is a power of two, so that (1 - t) a and t b are exact
        # in float64 and the sum rounds once (elsewhere a fused multiply-add may round the float64 sum the other way, and sums of
        # float32 values land on float32 ties often enough to show it): within the rounding of a coordinate below 4 there
        ids = pc.anchors(mesh)
        ts = np.array(pc.TS)[:, None, None]
        line = (1.0 - ts) * pc.key(mesh, a)[ids].astype(np.float64) + ts * pc.key(mesh, b)[ids].astype(np.float64)
        exact = [k for k, t in enumerate(pc.TS) if t in (0.0, 0.25, 0.5, 1.0)]
        assert np.array_equal(V[exact][:, ids], line[exact].astype(np.float32).astype(np.float64))
        assert float(np.abs(V[:, ids] - line).max()) <= 2.4e-7


# ---- 2. batches ----
@pytest.mark.parametrize("mesh, mode", [("torus_1073", "centroid"), ("two_tori", "centroid"), ("pinned", "anchors")])
def test_a_frame_does_not_depend_on_its_batch(mesh, mode):
    """the items of batches of 1, 5 and 64 (and of 70 frames, cut into two chains) equal single-frame calls bit for bit; order and
    repetition of ts move no bit"""
    p = _interp(mesh, mode)
    A, B = _keys(mesh, "twist", "turn179")
    ts = np.linspace(0.0, 1.0, 64)
    single = torch.stack([p.between(A, B, [t])[0] for t in ts], 0)
    stat1 = torch.cat([p.between(A, B, [t], want_stats=True)[1] for t in ts[:5]], 0)
    full, stat64 = p.between(A, B, ts, want_stats=True)
    assert same_bits(full, single) and same_bits(stat64[:5], stat1)
    assert same_bits(p.between(A, B, ts[17:18]), single[17:18])
    pick = [3, 60, 3, 17, 0]
    assert same_bits(p.between(A, B, ts[pick]), single[pick])
    assert same_bits(p.between(A, B, ts[::-1].copy()), single.flip(0))
    long = np.concatenate([ts, ts[10:16]])
    assert same_bits(p.between(A, B, long), torch.cat([single, single[10:16]], 0))
    assert not same_bits(single[20], single[21])


# ---- 3. repeatability ----
@pytest.mark.parametrize("mesh, mode", [("torus_1073", "centroid"), ("two_tori", "centroid"), ("pinned", "anchors"), ("flat_patch", "anchors")])
def test_same_bits_from_call_to_call_and_on_poisoned_memory(mesh, mode):
    """two calls give the same bits; so do runs whose every allocation (V_out, stats, the workspace of a fresh interpolator) was filled
    with 0x00, 0xFF and 0x5A beforehand, and no guard band around any of them is touched"""
    A, B = _keys(mesh, "rest", "twist")
    ts = [0.0, 0.3, 0.7, 1.0, 0.3]
    p = _interp(mesh, mode)
    first = p.between(A, B, ts, want_stats=True)
    assert same_bits(first, p.between(A, B, ts, want_stats=True))
    runs = run_under_fills(lambda: _interp(mesh, mode, fresh=True).between(A, B, ts, want_stats=True))
    assert all(r[0].handed_out >= 2 for r in runs)
    assert differing(runs) == [] and same_bits(runs[0][1][0], first[0]) and same_bits(runs[0][1][1], first[1])


def test_out_is_honoured_and_may_not_alias_a_key():
    p = _interp("torus_256")
    A, B = _keys("torus_256", "rest", "twist")
    ts = [0.25, 0.5]
    want = p.between(A, B, ts)
    big = torch.full((4, 256, 3), 7.0, device="cuda")
    got = p.between(A, B, ts, out=big[1:3])
    assert got.data_ptr() == big[1].data_ptr() and same_bits(got, want)
    assert bool((big[0] == 7.0).all()) and bool((big[3] == 7.0).all())
    keys = torch.stack([A, B], 0)
    for out in (keys, keys[1:], torch.empty((2, 256, 3), device="cuda", dtype=torch.float64), torch.empty((3, 256, 3), device="cuda"),
                torch.empty((2, 256, 3)), torch.empty((2, 3, 256), device="cuda").transpose(1, 2)):
        with pytest.raises(ValueError, match="out"):
            p.between(keys[0], keys[1], ts[:out.shape[0]], out=out)
    assert same_bits(keys, torch.stack([A, B], 0))


# ---- 4. sequence ----
def test_sequence_copies_the_keys_and_solves_only_between():
    from gaussianmesh_amd.pose_interp import segment_ts
    p = _interp("torus_256")
    keys = [_dev(pc.key("torus_256", k)) for k in ("rest", "twist", "turn179")]
    for ease in ("linear", "smoothstep"):
        seq = p.sequence(keys, 3, ease=ease)
        assert seq.shape == (9, 256, 3) and seq.dtype is torch.float32
        for k in range(3):
            assert torch.equal(seq[4 * k], keys[k])
        for k in range(2):
            assert same_bits(seq[4 * k + 1:4 * k + 4], p.between(keys[k], keys[k + 1], segment_ts(3, ease)))
    assert not torch.equal(p.sequence(keys, 3)[1], p.sequence(keys, 3, ease="smoothstep")[1])
    stacked = torch.stack(keys, 0)
    zero = p.sequence(stacked, 0)
    assert torch.equal(zero, stacked) and zero.data_ptr() != stacked.data_ptr()
    assert same_bits(p.sequence(stacked.double().cpu().numpy(), 3), p.sequence(keys, 3))
    for bad, n in ((keys[:1], 2), (stacked[:, :5], 2), (keys, -1), (keys, 1.5)):
        with pytest.raises(ValueError):
            p.sequence(bad, n)
    with pytest.raises(ValueError, match="ease"):
        p.sequence(keys, 2, ease="cubic")


# ---- 5. robustness ----
@pytest.mark.parametrize("mode", ["centroid", "anchors"])
def test_a_collapsed_face_in_a_key_gives_finite_output(mode):
    p = _interp("torus_96", mode)
    A, B = _keys("torus_96", "collapsed", "rest")
    for a, b in ((A, B), (B, A), (A, A)):
        V, stats = p.between(a, b, pc.TS, want_stats=True)
        assert bool(torch.isfinite(V).all()) and bool(torch.isfinite(stats).all())
        assert float(V.abs().max()) < 4.0


def test_stats_at_the_defaults_and_at_a_binding_cap():
    p = _interp("torus_1073")
    A, B = _keys("torus_1073", "rest", "twist")
    _, stats = p.between(A, B, [0.25, 0.5], want_stats=True)
    stats = stats.cpu().numpy()
    print("defaults: CG steps", stats[:, :3].reshape(-1), "residuals", stats[:, 3:].reshape(-1))
    assert (stats[:, :3] == np.round(stats[:, :3])).all() and (stats[:, :3] >= 1).all() and (stats[:, :3] <= 512).all()
    assert (stats[:, 3:] <= 1e-6).all()
    _, capped = p.between(A, B, [0.5], cg_iterations=3, cg_tolerance=1e-12, want_stats=True)
    capped = capped.cpu().numpy()
    assert (capped[:, :3] == 3).all() and (capped[:, 3:] > 1e-12).all() and np.isfinite(capped).all()
    V, none = p.between(A, A, [0.0, 0.5, 1.0], cg_tolerance=1e-3, want_stats=True)    # the test before the first step: nothing to do
    assert (none.cpu().numpy()[:, :3] == 0).all() and float((V - A).abs().max()) <= 1e-6


def test_python_refusals_launch_nothing():
    from gaussianmesh_amd import _lib
    p = _interp("torus_96")
    A, B = _keys("torus_96", "rest", "twist")
    out = torch.full((2, 96, 3), 5.0, device="cuda")
    for ts in ([0.5, 1.0000001], [-1e-9, 0.5], [0.5, float("nan")], [float("inf"), 0.5]):
        with pytest.raises(ValueError, match="ts"):
            p.between(A, B, ts, out=out)
    with pytest.raises(ValueError, match="ts"):
        p.between(A, B, [])
    for bad in (A[:50], A.long(), A.reshape(3, 96)):
        with pytest.raises(ValueError, match="must be a floating-point"):
            p.between(bad, B, [0.5, 0.6], out=out)
    for kw, what in ((dict(cg_iterations=0), "cg_iterations"), (dict(cg_tolerance=-1.0), "cg_tolerance"), (dict(cg_tolerance=float("nan")), "cg_tolerance")):
        with pytest.raises(_lib.GmeshError, match=what):
            p.between(A, B, [0.5, 0.6], out=out, **kw)
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())


def test_c_refusals_launch_nothing_and_the_workspace_is_kept_and_grown():
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    p = _interp("torus_96", fresh=True)
    A, B = _keys("torus_96", "rest", "twist")
    assert p._ws is None
    p.between(A, B, [0.5])
    one = p._ws
    assert one.numel() == l.gm_pose_interp_workspace_bytes(96, p.F, 1)
    p.between(A, B, [0.25])
    assert p._ws is one                                                # kept
    p.between(A, B, [0.1, 0.2, 0.3])
    three = p._ws
    assert three is not one and three.numel() == l.gm_pose_interp_workspace_bytes(96, p.F, 3)
    p.between(A, B, [0.5, 0.6])
    assert p._ws is three                                              # not shrunk
    p.between(A, B, np.linspace(0, 1, 100))
    assert p._ws.numel() == l.gm_pose_interp_workspace_bytes(96, p.F, 64)
    # straight through ctypes, on real device memory: every refusal leaves a poisoned V_out and stats untouched
    T = 2
    ts = _dev([0.25, 0.75], torch.float64)
    out = torch.full((T, 96, 3), 5.0, device="cuda")
    stats = torch.full((T, 6), -3.0, dtype=torch.float64, device="cuda")
    ws = p._ws
    stream = torch.cuda.current_stream().cuda_stream

    def call(T=T, Vm=96, F=p.F, C=p.C, cg=16, tol=1e-6, nbytes=None, **kw):
        a = dict(off=p._off, cols=p._cols, w=p._w, V0=p.rest, faces=p._faces, vf_off=p._vf_off, vf_faces=p._vf_faces, held=p._held, c_off=p._comp_off,
                 c_rows=p._comp_rows, label=p._label, A=A, B=B, ts=ts, out=out, stats=stats, ws=ws)
        a.update(kw)
        q = {k: (v.data_ptr() if torch.is_tensor(v) else v) for k, v in a.items()}
        return l.gm_pose_interp(T, Vm, F, q["off"], q["cols"], q["w"], q["V0"], q["faces"], q["vf_off"], q["vf_faces"], q["held"], C, q["c_off"],
                                q["c_rows"], q["label"], q["A"], q["B"], q["ts"], cg, tol, q["out"], q["stats"], q["ws"],
                                ws.numel() if nbytes is None else nbytes, ctypes.c_void_p(stream))
    for kw, rc in ((dict(T=0), 1), (dict(T=65), 1), (dict(Vm=0), 1), (dict(F=-1), 1), (dict(C=-1), 1), (dict(C=97), 1), (dict(cg=0), 1),
                   (dict(tol=-1.0), 1), (dict(A=None), 1), (dict(ts=None), 1), (dict(out=None), 1), (dict(ws=None), 1), (dict(label=None), 1),
                   (dict(out=A), 1), (dict(out=B), 1), (dict(stats=out), 1), (dict(ws=out), 1), (dict(out=p.rest), 1),
                   (dict(nbytes=l.gm_pose_interp_workspace_bytes(96, p.F, T) - 1), 3), (dict(nbytes=0), 3)):
        assert call(**kw) == rc and b"gm_pose_interp" in l.gm_last_error(), (kw, l.gm_last_error())
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((stats == -3.0).all())
    assert call() == 0                                                 # and the same call, unrefused, writes both
    torch.cuda.synchronize()
    want, want_stats = p.between(A, B, [0.25, 0.75], cg_iterations=16, want_stats=True)
    assert same_bits(out, want) and same_bits(stats, want_stats)


def test_a_mesh_without_faces_moves_linearly():
    """F = 0: every vertex is pinned, so each is its own component on its linear path (t a power of two: (1 - t) a and t b are exact
    in float64, so the device's sum and numpy's round alike whether or not a multiply-add is fused)"""
    from gaussianmesh_amd.pose_interp import PoseInterpolator
    rng = np.random.default_rng(3)
    V0, A, B = (rng.uniform(-2, 2, (300, 3)).astype(np.float32) for _ in range(3))
    for anchors in (None, [4, 7]):
        p = PoseInterpolator(V0, np.zeros((0, 3), np.int32), anchors=anchors)
        ts = np.array([0.0, 0.25, 1.0])
        V, stats = p.between(_dev(A), _dev(B), ts, want_stats=True)
        want = (1.0 - ts)[:, None, None] * A.astype(np.float64) + ts[:, None, None] * B.astype(np.float64)
        assert np.array_equal(V.cpu().numpy(), want.astype(np.float32)) and bool((stats == 0).all())


# ---- 6. the edit surface ----
def test_interpolate_to_is_sequence_and_leaves_the_object_at_the_target(tmp_path):
    from gaussianmesh_amd.deform import SingleObjectDeform as TensorObject
    from gaussianmesh_amd.pose_interp import PoseInterpolator
    d = str(tmp_path)
    _scene64(d)
    tool, other = _tool(d), _tool(d)
    o, q = tool.gaussians_list[0], other.gaussians_list[0]
    rest = o.vertex.cpu().numpy().astype(np.float64)
    first, second = _dev(pc.twisted(rest)), _dev(pc.turned(rest, 2.0))
    p = PoseInterpolator(o.vertex, o.faces)
    got = o.interpolate_to(first, 3)
    assert got.shape == (5, o.vertex.shape[0], 3) and same_bits(got, p.sequence([o.vertex, first], 3))
    assert torch.equal(o.mesh_vertex_current, first)
    exp = q.deform_vertices(first)
    assert all(torch.equal(g, e) for g, e in zip(o.deform_vertices(o.mesh_vertex_current), exp))
    kept = o._operators["pose_interp"]
    again = o.interpolate_to(second, 2, ease="smoothstep", cg_tolerance=1e-8)      # from the current mesh, with the kept interpolator
    assert o._operators["pose_interp"] is kept and same_bits(again, p.sequence([first, second], 2, ease="smoothstep", cg_tolerance=1e-8))
    assert torch.equal(o.mesh_vertex_current, second)
    anchored = o.interpolate_to(first, 1, anchors=[0, 5])
    assert o._operators["pose_interp"] is not kept
    assert same_bits(anchored, PoseInterpolator(o.vertex, o.faces, anchors=[0, 5]).sequence([second, first], 1))
    # the tool's wrapper, and an object built from tensors alone
    third = _tool(d)
    assert same_bits(third.interpolate_one_gaussian("Object", first, 3), got) and third.interpolate_one_gaussian("Nobody", first, 3) is None
    assert torch.equal(third.gaussians_list[0].mesh_vertex_current, first)
    t = TensorObject(o.gaussian_pos, o.gaussian_cov, o.gaussian_o, o.gaussian_feature, o.gaussian_triangles, o.coord, o.vertex, name="T")
    with pytest.raises(ValueError, match="no faces"):
        t.interpolate_to(first, 3)
    assert same_bits(t.interpolate_to(first, 3, faces=o.faces.cpu().numpy()), got)


def test_render_sequence_over_the_inbetweens(tmp_path):
    """render_sequence over the meshes against deform_vertices + render_gaussian per frame, at 64 x 64, under the forward gate that
    holds the two routes together everywhere else (test_gpu_edit_sequence._gate)"""
    d = str(tmp_path)
    _scene64(d)
    tool, ref_tool = _tool(d), _tool(d)
    o = tool.gaussians_list[0]
    target = _dev(pc.turned(o.vertex.cpu().numpy().astype(np.float64), 2.0, shift=(0.2, 0.1, 0.0)))
    meshes = o.interpolate_to(target, 3)
    cams = tool.get_camera(d)
    got = list(tool.render_sequence([(cams[k % 3], {"Object": meshes[k]}) for k in range(5)], frames_per_launch=4))
    assert len(got) == 5
    for k in range(5):
        ref_tool.gaussians_list[0].deform_vertices(meshes[k])
        assert got[k].shape == (3, 64, 64)
        _gate(got[k], ref_tool.render_gaussian(cams[k % 3]), "frame %d vs deform_vertices + render_gaussian" % k)
        assert float((got[k] - 1.0).abs().max()) > 0.1                               # the object is in the picture


def _cli(d, out, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "gaussianmesh_amd.edit_sequence", "--object_gaussian", os.path.join(d, "object.ply"),
                        "--object_origin_mesh", os.path.join(d, "rest.obj"), "--camera_path", d, "--render_path", out,
                        "--handle_sequence", os.path.join(d, "handles.npz"), "--save_meshes"] + list(extra), cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]


def _handles_file(d):
    from gaussianmesh_amd import io as gio
    verts, faces = gio.read_obj(os.path.join(d, "rest.obj"))
    ids, pos = _drags(verts)
    np.savez(os.path.join(d, "handles.npz"), handles=ids, positions=pos)
    return verts, faces, ids, pos


def test_cli_inbetweens_writes_keys_and_inbetweens(tmp_path):
    from gaussianmesh_amd import io as gio
    from gaussianmesh_amd.arap import ArapSolver
    from gaussianmesh_amd.pose_interp import PoseInterpolator
    d = str(tmp_path)
    _scene64(d)
    verts, faces, ids, pos = _handles_file(d)
    out = os.path.join(d, "renders")
    _cli(d, out, "--inbetweens", "2", "--ease", "smoothstep")
    rest = _dev(verts.astype(np.float32))
    keys = [rest] + list(ArapSolver(verts.astype(np.float32), faces, ids).solve_sequence(pos, batch=1))
    want = PoseInterpolator(rest, faces).sequence(keys, 2, ease="smoothstep").cpu().numpy().astype(np.float64)
    assert sorted(os.listdir(out)) == ["%05d.%s" % (k, e) for k in range(10) for e in ("obj", "png")]      # 3 keys after the rest pose
    for k in range(10):
        v, f = gio.read_obj(os.path.join(out, "%05d.obj" % k))
        assert np.array_equal(f, faces) and np.array_equal(v, want[k]), k


def test_cli_default_is_inbetweens_0_byte_for_byte(tmp_path):
    d = str(tmp_path)
    _scene64(d)
    _handles_file(d)
    plain, zero = os.path.join(d, "plain"), os.path.join(d, "zero")
    _cli(d, plain)
    _cli(d, zero, "--inbetweens", "0", "--ease", "smoothstep")
    names = sorted(os.listdir(plain))
    assert names == sorted(os.listdir(zero)) == ["%05d.%s" % (k, e) for k in range(3) for e in ("obj", "png")]
    for n in names:
        assert open(os.path.join(plain, n), "rb").read() == open(os.path.join(zero, n), "rb").read(), n
