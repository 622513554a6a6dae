"""Host side of the pose interpolation (gm_pose_interp, pose_interp.PoseInterpolator, edit_sequence --inbetweens): the float64
reference of tests/pose_interp_ref.py on float64 keys - that the definition is consistent: it returns the keys, a spin about the
centroid stays a spin, anchors keep their linear path - the shared cases' own promises (coordinates below 4, no face within the band
near a half turn), the constructors' refusals without a device, sequence's frame count and parameters, the declaration and typing of
the two entry points and the C refusals that need no device (made on pointers that are never dereferenced)."""
import math
import os
import re

import numpy as np
import pytest
import torch

import arap_cases as ac
import pose_interp_cases as pc
import pose_interp_ref as pr
from gaussianmesh_amd import _lib, edit_sequence, pose_interp
from gaussianmesh_amd.pose_interp import PoseInterpolator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ("torus_96", "flat_patch", "two_tori", "pinned")


def _keys64(name):
    """float64 keys of a small mesh: rest, a twist with stretch, a rigid turn of 170 degrees about the centroid plus a shift"""
    V0 = pc.mesh(name)[0].astype(np.float64)
    return V0, pc.twisted(V0), pc.turned(V0, math.radians(170.0))


@pytest.mark.parametrize("name", SMALL)
def test_reference_reproduces_both_keys(name):
    """to 1e-12 (the prototype gave 2e-14), in both modes, for every pairing of the three keys"""
    V0, tw, tu = _keys64(name)
    for mode in ("centroid", "anchors"):
        ref = pc.reference(name, mode)
        for A, B in ((V0, tw), (tw, tu), (V0, tu)):
            X = ref.between(A, B, [0.0, 1.0])
            err = max(float(np.abs(X[0] - A).max()), float(np.abs(X[1] - B).max()))
            print(name, mode, "key error %.3g" % err)
            assert err <= 1e-12


@pytest.mark.parametrize("name", SMALL)
def test_reference_keeps_a_spin_about_the_centroid_a_spin(name):
    """rest -> the rest pose turned 170 degrees about its centroid and shifted: at every t the rest pose turned by t 170 degrees and
    shifted by t of the shift, to 1e-12 (the prototype gave 1e-14); the linear blend's midpoint is far from it.  two_tori and pinned
    turn as ONE body about the whole mesh's centroid, so only their per-component means move linearly; they are held to the rigid pose of
    each component about its own centroid, which is what the centroid rule promises."""
    V0 = pc.mesh(name)[0].astype(np.float64)
    ref = pc.reference(name, "centroid")
    if name in ("two_tori", "pinned"):
        B = V0.copy()
        for l in np.unique(ref.label):
            m = ref.label == l
            B[m] = pc.turned(V0[m], math.radians(170.0))
    else:
        B = pc.turned(V0, math.radians(170.0))
    ts = [0.0, 1e-9, 0.25, 0.5, 0.9, 1.0]
    X = ref.between(V0, B, ts)
    for k, t in enumerate(ts):
        want = V0.copy()
        for l in np.unique(ref.label):
            m = ref.label == l
            want[m] = pc.turned(V0[m], t * math.radians(170.0), shift=t * pc.SHIFT)
        err = float(np.abs(X[k] - want).max())
        print(name, "t = %g: %.3g from the rigid pose" % (t, err))
        assert err <= 1e-12
    if name == "torus_96":
        assert float(np.abs(0.5 * (V0 + B) - X[3]).max()) > 2.0        # the collapse of the linear blend


@pytest.mark.parametrize("name", SMALL)
def test_reference_keeps_anchors_on_their_linear_path_and_equal_keys_fixed(name):
    V0, tw, tu = _keys64(name)
    ref = pc.reference(name, "anchors")
    ids = pc.anchors(name)
    ts = np.array([0.0, 0.3, 0.5, 1.0])
    X = ref.between(tw, tu, ts)
    want = (1.0 - ts)[:, None, None] * tw[ids] + ts[:, None, None] * tu[ids]
    assert np.array_equal(X[:, ids], want)
    pinned = np.nonzero(ref.held & ~np.isin(np.arange(len(V0)), ids))[0]
    assert len(pinned) == (2 if name == "pinned" else 0)
    assert np.array_equal(X[:, pinned], (1.0 - ts)[:, None, None] * tw[pinned] + ts[:, None, None] * tu[pinned])
    for mode in ("centroid", "anchors"):                               # A == B gives A at every t
        same = pc.reference(name, mode).between(tu, tu, ts)
        assert float(np.abs(same - tu).max()) <= 1e-12


def test_the_shared_cases_keep_their_promises():
    """every coordinate of every key below 4; every valid face's rotation between paired keys below 3.1 rad; the pairs the issue names
    are there: the rest pose, a rigid turn of 179 degrees plus a shift, a twist with stretch, a solved ARAP pose, A == B"""
    for m in pc.MESHES:
        names = set(sum(pc.pairs(m), ()))
        assert {"rest", "turn179", "twist"} <= names and ("turn179", "turn179") in pc.pairs(m)
        assert ("arap" in names) == (m in pc.ARAP)
        ref = pc.reference(m, "centroid")
        for a, b in pc.pairs(m):
            A, B = pc.key(m, a), pc.key(m, b)
            assert A.dtype == np.float32 and max(float(np.abs(A).max()), float(np.abs(B).max())) < 4.0
            ang = float(ref.relative_angles(A, B).max())
            assert ang < 3.1, (m, a, b, ang)
    sizes = [pc.mesh(m)[0].shape[0] for m in ("torus_96", "torus_256", "torus_1073")]
    assert sizes == [96, 256, 1073]
    lab = pc.reference("two_tori", "centroid").label
    assert sorted(np.unique(lab).tolist()) == [0, 96]
    assert float(ref.relative_angles(pc.key("pinned", "rest"), pc.key("pinned", "turn177")).min()) > 3.0   # (the largest turns tested)


def test_rotation_log_rule():
    """the three branches of the logarithm against known rotations, exp(log) round trips, and the half turn's axis"""
    rng = np.random.default_rng(5)
    for angle in (0.0, 1e-9, 1e-7, 1e-3, 1.0, 3.0, 3.14, math.pi - 1e-7, math.pi - 1e-9, math.pi):
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        Q = ac.rotation(axis, angle)
        w = pr.rotation_log(Q)
        assert abs(np.linalg.norm(w) - angle) <= 1e-9 and 0.0 <= np.linalg.norm(w) <= math.pi + 1e-15
        assert np.abs(pr.rotation_exp(w) - Q).max() <= 1e-9
        if 1e-3 <= angle < 3.1:
            assert np.abs(w - angle * axis).max() <= 1e-12


def test_constructor_refusals_and_set_up_without_a_device():
    V0, faces = pc.mesh("two_tori")
    p = PoseInterpolator(V0, faces, device="cpu")
    assert p.Vm == 159 and p.F == len(faces) and p.anchors is None and len(p.pinned) == 0
    assert sorted(np.nonzero(p.held)[0].tolist()) == [0, 96]           # the least id of each component
    for bad in (V0[:, :2], V0[:0], V0.reshape(-1)):
        with pytest.raises(ValueError, match="rest_vertices"):
            PoseInterpolator(bad, faces, device="cpu")
    with pytest.raises(ValueError, match="face index"):
        PoseInterpolator(V0, faces + 100, device="cpu")
    for anchors, what in (([], "empty"), ([0.5], "integer"), ([0, 159], "outside"), ([-1], "outside"), ([3, 3], "twice"), ([0, 5], "without an anchor")):
        with pytest.raises(ValueError, match=what):
            PoseInterpolator(V0, faces, anchors=anchors, device="cpu")
    q = PoseInterpolator(V0, faces, anchors=[7, 100], device="cpu")
    assert sorted(np.nonzero(q.held)[0].tolist()) == [7, 100]
    V0p, facesp = pc.mesh("pinned")
    pp = PoseInterpolator(V0p, facesp, anchors=[5], device="cpu")      # pinned vertices need no anchor: they are held
    assert pp.pinned.tolist() == [96, 97] and sorted(np.nonzero(pp.held)[0].tolist()) == [5, 96, 97]
    assert sorted(np.nonzero(PoseInterpolator(V0p, facesp, device="cpu").held)[0].tolist()) == [0, 96, 97]
    keys = np.stack([V0, V0], 0)
    for call in (lambda: p.between(V0, V0, [0.5]), lambda: p.sequence(keys, 2)):
        with pytest.raises(_lib.GmeshError, match="no CPU path"):
            call()


def test_component_rows():
    index, off, rows = pose_interp.component_rows(np.array([0, 0, 2, 0, 2, 5]))
    assert index.tolist() == [0, 0, 1, 0, 1, 2] and off.tolist() == [0, 3, 5, 6] and rows.tolist() == [0, 1, 3, 2, 4, 5]
    assert index.dtype == off.dtype == rows.dtype == np.int32


def test_segment_ts_and_frame_count():
    assert pose_interp.segment_ts(0).tolist() == []
    assert pose_interp.segment_ts(3).tolist() == [0.25, 0.5, 0.75]
    assert np.array_equal(pose_interp.segment_ts(4), np.arange(1, 5) / 5.0)
    s = pose_interp.segment_ts(3, "smoothstep")
    assert s.tolist() == [3 * 0.0625 - 2 * 0.015625, 0.5, 3 * 0.5625 - 2 * 0.421875] and s.dtype == np.float64
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="inbetweens"):
            pose_interp.segment_ts(bad)
    with pytest.raises(ValueError, match="ease"):
        pose_interp.segment_ts(2, "cubic")


@pytest.mark.parametrize("name, ret, n", [("gm_pose_interp", "int", 25), ("gm_pose_interp_workspace_bytes", "size_t", 3)])
def test_header_declares_and_lib_types_the_entry_points(name, ret, n):
    text = open(os.path.join(ROOT, "include", "gmesh_hip.h")).read()
    m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, name), text)
    assert m and len(m.group(1).split(",")) == n
    assert name in _lib.header_symbols()
    assert len(_lib.SIGNATURES[name][1]) == n
    assert hasattr(_lib.lib(), name)
    assert "#define GM_POSE_INTERP_BATCH_MAX 64" in text and _lib.GM_POSE_INTERP_BATCH_MAX == 64


def test_workspace_bytes():
    """0 for arguments that would be refused; otherwise the face records once, and per frame 9 doubles per face and 15 per vertex"""
    l = _lib.lib()
    for Vm, F, T in ((0, 10, 1), (-1, 10, 1), (10, -1, 1), (10, 10, 0), (10, 10, 65), (10, 10, -2)):
        assert l.gm_pose_interp_workspace_bytes(Vm, F, T) == 0, (Vm, F, T)
    for Vm, F in ((1, 0), (96, 192), (1073, 2146), (7500, 15000)):
        got = [l.gm_pose_interp_workspace_bytes(Vm, F, T) for T in (1, 2, 3, 64)]
        assert got == sorted(got) and len(set(got)) == 4
        assert got[0] >= 8 * (27 * F + 9 * F + Vm + 15 * Vm)
        assert got[2] - got[1] >= 8 * (9 * F + 15 * Vm)
        assert got[3] <= got[0] + 63 * (8 * (9 * F + 15 * Vm) + 8 * 256)


def test_pose_interp_refuses_before_any_gpu_work():
    l = _lib.lib()
    Vm, F, T, C = 100, 180, 4, 2
    a = 1 << 30                                                        # non-null "pointers", 4 MiB apart: never dereferenced
    names = ("off", "cols", "w", "V0", "faces", "vf_off", "vf_faces", "held", "c_off", "c_rows", "label", "A", "B", "ts", "out", "stats", "ws")
    P = {k: a + (i << 22) for i, k in enumerate(names)}

    def call(T=T, Vm=Vm, F=F, C=C, cg=8, tol=1e-6, nbytes=None, **kw):
        p = dict(P, **kw)
        if nbytes is None:
            nbytes = l.gm_pose_interp_workspace_bytes(Vm, F, T)
        return l.gm_pose_interp(T, Vm, F, p["off"], p["cols"], p["w"], p["V0"], p["faces"], p["vf_off"], p["vf_faces"], p["held"], C, p["c_off"],
                                p["c_rows"], p["label"], p["A"], p["B"], p["ts"], cg, tol, p["out"], p["stats"], p["ws"], nbytes, None)

    def refused(what, rc=1, **kw):
        assert call(**kw) == rc and b"gm_pose_interp" in l.gm_last_error() and what in l.gm_last_error(), (kw, l.gm_last_error())
    need = l.gm_pose_interp_workspace_bytes(Vm, F, T)
    for t in (0, -1, 65):
        refused(b"T =", T=t, nbytes=1 << 20)
    for vm in (0, -5):
        refused(b"Vm", Vm=vm, nbytes=need)
    refused(b"F =", F=-1, nbytes=need)
    for c in (-1, Vm + 1):
        refused(b"C =", C=c)
    refused(b"cg_iterations", cg=0)
    for tol in (-1e-3, float("nan"), float("inf")):
        refused(b"cg_tolerance", tol=tol)
    for k in names:
        if k != "stats":
            refused(b"null", **{k: None})
    # what may be NULL: the faces of a mesh without any, the component arrays without components, stats - these reach the workspace check
    refused(b"workspace", rc=3, F=0, faces=None, vf_faces=None, nbytes=l.gm_pose_interp_workspace_bytes(Vm, 0, T) - 1)
    refused(b"workspace", rc=3, C=0, c_off=None, c_rows=None, label=None, nbytes=need - 1)
    refused(b"workspace", rc=3, stats=None, nbytes=need - 1)
    refused(b"workspace", rc=3, A=P["V0"], B=P["V0"], nbytes=need - 1)             # the keys may be the rest pose, and each other
    refused(b"workspace", rc=3, nbytes=0)
    outs = ("out", "stats", "ws")
    for i, x in enumerate(outs):
        for y in ("V0", "A", "B", "ts") + outs[i + 1:]:
            refused(b"overlaps", **{x: P[y] + 4})
    refused(b"overlaps", A=P["out"] + 12 * Vm * (T - 1) + 4)                        # the [T] extent of V_out
    refused(b"overlaps", ws=P["stats"] + 48 * (T - 1) + 8)
    refused(b"workspace", rc=3, stats=P["out"] + 12 * Vm * T, nbytes=need - 1)


@pytest.mark.parametrize("n", ["-1", "-7"])
def test_cli_refuses_negative_inbetweens_before_any_device_work(n, monkeypatch):
    """SystemExit with a message, raised ahead of every import that would touch the device or read a file (none of the named files
    exists)"""
    import builtins
    real = builtins.__import__

    def no_torch(name, *a, **kw):
        assert name != "torch" and not name.endswith("edittool"), name
        return real(name, *a, **kw)
    monkeypatch.setattr(builtins, "__import__", no_torch)
    with pytest.raises(SystemExit) as e:
        edit_sequence.main(["--object_gaussian", "o.ply", "--object_origin_mesh", "m.obj", "--camera_path", ".", "--render_path", "out",
                            "--handle_sequence", "h.npz", "--inbetweens", n])
    assert "--inbetweens" in str(e.value) and "0 or more" in str(e.value)
