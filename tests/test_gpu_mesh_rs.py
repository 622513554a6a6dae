"""-m gpu: gm_mesh_rs (the (R, S) producer that replaces pyACAP.GetRS, edittool/__init__.py:102, 109) against its numpy
oracle and the invariants of the construction; then through the Gaussian deformation."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rs(V0, V1, faces, **kw):
    from gpu_utils import T
    from gaussianmesh_amd.deform import mesh_rs
    out = mesh_rs(T(V0), T(V1), T(faces, dtype=torch.int32), **kw)
    return [x.cpu().numpy().astype(np.float64) for x in out]


def _rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def test_invariants_identity_rigid_scale_affine():
    from gaussianmesh_amd import scenes
    verts, faces = scenes.torus_mesh(30, 20)
    I = np.eye(3)
    R, S = _rs(verts, verts, faces)
    assert np.abs(R - I).max() <= 1e-6 and np.abs(S - I).max() <= 1e-6                       # identity -> (I, I)
    Q = _rot([1, 2, -0.5], 0.9)
    R, S = _rs(verts, verts @ Q.T + np.array([0.3, -2.0, 5.0]), faces)
    assert np.abs(R - Q.T).max() <= 1e-5 and np.abs(S - I).max() <= 1e-5                     # rigid motion -> (rotation^T, I)
    R, S = _rs(verts, 1.7 * verts, faces)
    assert np.abs(R - I).max() <= 1e-5 and np.abs(S - 1.7 * I).max() <= 1e-5                 # uniform scale s -> (I, s I)
    # a general affine map A (rotation x shear x anisotropic scale): the one-ring fit reproduces it, R^T S = A
    A = _rot([0.2, 1, 0.4], 0.7) @ np.array([[1.4, 0.3, 0.1], [0.1, 0.8, -0.2], [0.0, 0.25, 1.1]])
    R, S = _rs(verts, verts @ A.T + 0.5, faces)
    Fm = np.einsum("nji,njk->nik", R, S)                                                      # R^T S
    assert np.abs(Fm - A[None]).max() <= 2e-4        # float32 vertices; the normal component rests on the one-ring's O(h^2) bulge
    assert np.abs(np.linalg.det(R) - 1).max() <= 1e-5 and np.abs(S - np.transpose(S, (0, 2, 1))).max() <= 1e-6
    # a FLAT patch (planar one-rings): in-plane exact, the normal direction follows the deformed normal
    g = np.stack(np.meshgrid(np.linspace(-1, 1, 12), np.linspace(-1, 1, 9), indexing="ij"), -1).reshape(-1, 2)
    flat = np.concatenate([g, np.zeros((g.shape[0], 1))], 1)
    idx = np.arange(12 * 9).reshape(12, 9)
    ff = np.concatenate([np.stack([idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:]], -1).reshape(-1, 3),
                         np.stack([idx[:-1, :-1], idx[1:, 1:], idx[:-1, 1:]], -1).reshape(-1, 3)], 0).astype(np.int32)
    R, S = _rs(flat, flat @ A.T, ff)
    Fm = np.einsum("nji,njk->nik", R, S)
    tang = np.array([[1, 0, 0], [0, 1, 0]], float).T
    assert np.abs(Fm @ tang - (A @ tang)[None]).max() <= 2e-5
    nA = np.cross(A[:, 0], A[:, 1]); nA /= np.linalg.norm(nA)
    got_n = Fm @ np.array([0, 0, 1.0])
    assert np.abs(got_n / np.linalg.norm(got_n, axis=1, keepdims=True) - nA).max() <= 1e-4
    assert np.isfinite(R).all() and np.isfinite(S).all()


def test_matches_numpy_oracle_on_random_deformations():
    from gaussianmesh_amd import scenes
    from oracle import mesh_oracle
    rng = np.random.default_rng(2)
    verts, faces = scenes.torus_mesh(40, 24)
    V1 = verts @ _rot([0, 1, 1], 0.4).T * np.array([1.3, 0.8, 1.1]) + 0.05 * rng.normal(size=verts.shape)
    verts32, V132 = verts.astype(np.float32), V1.astype(np.float32)
    R, S, state = _rs(verts32, V132, faces, want_state=True)
    Ro, So = mesh_oracle.mesh_rs(verts32, V132, faces)
    assert np.abs(R - Ro).max() <= 2e-5 and np.abs(S - So).max() <= 2e-5
    assert np.array_equal(state[:, :3], V132.astype(np.float64)) and np.array_equal(state[:, 3:12], R.reshape(-1, 9))
    assert np.array_equal(state[:, 12:], S.reshape(-1, 9))
    # the one-launch variant writes the deformation kernels' gather table directly: identical to state -> gm_pack_mesh_state
    from gpu_utils import T
    from gaussianmesh_amd.deform import mesh_rs, mesh_rs_packed, pack_mesh_state, vertex_face_adjacency
    off, adj = vertex_face_adjacency(faces, verts32.shape[0])
    adjacency = (torch.tensor(off, device="cuda"), torch.tensor(adj, device="cuda"))
    ft = T(faces, dtype=torch.int32)
    st = mesh_rs(T(verts32), T(V132), ft, adjacency=adjacency, want_state=True)[2]
    assert torch.equal(mesh_rs_packed(T(verts32), T(V132), ft, adjacency), pack_mesh_state(st, T(verts32)))
    # a reflected neighbourhood (det F < 0) still gives a proper rotation, and degenerate faces / isolated vertices are inert
    V2 = V132.copy(); V2[:, 0] *= -1
    R2, S2 = _rs(verts32, V2, faces)
    assert np.abs(np.linalg.det(R2) - 1).max() <= 1e-4
    assert np.abs(np.einsum("nji,njk->nik", R2, S2) - np.einsum("nji,njk->nik", *mesh_oracle.mesh_rs(verts32, V2, faces))).max() <= 5e-5
    f_deg = np.concatenate([faces, np.array([[0, 0, 1]], np.int32)], 0)
    v_iso = np.concatenate([verts32, np.array([[9, 9, 9]], np.float32)], 0)
    R3, S3 = _rs(v_iso, np.concatenate([V132, [[1, 2, 3]]], 0).astype(np.float32), f_deg)
    assert np.abs(R3[:-1] - R).max() <= 1e-6 and np.array_equal(R3[-1], np.eye(3)) and np.array_equal(S3[-1], np.eye(3))


def test_converges_to_the_analytic_twist_and_drives_the_deformation():
    """The per-vertex map from the mesh converges (first order in the edge length) to the analytic Jacobian of
    scenes.twist_bend_frame on tangent vectors as the mesh is refined; and the edit step from vertices alone (gm_mesh_rs
    feeding gm_deform) equals the oracle chain."""
    from gpu_utils import T
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.deform import deform_tensors
    errs = []
    for nu, nv in ((50, 38), (100, 75), (200, 150)):
        verts, faces = scenes.torus_mesh(nu, nv)
        V1, Ra, Sa = scenes.twist_bend_frame(verts, t=11)
        R, S = _rs(verts.astype(np.float32), V1.astype(np.float32), faces)
        # compare the action on tangent vectors: a surface cannot tell how the analytic map stretches along the normal
        tri = faces[:: max(1, faces.shape[0] // 4000)]
        v = tri[:, 0]
        e = verts[tri[:, 1]] - verts[v]
        e /= np.linalg.norm(e, axis=1, keepdims=True)
        got = np.einsum("nji,njk,nk->ni", R[v], S[v], e)            # R^T S: the one-ring affine map
        want = np.einsum("nji,njk,nk->ni", Ra[v], Sa[v], e)         # the analytic Jacobian
        errs.append(np.abs(got - want).max())
    assert errs[1] < 0.6 * errs[0] and errs[2] < 0.6 * errs[1] and errs[2] <= 2e-2, errs
    # the whole edit step from vertices alone: gm_mesh_rs -> gm_deform on the GPU == oracle mesh_rs -> oracle deform
    from oracle import mesh_oracle, oracle as orc
    verts, faces = scenes.torus_mesh(100, 75)
    V1, _, _ = scenes.twist_bend_frame(verts, t=11)
    verts32, V132 = verts.astype(np.float32), V1.astype(np.float32)
    cl = scenes.bind_cloud_to_mesh(4000, verts, faces, seed=3)
    cov = scenes.cov3d_from_scale_rot(cl["scales"], cl["rots"]).astype(np.float32)
    R, S = _rs(verts32, V132, faces)
    p1, c1, r1, _ = deform_tensors(T(cl["tri"], dtype=torch.int32), T(cl["weights"]), T(V132 - verts32), T(R), T(S), T(cov), T(cl["means"]))
    Ro, So = mesh_oracle.mesh_rs(verts32, V132, faces)
    p_ref, c_ref, r_ref = orc.deform(cl["tri"], cl["weights"], V132 - verts32, Ro.astype(np.float32), So.astype(np.float32), cov, cl["means"])
    assert np.abs(p1.cpu().numpy() - p_ref).max() <= 1e-5 * np.abs(p_ref).max()
    assert np.abs(c1.cpu().numpy() - c_ref).max() <= 1e-4 * np.abs(c_ref).max()
    assert np.abs(r1.cpu().numpy() - r_ref).max() <= 1e-4


# ---------------------------------------------------------------------------------------------------------------------------
# every path of mesh_rs_kernel: the cases of mesh_rs_cases.py (test_mesh_rs_cases_host.py pins which case reaches which path)
import functools  # noqa: E402

import mesh_rs_cases as mc  # noqa: E402

I3 = np.eye(3)


def _device_mesh(c):
    from gpu_utils import T
    from gaussianmesh_amd.deform import vertex_face_adjacency
    off, adj = vertex_face_adjacency(c["faces"], c["V0"].shape[0])
    return T(c["V0"]), T(c["V1"]), T(c["faces"], dtype=torch.int32), (torch.tensor(off, device="cuda"), torch.tensor(adj, device="cuda"))


@functools.lru_cache(maxsize=None)
def _gpu(name):
    """One launch of each entry point on the case, shared by the tests below: R, S, state (float64 copies), the packed table and
    what pack_mesh_state makes of state."""
    from gaussianmesh_amd.deform import mesh_rs, mesh_rs_packed, pack_mesh_state
    V0, V1, faces, adjacency = _device_mesh(mc.cases()[name])
    R, S, state = mesh_rs(V0, V1, faces, adjacency=adjacency, want_state=True)
    packed = mesh_rs_packed(V0, V1, faces, adjacency)
    repacked = pack_mesh_state(state, V0)
    return tuple(x.cpu().numpy().astype(np.float64) for x in (R, S, state)) + (packed.cpu(), repacked.cpu())


def _bar(expected):
    return 2e-5 * max(1.0, float(np.abs(expected).max()))


@pytest.mark.parametrize("name", list(mc.cases()))
def test_case_structure_and_oracle(name):
    """Structure on every vertex of every case (the collapses included), the oracle's S everywhere, its F = R^T S wherever two
    stretches survive, its R wherever the proper polar factor is well conditioned ((s2 + s3) / s1 >= 0.1) - which on the plane
    squashes, stretches, the reflection and every fan apex is everywhere."""
    c = mc.cases()[name]
    R, S, state, _, _ = _gpu(name)
    Ro, So, F, sv = mc.oracle_of(name)
    assert np.isfinite(R).all() and np.isfinite(S).all()
    orth = np.abs(np.einsum("nji,njk->nik", R, R) - I3).max()
    det = np.abs(np.linalg.det(R) - 1).max()
    sym = np.abs(S - S.transpose(0, 2, 1)).max()
    wc = mc.well_conditioned(sv, F)
    rank2 = sv[:, 1] > mc.DEAD * sv[:, 0]
    dR = np.abs(R - Ro)[wc].max(initial=0.0)
    dS = np.abs(S - So).max()
    dF = np.abs(np.einsum("nji,njk->nik", R, S) - F)[rank2].max(initial=0.0)
    print("%s: |R^T R - I| %.2e  |det R - 1| %.2e  |S - S^T| %.2e  |R - Ro| %.2e on %d of %d (all: %.2e)  |S - So| %.2e  |R^T S - F| %.2e"
          % (name, orth, det, sym, dR, wc.sum(), wc.size, np.abs(R - Ro).max(), dS, dF))
    assert orth <= 1e-5 and det <= 1e-5
    assert sym <= 1e-6 * max(1.0, float(np.abs(So).max()))
    assert dS <= _bar(So)
    assert dF <= _bar(F)
    assert not (~wc & ~mc.may_exclude(c)).any()
    assert dR <= _bar(Ro)
    if c["apex"] is not None:                                       # ring chunking: 3 .. 33 faces at the apex, never excluded
        assert wc[c["apex"]].all()
        assert np.abs(R - Ro)[c["apex"]].max() <= 2e-5 and np.abs(S - So)[c["apex"]].max() <= _bar(So[c["apex"]])
    inert = mc.inert_vertices(c)
    assert np.array_equal(R[inert], np.broadcast_to(I3, R[inert].shape)) and np.array_equal(S[inert], np.broadcast_to(I3, S[inert].shape))
    if name == "point":                                             # F = 0: no rotation, no stretch
        assert np.array_equal(R, np.broadcast_to(I3, R.shape)) and not S.any()
    if name == "line_exact":                                        # rank 1: the identity rotation by convention, S = |F| along the line
        assert np.array_equal(R, np.broadcast_to(I3, R.shape))


@pytest.mark.parametrize("name", ["extras_noisy", "extras_squash_0"])
def test_extras_touch_only_their_rows(name):
    """A vertex in no face and one whose only face is degenerate come out as (I, I) exactly; a duplicated face, a reversed one and a
    179.8-degree sliver change the rows of their own corners only - and those still match the oracle, which scatters per face."""
    c = mc.cases()[name]
    rows = c["rows"]
    R, S, _, _, _ = _gpu(name)
    Ro, So, F, sv = mc.oracle_of(name)
    for k in (rows["isolated"], rows["degenerate_only"]):
        assert np.array_equal(R[k], I3) and np.array_equal(S[k], I3)
    touched = sorted(set(rows["duplicate"] + rows["reversed"] + rows["sliver"] + [rows["degenerate_other"]]))
    assert mc.well_conditioned(sv, F)[touched].all()
    print("%s: touched rows |R - Ro| %.2e |S - So| %.2e" % (name, np.abs(R - Ro)[touched].max(), np.abs(S - So)[touched].max()))
    assert np.abs(R - Ro)[touched].max() <= 2e-5 and np.abs(S - So)[touched].max() <= _bar(So[touched])
    # the plain torus under the same deformation: every other row is the same, bit for bit
    plain = "torus_noisy" if name == "extras_noisy" else mc.eps_name(0.0)
    assert np.array_equal(mc.cases()[plain]["V1"], c["V1"][:600])
    Rp, Sp, _, _, _ = _gpu(plain)
    same = np.setdiff1d(np.arange(600), touched)
    assert np.array_equal(R[same], Rp[same]) and np.array_equal(S[same], Sp[same])
    changed = np.setdiff1d(touched, [rows["degenerate_other"], 602])
    assert (np.abs(R[changed] - Rp[changed]).max((1, 2)) > 0).all()             # ... and the extras did reach the kernel


@pytest.mark.parametrize("name", list(mc.cases()))
def test_case_three_outputs_agree(name):
    c = mc.cases()[name]
    R, S, state, packed, repacked = _gpu(name)
    assert np.array_equal(state[:, :3], c["V1"].astype(np.float64))
    assert np.array_equal(state[:, 3:12], R.reshape(-1, 9)) and np.array_equal(state[:, 12:], S.reshape(-1, 9))
    assert packed.shape == (c["V0"].shape[0], 24) and torch.equal(packed, repacked)


def test_batch_of_diverging_frames_equals_single_launches():
    """GM_BATCH_MAX frames over the torus in one launch, every frame on another route (Newton, eigen-decomposition at full rank,
    squashed flat, reflected, collapsed to a line and to a point, identity): bit-equal to the eight single launches."""
    from gpu_utils import T
    from gaussianmesh_amd import _lib
    from gaussianmesh_amd.deform import mesh_rs_packed_batch
    assert len(mc.BATCH_FRAMES) == _lib.GM_BATCH_MAX == 8
    cs = [mc.cases()[n] for n in mc.BATCH_FRAMES]
    assert all(np.array_equal(c["V0"], cs[0]["V0"]) and np.array_equal(c["faces"], cs[0]["faces"]) for c in cs)
    V0, _, faces, adjacency = _device_mesh(cs[0])
    tables = mesh_rs_packed_batch(V0, [T(c["V1"]) for c in cs], faces, adjacency)
    for n, t in zip(mc.BATCH_FRAMES, tables):
        assert torch.equal(t.cpu(), _gpu(n)[3]), n


def test_squashed_frame_drives_the_deformation():
    """2000 Gaussians bound to the torus, deformed by the frame that squashes it onto a plane: the rotations gm_deform returns
    are orthonormal and the whole step equals the oracle chain (mesh_oracle.mesh_rs -> oracle.deform)."""
    from gpu_utils import T
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.deform import deform_tensors
    from oracle import oracle as orc
    c = mc.cases()[mc.eps_name(0.0)]
    V0, V1, faces = c["V0"], c["V1"], c["faces"]
    cl = scenes.bind_cloud_to_mesh(2000, V0.astype(np.float64), faces, seed=3)
    cov = scenes.cov3d_from_scale_rot(cl["scales"], cl["rots"]).astype(np.float32)
    R, S, _, _, _ = _gpu(c["name"])
    p1, c1, r1, _ = deform_tensors(T(cl["tri"], dtype=torch.int32), T(cl["weights"]), T(V1 - V0), T(R), T(S), T(cov), T(cl["means"]))
    Ro, So, _, _ = mc.oracle_of(c["name"])
    p_ref, c_ref, r_ref = orc.deform(cl["tri"], cl["weights"], V1 - V0, Ro.astype(np.float32), So.astype(np.float32), cov, cl["means"])
    r1 = r1.cpu().numpy().astype(np.float64)
    orth = np.abs(np.einsum("nij,nkj->nik", r1, r1) - I3).max()
    print("squashed frame: rotation |r r^T - I| %.2e  |r - r_ref| %.2e  pos %.2e  cov %.2e" % (
        orth, np.abs(r1 - r_ref).max(), np.abs(p1.cpu().numpy() - p_ref).max() / np.abs(p_ref).max(),
        np.abs(c1.cpu().numpy() - c_ref).max() / np.abs(c_ref).max()))
    assert orth <= 1e-4
    assert np.abs(p1.cpu().numpy() - p_ref).max() <= 1e-5 * np.abs(p_ref).max()
    assert np.abs(c1.cpu().numpy() - c_ref).max() <= 1e-4 * np.abs(c_ref).max()
    assert np.abs(r1 - r_ref).max() <= 1e-4
