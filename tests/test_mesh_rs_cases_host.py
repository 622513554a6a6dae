"""Host only: the mesh_rs cases (mesh_rs_cases.py) reach the kernel paths they are named for, and the float64 oracle
(oracle/mesh_oracle.py) is right on them - against its own construction everywhere and against the closed form where the
deformation is affine.  The GPU tests (test_gpu_mesh_rs.py) then compare the kernel with this oracle."""
import numpy as np
import pytest

import mesh_rs_cases as mc

NAMES = list(mc.cases())
I3 = np.eye(3)


def _bar(expected, rel=2e-5):
    """The bar test_gpu_mesh_rs.py grants on random deformations, relative to the largest entry of the expected tensor."""
    return rel * max(1.0, float(np.abs(expected).max()))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_is_a_polar_decomposition_of_its_fit(name):
    c = mc.cases()[name]
    R, S, F, sv = mc.oracle_of(name)
    Vm = c["V0"].shape[0]
    assert R.shape == S.shape == F.shape == (Vm, 3, 3) and sv.shape == (Vm, 3)
    assert np.isfinite(R).all() and np.isfinite(S).all() and np.isfinite(F).all()
    assert (sv[:, 0] >= sv[:, 1]).all() and (sv[:, 1] >= sv[:, 2]).all() and (sv[:, 2] >= 0).all()
    assert np.abs(np.einsum("nji,njk->nik", R, R) - I3).max() <= 1e-12 and np.abs(np.linalg.det(R) - 1).max() <= 1e-12
    scale = max(1.0, float(np.abs(F).max()))
    assert np.abs(S - S.transpose(0, 2, 1)).max() <= 1e-12 * scale
    assert np.abs(np.einsum("nji,njk->nik", S, S) - np.einsum("nji,njk->nik", F, F)).max() <= 1e-12 * scale * scale
    rank2 = sv[:, 1] > mc.DEAD * sv[:, 0]
    assert np.abs(np.einsum("nji,njk->nik", R, S) - F)[rank2].max(initial=0.0) <= 1e-12 * scale
    inert = mc.inert_vertices(c)
    assert np.array_equal(R[inert], np.broadcast_to(I3, R[inert].shape)) and np.array_equal(S[inert], np.broadcast_to(I3, S[inert].shape))
    # the two-value return is what it was
    from oracle import mesh_oracle
    two = mesh_oracle.mesh_rs(c["V0"], c["V1"], c["faces"])
    assert len(two) == 2 and np.array_equal(two[0], R) and np.array_equal(two[1], S)


@pytest.mark.parametrize("name", [n for n in NAMES if mc.cases()[n]["A"] is not None])
def test_oracle_matches_the_closed_form_on_affine_cases(name):
    """V1 = float32(V0 A^T + t), A = U diag(sigma) W^T: the fit is A, S = W diag(sigma) W^T whatever the rank, and
    R = (U W^T)^T wherever two stretches survive and the proper polar factor is well conditioned.  (Every vertex of the torus
    has a non-planar one-ring, so none of them leans on the normal regularisation.)"""
    c = mc.cases()[name]
    R, S, F, sv = mc.oracle_of(name)
    A, Sa = c["A"], c["W"] @ np.diag(c["sigma"]) @ c["W"].T
    Ra = (c["U"] @ c["W"].T).T
    assert not mc.inert_vertices(c).any()
    eF, eS = np.abs(F - A).max(), np.abs(S - Sa).max()
    wc = mc.well_conditioned(sv, F) & (sv[:, 1] > mc.DEAD * sv[:, 0])
    eR = np.abs(R - Ra)[wc].max(initial=0.0)
    print("%s: |F - A| %.2e  |S - Sa| %.2e  |R - Ra| %.2e on %d vertices" % (name, eF, eS, eR, wc.sum()))
    # F and S carry the float32 rounding of V1's coordinates, which grows with |A|: bars relative to the largest expected entry.
    # R inherits the error of F divided by s2 + s3 (first-order perturbation of the proper polar factor; s3 signed).
    s = sorted(np.abs(c["sigma"]), reverse=True)
    gap = s[1] + (s[2] if np.prod(c["sigma"]) >= 0 else -s[2])
    assert eF <= _bar(A) and eS <= _bar(Sa)
    assert not wc.any() or eR <= _bar(A) / min(1.0, gap)
    if c["full"]:
        assert wc.all()


@pytest.mark.parametrize("name", NAMES)
def test_conditioning_rule_excludes_only_what_it_may(name):
    c = mc.cases()[name]
    _, _, F, sv = mc.oracle_of(name)
    wc = mc.well_conditioned(sv, F)
    assert not (~wc & ~mc.may_exclude(c)).any(), "the rule hides vertices %s of %s" % (np.nonzero(~wc & ~mc.may_exclude(c))[0], name)
    if c["apex"] is not None:
        assert wc[c["apex"]].all()                                  # never an apex


def test_every_route_is_populated_by_its_case():
    got = {}
    for name, c in mc.cases().items():
        _, _, F, _ = mc.oracle_of(name)
        inert = mc.inert_vertices(c)
        r = mc.route(F, inert)
        got[name] = r
        if c["route"] is not None:
            assert not inert.any() and (r == c["route"]).all(), (name, c["route"], dict(zip(*np.unique(r, return_counts=True))))
    for name in ("squash_0.01", "squash_0.001", "identity", "stretch_100_100_1", "stretch_20_1_1", "stretch_16_1_1"):
        assert (got[name] == mc.NEWTON).sum() == 600
    for name in ("squash_0.0004", "reflection", "stretch_100_1_1"):       # both sides of 27 det^2 > 1e-6 fro^3, det < 0, the fro^3 side
        assert (got[name] == mc.JACOBI_FULL).sum() == 600
    for e in (1e-5, 1e-6, 1e-7, 1e-9, 0.0):
        assert (got[mc.eps_name(e)] == mc.ONE_COLLAPSED).sum() == 600
    for name in ("plane_exact", "line", "line_1e-7"):
        assert (got[name] == mc.ONE_COLLAPSED).sum() == 600
    for name in ("line_exact", "point"):
        assert (got[name] == mc.MORE_COLLAPSED).sum() == 600
    # an exactly representable collapse really is one: no float32 residue in the fit
    assert mc.oracle_of("point")[2].any() == False and (mc.oracle_of("line_exact")[3][:, 1] <= 1e-15).all()  # noqa: E712
    for name in ("extras_noisy", "extras_squash_0"):
        rows = mc.cases()[name]["rows"]
        assert got[name][rows["isolated"]] == mc.INERT and got[name][rows["degenerate_only"]] == mc.INERT and (got[name] == mc.INERT).sum() == 2
    assert (got["strip1"] == mc.INERT).all() and got["strip1"].shape == (1,)
    # the noisy cases mix routes inside one wave
    for name in ("torus_noisy", "fans_concatenated", "strip65"):
        assert {mc.NEWTON, mc.JACOBI_FULL} <= set(got[name])
    # a batch of BATCH_FRAMES diverges in control flow: four routes among its frames
    assert {got[n][0] for n in mc.BATCH_FRAMES} == {mc.NEWTON, mc.JACOBI_FULL, mc.ONE_COLLAPSED, mc.MORE_COLLAPSED}


def test_every_ring_size_and_chunk_count_is_populated():
    """The kernel reads a one-ring in chunks of 8 faces: 1 chunk (rings 1 .. 8), exactly full (8, 16), one over (9, 17), five chunks
    with a clamped tail of one (33)."""
    cs = mc.cases()
    for n in mc.FAN_VALENCES:
        for kind in ("regular", "random"):
            c = cs["fan%d_%s" % (n, kind)]
            ring = mc.ring_sizes(c)
            assert ring[0] == n and (ring[1:] == 2).all() and c["V0"].shape[0] == n + 1
    cat = cs["fans_concatenated"]
    assert sorted(mc.ring_sizes(cat)[cat["apex"]]) == sorted(mc.FAN_VALENCES) and cat["apex"].max() < 128     # all apexes in the first two waves
    assert sorted({(int(n) + 7) // 8 for n in mc.ring_sizes(cat)[cat["apex"][cat["apex"] < 64]]}) == [1, 2, 3]
    assert (mc.ring_sizes(cs["squash_0"]) == 6).all() and cs["squash_0"]["V0"].shape[0] == 600 and 600 % 64 != 0
    for Vm in mc.STRIP_SIZES:
        c = cs["strip%d" % Vm]
        assert c["V0"].shape[0] == Vm and c["faces"].shape[0] == max(Vm - 2, 0)
        if Vm > 1:
            assert sorted(set(mc.ring_sizes(c))) == [1, 2, 3]
    ex = cs["extras_noisy"]
    ring, rows = mc.ring_sizes(ex), ex["rows"]
    assert ring[rows["isolated"]] == 0 and ring[rows["degenerate_only"]] == 2 and ring[602] == 1
    assert (ring[rows["duplicate"]] == 7).all() and ring[rows["degenerate_other"]] == 7
    # negative cotangents: the sliver (179.8 degrees), the valence-3 apex (120 degrees), the irregular rims
    a, b = ex["V0"][rows["sliver"][0]].astype(float) - ex["V0"][602], ex["V0"][rows["sliver"][2]].astype(float) - ex["V0"][602]
    assert (a * b).sum() / np.linalg.norm(a) / np.linalg.norm(b) < np.cos(np.radians(179.0))
    assert mc.obtuse_corners(cs["fan3_regular"]) == 3 and mc.obtuse_corners(cs["fan3_random"]) > 0
    assert sum(mc.obtuse_corners(cs["fan%d_random" % n]) for n in mc.FAN_VALENCES[1:]) > 0
    assert mc.obtuse_corners(ex) > mc.obtuse_corners(cs["torus_noisy"])


def test_reflection_sign_comes_from_the_svd_factors():
    """At rank 2 det(F) is rounding noise of either sign; the oracle's R must be proper regardless."""
    from oracle import mesh_oracle
    V0, faces = mc.torus()
    for seed in range(4):                                           # exact plane squashes along random axes
        rng = np.random.default_rng(seed)
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        V1, _ = mc.affine(V0, (1.3, 0.8, 0.0), U=q, W=mc.W_ROT)
        R, S = mesh_oracle.mesh_rs(V0, V1, faces)
        assert np.abs(np.linalg.det(R) - 1).max() <= 1e-12
