"""CPU: the numpy definition of the deform / shade row body (deform_ref.py) on the cases of deform_cases.py.

  * r_f32: what a correct float32 evaluator reaches against float64, per kind and tensor, in units of 2^-24 S_abs - measured here, stored in
    deform_ref.R_F32, and under the first-order rounding count of each chain (derived in deform_ref's docstring);
  * the per-element gate ratio <= 2 r_f32 of test_gpu_deform_rows.py rejects every wrong variant of the emulation, among them ones the
    tensor max-norm gate of test_gpu_parity.py::test_deform_and_sh_colors lets through;
  * exact facts: one-hot weights copy a vertex's rotation and displacement, the identity table copies the rest covariance, the clamp rows
    lie on the side they were built for.
Run with -s for the two tables."""
import math

import numpy as np
import pytest

import deform_cases as dc
import deform_ref as ref


def _emulate(kind, deg, campos, variant=None, case=None):
    """the float32 evaluator (or a wrong variant of it) on all 257 rows: stage 2 from its own stage 1"""
    c = case or dc.case(kind)
    v1 = variant if variant in ref.STAGE1_VARIANTS else None
    v2 = variant if variant in ref.STAGE2_VARIANTS else None
    pos, O, Rt = ref.stage1(*ref.stage1_inputs(c), np.float32, variant=v1)
    rgb = ref.stage2(deg, pos, Rt, campos, dc.shs(kind, deg), np.float32, variant=v2)
    assert all(a.dtype == np.float32 for a in (pos, O, Rt, rgb))
    return pos, O, Rt, rgb


def test_r_f32_is_measured_and_under_its_rounding_count():
    measured = {k: dict.fromkeys(ref.TENSORS, 0.0) for k in dc.KINDS}
    per_degree = {k: [0.0] * 4 for k in dc.KINDS}
    for kind in dc.KINDS:
        for deg in range(4):
            for _, campos in dc.colour_cameras(kind):
                pos, O, Rt, rgb = _emulate(kind, deg, campos)
                w = ref.worst(ref.row_ratios(dc.case(kind), deg, campos, dc.shs(kind, deg), pos, O, Rt, rgb))
                for t in ref.TENSORS:
                    measured[kind][t] = max(measured[kind][t], w[t][0])
                per_degree[kind][deg] = max(per_degree[kind][deg], w["colour"][0])
    print("\nr_f32 (worst ratio of the float32 emulation, 257 rows, degrees 0..3, both cameras) / stored / rounding count")
    for kind in dc.KINDS:
        print("  %-8s" % kind + "".join("  %s %.3f / %.1f / %s" % (t, measured[kind][t], ref.R_F32[kind][t],
                                                                 ref.COUNT[t] if t != "colour" else max(ref.COUNT[t])) for t in ref.TENSORS))
        print("           colour per degree: " + "  ".join("D%d %.3f (count %.1f)" % (d, per_degree[kind][d], ref.COUNT["colour"][d]) for d in range(4)))
    for kind in dc.KINDS:
        for t in ("pos", "rot", "cov"):
            assert measured[kind][t] <= ref.COUNT[t], (kind, t, measured[kind][t])
        for d in range(4):
            assert per_degree[kind][d] <= ref.COUNT["colour"][d], (kind, d, per_degree[kind][d])
        for t in ref.TENSORS:                           # the stored constants are these measurements, rounded up to one decimal
            assert measured[kind][t] <= ref.R_F32[kind][t] <= measured[kind][t] + 0.15, (kind, t, measured[kind][t], ref.R_F32[kind][t])


def _fails_new_gate(kind, ratios):
    return any(not (ratios[t].max() <= 2.0 * ref.R_F32[kind][t]) for t in ref.TENSORS)


@pytest.mark.parametrize("variant", ref.STAGE1_VARIANTS + ref.STAGE2_VARIANTS)
def test_the_per_element_gate_rejects_a_wrong_evaluator(variant):
    """each wrong variant of the emulation on every kind (stage-1 variants at degree 3, colour variants at every degree), far camera:
    it must fail ratio <= 2 r_f32 somewhere; printed next to the verdict of the old tensor max-norm gate on the same results"""
    degrees = (3,) if variant in ref.STAGE1_VARIANTS else (0, 1, 2, 3)
    rejected, lines = {}, []
    for kind in dc.KINDS:
        for deg in degrees:
            out = _emulate(kind, deg, dc.CAMPOS, variant)
            ratios = ref.row_ratios(dc.case(kind), deg, dc.CAMPOS, dc.shs(kind, deg), *out)
            new = _fails_new_gate(kind, ratios)
            old = not ref.old_gate_passes(dc.case(kind), deg, dc.CAMPOS, dc.shs(kind, deg), *out)
            rejected[kind, deg] = (new, old)
            w = ref.worst(ratios)
            of_bar = {n: (w[n][0] / (2.0 * ref.R_F32[kind][n]) if ref.R_F32[kind][n] else (math.inf if w[n][0] else 0.0)) for n in ref.TENSORS}
            t = max(ref.TENSORS, key=of_bar.get)
            lines.append("  %-18s %-8s D%d  new gate: %-6s (worst %s %.3g x its bar, row %d)  old 1e-5 max gate: %s" % (
                variant, kind, deg, "FAILS" if new else "passes", t, of_bar[t], w[t][1], "FAILS" if old else "passes"))
    print("\n" + "\n".join(lines))
    assert any(new for new, _ in rejected.values()), variant
    if variant == "flush_O":
        assert rejected["needle", 3] == (True, False), "the flushed small covariances: through the old gate, caught by the new one"
    # none of these is a borderline miss: the correct evaluator is at most 0.5 of the bar by construction, a wrong one far beyond it
    correct = _emulate("twist", 3, dc.CAMPOS)
    assert not _fails_new_gate("twist", ref.row_ratios(dc.case("twist"), 3, dc.CAMPOS, dc.shs("twist", 3), *correct))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_onehot_rows_copy_their_vertex_exactly(dtype):
    c = dc.case("onehot")
    pos, O, Rt = ref.stage1(*ref.stage1_inputs(c), dtype)
    corner = np.arange(dc.NMAX) % 3
    assert set(corner) == {0, 1, 2}
    v = c["tri"][np.arange(dc.NMAX), corner]
    assert np.array_equal(Rt, c["Rv"][v].reshape(-1, 3, 3).transpose(0, 2, 1).reshape(-1, 9).astype(dtype))
    assert np.array_equal(pos, c["pos"].astype(dtype) + c["dV"][v].astype(dtype))
    # R = S = I, dV = 0: the covariance and the centre come through untouched
    ident = dict(c, **dc.identity_table())
    assert not ident["dV"].any()
    pos, O, Rt = ref.stage1(*ref.stage1_inputs(ident), dtype)
    assert np.array_equal(O, c["cov"].reshape(-1, 9).astype(dtype)) and np.array_equal(pos, c["pos"].astype(dtype))
    assert np.array_equal(Rt, np.tile(np.eye(3).reshape(1, 9), (dc.NMAX, 1)))


def test_clamp_rows_land_on_their_side():
    c = dc.case("clamp")
    pos, _, Rt = ref.stage1(*ref.stage1_inputs(c), np.float64)
    for D, rows in dc.CLAMP_ROWS.items():
        rows = np.array(rows)
        shs = dc.shs("clamp", D)[rows].astype(np.float64)
        lifted = shs.copy()
        lifted[:, 0, :] += 8.0 / float(np.float32(ref.SH_C0))                  # r + 0.5 itself, from under the clamp
        v = ref.stage2(D, pos[rows], Rt[rows], dc.CAMPOS, lifted, np.float64) - 8.0
        target = np.tile(np.array(dc.CLAMP_TARGETS), 2)[:, None]
        assert np.array_equal(np.sign(v), np.sign(np.broadcast_to(target, v.shape))), (D, v)
        assert (np.abs(v - target) <= 1.5 * ref.U).all(), (D, v - target)      # (the DC's own float32 rounding: half an ulp of |S0| < 8, times C0)
        rgb = ref.stage2(D, pos[rows], Rt[rows], dc.CAMPOS, shs, np.float64)
        assert np.array_equal(rgb > 0, np.broadcast_to(target > 0, rgb.shape)), D


def test_the_cases_are_what_they_claim():
    for kind in dc.KINDS:
        c = dc.case(kind)
        assert c["tri"].shape == (dc.NMAX, 3) and c["cov"].shape == (dc.NMAX, 3, 3) and c["shs"].shape == (dc.NMAX, 16, 3)
        assert all(not c[k].flags.writeable for k in ("tri", "w", "cov", "pos", "shs", "state", "dV", "Rv", "Sv"))
        skew = np.where((c["cov"] != c["cov"].transpose(0, 2, 1)).any((1, 2)))[0]
        assert tuple(skew) == (dc.SKEW_ROWS if kind == "needle" else ()), (kind, skew)
        for deg in range(4):
            s = dc.shs(kind, deg)
            assert np.isnan(s[:, (deg + 1) ** 2:]).all() and np.isfinite(s[:, :(deg + 1) ** 2]).all()
        near = dc.near_camera(kind)
        dist = np.linalg.norm(ref.stage1_reference(c)["pos"][0][dc.NEAR_ROW] - near.astype(np.float64))
        assert 0.9e-3 < dist < 1.1e-3, (kind, dist)
    w = dc.case("outside")["w"]
    assert (w < 0).any(1).sum() > 60 and (w > 1).any(1).sum() > 60 and np.abs(w.sum(1) - 1).max() < 1e-5
    assert np.array_equal(np.sort(dc.case("onehot")["w"], axis=1), np.tile(np.array([0, 0, 1], np.float32), (dc.NMAX, 1)))
    O = ref.stage1_reference(dc.case("needle"))["cov"][0]
    assert math.log10(np.abs(O).max() / np.abs(O).max(1).min()) > 6, "needle: covariances over many orders of magnitude"
