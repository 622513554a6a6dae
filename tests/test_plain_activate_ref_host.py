"""CPU: the numpy definition of the plain model's activation and adjoint (plain_activate_ref.py), its cases, and the gate of
test_gpu_plain_activate.py - shown here to reject five wrong kernels before it is used on the device.

  * the float64 chain equals torch-float64 autograd (F.normalize with eps = 1e-12f, exp, sigmoid) on every row, to 1e-13 of S_abs;
  * the cases are what they claim: read-only, the edge rows where the docstring puts them, the float32 |q| of every clamp-edge row on
    the float64 side of 1e-12f, every gated reference value zero or a normal float32;
  * r_f32: what the float32 restatement reaches per tensor, in units of 2^-24 S_abs - measured here, stored in plain_activate_ref.R_F32;
  * the gate rejects (a) the projection term dropped, (b) the clamp decided at 1e-6, (c) an exp of relative error 1e-5 in d_scaling,
    (d) an accurate 1 - s where s has rounded to 1, (e) upstream rows read without row0 - and accepts the restatement at every N and row0;
  * the norm-wise figure of test_plain_activate_matches_float64_autograd (max |a - b| / max |b| <= 1e-5) accepts (a) and (b) on that
    test's own inputs, which the per-element gate rejects there;
  * the rows kept out of the gate (inf, NaN, an overflowing |q|^2): the float32 restatement does what special_case() states.
Run with -s for the tables."""
import numpy as np
import pytest
import torch

import plain_activate_ref as P


def _sentinel_buffers(n, row0, cap):
    """upstream buffers of `cap` rows, the case's rows at [row0, row0 + n), 0x5A5A5A5A (1.5e16) elsewhere"""
    out = []
    for g in P.upstream(n):
        b = np.full((cap,) + g.shape[1:], np.uint32(0x5A5A5A5A).view(np.float32), np.float32)
        b[row0:row0 + n] = g
        out.append(b)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
def test_float64_chain_equals_autograd():
    xyz, scaling, rot, opac = P.inputs()
    ups = P.upstream()
    leaves = [torch.tensor(a.astype(np.float64), requires_grad=True) for a in (xyz, scaling, rot, opac)]
    outs = (leaves[0] * 1.0, torch.exp(leaves[1]), torch.nn.functional.normalize(leaves[2], eps=float(P.EPS32)), torch.sigmoid(leaves[3]))
    sum((o * torch.tensor(u.astype(np.float64))).sum() for o, u in zip(outs, ups)).backward()
    ref, s_abs = P.case_reference()
    # F.normalize in float64 decides the clamp by the float64 |q|: the same side as the float32 one on every row of the case (asserted below)
    for t, want in zip(P.FWD, outs):
        err = np.abs(ref[t] - want.detach().numpy())
        assert (err <= 1e-13 * s_abs[t]).all(), (t, float(err.max()))
    for t, leaf in zip(P.BWD, leaves):
        err = np.abs(ref[t] - leaf.grad.numpy())
        assert (err <= 1e-13 * s_abs[t]).all(), (t, int(np.argmax(err / np.maximum(s_abs[t], 1e-300))), float(err.max()))


def test_the_cases_are_what_they_claim():
    c = P.case()
    assert all(not v.flags.writeable and v.dtype == np.float32 and v.shape[0] == P.NMAX for k, v in c.items() if k != "row_m87")
    assert (c["scaling"][list(P.ROWS["scaling_edges"])] == np.array(P.SCALING_EDGES, np.float32)[:, None]).all()
    assert 15 <= c["row_m87"] < 255 and (c["scaling"][c["row_m87"]] == -87).all() and (np.abs(c["g_scales"][c["row_m87"]]) >= 0.75).all()
    l64 = np.sqrt((c["rot"].astype(np.float64) ** 2).sum(axis=1))
    l32 = P._len(c["rot"], np.float32)[:, 0]
    # every clamp-edge row: the float32 |q| on the same side of 1e-12f as the float64 one, and neither within 2^-20 of it
    eps = float(P.EPS32)
    assert ((l32 > P.EPS32) == (l64 > eps)).all()
    assert (np.abs(l64 - eps) > 2.0 ** -20 * eps).all() and (np.abs(l32.astype(np.float64) - eps) > 2.0 ** -20 * eps).all()
    below = np.flatnonzero(~(l32 > P.EPS32)).tolist()
    assert below == sorted(list(P.ROWS["rot_below_clamp"]) + [P.ROWS["rot_zero"]])
    assert abs(l64[P.ROWS["rot_above_clamp"]] / 2e-12 - 1) < 1e-6 and all(abs(l64[r] / 5e-13 - 1) < 1e-6 for r in P.ROWS["rot_below_clamp"])
    assert all(1e-8 < l64[r] < 1e-6 for r in P.ROWS["rot_1e-7"]) and all(1e-12 < l64[r] < 1e-10 for r in P.ROWS["rot_1e-11"])
    assert l64[P.ROWS["rot_1e3"]] > 100 and np.count_nonzero(c["rot"][P.ROWS["rot_one_component"]]) == 1
    x = c["opac"][:, 0]
    assert {17.0, -17.0, 80.0, -80.0, 30.0, -30.0, 0.0, 18.0} <= set(x.tolist())
    assert (x > P.BAND_X).sum() >= 10 and ((x > 10) & (x <= P.BAND_X)).sum() >= 10 and (x >= P.ZERO_X).sum() >= 10
    # the gate has no underflow term: every gated reference value is zero or a normal float32 (and finite)
    ref, s_abs = P.case_reference()
    for t in P.TENSORS:
        a = np.abs(ref[t])
        assert np.isfinite(a).all() and ((a == 0) | (a >= P.MIN_NORMAL)).all() and (a <= 3.4e38).all(), t
        assert (s_abs[t] >= a * (1 - 1e-12)).all(), t
    for n in P.NS:                                              # the prefixes are prefixes
        r, _ = P.case_reference(n)
        assert all(np.array_equal(r[t], ref[t][:n]) for t in P.TENSORS)
    s = P.special_case()
    assert all(not v.flags.writeable for v in s.values()) and np.isinf(s["scaling"]).any() and np.isnan(s["rot"]).any()


def test_r_f32_is_measured():
    ref, s_abs = P.case_reference()
    got = P.restatement(*P.inputs(), *P.upstream())
    measured = {t: float(P.ratio(got[t], ref[t], s_abs[t]).max()) for t in P.TENSORS}
    print("\nr_f32 measured / stored: " + "  ".join("%s %.3f / %.1f" % (t, measured[t], P.R_F32[t]) for t in P.TENSORS))
    for t in P.TENSORS:
        assert measured[t] <= P.R_F32[t] <= measured[t] + 0.15, (t, measured[t], P.R_F32[t])
    assert measured["xyz"] == 0 and measured["d_xyz"] == 0                     # copies
    # first-order rounding counts, one unit (2^-24 of the magnitude) per rounding: exp 1; |q|: (squares 1 + sums 3) / 2 + the root 1 = 3, the
    # division 1; sigmoid: exp, sum, division; d_rotation: the reciprocal 4, y 5, y.g 9, y (y.g) 15 beside g, the difference and the product
    # 17; d_opacity: s 3, 1 - s 4, two products
    count = {"scales": 1.0, "rots": 4.0, "opac": 3.0, "d_scaling": 2.0, "d_rotation": 17.0, "d_opacity": 9.0}
    assert all(measured[t] <= count[t] for t in count), measured


@pytest.mark.parametrize("n", P.NS)
@pytest.mark.parametrize("row0, extra", [(0, 0), (37, 0), (37, 63)])
def test_the_gate_accepts_the_restatement(n, row0, extra):
    ref, s_abs = P.case_reference(n)
    ups = _sentinel_buffers(n, row0, row0 + n + extra)
    got = P.restatement(*P.inputs(n), *ups, row0=row0)
    fig = P.check(got, ref, s_abs, P.inputs(n)[3], ups[3], row0)
    assert not P.failures(fig), P.failures(fig)
    assert max(P.worst(fig).values()) <= 0.5 + 1e-9                            # (at most half the bar, by construction)
    # a missing upstream gradient is a zero one
    for k in range(4):
        some = list(ups)
        some[k] = None
        zeros = list(ups)
        zeros[k] = np.zeros_like(ups[k])
        a = P.backward(*P.inputs(n)[1:], *some, np.float64, row0=row0)
        b = P.backward(*P.inputs(n)[1:], *zeros, np.float64, row0=row0)
        assert all(np.array_equal(a[t], b[t]) for t in P.BWD)


@pytest.mark.parametrize("variant", P.VARIANTS)
def test_the_gate_rejects_a_wrong_kernel(variant):
    """each wrong backward must fail one element at least, at the N the device test runs (row0 = 37 for the row0 variant, which equals the
    right kernel at row0 = 0)"""
    expect = {"no_projection": "d_rotation", "clamp_at_1e-6": "d_rotation", "exp_rel_1e-5": "d_scaling", "accurate_one_minus_s": "d_opacity",
              "no_row0": None}[variant]
    for n in P.NS:
        row0 = 37
        ref, s_abs = P.case_reference(n)
        ups = _sentinel_buffers(n, row0, row0 + n + 63)
        got = P.restatement(*P.inputs(n), *ups, variant=variant, row0=row0)
        fig = P.check(got, ref, s_abs, P.inputs(n)[3], ups[3], row0)
        bad = P.failures(fig)
        print("%s, N = %d: %s" % (variant, n, ", ".join("%s %d element(s), worst %.3g x the bar at flat index %d" % b for b in bad) or "accepted"))
        if n == 1 and variant in ("clamp_at_1e-6", "accurate_one_minus_s"):
            continue                                            # (row 0 is an ordinary row: these two differ on edge rows only)
        assert bad, (variant, n)
        assert all(t in P.BWD for t, *_ in bad)                 # the forward half is untouched
        if expect:
            assert [t for t, *_ in bad] == [expect], (variant, n, bad)
        else:
            assert {t for t, *_ in bad} == set(P.BWD), (variant, n, bad)
    # which rows: the clamp variant on the rows between 1e-12 and 1e-6 only, the 1 - s variant on x >= 18 only
    ref, s_abs = P.case_reference()
    got = P.restatement(*P.inputs(), *P.upstream(), variant=variant)
    if variant == "no_row0":
        return
    fig = P.check(got, ref, s_abs, P.inputs()[3], P.upstream()[3])
    rows = np.flatnonzero(~(fig[expect].reshape(P.NMAX, -1) <= 1.0).all(axis=1))
    if variant == "clamp_at_1e-6":
        assert rows.tolist() == sorted(P.ROWS["rot_1e-7"] + P.ROWS["rot_1e-11"] + (P.ROWS["rot_above_clamp"],))
    if variant == "accurate_one_minus_s":
        x = P.inputs()[3][:, 0]
        assert (x[rows] >= P.ZERO_X).all() and rows.size == int((x >= P.ZERO_X).sum())
    if variant in ("no_projection", "exp_rel_1e-5"):
        assert rows.size >= 0.9 * P.NMAX


def test_the_present_norm_wise_figure_accepts_two_of_them():
    """test_plain_activate_matches_float64_autograd holds each gradient to max |a - b| / max |b| <= 1e-5; its rotation gradient's largest
    element is 1.2e12 (row 8, under the clamp), so the ordinary rows are held to ~1e7 absolute: (a) and (b) pass, and so does any
    gradient at all on rows 9.. - while the per-element gate rejects both on the same inputs"""
    xyz, scaling, rot, opac, ups = (P.present_test_inputs())
    a = [t.numpy() for t in (xyz, scaling, rot, opac)]
    u = [t.numpy() for t in ups]
    ref, s_abs = P.reference(*a, *u)
    assert np.abs(ref["d_rotation"]).max() > 1e12
    for variant in (None, "no_projection", "clamp_at_1e-6"):
        got = P.restatement(*a, *u, variant=variant)
        rel = P.present_rel(got["d_rotation"], ref["d_rotation"])
        bad = P.failures(P.check(got, ref, s_abs, a[3], u[3]))
        print("%s: present figure %.3g (bar 1e-5); per-element gate: %s" % (variant, rel, bad or "passes"))
        assert rel <= 1e-5, (variant, rel)                      # the present figure accepts all three
        assert bool(bad) == (variant is not None), (variant, bad)
    # ... and any gradient at all on the ordinary rows
    wrong = ref["d_rotation"].copy()
    wrong[9:] = -3.0 * wrong[9:] + 5.0
    assert P.present_rel(wrong, ref["d_rotation"]) <= 1e-5


def test_the_rows_kept_out_of_the_gate():
    c = P.special_case()
    a = [c[k] for k in ("xyz", "scaling", "rot", "opac")]
    u = [c[k] for k in P.UPSTREAM]
    got = P.restatement(*a, *u)
    assert not P.special_failures(got), P.special_failures(got)
    # the ordinary rows among them pass the gate: nothing leaks from a neighbouring row
    ref, s_abs = P.reference(*a, *u)
    rows = P.ordinary_special_rows()
    fig = P.check({t: got[t][rows] for t in P.TENSORS}, {t: ref[t][rows] for t in P.TENSORS}, {t: s_abs[t][rows] for t in P.TENSORS},
                  a[3][rows], u[3][rows])
    assert not P.failures(fig), P.failures(fig)
    # special_failures itself notices a NaN that spreads, a finite value for exp(89) and a normalised overflowing quaternion
    for t, row, v in (("d_xyz", 3, np.nan), ("scales", P.SPECIAL_ROWS["scaling_89"], 3e38), ("rots", P.SPECIAL_ROWS["rot_1e20"], 0.5)):
        w = {k: v_.copy() for k, v_ in got.items()}
        w[t][row] = v
        assert P.special_failures(w), t
