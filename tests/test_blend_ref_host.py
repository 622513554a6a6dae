"""CPU tests of the blend stage's float64 reference (blend_ref.py) and of the edge scenes (blend_edge_scenes.py) against the C oracle.
No GPU.  For every family: the preconditions hold on the oracle's preprocess and binning; the float64 forward agrees with
oracle.render_fwd (colour to FWD_TOL, final_T to the pixel's rounding bound, n_contrib exactly on unambiguous pixels); the float64 backward
agrees with oracle.render_bwd element by element in units of 2^-23 S_abs - the worst ratio, r_oracle, is what the GPU bound
c = 4 max(r_oracle, 4) of test_gpu_blend_edges.py is built on (blend_edge_scenes.R_ORACLE records it per kind of family; this test
holds the record to the measurement)."""
import functools

import numpy as np
import pytest

import blend_edge_scenes as es
import blend_ref

FWD_TOL = 1e-4
U = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def case(name):
    from oracle import oracle as orc
    orc.build()
    sc, info = es.family(name, orc)
    W, H = sc["W"], sc["H"]
    fw = es.oracle_forward(orc, sc)
    ref0 = es.reference_of(fw, W, H)
    dpix = es.dpix_for(sc, info, ref0)
    ref = es.reference_of(fw, W, H, dL_dpix=dpix)
    bw = orc.render_bwd(W, H, fw["bins"], fw["geo"], es.BG, fw["final_T"], fw["n_contrib"], dpix)
    return sc, info, fw, ref, dpix, bw


def ratios(got, ref, what=""):
    """per output: worst |got - ref| / (2^-23 S_abs); elements with S_abs == 0 must be exactly 0 in both"""
    dm, dc, dop, dcol = got
    out = {}
    for name, g in (("dmean2D", dm[:, :2]), ("dconic", dc[:, [0, 1, 3]]), ("dopacity", dop.reshape(-1)), ("dcolor", dcol)):
        r, S = ref[name], ref["S_" + name]
        g = np.asarray(g, np.float64).reshape(r.shape)
        zero = S == 0
        assert (g[zero] == 0).all() and (r[zero] == 0).all(), "%s %s: an element nothing contributes to is not 0" % (what, name)
        out[name] = float((np.abs(g - r)[~zero] / (U * S[~zero])).max()) if (~zero).any() else 0.0
    return out


@pytest.mark.parametrize("name", es.FAMILIES)
def test_family_preconditions_and_ambiguity_cap(name, oracle):
    """what a family relies on holds on the oracle's records, and outside the pairs it names the reference finds NO ambiguous
    (pixel, entry) pair: every family here could be nudged to zero (the cap of 0.5 % of the pixels is not used)"""
    sc, info, fw, ref, _, _ = case(name)
    stray = es.check_preconditions(sc, info, fw, ref)
    named = sum(1 for d in info["designated"] if d["ambiguous"])
    print("ambiguity %-20s %dx%d: %d pixel(s) with a named ambiguous pair, %d other(s)" % (name, sc["W"], sc["H"], named, stray))
    assert stray == 0, ref["pairs"]


@pytest.mark.parametrize("name", es.FAMILIES)
def test_forward_agrees_with_the_oracle(name, oracle):
    sc, info, fw, ref, _, _ = case(name)
    W, H = sc["W"], sc["H"]
    ok = ~ref["amb_oracle"]
    assert np.array_equal(ref["n_contrib"][ok], fw["n_contrib"].reshape(H, W)[ok].astype(np.int64))
    err = np.abs(ref["color"] - fw["color"]).max(axis=0)
    assert err[ok].max() <= FWD_TOL, err[ok].max()
    bound = ref["bound_exact"]
    assert (err[ok] <= bound["color"][ok]).all(), float((err / bound["color"])[ok].max())
    eT = np.abs(ref["final_T"] - fw["final_T"].reshape(H, W))
    assert (eT[ok] <= bound["final_T"][ok]).all(), float((eT / bound["final_T"])[ok].max())
    # an ambiguous pixel: one flipped entry's weight at the most (helpers.assert_forward_gate), times the largest colour among the entries
    # the pixel itself can blend (1 wherever no loud entry is within its reach)
    assert (err[~ok] <= (2.0 / 255.0 + 1e-3) * ref["loud"][~ok]).all()


@functools.lru_cache(maxsize=None)
def family_ratios(name):
    """{output: worst |oracle - ref64| / (2^-23 S_abs)} of one family.  The oracle's walk is driven by its own forward, which takes the
    reference's decisions on every unambiguous pixel (test above); dL/dpixel is zeroed on the ambiguous (named) pixels, so that they
    contribute nothing on either side, and both sides run again."""
    sc, info, fw, ref, dpix, bw = case(name)
    W, H = sc["W"], sc["H"]
    amb = ref["amb_oracle"]
    if amb.any():
        from oracle import oracle as orc
        dp = dpix.copy(); dp[:, amb] = 0.0
        ref = es.reference_of(fw, W, H, dL_dpix=dp)
        bw = orc.render_bwd(W, H, fw["bins"], fw["geo"], es.BG, fw["final_T"], fw["n_contrib"], dp)
    return ratios(bw, ref, name)


@pytest.mark.parametrize("name", es.FAMILIES)
def test_backward_agrees_with_the_oracle(name, oracle):
    """element by element, in units of 2^-23 S_abs, within the record of the family's kind"""
    r = family_ratios(name)
    print("r_oracle %-20s %s" % (name, "  ".join("%s %.2f" % kv for kv in r.items())))
    assert max(r.values()) <= es.R_ORACLE[es.kind_of(name)], r


def test_r_oracle_record_and_c(oracle):
    """the constants of the GPU bound come from HERE: c = 4 max(r_oracle, 4), r_oracle the worst ratio of the C oracle over the families of
    a kind.  The record is the measurement: where it decides c (above 4) it may exceed what is measured by 2 % at the most."""
    worst = {}
    for name in es.FAMILIES:
        k = es.kind_of(name)
        worst[k] = max(worst.get(k, 0.0), max(family_ratios(name).values()))
    assert set(worst) == set(es.R_ORACLE)
    for k, w in worst.items():
        print("r_oracle %-12s measured %.3f, recorded %.2f, c = %.1f" % (k, w, es.R_ORACLE[k], 4 * max(es.R_ORACLE[k], 4)))
    print("r_oracle = %.2f over all families" % max(worst.values()))
    for k, w in worst.items():
        assert w <= es.R_ORACLE[k], "%s: r_oracle measures %.3f, the record says %.2f" % (k, w, es.R_ORACLE[k])
        assert max(es.R_ORACLE[k], 4.0) <= 1.02 * max(w, 4.0), "%s: the record %.2f is stale: r_oracle measures %.3f" % (k, es.R_ORACLE[k], w)
    for name in es.FAMILIES:
        assert es.c_gpu(name) == 4 * max(es.R_ORACLE[es.kind_of(name)], 4)


def test_aux_gradients_are_the_forward_s_derivatives(oracle):
    """the oracle has no depth / alpha channel: the reference's dL/dz, and the opacity gradient with dL/ddepth and dL/dalpha set, are checked
    against central differences of the reference's own float64 forward"""
    sc, info, fw, _, _, _ = case("ragged:17x9")
    W, H = sc["W"], sc["H"]
    rng = np.random.default_rng(5)
    dpix, dd, da = rng.normal(size=(3, H, W)), rng.normal(size=(H, W)), rng.normal(size=(H, W))
    rec = blend_ref.records(fw["geo"])
    rec = {k: v.astype(np.float64) for k, v in rec.items()}
    li = blend_ref.lists(fw["bins"]["ranges"], fw["bins"]["point_list"])
    ref = blend_ref.reference(W, H, rec, li, es.BG, dL_dpix=dpix, dL_ddepth=dd, dL_dalpha=da)

    def loss(r):
        f = blend_ref.reference(W, H, r, li, es.BG)
        return (f["color"] * dpix).sum() + (f["depth"] * dd).sum() + (f["alpha"] * da).sum()
    vis = np.nonzero(ref["S_dopacity"] > 0)[0][:12]
    for g in vis:
        for field, col, name in (("z", None, "dz"), ("conic_op", 3, "dopacity")):
            h = 1e-6
            lo, hi = {k: v.copy() for k, v in rec.items()}, {k: v.copy() for k, v in rec.items()}
            if col is None:
                lo[field][g] -= h; hi[field][g] += h
            else:
                lo[field][g, col] -= h; hi[field][g, col] += h
            fd = (loss(hi) - loss(lo)) / (2 * h)
            an = ref[name][g]
            if name == "dopacity" and rec["conic_op"][g, 3] > 0.98:
                continue                                         # (through the clamp the analytic gradient flows by convention, the function does not move)
            assert abs(fd - an) <= 1e-6 * max(1.0, ref["S_" + name][g]), (g, name, fd, an)
