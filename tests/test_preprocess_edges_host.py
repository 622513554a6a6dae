"""Host side of the preprocess edge tests (no GPU): the edge scene covers what it claims to cover, the float64 stage reference
(oracle/torch_dense.py per_gaussian / stage_vjp) is the end-to-end reference cut at the blend stage, the C oracle is per ROW within
rounding of it once the reference takes the float32 decisions, and the per-row gate of tests/test_gpu_preprocess_edges.py rejects wrong
kernels that the tensor max-norm gate lets through.
"""
import numpy as np
import pytest
import torch

import preprocess_edge_scene as es
from helpers import small_scene

BG = np.array([0.2, 0.5, 0.7], np.float32)
TENSORS = ("means", "scales", "rots", "shs")


def _rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.fixture(scope="module")
def edge(oracle):
    """the edge scene, the oracle's forward and blend-stage gradients (D = 3, scales / rotations / SH), the float32 decisions, the float64
    stage reference with them and the oracle's preprocess backward: computed once, shared, never modified"""
    sc, cam, groups = es.cached_edge_scene()
    fw = oracle.forward_full(sc, cam, BG, D=3)
    dpix = np.random.default_rng(1).normal(size=(3, es.H, es.W)).astype(np.float32)
    dmean2D, dconic, _, dcolor = oracle.render_bwd(es.W, es.H, fw["bins"], fw["geo"], BG, fw["final_T"], fw["n_contrib"], dpix)
    dec = es.decisions(sc, cam, fw["geo"])
    ref = es.stage_reference(sc, cam, dec, dmean2D, dconic, dcolor, 3)
    orc = es.stage_oracle(oracle, sc, cam, fw["geo"], dmean2D, dconic, dcolor, 3)
    return dict(sc=sc, cam=cam, groups=groups, fw=fw, geo=fw["geo"], g=(dmean2D, dconic, dcolor), dec=dec, ref=ref, orc=orc,
                vis=fw["geo"]["radii"] > 0)


def test_the_edge_scene_covers_every_decision(edge):
    sc, cam, groups, geo, vis = edge["sc"], edge["cam"], edge["groups"], edge["geo"], edge["vis"]
    d32 = es.decisions_f32(sc["means"], cam, geo["cov3D"]); d64 = es.decisions_f64(sc["means"], cam)
    for name in ("near", "clamp_x", "clamp_y", "clamp_xy", "colour", "rect", "iso", "overflow", "nonunit", "ordinary", "culled_block"):
        assert len(groups[name]) > 0, name
    assert sc["means"].shape[0] == es.P == 2 * 256 + 88 and not vis[256:512].any() and vis[:256].any() and vis[512:].any()
    n = groups["near"]
    below, above = d32["depth"][n] <= np.float32(0.2), d32["depth"][n] > np.float32(0.2)
    assert (vis[n] == above).all() and below.sum() >= 4 and above.sum() >= 4
    assert {float(x) for x in (d32["depth"][n][:7].astype(np.float64) - float(np.float32(0.2))) / 2.0 ** -26} == {0, 1, -1, 2, -2, 8, -8}
    for name, keys in (("clamp_x", ["inx"]), ("clamp_y", ["iny"]), ("clamp_xy", ["inx", "iny"])):
        r = groups[name][vis[groups[name]]]
        for k in keys:
            assert d32[k][r].any() and (~d32[k][r]).any(), (name, k)                   # visible rows on both sides of the threshold
            assert (d32[k][r] != d64[k][r]).any(), (name, k, "no row where float32 and float64 decide differently")
            q, lim = (d32["txtz"], d32["limx"]) if k == "inx" else (d32["tytz"], d32["limy"])
            assert (np.abs(q[r]) == lim).any(), (name, k, "no row with the float32 quotient AT the limit")
    signs = {(int(np.sign(d32["txtz"][i])), int(np.sign(d32["tytz"][i]))) for i in groups["clamp_xy"] if not d32["inx"][i] and not d32["iny"][i]}
    assert signs == {(1, 1), (1, -1), (-1, 1), (-1, -1)}
    c = groups["colour"]
    assert vis[c].all()
    for ch in range(3):
        assert geo["clamped"][c, ch].any() and (geo["clamped"][c, ch] == 0).any(), ch
    assert {int(x) for x in geo["clamped"][c].sum(1)} == {0, 1, 2, 3}
    assert (geo["rgb"][c] == 0).sum() > geo["clamped"][c].sum()                           # colours AT zero that are not clamped
    rect = groups["rect"].reshape(4, -1)
    for border in range(4):
        assert vis[rect[border]].any() and (~vis[rect[border]]).any(), border
    i = groups["iso"]
    assert vis[i].all() and (d32["mid2_minus_det"][i] < 0.1).sum() >= 4 and (d32["mid2_minus_det"][i] > 0.1).sum() >= 2
    assert (sc["scales"][i] == 0).all(1).sum() >= 4
    o = groups["overflow"]
    assert vis[o].all() and d32["overflow"][o].sum() >= 3 and (~d32["overflow"][o]).sum() >= 3 and not d32["overflow"][vis & ~np.isin(np.arange(es.P), o)].any()
    assert geo["radii"].max() < 2 ** 24
    safe = o[~d32["overflow"][o]]
    assert (np.abs(d32["denom"][safe]) < 1.8446744e19 / 5).all()                          # (2^64: denom^2 = 2^128 overflows float32)
    norms = np.linalg.norm(sc["rots"][groups["nonunit"]].astype(np.float64), axis=1)
    assert np.allclose(np.sort(norms), [0.5] * 4 + [2.0] * 4, rtol=1e-6) and vis[groups["nonunit"]].all()
    # the gate is vacuous on a row no pixel reaches: (nearly) every visible edge row has a blend-stage gradient (the two farthest corner
    # rows of clamp_xy, 2 x the limit on both axes, reach no pixel with alpha >= 1/255 at scales <= 1.5)
    live = np.abs(edge["g"][1]).max(1) > 0
    for name, r in groups.items():
        if name not in ("ordinary", "culled_block"):
            assert (live[r] | ~vis[r]).sum() >= len(r) - 2, name
    print("edge scene census (rows, visible, x-clamped, y-clamped, f32 != f64 decision, colour bits set, denom2inv == 0):")
    for name, r in groups.items():
        v = vis[r]
        print("  %-12s %4d %4d %4d %4d %4d %4d %4d" % (name, len(r), v.sum(), (~d32["inx"][r] & v).sum(), (~d32["iny"][r] & v).sum(),
              (((d32["inx"][r] != d64["inx"][r]) | (d32["iny"][r] != d64["iny"][r])) & v).sum(), geo["clamped"][r][v].sum(), (d32["overflow"][r] & v).sum()))


def _t64(a, rg=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=rg)


@pytest.mark.parametrize("pre", [False, True], ids=["sh_scale_rot", "precomp"])
def test_stage_reference_is_the_end_to_end_reference_cut_at_the_blend(oracle, pre):
    """td.render's end-to-end autograd on an ordinary scene = stage_vjp applied to the blend-stage gradients: to 1e-9 with the float64
    interface gradients of td.render itself (the conventions: ndc-scaled mean2D gradient, half the off-diagonal conic derivative), and to
    2e-5 of the tensor's size (the bar of test_oracle_dense.py) with the C oracle's float32 blend-stage gradients."""
    from oracle import torch_dense as td
    D = 3
    sc, cam = small_scene(P=160, W=40, H=36, seed=0, D=D)
    Wd, Hd = cam["W"], cam["H"]
    leaves = dict(means=_t64(sc["means"], True))
    kw = {}
    if pre:
        kw["colors_precomp"] = leaves["colors"] = _t64(sc["colors_precomp"], True); kw["cov3D_precomp"] = leaves["cov"] = _t64(sc["cov3D_precomp"], True)
    else:
        kw["shs"] = leaves["shs"] = _t64(sc["shs"], True); kw["scales"] = leaves["scales"] = _t64(sc["scales"], True); kw["rots"] = leaves["rots"] = _t64(sc["rots"], True)
    out, aux = td.render(leaves["means"], _t64(sc["opac"]), _t64(cam["view"]), _t64(cam["proj"]), _t64(cam["campos"]), Wd, Hd, cam["tanx"],
                         cam["tany"], _t64(BG), D=D, **kw)
    live = aux["live"]
    for v in live.values():
        v.retain_grad()
    dpix = np.random.default_rng(5).normal(size=(3, Hd, Wd)).astype(np.float32)
    (out * _t64(dpix)).sum().backward()
    e2e = {k: v.grad.numpy() for k, v in leaves.items()}
    fw = oracle.forward_full(sc, cam, BG, D=D, use_precomp_cov=pre, use_precomp_color=pre)
    assert np.array_equal(aux["radii"].numpy(), fw["geo"]["radii"])
    bw = oracle.backward_full(sc, cam, BG, fw, dpix, D=D, use_precomp_cov=pre, use_precomp_color=pre)
    P = sc["means"].shape[0]
    # float64 interface gradients; dL/dcolour by solving the (linear, per-row) colour VJP is not needed: take the oracle's, compared below
    dm = np.stack([live["px"].grad.numpy() * 0.5 * Wd, live["py"].grad.numpy() * 0.5 * Hd], 1)
    c64 = live["conic"].grad.numpy()
    dc = np.zeros((P, 4)); dc[:, 0] = c64[:, 0]; dc[:, 1] = 0.5 * c64[:, 1]; dc[:, 3] = c64[:, 2]
    assert _rel(bw["dmean2D"][:, :2], dm) <= 2e-5 and _rel(bw["dconic"][:, [0, 1, 3]], dc[:, [0, 1, 3]]) <= 2e-5
    mk = es.mode_kw(sc, pre, pre)
    exact = td.stage_vjp(dm, dc, np.zeros((P, 3)), sc["means"], cam, D=D, **mk)           # no colour gradient: the geometry chain alone
    colour = td.stage_vjp(np.zeros((P, 2)), np.zeros((P, 4)), e2e["colors"] if pre else bw["dcolor"], sc["means"], cam, D=D, **mk)
    for k in ("cov",) if pre else ("scales", "rots"):
        assert _rel(exact[k], e2e[k]) <= 1e-9, k                                           # (colour does not reach the covariance)
    if pre:
        assert _rel(exact["means"], e2e["means"]) <= 1e-9 and np.array_equal(colour["colors"], e2e["colors"] * (fw["geo"]["radii"] > 0)[:, None])
    else:
        assert _rel(exact["means"] + colour["means"], e2e["means"]) <= 2e-5               # (the colour leg has the oracle's float32 dL/dcolour)
    fed = td.stage_vjp(bw["dmean2D"], bw["dconic"], bw["dcolor"], sc["means"], cam, D=D, **mk)
    for k, v in e2e.items():
        assert _rel(fed[k], v) <= 2e-5, (k, _rel(fed[k], v))


def _percentiles(err, rows):
    e = err[rows]
    e = e[np.isfinite(e)]
    return (float(e.max()), float(np.percentile(e, 99.9))) if e.size else (0.0, 0.0)


FLOOR_SEEDS = range(1, 9)


def _pooled_floor(oracle, edge, pre_cov):
    """{tensor: 99.9th percentile of err_orc over the ordinary rows}, pooled over eight image gradients (8 x 165 rows: with one
    gradient that percentile is the maximum of a small sample and moves by a factor two between two draws)"""
    sc, cam, fw, vis = edge["sc"], edge["cam"], edge["fw"], edge["vis"]
    rows = edge["groups"]["ordinary"][vis[edge["groups"]["ordinary"]]]
    dec = es.decisions(sc, cam, edge["geo"], pre_cov=pre_cov)
    pool = {}
    for seed in FLOOR_SEEDS:
        dpix = np.random.default_rng(seed).normal(size=(3, es.H, es.W)).astype(np.float32)
        dmean2D, dconic, _, dcolor = oracle.render_bwd(es.W, es.H, fw["bins"], fw["geo"], BG, fw["final_T"], fw["n_contrib"], dpix)
        ref = es.stage_reference(sc, cam, dec, dmean2D, dconic, dcolor, 3, pre_cov=pre_cov)
        orc = es.stage_oracle(oracle, sc, cam, edge["geo"], dmean2D, dconic, dcolor, 3, pre_cov=pre_cov)
        for k in ref:
            pool.setdefault(k, []).append(es.row_errors(orc[k], ref[k])[rows])
    return {k: float(np.percentile(np.concatenate(v), 99.9)) for k, v in pool.items()}


def test_c_oracle_per_row_against_the_stage_reference(oracle, edge):
    """The float32 statements of the oracle against float64 with the SAME decisions, per row and tensor, error relative to the row's largest
    float64 entry.  Distribution per group printed (NOTEBOOK.md); every row within 1e-3 except the explained ones; the `ordinary` rows'
    99.9th percentile (pooled over eight image gradients) is the gate's floor: the committed FLOOR is that figure rounded up."""
    groups, vis, ref, orc = edge["groups"], edge["vis"], edge["ref"], edge["orc"]
    print("C oracle vs float64 stage reference with float32 decisions: max | 99.9th percentile of the per-row error, visible rows")
    unexplained = []
    floors = dict(_pooled_floor(oracle, edge, False), cov=_pooled_floor(oracle, edge, True)["cov"])
    for k in TENSORS:
        err = es.row_errors(orc[k], ref[k])
        assert np.isfinite(err).all(), k
        assert (np.asarray(orc[k]).reshape(es.P, -1)[~vis] == 0).all() and (ref[k].reshape(es.P, -1)[~vis] == 0).all()
        for name, r in groups.items():
            r = r[vis[r]]
            if len(r):
                print("  %-7s %-12s %.2e | %.2e" % ((k, name) + _percentiles(err, r)))
        p999 = floors[k]
        print("  %-7s floor from the ordinary rows: %.2e (committed: %.1e)" % (k, p999, es.FLOOR[k]))
        assert p999 <= es.FLOOR[k] <= 1.1 * p999, (k, p999)
        for i in np.nonzero(vis & (err > 1e-3))[0]:
            # the one known cause: + 1e-7 in denom2inv = 1 / (denom^2 + 1e-7) (backward.cu:203), worth 1e-7 / denom^2 = 1.2e-5 at denom = 0.09
            # (a zero-scale splat: cov2D is the low-pass alone) - it cannot explain 1e-3
            unexplained.append((k, int(i), float(err[i])))
    assert not unexplained, unexplained
    # the precomputed-covariance mode: dL/dcov3D is an output, and it has a floor of its own
    sc, cam = edge["sc"], edge["cam"]
    dec_c = es.decisions(sc, cam, edge["geo"], pre_cov=True)
    ref_c = es.stage_reference(sc, cam, dec_c, *edge["g"], 3, pre_cov=True)
    orc_c = es.stage_oracle(oracle, sc, cam, edge["geo"], *edge["g"], 3, pre_cov=True)
    err = es.row_errors(orc_c["cov"], ref_c["cov"])
    for name, r in groups.items():
        r = r[vis[r]]
        if len(r):
            print("  %-7s %-12s %.2e | %.2e" % (("cov", name) + _percentiles(err, r)))
    p999 = floors["cov"]
    print("  cov     floor from the ordinary rows: %.2e (committed: %.1e)" % (p999, es.FLOOR["cov"]))
    assert p999 <= es.FLOOR["cov"] <= 1.1 * p999 and err[vis].max() <= 1e-3 and not es.gate_failures(orc_c, orc_c, ref_c, vis)[0]
    # without the float32 decisions the reference itself is wrong at the thresholds: that is why it takes them
    own = es.stage_reference(sc, cam, dict(visible=vis, clamped=edge["dec"]["clamped"]), *edge["g"], 3)
    d = es.row_errors(own["means"], ref["means"])
    flips = np.nonzero(vis & (d > 1e-2))[0]
    print("  rows whose float64-decided clamp differs: dL/dmean moves by", np.round(d[flips], 3))
    assert len(flips) >= 3 and np.isin(flips, np.concatenate([groups[g] for g in ("clamp_x", "clamp_y", "clamp_xy")])).all()


# ---------------------------------------------------------------------------------------------- wrong kernels
MUTATIONS = ("xmul_ignored", "unclamped_tx_in_dtz", "clamp_ge", "colour_mask_ignored", "no_lowpass_in_det", "db_factor2_dropped",
             "cony_sign_flipped", "no_sh_direction_term", "culled_row_nonzero")


def _copy_vjp(mut, edge):
    """A copy of the stage VJP, structured like the kernel (autograd up to cov2D, the conic -> cov2D block by the kernel's closed form),
    with one deliberate error `mut` (None: no error, equal to the reference)."""
    from oracle import torch_dense as td
    sc, cam, dec = edge["sc"], edge["cam"], edge["dec"]
    g2d, gc, gcol = (_t64(x) for x in edge["g"])
    B = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.bool)
    means, scales, rots, shs = (_t64(sc[k], True) for k in ("means", "scales", "rots", "shs"))
    view, proj, campos = _t64(cam["view"]), _t64(cam["proj"]), _t64(cam["campos"])
    Wd, Hd, tanx, tany = cam["W"], cam["H"], cam["tanx"], cam["tany"]
    fx, fy = Wd / (2.0 * tanx), Hd / (2.0 * tany)
    ph = torch.cat([means, torch.ones(es.P, 1, dtype=torch.float64)], 1)
    hom = ph @ proj
    ndc = hom[:, :3] / (hom[:, 3:4] + 1e-7)
    t = (ph @ view)[:, :3]
    t0, t1, tz = t[:, 0], t[:, 1], t[:, 2]
    L = td.quat_to_rot(rots) * scales[:, None, :]
    Sig = L @ L.transpose(1, 2)
    limx, limy = 1.3 * tanx, 1.3 * tany
    inx, iny = B(dec["inx"]), B(dec["iny"])
    if mut == "clamp_ge":                                      # `>=` instead of `>`: a quotient AT the limit counts as clamped
        d32 = es.decisions_f32(sc["means"], cam)
        inx = inx & ~B(np.abs(d32["txtz"]) == d32["limx"]); iny = iny & ~B(np.abs(d32["tytz"]) == d32["limy"])
    tx = torch.where(inx, t0, ((t0 / tz).clamp(-limx, limx) * tz).detach())
    ty = torch.where(iny, t1, ((t1 / tz).clamp(-limy, limy) * tz).detach())
    if mut == "xmul_ignored":                                  # dtx / dty flow although the clamp is active
        tx = tx.detach() + (t0 - t0.detach()); ty = ty.detach() + (t1 - t1.detach())
    w = 1.0 / (tz * tz)
    j02, j12 = -fx * tx * w, -fy * ty * w
    if mut == "unclamped_tx_in_dtz":                           # d j02 / d tz formed from the unclamped t.x
        j02 = -fx * tx * w.detach() + (-fx * t0.detach()) * (w - w.detach())
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, j02, zero, fy / tz, j12], 1).reshape(-1, 2, 3)
    JW = J @ view[:3, :3].transpose(0, 1)
    cov2 = JW @ Sig @ JW.transpose(1, 2)
    a, b, c = cov2[:, 0, 0] + 0.3, cov2[:, 0, 1], cov2[:, 1, 1] + 0.3
    ad, bd, cd = a.detach(), b.detach(), c.detach()
    denom = ad * cd - bd * bd if mut != "no_lowpass_in_det" else (ad - 0.3) * (cd - 0.3) - bd * bd
    inv2 = torch.where(B(dec["overflow"]), torch.zeros_like(denom), 1.0 / (denom * denom))
    dcx, dcy, dcz = gc[:, 0], gc[:, 1] * (-1.0 if mut == "cony_sign_flipped" else 1.0), gc[:, 3]
    dL_da = inv2 * (-cd * cd * dcx + 2 * bd * cd * dcy + (denom - ad * cd) * dcz)
    dL_dc = inv2 * (-ad * ad * dcz + 2 * ad * bd * dcy + (denom - ad * cd) * dcx)
    dL_db = inv2 * (1.0 if mut == "db_factor2_dropped" else 2.0) * (bd * cd * dcx - (denom + 2 * bd * bd) * dcy + ad * bd * dcz)
    d = means - campos[None, :]
    d = d / d.norm(dim=1, keepdim=True)
    col = td.eval_sh(3, shs, d.detach() if mut == "no_sh_direction_term" else d) + 0.5
    if mut != "colour_mask_ignored":
        col = torch.where(B(dec["clamped"]), torch.zeros_like(col), col)
    vis = _t64(edge["vis"])
    (vis * (g2d[:, 0] * ndc[:, 0] + g2d[:, 1] * ndc[:, 1] + dL_da * a + dL_db * b + dL_dc * c + (gcol * col).sum(1))).sum().backward()
    out = dict(means=means.grad.numpy().copy(), scales=scales.grad.numpy().copy(), rots=rots.grad.numpy().copy(), shs=shs.grad.numpy().copy())
    if mut == "culled_row_nonzero":
        out["means"][np.nonzero(~edge["vis"])[0][0], 1] = 1e-12
    return out


def test_the_per_row_gate_rejects_wrong_kernels_the_max_norm_gate_accepts(edge):
    ref, orc, vis = edge["ref"], edge["orc"], edge["vis"]
    same = _copy_vjp(None, edge)
    for k in TENSORS:                                          # the copy is the reference (apart from the 1e-7 of p_w it shares)
        assert es.row_errors(same[k], ref[k])[vis].max() <= 1e-9, k
    assert not es.gate_failures(same, orc, ref, vis)[0] and not es.gate_failures(orc, orc, ref, vis)[0]
    missed_by_max_norm = []
    print("mutation: rows failing the per-row gate | the tensor gate (max-norm error <= 1e-3) per tensor")
    for mut in MUTATIONS:
        m = _copy_vjp(mut, edge)
        bad, worst = es.gate_failures(m, orc, ref, vis)
        old = {k: _rel(m[k], ref[k]) for k in TENSORS}
        old_rejects = not max(old.values()) <= 1e-3             # (a NaN rejects)
        print("  %-22s %4d row(s), worst ratio %.3g | %s -> %s" % (mut, len({(k, i) for k, i, _, _ in bad}), max(worst.values()),
              " ".join("%s %.1e" % kv for kv in old.items()), "rejects" if old_rejects else "ACCEPTS"))
        assert bad, "%s passes the per-row gate" % mut
        if not old_rejects:
            missed_by_max_norm.append(mut)
    for mut in MUTATIONS[:3]:
        assert mut in missed_by_max_norm, "%s: the max-norm gate was expected to miss it on this scene" % mut
