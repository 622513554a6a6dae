"""The blend kernels (gm_render.hip, gm_render_fwd_body.inc, gm_render_bwd_body.inc) per pixel and per Gaussian against the float64
reference (blend_ref.py) on the scenes of blend_edge_scenes.py, which put the lists on the kernels' own seams: the 4 x 64 key scan and
the 128-entry candidate ring, the survivor count of a batch (groups of 16, the four padding slots, the sub-blocks' early break), the
backward's two-register-set pipeline and seven-slot flush, the start position and the live-pixel culls, the three decision thresholds,
ragged images and the child-bit filter of policies 2 and 3.

Every (family, policy) runs rasterize_forward_begin(..).finish(..) as four builds - (a) the polynomial build, (b) image_only, (c)
exact_exponent, (d) aux + exact_exponent - and the backward after (c) and (d).
Forward: device records / lists / ranges == the oracle's (policy 0; the culled policies' own lists feed the reference); n_contrib exact and
final_T / colour / alpha / depth within the pixel's first-order rounding bound on every unambiguous pixel; ambiguous pixels (only the ones a
family names) within one flipped entry's weight; under the culled policies the walk over the device's lists agrees with the walk over the
oracle's complete lists; (a) and (b) the same colour bits; the designated pixels of `thresholds` and `stops`
spelled out one by one.
Backward: EVERY element of dmean2D, dconic, dopacity, dcolor (and dL/dz) within c 2^-23 S_abs of the reference, c = 4 max(r_oracle, 4)
with the r_oracle test_blend_ref_host.py measures for the family's kind (never fitted to the kernel); elements nothing contributes to exactly 0; the reconstructed front
transmittance 1 within the reciprocals' rounding."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import blend_edge_scenes as es
import blend_ref

pytestmark = pytest.mark.gpu
U = 2.0 ** -23
CASES = [(name, pol) for name in es.FAMILIES for pol in es.policies(name)]


@functools.lru_cache(maxsize=None)
def host_case(name):
    from oracle import oracle as orc
    orc.build()
    sc, info = es.family(name, orc)
    fw = es.oracle_forward(orc, sc)
    return sc, info, fw


@functools.lru_cache(maxsize=None)
def host_reference(name):
    """the float64 walk over the ORACLE's (policy 0) records and lists"""
    sc, info, fw = host_case(name)
    return es.reference_of(fw, sc["W"], sc["H"])


def last_gid(ref, li, W, H):
    """[H, W] Gaussian id of every pixel's last contributor (n_contrib is a position in the pixel's parent list), -1 for none"""
    side = 16 << max(li["policy"] - 1, 0)
    ys, xs = np.mgrid[0:H, 0:W]
    parent = (ys // side) * (-(-W // side)) + xs // side
    nc = ref["n_contrib"]
    at = np.clip(li["ranges"][parent, 0] + nc - 1, 0, max(li["point_list"].size - 1, 0))
    return np.where(nc > 0, li["point_list"][at] if li["point_list"].size else -1, -1)


def _args(sc):
    from gpu_utils import T
    cam = sc["cam"]
    return (T(es.BG), T(sc["means"]), T(sc["colors_precomp"]), T(sc["opac"]), None, None, 1.0, T(sc["cov3D_precomp"]), T(cam["view"]), T(cam["proj"]),
            cam["tanx"], cam["tany"])


def forward(sc, policy, image_only=False, exact=False, aux=False):
    """one build of the forward -> (outputs of finish(), state dict as numpy)"""
    from gpu_utils import T, _view
    from gaussianmesh_amd import _lib, rasterizer as R
    lib = _lib.lib()
    W, H = sc["W"], sc["H"]
    P = sc["means"].shape[0]
    a = _args(sc)
    out = R.rasterize_forward_begin(*a, H, W, None, 0, T(sc["cam"]["campos"]), emission_policy=policy, aux=aux).finish(
        image_only=image_only, exact_exponent=exact)
    torch.cuda.synchronize()
    nr, color, radii, geom, binning, img = out[:6]
    st = dict(R=nr, color=color.cpu().numpy(), radii=radii.cpu().numpy())
    gp = lambda n: lib.gm_geom_field(geom.data_ptr(), P, n.encode())
    SF = lib.gm_splat_floats()
    st["splat"] = _view(geom, gp("splat"), P * SF, torch.float32).reshape(P, SF)
    st["depth_key"] = _view(geom, gp("depth_key"), P, torch.int32).astype(np.uint32)
    st["tiles"] = _view(geom, gp("tiles_touched"), P, torch.int32).astype(np.uint32)
    st["clamped"] = _view(geom, gp("clamped"), P, torch.uint8)
    ip = lambda n: lib.gm_image_field(img.data_ptr(), W, H, n.encode())
    st["final_T"] = _view(img, ip("final_T"), W * H, torch.float32).reshape(H, W)
    st["n_contrib"] = _view(img, ip("n_contrib"), W * H, torch.int32).astype(np.int64).reshape(H, W)
    s = max(policy - 1, 0)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    tiles = ((gx + (1 << s) - 1) >> s) * ((gy + (1 << s) - 1) >> s)
    st["ranges"] = _view(img, ip("ranges"), tiles * 2, torch.int32).astype(np.uint32).reshape(tiles, 2)
    pairs = np.zeros((0, 2), np.uint32)
    if nr > 0:
        pp = lib.gm_binning_field(binning.data_ptr(), nr, W, H, policy, b"pairs")
        pairs = _view(binning, pp, 2 * nr, torch.int32).astype(np.uint32).reshape(nr, 2)
    st["point_list"] = np.ascontiguousarray(pairs[:, 1]); st["tile_keys"] = pairs[:, 0] & 0xFFFF; st["child_mask"] = pairs[:, 0] >> 16
    if aux:
        st["depth"], st["alpha"] = out[6].cpu().numpy().reshape(H, W), out[7].cpu().numpy().reshape(H, W)
    return out, st


def backward(sc, policy, out, dpix, dd=None, da=None):
    """rasterize_backward(want_conic=True) behind a forward's outputs -> blend-stage gradients, dL/dz (aux) and the front_T plane"""
    from gpu_utils import T, _view
    from gaussianmesh_amd import _lib, rasterizer as R
    W, H = sc["W"], sc["H"]
    P = sc["means"].shape[0]
    a = _args(sc)
    nr, color, radii, geom, binning, img = out[:6]
    lib = C.CDLL(_lib.lib()._name)
    front = torch.ones((H, W), dtype=torch.float32, device="cuda")
    lib.gm_debug_backward_front_T(C.c_void_p(front.data_ptr()))
    try:
        g = R.rasterize_backward(a[0], a[1], radii, a[2], None, None, 1.0, a[7], a[8], a[9], a[10], a[11], T(dpix), None, 0, T(sc["cam"]["campos"]), geom, nr,
                                 binning, img, False, emission_policy=policy, want_conic=True,
                                 dL_ddepth=None if dd is None else T(dd), dL_dalpha=None if da is None else T(da))
        torch.cuda.synchronize()
    finally:
        lib.gm_debug_backward_front_T(None)
    res = dict(dmean2D=g[0].cpu().numpy()[:, :2], dcolor=g[1].cpu().numpy(), dopacity=g[2].cpu().numpy().reshape(-1),
               dconic=g[8].cpu().numpy().reshape(-1, 4)[:, [0, 1, 3]], front=front.cpu().numpy())
    if dd is not None:
        acc = _view(geom, _lib.lib().gm_geom_field(geom.data_ptr(), P, b"grad_acc"), 12 * P, torch.float32).reshape(P, 12)
        res["dz"] = acc[:, 9].copy()
    return res


def check_forward(what, st, ref, mode, state=True, aux=False):
    ok = ~ref["amb_" + mode]
    B = ref["bound_" + mode]
    err = np.abs(st["color"].astype(np.float64) - ref["color"]).max(axis=0)
    ratio = float((err / B["color"])[ok].max())
    print("%-44s colour: worst error %.2e, worst error / bound %.2f on %d unambiguous pixels" % (what, err[ok].max(), ratio, ok.sum()))
    assert (err[ok] <= B["color"][ok]).all(), "%s: colour off by %.3g x its rounding bound" % (what, ratio)
    # one flipped entry's weight (helpers.assert_forward_gate), times the largest colour the pixel itself can blend (blend_ref `loud`:
    # 1 on every pixel that has no loud entry within reach - all five named pixels of `thresholds`)
    assert (err[~ok] <= (2.0 / 255.0 + 1e-3) * ref["loud"][~ok]).all(), "%s: an ambiguous pixel moved by more than one flipped entry" % what
    if state:
        bad = (st["n_contrib"] != ref["n_contrib"]) & ok
        assert not bad.any(), "%s: n_contrib differs on %d unambiguous pixels, first %s" % (what, bad.sum(), np.argwhere(bad)[:4].tolist())
        eT = np.abs(st["final_T"].astype(np.float64) - ref["final_T"])
        assert (eT[ok] <= B["final_T"][ok]).all(), "%s: final_T off by %.3g x bound" % (what, (eT / B["final_T"])[ok].max())
    if aux:
        eA = np.abs(st["alpha"].astype(np.float64) - ref["alpha"])
        assert (eA[ok] <= B["final_T"][ok] + U).all(), "%s: alpha map off by %.3g x bound" % (what, (eA / (B["final_T"] + U))[ok].max())
        eD = np.abs(st["depth"].astype(np.float64) - ref["depth"])
        assert (eD[ok] <= B["depth"][ok]).all(), "%s: depth map off by %.3g x bound" % (what, (eD[ok] / np.maximum(B["depth"][ok], 1e-300)).max())


def check_designated(what, info, st, ref, li, mode, state=True):
    """the designated pixels of `thresholds` and `stops`, one by one"""
    W = st["color"].shape[2]
    for d in info["designated"]:
        x, y = d["pixel"]
        if mode in d["ambiguous"]:
            continue                                             # (checked through the flip bound only)
        tag = "%s, %s at (%d, %d)" % (what, d["name"], x, y)
        s = max(li["policy"] - 1, 0)
        side = 16 << s
        parent = (y // side) * (-(-W // side)) + x // side
        r0, r1 = li["ranges"][parent]
        pos_of = lambda gid: int(np.nonzero(li["point_list"][r0:r1] == gid)[0][0])
        T_, nc, col = float(st["final_T"][y, x]), int(st["n_contrib"][y, x]), st["color"][:, y, x].astype(np.float64)
        e = d["expect"]
        if e == "not_taken":
            assert np.array_equal(st["color"][:, y, x], es.BG), "%s: the entry was blended" % tag
            if state:
                assert nc == 0 and T_ == 1.0, "%s: n_contrib %d, final_T %r" % (tag, nc, T_)
            continue
        if e == "taken" or e[0] == "alpha":
            al = float(ref["alpha"][y, x])
            if e != "taken":
                assert abs(al - e[1]) <= 1e-12, (tag, al, e[1])                               # (the reference itself clamps, or not, as designed)
            want = al * ref["_rgb"][d["gid"]] + (1 - al) * es.BG.astype(np.float64)
            tolC = 8 * U * np.abs(want).max() if mode == "exact" else ref["bound_poly"]["color"][y, x]
            tolT = 2 * U if mode == "exact" else ref["bound_poly"]["final_T"][y, x]
            assert np.abs(col - want).max() <= tolC, "%s: colour %s, wanted %s" % (tag, col, want)
            if state:
                assert nc == pos_of(d["gid"]) + 1, "%s: n_contrib %d" % (tag, nc)
                assert abs(T_ - (1 - al)) <= tolT, "%s: final_T %r, wanted %r" % (tag, T_, 1 - al)
            continue
        if e[0] == "last":
            if state:
                assert nc == pos_of(e[1]) + 1, "%s: stopped behind list position %d, wanted %d" % (tag, nc, pos_of(e[1]) + 1)
            if "loud" in d:
                # nothing behind the stop leaks: the pixel's colour is the reference's within its rounding bound, and that bound is a
                # small fraction of what the loud entry would add if it were blended at the transmittance the pixel is left with
                gl = d["loud"]
                leak = float(ref["final_T"][y, x]) * min(blend_ref.A_MAX, float(ref["_op"][gl])) * float(ref["_rgb"][gl].min())
                bound = float(ref["bound_" + mode]["color"][y, x])
                assert 8 * bound <= leak, "%s: the bound %.3g does not resolve a leak of %.3g" % (tag, bound, leak)
                assert np.abs(col - ref["color"][:, y, x]).max() <= bound, "%s: colour %s, wanted %s - the loud entry behind the stop leaked" % (
                    tag, col, ref["color"][:, y, x])


def check_backward(what, got, ref, ok, names, c):
    worst = {}
    for name in names:
        r, S = ref[name], ref["S_" + name]
        g = np.asarray(got[name], np.float64).reshape(r.shape)
        zero = S == 0
        assert (g[zero] == 0).all(), "%s %s: %d element(s) nothing contributes to are not 0" % (what, name, (g[zero] != 0).sum())
        ratio = np.abs(g - r)[~zero] / (U * S[~zero])
        worst[name] = float(ratio.max()) if ratio.size else 0.0
    print("%-44s |got - ref64| / (2^-23 S_abs): %s   (c = %.0f)" % (what, "  ".join("%s %.2f" % kv for kv in worst.items()), c))
    for name, w in worst.items():
        assert w <= c, "%s %s: an element is off by %.1f x 2^-23 S_abs (c = %.0f)" % (what, name, w, c)
    dev = np.abs(got["front"].astype(np.float64) - 1.0)
    assert (dev[ok] <= ref["front_bound"][ok]).all(), "%s: front transmittance off by %.3g x its rounding bound" % (what, (dev / ref["front_bound"])[ok].max())


@pytest.mark.parametrize("name,policy", CASES, ids=["%s-p%d" % c for c in CASES])
def test_blend_edges(name, policy):
    import helpers
    sc, info, fw = host_case(name)
    W, H = sc["W"], sc["H"]
    c = es.c_gpu(name)
    builds = dict(a=dict(), b=dict(image_only=True), c=dict(exact=True), d=dict(exact=True, aux=True))
    outs, sts = {}, {}
    for k, kw in builds.items():
        outs[k], sts[k] = forward(sc, policy, **kw)
    st = sts["a"]
    # ---- the device's records and lists
    if policy == 0:
        helpers._check_geometry(None, st, fw, sc, True)
    else:
        helpers._check_per_gaussian(st, fw["geo"], True)
    vis = st["radii"] > 0
    for k in "bcd":                                          # (a culled Gaussian's record is never written)
        assert np.array_equal(sts[k]["splat"][vis], st["splat"][vis]), "build (%s): splat records differ from build (a)'s" % k
        for f in ("depth_key", "ranges", "point_list", "child_mask"):
            assert np.array_equal(sts[k][f], st[f]), "build (%s): %s differs from build (a)'s" % (k, f)
    rec = blend_ref.records_from_state(st)
    for f in ("xy", "conic_op", "rgb"):                      # (so that the walk over a list never meets uninitialised memory)
        rec[f][~vis] = 0.0
    assert np.array_equal(rec["z"].view(np.uint32)[vis], fw["geo"]["depths"].view(np.uint32)[vis])
    li = blend_ref.lists(st["ranges"], st["point_list"], policy, st["child_mask"])
    ref0 = blend_ref.reference(W, H, rec, li, es.BG)
    amb = ref0["amb_exact"]
    rng = np.random.default_rng(17)
    dpix = es.dpix_for(sc, info, ref0)
    dpix[:, amb] = 0.0                                       # ambiguous (named) pixels contribute nothing to the gradients on either side
    dd = rng.normal(size=(H, W)).astype(np.float32); da = rng.normal(size=(H, W)).astype(np.float32)
    dd[amb] = 0.0; da[amb] = 0.0
    ref = blend_ref.reference(W, H, rec, li, es.BG, dL_dpix=dpix)
    refx = blend_ref.reference(W, H, rec, li, es.BG, dL_dpix=dpix, dL_ddepth=dd, dL_dalpha=da)
    ref["_rgb"] = rec["rgb"].astype(np.float64); ref["_op"] = rec["conic_op"][:, 3].astype(np.float64)
    for d in info["designated"]:                             # the named pixels' flip bound is the helper's, unscaled
        if d["ambiguous"]:
            assert ref["loud"][d["pixel"][1], d["pixel"][0]] == 1.0, d["name"]
    if policy != 0:
        # the culled lists feed the reference: a list entry or a child bit that the emission dropped WRONGLY would vanish from both sides.
        # So the same walk over the ORACLE's complete lists must see the same pixels: colour and final_T (an entry the cull may drop adds
        # exactly nothing) and the same last contributor, by Gaussian id - list positions differ between the two lists.
        full = host_reference(name)
        both = ~(full["amb_poly"] | ref["amb_poly"])
        assert (np.abs(full["color"] - ref["color"]).max(axis=0)[both] <= 1e-12 * ref["loud"][both]).all(), "policy %d: the culled lists change a pixel's colour" % policy
        assert (np.abs(full["final_T"] - ref["final_T"])[both] <= 1e-14).all(), "policy %d: the culled lists change a pixel's final_T" % policy
        lo = blend_ref.lists(fw["bins"]["ranges"], fw["bins"]["point_list"])
        assert np.array_equal(last_gid(full, lo, W, H)[both], last_gid(ref, li, W, H)[both]), "policy %d: another last contributor" % policy
    if policy == 0:                                          # the device's lists are the oracle's: so are the ambiguity counts of the host test
        named = np.zeros((H, W), bool)
        for d in info["designated"]:
            if d["ambiguous"]:
                named[d["pixel"][1], d["pixel"][0]] = True
        assert not ((ref["amb_poly"] | ref["amb_exact"]) & ~named).any()
    else:                                                    # culled lists are sub-lists: nothing new can become ambiguous
        assert (ref["amb_poly"] | ref["amb_exact"]).sum() <= sum(1 for d in info["designated"] if d["ambiguous"])
    if "first_own_beyond" in info["waves"].get((56, 56), {}) and policy == 3:      # the four waves of child (3, 3): bit 15 of the 64-px parent's masks
        mine = np.nonzero(st["child_mask"][st["ranges"][0, 0]:st["ranges"][0, 1]] & (1 << 15))[0]
        assert mine.size and mine[0] > 256, mine[:3]
    # ---- forward, the four builds
    what = "%s policy %d" % (name, policy)
    check_forward(what + " (a) polynomial", sts["a"], ref, "poly")
    check_forward(what + " (b) image_only", sts["b"], ref, "poly", state=False)
    check_forward(what + " (c) exact", sts["c"], ref, "exact")
    check_forward(what + " (d) aux + exact", sts["d"], ref, "exact", aux=True)
    assert np.array_equal(sts["a"]["color"].view(np.uint32), sts["b"]["color"].view(np.uint32)), "%s: (a) and (b) differ in colour bits" % what
    assert np.array_equal(sts["c"]["color"].view(np.uint32), sts["d"]["color"].view(np.uint32)), "%s: (c) and (d) differ in colour bits" % what
    for k, mode in (("a", "poly"), ("c", "exact"), ("d", "exact")):
        check_designated("%s (%s)" % (what, k), info, sts[k], ref, li, mode)
    check_designated("%s (b)" % what, info, sts["b"], ref, li, "poly", state=False)
    # ---- backward after (c) and after (d)
    ok = ~amb
    got = backward(sc, policy, outs["c"], dpix)
    check_backward(what + " backward after (c)", got, ref, ok, ("dmean2D", "dconic", "dopacity", "dcolor"), c)
    gotx = backward(sc, policy, outs["d"], dpix, dd, da)
    check_backward(what + " backward after (d), aux", gotx, refx, ok, ("dmean2D", "dconic", "dopacity", "dcolor", "dz"), c)
