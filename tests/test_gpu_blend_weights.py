"""-m gpu: gm_blend_weights / gaussianmesh_amd.contribution against the float64 reference of tests/blend_weights_ref.py, per pixel
against the GM_FWD_EXACT_EXPONENT blend's own opacity map, and the exact properties of its integer accumulators."""
import math

import numpy as np
import pytest
import torch

import blend_weights_ref as ref

pytestmark = pytest.mark.gpu

UNIT = 2.0 ** -24


@pytest.fixture(autouse=True)
def _default_emission_policy():
    from gaussianmesh_amd import rasterizer as R
    yield
    R.set_default_emission_policy("auto")


def _frame(sc, cam, policy, image_only=False, exact=False, aux=False, pre_col=True):
    """a completed forward: (num_rendered, color, radii, geom, binning, img[, depth, alpha])"""
    from gpu_utils import T
    from gaussianmesh_amd import rasterizer as R
    H, W = cam["H"], cam["W"]
    h = R.rasterize_forward_begin(T(np.zeros(3, np.float32)), T(sc["means"]), T(sc["colors_precomp"]) if pre_col else None, T(sc["opac"]),
                                  T(sc["scales"]), T(sc["rots"]), 1.0, None, T(cam["view"]), T(cam["proj"]), cam["tanx"], cam["tany"],
                                  H, W, None if pre_col else T(sc["shs"]), 3, T(cam["campos"]), emission_policy=policy, aux=aux)
    return h.finish(image_only=image_only, exact_exponent=exact)


def _weights(sc, cam, policy, mask=None, sums=None, peak=None, **kw):
    """one frame + one gm_blend_weights; mask: numpy uint8 [H,W] or None.  Returns (sums int64 [P,2], peak bits int32 [P]) as numpy"""
    from gpu_utils import T
    from gaussianmesh_amd import contribution as cb
    out = _frame(sc, cam, policy, **kw)
    P = sc["means"].shape[0]
    m = None if mask is None else T(mask, dtype=torch.uint8)
    s, p = cb.blend_weights(policy, out[3], out[4], out[5], P, cam["W"], cam["H"], m, sums, peak, num_rendered=out[0])
    torch.cuda.synchronize()
    return s.cpu().numpy(), p.cpu().numpy()


def _peak_f(bits):
    return np.asarray(bits, np.int32).view(np.float32).astype(np.float64)


def _assert_matches_reference(name, r, sums, peak, what):
    """Per Gaussian: |total - ref| and |inside - ref| <= n 2^-25 + e, n = its accepted pixels (each quantised to 2^-24: half a unit), e = the
    rounding model's own distance summed over them, w (d_pow + d_T) - no flat allowance, no factor; peak within the largest such term;
    a row the reference never accepts exactly zero."""
    total, inside, pk = sums[:, 0] * UNIT, sums[:, 1] / 255.0 * UNIT, _peak_f(peak)
    bound = r["n_acc"] * 2.0 ** -25 + r["err"]
    e_t, e_i, e_p = np.abs(total - r["total"]), np.abs(inside - r["inside"]), np.abs(pk - r["peak"])
    seen = r["n_acc"] > 0
    use = lambda e, b: float((e[seen] / b[seen]).max()) if seen.any() else 0.0
    print("%s %s: %d rows, worst |total| %.3g, |inside| %.3g, |peak| %.3g; worst share of the bound: total %.3f inside %.3f peak %.3f" % (
        name, what, int(seen.sum()), e_t.max(), e_i.max(), e_p.max(), use(e_t, bound), use(e_i, bound), use(e_p, r["err_max"] + 2.0 ** -25)))
    never = ~seen
    assert not sums[never].any() and not peak[never].any(), "%s: a row the reference never accepts has a weight" % name
    assert (sums[seen, 0] > 0).all() and (peak[seen] != 0).all()
    assert (e_t <= bound).all(), (name, what, int(np.argmax(e_t - bound)))
    assert (e_i <= bound).all(), (name, what, int(np.argmax(e_i - bound)))
    # the largest weight: a float32 w, within the model's distance of the float64 one (its own rounding is the model's last ulp)
    assert (e_p <= r["err_max"] + 2.0 ** -25).all(), (name, what, int(np.argmax(e_p - r["err_max"])))


@pytest.mark.parametrize("policy", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ref.SCENES)
def test_against_the_reference(oracle, name, policy):
    sc, cam, fw, mask, r = ref.reference(oracle, name)
    assert r["census"] == 0                        # no pixel with a decision at a threshold: nothing to excuse
    sums, peak = _weights(sc, cam, policy, mask)
    _assert_matches_reference(name, r, sums, peak, "policy %d" % policy)


PROBES = [("s0", 0, 0, "corner"), ("s0", 16, 15, "tile edge"), ("s0", 47, 39, "partial tile"), ("mid", 69, 49, "last pixel, partial tile"),
          ("sat", None, None, "stopped pixel")]


@pytest.mark.parametrize("policy", [0, 2, 3])
@pytest.mark.parametrize("name,x,y,what", PROBES)
def test_per_pixel_probe(oracle, name, x, y, what, policy):
    """A mask that is 255 at one pixel: inside / 255 is that pixel's weight per Gaussian, and its sum over the Gaussians is out_alpha of
    gm_forward_1_aux with GM_FWD_EXACT_EXPONENT there - the same arithmetic; only the quantisation (half a unit of 2^-24 per entry) and
    the order of a float sum (the other half) differ: within (accepted entries) 2^-24."""
    sc, cam, fw, _, r = ref.reference(oracle, name)
    W, H = cam["W"], cam["H"]
    if x is None:                                   # a stopped pixel with the most accepted entries
        y, x = np.unravel_index(int(np.argmax(np.where(r["stopped"], r["accepted"], -1))), (H, W))
        assert r["stopped"][y, x] and r["accepted"][y, x] > 64
    mask = np.zeros((H, W), np.uint8); mask[y, x] = 255
    sums, _ = _weights(sc, cam, policy, mask)
    assert not (sums[:, 1] % 255).any()
    u = sums[:, 1] // 255
    n = int((u > 0).sum())
    alpha = _frame(sc, cam, policy, exact=True, aux=True)[7]
    torch.cuda.synchronize()
    a = float(alpha[0, y, x])
    got = float(u.sum()) * UNIT
    print("%s (%d, %d) %s, policy %d: %d accepted entries (reference %d), sum of weights %.9f, out_alpha %.9f, difference %.3g (allowed %.3g)" % (
        name, x, y, what, policy, n, int(r["accepted"][y, x]), got, a, abs(got - a), n * UNIT))
    assert n == r["accepted"][y, x]
    assert abs(got - a) <= n * UNIT
    assert abs(got - r["one_minus_T"][y, x]) <= 1e-4


@pytest.mark.parametrize("name", ["mid", "sat", "wide"])
def test_exact_integer_properties(oracle, name):
    from gaussianmesh_amd import scenes
    sc, cam, fw, mask, r = ref.reference(oracle, name)
    W, H = cam["W"], cam["H"]
    same = lambda a, b: np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    base = _weights(sc, cam, 0, mask)
    for policy in (1, 2, 3):
        assert same(base, _weights(sc, cam, policy, mask)), "policy %d differs from policy 0" % policy
    assert same(base, _weights(sc, cam, 0, mask)), "two runs differ"
    # no mask = 255 everywhere: inside == 255 total
    full = _weights(sc, cam, 2, None)
    assert same(full, _weights(sc, cam, 2, np.full((H, W), 255, np.uint8)))
    assert np.array_equal(full[0][:, 1], 255 * full[0][:, 0]) and np.array_equal(full[0][:, 0], base[0][:, 0]) and np.array_equal(full[1], base[1])
    zero = _weights(sc, cam, 2, np.zeros((H, W), np.uint8))
    assert not zero[0][:, 1].any() and np.array_equal(zero[0][:, 0], base[0][:, 0])
    # inside is linear in the mask
    m1 = (mask // 3).astype(np.uint8); m2 = (mask - m1).astype(np.uint8)
    assert np.array_equal(_weights(sc, cam, 3, m1)[0][:, 1] + _weights(sc, cam, 3, m2)[0][:, 1], base[0][:, 1])
    # two views into one buffer = the sum of the two single-view results (peak: the larger)
    cam2 = scenes.orbit_camera(3, 7, W, H, radius=6.0)
    mask2 = np.ascontiguousarray(mask[::-1])
    one = _weights(sc, cam2, 2, mask2)
    from gpu_utils import T
    s = T(base[0], dtype=torch.int64); p = T(base[1], dtype=torch.int32)
    both = _weights(sc, cam2, 2, mask2, sums=s, peak=p)
    assert np.array_equal(both[0], base[0] + one[0])
    assert np.array_equal(both[1].view(np.uint32), np.maximum(base[1].view(np.uint32), one[1].view(np.uint32)))
    # after an image-only second half, after the exact-exponent one, after one that also wrote the maps: the same
    for kw in (dict(image_only=True), dict(exact=True), dict(aux=True), dict(aux=True, image_only=True)):
        assert same(base, _weights(sc, cam, 1, mask, **kw)), kw


def test_refused_or_mismatched_frames_add_nothing(oracle):
    from gpu_utils import T
    from gaussianmesh_amd import contribution as cb
    sc, cam, fw, mask, r = ref.reference(oracle, "s1")
    P, W, H = 300, cam["W"], cam["H"]
    nr, _, _, geom, binning, img = _frame(sc, cam, 2)
    s, p = cb.blend_weights(3, geom, binning, img, P, W, H, T(mask, dtype=torch.uint8), num_rendered=nr)     # lists of policy 2 walked as policy 3
    assert not s.any() and not p.any()
    s, p = cb.blend_weights(2, geom, binning, img, P, W, H, T(mask, dtype=torch.uint8), num_rendered=nr)
    assert s[:, 0].sum() > 0
    # a sync-free frame whose instances do not fit its capacity is refused (status word 3): nothing is added
    from gaussianmesh_amd import rasterizer as R
    h = R.rasterize_forward_begin(T(np.zeros(3, np.float32)), T(sc["means"]), T(sc["colors_precomp"]), T(sc["opac"]), T(sc["scales"]), T(sc["rots"]),
                                  1.0, None, T(cam["view"]), T(cam["proj"]), cam["tanx"], cam["tany"], H, W, None, 3, T(cam["campos"]), emission_policy=2)
    out = h.finish(sync_free=True, capacity=8)
    ok, count = h.check()
    assert not ok and count > 8
    s, p = cb.blend_weights(2, out[3], out[4], out[5], P, W, H, None, num_rendered=8)
    torch.cuda.synchronize()
    assert not s.any() and not p.any()
    # the same frame with room: the sync-free layout (the capacity, not the count) gives the exact path's result
    h = R.rasterize_forward_begin(T(np.zeros(3, np.float32)), T(sc["means"]), T(sc["colors_precomp"]), T(sc["opac"]), T(sc["scales"]), T(sc["rots"]),
                                  1.0, None, T(cam["view"]), T(cam["proj"]), cam["tanx"], cam["tany"], H, W, None, 3, T(cam["campos"]), emission_policy=2)
    out = h.finish(sync_free=True, capacity=5000, image_only=True)
    assert h.check()[0]
    s, p = cb.blend_weights(2, out[3], out[4], out[5], P, W, H, T(mask, dtype=torch.uint8), num_rendered=5000)
    torch.cuda.synchronize()
    base = _weights(sc, cam, 2, mask)
    assert np.array_equal(s.cpu().numpy(), base[0]) and np.array_equal(p.cpu().numpy(), base[1])


def _one_gaussian():
    from gaussianmesh_amd import scenes
    sc = scenes.make_cloud(1, seed=0)
    sc["means"][:] = 0.0; sc["scales"][:] = 3.0; sc["opac"][:] = 1.0
    sc["colors_precomp"] = np.full((1, 3), 0.5, np.float32)
    return sc, scenes.orbit_camera(0, 7, 17, 17, radius=8.0, height=0.0)


def test_edges(oracle):
    from gpu_utils import T
    from gaussianmesh_amd import contribution as cb, scenes
    # one Gaussian of opacity 1 over the whole 17 x 17 frame: every pixel accepts it, min(0.99, .) clamps it at the centre
    sc, cam = _one_gaussian()
    fw = oracle.forward_full(sc, cam, np.zeros(3, np.float32), use_precomp_color=True)
    mask = np.random.default_rng(5).integers(0, 256, size=(17, 17)).astype(np.uint8)
    r = ref.walk(fw, 17, 17, mask)
    assert r["census"] == 0 and r["n_acc"][0] == 289 and r["peak"][0] == 0.99
    for policy in (0, 1, 2, 3):
        sums, peak = _weights(sc, cam, policy, mask)
        _assert_matches_reference("one Gaussian", r, sums, peak, "policy %d" % policy)
        assert peak.view(np.float32)[0] == np.float32(0.99)
    # nothing visible: every Gaussian behind the camera
    sc, cam, *_ = ref.reference(oracle, "s0")
    hidden = dict(sc); hidden["means"] = np.repeat(cam["campos"][None] * 1.5, 300, axis=0).astype(np.float32)
    sums, peak = _weights(hidden, cam, 2, None)
    assert not sums.any() and not peak.any()
    # P == 0: GM_OK, nothing touched
    out = _frame(sc, cam, 2)
    s, p = cb.blend_weights(2, out[3], out[4], out[5], 0, cam["W"], cam["H"], None, num_rendered=0)
    assert s.shape == (0, 2) and p.shape == (0,)
    from gaussianmesh_amd._lib import GmeshError
    with pytest.raises(GmeshError, match="mask"):
        cb.blend_weights(2, out[3], out[4], out[5], 300, cam["W"], cam["H"], torch.zeros((cam["H"], cam["W"] + 1), dtype=torch.uint8, device="cuda"),
                         num_rendered=out[0])
    with pytest.raises(GmeshError, match="sums"):
        cb.blend_weights(2, out[3], out[4], out[5], 300, cam["W"], cam["H"], None, torch.zeros((300, 2), dtype=torch.int32, device="cuda"),
                         num_rendered=out[0])
    with pytest.raises(GmeshError, match="overlaps"):
        both = torch.zeros((300 * 5,), dtype=torch.int32, device="cuda")
        cb.blend_weights(2, out[3], out[4], out[5], 300, cam["W"], cam["H"], None, both[:1200].view(torch.int64).view(300, 2), both[1196:1496],
                         num_rendered=out[0])


@pytest.mark.parametrize("name", ["s2", "wide"])
def test_poisoned_guard_banded_buffers(oracle, name):
    """sums, peak and mask inside poisoned blocks with guard bands: nothing outside [P] is written, and - the result being the same bit
    for bit whatever surrounds the mask - the mask is never read outside [H * W]."""
    from poison import differing, run_under_fills
    from gpu_utils import T
    from gaussianmesh_amd import contribution as cb
    sc, cam, fw, mask, r = ref.reference(oracle, name)
    P, W, H = sc["means"].shape[0], cam["W"], cam["H"]
    mask_t = T(mask, dtype=torch.uint8)

    def route():
        m = torch.empty((H, W), dtype=torch.uint8, device="cuda"); m.copy_(mask_t)
        s = torch.empty((P, 2), dtype=torch.int64, device="cuda"); s.zero_()
        p = torch.empty((P,), dtype=torch.int32, device="cuda"); p.zero_()
        nr, _, _, geom, binning, img = _frame(sc, cam, 3)
        cb.blend_weights(3, geom, binning, img, P, W, H, m, s, p, num_rendered=nr)
        return s, p

    runs = run_under_fills(route)
    assert differing(runs) == []
    s, p = runs[0][1]
    _assert_matches_reference(name, r, s.cpu().numpy(), p.cpu().numpy(), "poisoned")


class _Cloud:
    """the model getters accumulate() reads, over activated tensors"""

    def __init__(self, sc):
        from gpu_utils import T
        self.get_xyz, self.get_features, self.get_opacity = T(sc["means"]), T(sc["shs"]), T(sc["opac"])
        self.get_scaling, self.get_rotation, self.active_sh_degree = T(sc["scales"]), T(sc["rots"]), 3


def test_accumulate_equals_hand_driven_calls():
    from helpers import small_scene
    from gpu_utils import T
    from gaussianmesh_amd import contribution as cb, scenes
    from gaussianmesh_amd.dataset import GroundTruth
    from gaussianmesh_amd.renderer import Camera
    sc, _ = small_scene(P=800, W=70, H=50, seed=9)
    sc["rots"] /= np.linalg.norm(sc["rots"], axis=1, keepdims=True)
    W, H = 70, 50
    cams = [scenes.orbit_camera(k, 3, W, H, radius=6.0) for k in range(3)]
    rng = np.random.default_rng(2)
    masks = [rng.integers(0, 256, size=(H, W)).astype(np.uint8) for _ in range(3)]
    given = [T(masks[0], dtype=torch.uint8), GroundTruth(torch.zeros((3, H, W), dtype=torch.uint8, device="cuda"), T(masks[1][None], dtype=torch.uint8)),
             GroundTruth(torch.zeros((3, H, W), dtype=torch.uint8, device="cuda"))]          # the third view has no mask: all inside
    masks[2] = None
    con = cb.accumulate(_Cloud(sc), [Camera(c, "cuda") for c in cams], given, emission_policy=2)
    torch.cuda.synchronize()
    s = p = None
    for c, m in zip(cams, masks):
        out = _weights(sc, c, 2, m, sums=s, peak=p, pre_col=False)
        s, p = T(out[0], dtype=torch.int64), T(out[1], dtype=torch.int32)
    assert con.views == 3 and np.array_equal(con.sums.cpu().numpy(), out[0]) and np.array_equal(con.peak_bits.cpu().numpy(), out[1])
    assert np.array_equal(con.total.cpu().numpy(), out[0][:, 0] * UNIT) and con.inside.dtype == torch.float64
    assert np.array_equal(con.peak.cpu().numpy(), out[1].view(np.float32))
    # no masks at all: inside == total
    con0 = cb.accumulate(_Cloud(sc), [Camera(c, "cuda") for c in cams], None, emission_policy=3)
    assert torch.equal(con0.sums[:, 1], 255 * con0.sums[:, 0]) and torch.equal(con0.sums[:, 0], con.sums[:, 0])


def test_select_and_split_on_the_torus_scene():
    """contribution_scene.torus_in_shell, six views, masks = where the torus ALONE covers the pixel (its rendered opacity >= 0.1).
    A shell row has a view that sees it beside the object: a whole splat's mass outside the mask, against what other views see of it
    through the object (T ~ 0 there).  An object row keeps >= 89 % of a front-most splat's mass where its own alpha >= 0.1
    (1 - 0.1 / 0.95); rows seen only edge-on behind others may fall short: at least 98 % of the object rows some view saw are selected,
    and no shell row."""
    from contribution_scene import torus_in_shell
    from gaussianmesh_amd import contribution as cb
    W, H = 120, 90
    pc, n_obj, cams, alphas = torus_in_shell(W, H, 6, 60.0, 60, 24, 0.09, 1500, 1.2)
    P = pc.get_number
    n_bg = P - n_obj
    assert n_bg > 100
    masks = [((a >= 0.1) * 255).to(torch.uint8).contiguous() for a in alphas]
    con = cb.accumulate(pc, cams, masks)
    rows = cb.select(con, 0.5)
    seen = con.total > 0
    obj = torch.arange(P, device="cuda") < n_obj
    frac = float(rows[obj & seen].float().mean())
    print("torus: %d of %d object rows seen, %.4f of them selected; %d of %d shell rows seen, %d selected" % (
        int((obj & seen).sum()), n_obj, frac, int((~obj & seen).sum()), n_bg, int(rows[~obj].sum())))
    assert int((obj & seen).sum()) > 0.9 * n_obj and bool(seen[~obj].all())
    assert not rows[~obj].any()
    assert frac >= 0.98
    assert not rows[~seen].any()
    sel, rest = cb.split_plain(pc, rows)
    assert sel.get_number == int(rows.sum()) and sel.get_number + rest.get_number == P
    assert torch.equal(sel._xyz, pc._xyz[rows]) and torch.equal(rest._opacity, pc._opacity[~rows])
    # pruning: 1/255 as the least peak keeps only rows some view accepted
    keep = cb.importance_rows(con, min_peak=1.0 / 255.0)
    assert not keep[~seen].any() and int(keep.sum()) > 0.5 * int(seen.sum())
    half = cb.importance_rows(con, keep_fraction=0.5)
    assert int(half.sum()) == round(0.5 * P) and con.sums[half, 0].min() >= con.sums[~half, 0].max()


def test_after_a_direct_depth_placement_frame():
    """A frame begun with direct depth placement (GM_STREAM_DIRECT: depth_key is not written) is accepted - the walk reads the lists and
    the splat records only - and gives the partition path's result bit for bit."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from gpu_utils import T
    from gaussianmesh_amd import contribution as cb, rasterizer as Rz, scenes
    from gaussianmesh_amd.deform import mesh_rs_packed, vertex_face_adjacency
    P, W, H = 3000, 160, 96
    host = bench.build_scene(P, W, H, 2)
    g = {k: T(host[k]) for k in ("weights", "pos", "cov", "opac", "shs", "verts")}
    tri, faces = T(host["tri"], dtype=torch.int32), T(host["faces"], dtype=torch.int32)
    off, adj = vertex_face_adjacency(host["faces"], host["verts"].shape[0])
    packed = mesh_rs_packed(g["verts"], T(np.ascontiguousarray(host["mesh"][0][:, 0:3])), faces, (torch.tensor(off, device="cuda"), torch.tensor(adj, device="cuda")))
    cam = scenes.orbit_camera(1, 12, W, H)
    bg = torch.zeros(3, device="cuda")
    mask = T(np.random.default_rng(8).integers(0, 256, size=(H, W)), dtype=torch.uint8)
    plan, ws = Rz.new_depth_plan(bg.device), Rz.RasterWorkspace()
    results, direct = [], []
    for i in range(3):
        h = Rz.forward_deformed_begin(bg, tri, g["weights"], packed, g["cov"], g["pos"], g["shs"], g["opac"], T(cam["view"]), T(cam["proj"]), cam["tanx"],
                                      cam["tany"], H, W, 3, T(cam["campos"]), False, workspace=ws, depth_plan=plan)
        direct.append(bool(h.direct))
        out = h.finish(image_only=True)
        s, p = cb.blend_weights(h.policy, out[3], out[4], out[5], P, W, H, mask, num_rendered=out[0])
        torch.cuda.synchronize()
        results.append((s.cpu().numpy(), p.cpu().numpy()))
    assert direct == [False, True, True] and plan.refused == 0
    assert results[0][0][:, 0].sum() > 0
    for r in results[1:]:
        assert np.array_equal(r[0], results[0][0]) and np.array_equal(r[1], results[0][1])
