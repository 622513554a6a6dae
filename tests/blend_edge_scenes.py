"""Scenes that put the blend kernels' lists on their seams (gm_render.hip, gm_render_fwd_body.inc, gm_render_bwd_body.inc).

The builder generalises ordering_scenes.build: the camera sits at the origin and looks along +z; a Gaussian is given by the pixel its
centre projects to, a depth rank (z = 8 + rank / 1000: list order = rank order), a screen-space sigma in pixels (an isotropic
cov3D_precomp of (sigma z / fx)^2; the projected conic is about 1 / (sigma^2 + 0.3), exactly so at the image centre), an opacity and a
precomputed colour.  Nothing of that is assumed: a family states what it relies on as (pixel, entry) facts, and check_preconditions()
asserts them on the ORACLE's preprocess and binning through the float64 walk of blend_ref.

A family returns (scene, info).  info names the pixels, waves or Gaussians that carry its point:
    waves      {(x0, y0): dict(...)}   8 x 8 quadrants by their top-left pixel, with the facts wanted of them:
               survivors=[per 64-entry batch of the tile's list, the number of entries that reach the wave],
               taken=t (entries some pixel of the wave applies), empty=True (every n_contrib 0 although the list is not empty),
               all_stop=True (every pixel stops before the list ends), distinct=k (n_contrib takes >= k values), ...
    lengths    {tile: list length}
    designated [dict(name, pixel=(x, y), gid, expect=..., ambiguous=<set of 'exact' / 'poly'>)]: pairs that are checked one by one
    loud       Gaussian ids with colours of 40 .. 90 that lie BEHIND a stop: whatever leaks past the stop is visible at once
    stops      True: dpix_for() makes dL/dpixel a hundred times larger on the pixels that stop (a leak is then loud in the gradients too)"""
import numpy as np

import blend_ref
import ordering_scenes

BG = np.array([0.25, 0.5, 0.125], np.float32)
# Worst |C oracle - float64| / (2^-23 S_abs) over all families and blend-stage gradients, MEASURED by test_blend_ref_host.py (which fails
# when this record goes stale), and the GPU bound built on it: the factor 4 covers the kernel's one-ulp v_rcp / v_exp, its moment
# formulation and the atomics' summation order.  Neither number is fitted to what the HIP kernel produces.
# Recorded per KIND of family: the 90-entry stacks of `thresholds`, where the oracle rebuilds T by 90 float32 divisions, would otherwise set
# the bound of the families that carry the staging seams.  r_oracle of the whole suite is the largest entry (13.8).
R_ORACLE = dict(lengths=0.86, survivors=3.32, flush=2.26, stops=5.32, thresholds=13.78, ragged=4.03, children=1.83)


def kind_of(name):
    return name.partition(":")[0]


def c_gpu(name):
    """c = 4 max(r_oracle, 4) with the r_oracle of the family's kind"""
    return 4.0 * max(R_ORACLE[kind_of(name)], 4.0)
EPS = 2.0 ** -23


def build(W, H, cx, cy, rank, sigma, opac, color, orc=None, exact=None):
    """per Gaussian: centre pixel (cx, cy), depth rank, sigma [px], opacity, colour [P, 3].  exact ([P] bool, needs orc): nudge the mean by
    float32 neighbours until the ORACLE projects it to exactly (cx, cy)."""
    cx, cy, rank, sigma, opac = (np.asarray(v, np.float64).reshape(-1) for v in (cx, cy, rank, sigma, opac))
    P = cx.size
    cam = ordering_scenes.camera(W, H)
    z = 8.0 + rank * 1e-3
    ndcx = (2 * cx + 1) / W - 1; ndcy = (2 * cy + 1) / H - 1
    means = np.stack([cam["view"][0, 0] * ndcx * cam["tanx"] * z, cam["view"][1, 1] * ndcy * cam["tany"] * z, z], 1).astype(np.float32)
    fx = W / (2.0 * cam["tanx"])
    s = sigma * z / fx
    cov = np.zeros((P, 6), np.float32); cov[:, 0] = cov[:, 3] = cov[:, 5] = s * s
    sc = dict(means=means, opac=np.asarray(opac, np.float32).reshape(P, 1).copy(), cov3D_precomp=cov,
              colors_precomp=np.ascontiguousarray(color, np.float32).reshape(P, 3), W=W, H=H, cam=cam, rank=rank, cx=cx, cy=cy, sigma=sigma)
    if exact is not None and np.any(exact):
        want = np.stack([cx, cy], 1).astype(np.float32)
        for _ in range(16):
            xy = ordering_scenes.oracle_geo(orc, sc)["xy"]
            off = (xy != want) & np.asarray(exact, bool)[:, None]
            if not off.any():
                break
            for k in range(2):                                      # screen x, y grow as mean x, y FALL (view = diag(-1, -1, 1))
                up = off[:, k] & (xy[:, k] > want[:, k]); dn = off[:, k] & (xy[:, k] < want[:, k])
                means[up, k] = np.nextafter(means[up, k], np.float32(np.inf)); means[dn, k] = np.nextafter(means[dn, k], np.float32(-np.inf))
    return sc


def oracle_forward(orc, sc):
    """the oracle's preprocess + binning + forward of a scene"""
    return orc.forward_full(sc, sc["cam"], BG, D=0, use_precomp_cov=True, use_precomp_color=True)


def reference_of(fw, W, H, **kw):
    """blend_ref on the oracle's records and lists"""
    return blend_ref.reference(W, H, blend_ref.records(fw["geo"]), blend_ref.lists(fw["bins"]["ranges"], fw["bins"]["point_list"]), BG, **kw)


def reach(fw, W, H, x0, y0):
    """[list length] bool per entry of the 16-px tile of pixel (x0, y0): some pixel of the 8 x 8 wave at (x0, y0) takes it on its own
    (opacity * G >= 1/255), and the float64 minimum of the quadratic form over the wave's box minus 2 ln(255 opacity): > 0.1 = the cull
    (gm_cull.h may_touch, margin <= ~1e-2 here) surely drops the entry."""
    gx = (W + 15) // 16
    r0, r1 = fw["bins"]["ranges"][(y0 // 16) * gx + x0 // 16]
    g = fw["bins"]["point_list"][r0:r1].astype(np.int64)
    xy = fw["geo"]["xy"].astype(np.float64)[g]; co = fw["geo"]["conic_op"].astype(np.float64)[g]
    ys, xs = np.mgrid[y0:min(y0 + 8, H), x0:min(x0 + 8, W)]
    dx = xy[:, 0][:, None] - xs.reshape(1, -1); dy = xy[:, 1][:, None] - ys.reshape(1, -1)
    q = co[:, 0:1] * dx * dx + 2 * co[:, 1:2] * dx * dy + co[:, 2:3] * dy * dy
    with np.errstate(divide="ignore", invalid="ignore"):
        thr = 2 * np.log(255.0 * co[:, 3])
    # minimum over the (continuous) box: sample it finely - the forms here are far from degenerate
    fy, fxs = np.mgrid[y0:min(y0 + 7, H - 1) + 1e-9:0.125, x0:min(x0 + 7, W - 1) + 1e-9:0.125]
    ddx = xy[:, 0][:, None] - fxs.reshape(1, -1); ddy = xy[:, 1][:, None] - fy.reshape(1, -1)
    qmin = (co[:, 0:1] * ddx * ddx + 2 * co[:, 1:2] * ddx * ddy + co[:, 2:3] * ddy * ddy).min(axis=1)
    takes = (q <= thr[:, None]).any(axis=1) & (co[:, 3] >= blend_ref.A_MIN)
    return g, takes, qmin - thr


# ------------------------------------------------------------------------------------------------------------------------ families
LENGTHS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 321, 600)
SURVIVORS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 60, 61, 62, 63, 64)
FLUSH = (1, 2, 6, 7, 8, 13, 14, 15, 22, "8:one_lane")
RAGGED = ((37, 21), (17, 9), (8, 8))


# sigma of a "flat" splat.  Not the 40 first planned: at opacity 0.008 alpha >= 1/255 reaches sqrt(2 ln(255 * 0.008)) sigma = 1.19 sigma,
# 48 px at sigma 40 - short of the 89-px diagonal of the 64 x 64 frame of `children` (61 of 64 quadrants reached) and barely past the
# 44 px of 32 x 32.  At 60 it is 71 px from centres inside the frame's middle and the preconditions hold with room.
BIG = 60.0


def _between(rng, lo, hi, n):
    """centres BETWEEN pixel centres (k + 0.5 +- 0.3): a flat splat's exponent is then nowhere within rounding of 0 (the oracle's power > 0 skip)"""
    return np.floor(rng.uniform(lo, hi, n)) + 0.5 + rng.uniform(-0.3, 0.3, n)


def _colors(rng, n):
    return rng.uniform(0.05, 1.0, (n, 3))


def lengths(n):
    """full-tile splats (sigma BIG = 60, opacity 0.01: no pixel stops within 600 entries) on 32 x 32: every tile's list has n entries - the key
    chunks of 64, the ring's room test, the clamped tail loads list[min(.., nlast)] / list[max(.., 0)]"""
    rng = np.random.default_rng(1000 + n)
    W = H = 32
    sc = build(W, H, _between(rng, 0, W - 1, n), _between(rng, 0, H - 1, n), rng.permutation(n), np.full(n, BIG), rng.uniform(0.008, 0.012, n), _colors(rng, n))
    return sc, dict(lengths={t: n for t in range(4)}, no_stop=[(0, 0, 32, 32)])


def _big_and_far(rng, W, H, kinds, big_xy, far_xy):
    """list in rank order: kinds[i] True = a big splat (sigma BIG = 60) every pixel takes, False = a sigma 1.5 splat about far_xy"""
    n = len(kinds)
    kinds = np.asarray(kinds, bool)
    cx = np.where(kinds, _between(rng, big_xy[0] - 4, big_xy[0] + 4, n), rng.uniform(far_xy[0] - 0.5, far_xy[0] + 0.5, n))
    cy = np.where(kinds, _between(rng, big_xy[1] - 4, big_xy[1] + 4, n), rng.uniform(far_xy[1] - 0.5, far_xy[1] + 0.5, n))
    sigma = np.where(kinds, BIG, 1.5)
    opac = np.where(kinds, rng.uniform(0.008, 0.012, n), rng.uniform(0.3, 0.6, n))
    return cx, cy, sigma, opac


def survivors(s):
    """one 16-px tile; the wave of quadrant (0, 0) sees batches of 64 candidates of which exactly s, (3 s + 1) % 65 and 3 of a tail of 10
    survive the cull (the others: sigma 1.5 splats about (12.5, 12.5), out of the quadrant's reach): groups of 16 exponents, the four
    padding slots behind the last survivor, the GM_FWD_SUB sub-blocks' early break; s = 0: a first batch without survivors, then one"""
    rng = np.random.default_rng(2000 + s)
    per = [s, (3 * s + 1) % 65, 3]
    kinds = []
    for size, k in zip((64, 64, 10), per):
        m = np.zeros(size, bool); m[rng.choice(size, k, replace=False)] = True
        kinds += list(m)
    n = len(kinds)
    cx, cy, sigma, opac = _big_and_far(rng, 16, 16, kinds, (3.5, 3.5), (12.5, 12.5))
    sc = build(16, 16, cx, cy, np.arange(n), sigma, opac, _colors(rng, n))
    return sc, dict(lengths={0: n}, waves={(0, 0): dict(survivors=per)}, no_stop=[(0, 0, 8, 8)])


def flush(t):
    """one 16-px tile, a list of 64: the wave of quadrant (0, 0) takes exactly t entries in the backward (one batch: ns == t) - the
    seven-slot phase-2 flush, its 63-lane commit, the final partial flush, the two-register-set entry pipeline with ns odd and even
    (t = 7, 15 odd and 8, 14, 22 even on either residue 0 / 1 modulo 7).  '8:one_lane': one of the 8 is taken by a single pixel."""
    one_lane = isinstance(t, str)
    tt = int(str(t).split(":")[0])
    rng = np.random.default_rng(3000 + tt + (100 if one_lane else 0))
    kinds = np.zeros(64, bool); kinds[rng.choice(64, tt, replace=False)] = True
    cx, cy, sigma, opac = _big_and_far(rng, 16, 16, kinds, (3.5, 3.5), (12.5, 12.5))
    info = dict(lengths={0: 64}, waves={(0, 0): dict(taken=tt, survivors=[tt])}, no_stop=[(0, 0, 8, 8)])
    if one_lane:
        i = int(np.nonzero(kinds)[0][3])
        cx[i], cy[i], sigma[i], opac[i] = 5.0, 2.0, 0.5, 0.006          # opacity * G < 1/255 one pixel away
        info["single"] = dict(gid=i, pixel=(5, 2))
    sc = build(16, 16, cx, cy, np.arange(64), sigma, opac, _colors(rng, 64))
    return sc, info


def stops():
    """32 x 32.  Tile 0: a stack of 300 high-opacity sigma-2.5 splats about (-3, 3) - a pixel's stop position falls with its distance, so
    n_contrib takes many values inside the wave at (0, 0), from 1 (pixel (5, 5): two opacity-1 splats centred on it come first) to beyond
    128 - followed by loud entries of the same footprint; the wave at (8, 0) is reached by nothing (n_contrib == 0, list not empty).
    Tile 3: a wall of 24 sigma-4 splats about (27, 27) stops every pixel of the wave at (24, 24) before the list's loud end."""
    rng = np.random.default_rng(4000)
    W = H = 32
    cx, cy, sg, op, col, rk = [], [], [], [], [], []

    def put(x, y, s_, o, c, r):
        cx.append(x); cy.append(y); sg.append(s_); op.append(o); col.append(c); rk.append(r)
    loud = []
    put(5.0, 5.0, 0.5, 1.0, (0.9, 0.1, 0.3), 0); put(5.0, 5.0, 0.5, 1.0, (0.2, 0.8, 0.4), 1)
    for i in range(300):
        put(-3.0 + rng.uniform(-0.05, 0.05), 3.0 + rng.uniform(-0.05, 0.05), 2.5, rng.uniform(0.80, 0.90), tuple(rng.uniform(0.05, 1, 3)), 2 + i)
    for i in range(6):
        loud.append(len(cx)); put(-3.0, 3.0, 2.5, 0.7, (60.0, 45.0, 80.0), 400 + i)
    for i in range(24):
        put(27.0 + rng.uniform(-0.05, 0.05), 27.0 + rng.uniform(-0.05, 0.05), 4.0, rng.uniform(0.9, 0.97), tuple(rng.uniform(0.05, 1, 3)), 500 + i)
    for i in range(6):
        loud.append(len(cx)); put(27.0, 27.0, 4.0, 0.7, (70.0, 55.0, 40.0), 600 + i)
    exact = np.zeros(len(cx), bool); exact[:2] = True
    return (cx, cy, rk, sg, op, col, exact), dict(waves={(0, 0): dict(distinct=8, lo=1, hi=129), (8, 0): dict(empty=True), (24, 24): dict(all_stop=True)},
                                                 loud=loud, stops=True,
                                                 designated=[dict(name="second of two clamped entries stops", pixel=(5, 5), gid=1, expect=("last", 0), ambiguous=set())])


def thresholds():
    """32 x 32, sigma-0.4 splats centred EXACTLY on pixels four apart (power exactly 0 there, alpha = min(0.99, opacity); nothing of a
    neighbour reaches them): opacities at and around 1/255, on either side of may_touch's 0.0039 guard, around the 0.99 clamp; stop products
    T (1 - alpha) at 1e-4 (1 +- k d_T) from two entries and from 90.  A loud entry lies behind every stack that is meant to stop."""
    rng = np.random.default_rng(5000)
    W = H = 32
    f = np.float32
    a = float(f(1.0) / f(255.0))
    d_e = 8 * EPS
    slots = [(2 + 4 * i, 2 + 4 * j) for j in range(8) for i in range(8)]
    rng.shuffle(slots)
    cx, cy, op, col, rk = [], [], [], [], []
    des = []
    loud = []
    SIG = 0.4
    # the polynomial's distance at a centred pixel: d_pow + 8 ulp (mag' + 1), mag' the conic's terms at 3.5 px (conic <= 1 / (0.16 + 0.3) + 10 %)
    d_p = d_e + 8 * EPS * (2.4 * 3.5 * 3.5 * 2.0 + 1.0)

    def put(px, o, c, r):
        cx.append(px[0]); cy.append(px[1]); op.append(o); col.append(c); rk.append(r)
        return len(cx) - 1
    r = [0]

    def single(name, o, expect, amb=()):
        px = slots.pop()
        g = put(px, float(f(o)), tuple(rng.uniform(0.3, 1, 3)), r[0]); r[0] += 1
        des.append(dict(name=name, pixel=px, gid=g, expect=expect, ambiguous=set(amb)))
    af = f(a)
    single("opacity == 1/255", af, "taken", ("exact", "poly"))
    single("1/255 + 1 ulp", np.nextafter(af, f(1)), "taken", ("exact", "poly"))
    single("1/255 - 1 ulp", np.nextafter(af, f(0)), "not_taken", ("exact", "poly"))
    for k in (4, 64):
        amb = ("poly",) if k == 4 else ()               # (64 d_pow lies beyond the polynomial's distance as well)
        single("1/255 (1 + %d d_pow)" % k, a * (1 + k * d_e), "taken", amb)
        single("1/255 (1 - %d d_pow)" % k, a * (1 - k * d_e), "not_taken", amb)
        single("1/255 (1 + %d d_pol)" % k, a * (1 + k * d_p), "taken")
        single("1/255 (1 - %d d_pol)" % k, a * (1 - k * d_p), "not_taken")
    # may_touch drops op < 0.0039f before anything else; 0.0039f itself and 0.00392 pass the guard and fall to the 1/255 test
    single("0.0039f - 1 ulp: below may_touch's guard", np.nextafter(f(0.0039), f(0)), "not_taken")
    single("0.0039f: on the guard (passes it), below 1/255", 0.0039, "not_taken")
    single("0.00392: above the guard, below 1/255", 0.00392, "not_taken")
    single("0.98", 0.98, ("alpha", float(f(0.98))))
    single("0.99", 0.99, ("alpha", blend_ref.A_MAX))
    single("0.99 + 1 ulp", np.nextafter(f(0.99), f(1)), ("alpha", blend_ref.A_MAX))
    single("0.99 - 1 ulp", np.nextafter(f(0.99), f(0)), ("alpha", float(np.nextafter(f(0.99), f(0)))))
    single("0.999", 0.999, ("alpha", blend_ref.A_MAX))
    single("1.0", 1.0, ("alpha", blend_ref.A_MAX))

    def stack(name, ops, last_target, stop, k):
        """entries `ops`, then one whose 1 - alpha = last_target / T, then a loud one"""
        px = slots.pop()
        T = 1.0
        for o in ops:
            put(px, float(f(o)), tuple(rng.uniform(0.3, 1, 3)), r[0]); r[0] += 1
            T *= 1.0 - min(blend_ref.A_MAX, float(f(o)))
        o_last = float(f(1.0 - last_target / T))
        g = put(px, o_last, (0.9, 0.6, 0.3), r[0]); r[0] += 1
        gl = put(px, 0.6, (90.0, 70.0, 50.0), r[0]); r[0] += 1
        loud.append(gl)
        des.append(dict(name=name, pixel=px, gid=g, expect=("last", g - 1 if stop else g), ambiguous=set(), loud=gl))
    # two entries: d_T = ulp + (ulp) [the clamped first entry does not move] + alpha / (1 - alpha) d + ulp
    for k in (4, 64):
        dT2 = 3 * EPS + 99.0 * d_p
        stack("two entries, T (1 - alpha) = 1e-4 (1 + %d d_T)" % k, [0.995], blend_ref.T_MIN * (1 + k * dT2), False, k)
    stack("two clamped entries: T (1 - alpha) = (1 - 0.99f)^2 < 1e-4", [0.995], 0.0, True, 0)
    # ~90 entries of alpha 0.0973 (0.9027^90 ~ 1e-4)
    for k in (4, 64):
        for sign in (1, -1):
            al = 0.0973
            dT = EPS + 90 * (al / (1 - al) * d_p + EPS)
            stack("90 entries, T (1 - alpha) = 1e-4 (1 %s %d d_T)" % ("+" if sign > 0 else "-", k), [al] * 89, blend_ref.T_MIN * (1 + sign * k * dT), sign < 0, k)
    n = len(cx)
    args = (cx, cy, rk, np.full(n, SIG), op, col, np.ones(n, bool))
    return args, dict(designated=des, loud=loud, stops=True)


def ragged(W, H):
    """image sizes that leave waves fully outside (8 x 8: three of four; 17 x 9: the right waves of tile 1), with one column (17 wide) or
    one row (9 high) inside; a third of the splats are centred outside the image"""
    rng = np.random.default_rng(6000 + W)
    n = 70
    cx = rng.uniform(-6, W + 5, n); cy = rng.uniform(-6, H + 5, n)
    sc = build(W, H, cx, cy, rng.permutation(n), rng.uniform(0.5, 6.0, n), rng.uniform(0.05, 0.95, n), _colors(rng, n))
    return sc, dict(ragged=True)


def children():
    """64 x 64: splats that reach one 8-px quadrant (sigma 0.6), one 16-px child (sigma 2), a 2 x 2 block of tiles (sigma 5), or the whole
    frame (sigma BIG = 60, opacity 0.01), interleaved in depth: under policies 2 and 3 a wave's own entries are few among long runs of others'
    (ring fill with sparse `mine`).  Whatever reaches the 16-px child (3, 3) comes in the last ranks: under policy 3 the first own entry
    of its four waves, the one at (56, 56) among them, lies beyond list position 256 of the 64-px parent."""
    rng = np.random.default_rng(7001)
    W = H = 64
    cx, cy, sg, op = [], [], [], []
    late = []
    for qy in range(8):
        for qx in range(8):
            for _ in range(8):
                cx.append(8 * qx + 3.5 + rng.uniform(-0.7, 0.7)); cy.append(8 * qy + 3.5 + rng.uniform(-0.7, 0.7)); sg.append(0.6); op.append(rng.uniform(0.3, 0.6))
                late.append(qx >= 6 and qy >= 6)
    for ty in range(4):
        for tx in range(4):
            for _ in range(2):
                cx.append(16 * tx + 7.5 + rng.uniform(-0.5, 0.5)); cy.append(16 * ty + 7.5 + rng.uniform(-0.5, 0.5)); sg.append(2.0); op.append(rng.uniform(0.3, 0.6))
                late.append(tx == 3 and ty == 3)
    for (bx, by) in ((15.5, 15.5), (47.5, 15.5), (15.5, 47.5), (47.5, 47.5), (31.5, 31.5)):
        for _ in range(3):
            cx.append(bx + rng.uniform(-0.5, 0.5)); cy.append(by + rng.uniform(-0.5, 0.5)); sg.append(5.0); op.append(rng.uniform(0.2, 0.4))
            late.append(bx > 40 and by > 40)
    for _ in range(20):
        cx.append(_between(rng, 0, 63, 1)[0]); cy.append(_between(rng, 0, 63, 1)[0]); sg.append(BIG); op.append(rng.uniform(0.008, 0.012)); late.append(True)
    late = np.asarray(late)
    n = late.size
    rank = np.empty(n, np.int64)
    rank[~late] = rng.permutation(int((~late).sum()))
    rank[late] = int((~late).sum()) + rng.permutation(int(late.sum()))
    sc = build(W, H, cx, cy, rank, sg, op, _colors(rng, n))
    sc["late"] = late
    return sc, dict(waves={(56, 56): dict(first_own_beyond=256)}, children=True)


def family(name, orc=None):
    """'lengths:65', 'survivors:17', 'flush:8', 'flush:8:one_lane', 'stops', 'thresholds', 'ragged:37x21', 'children' -> (scene, info)"""
    kind, _, arg = name.partition(":")
    if kind == "lengths":
        sc, info = lengths(int(arg))
    elif kind == "survivors":
        sc, info = survivors(int(arg))
    elif kind == "flush":
        sc, info = flush(arg if ":" in arg else int(arg))
    elif kind in ("stops", "thresholds"):
        (cx, cy, rk, sg, op, col, exact), info = stops() if kind == "stops" else thresholds()
        sc = build(32, 32, cx, cy, rk, sg, op, np.asarray(col), orc=orc, exact=exact)
        info["exact"] = exact
    elif kind == "ragged":
        w, h = arg.split("x")
        sc, info = ragged(int(w), int(h))
    elif kind == "children":
        sc, info = children()
    else:
        raise KeyError(name)
    info["name"] = name
    info.setdefault("designated", []); info.setdefault("loud", []); info.setdefault("waves", {})
    return sc, info


FAMILIES = (["lengths:%d" % n for n in LENGTHS] + ["survivors:%d" % s for s in SURVIVORS] + ["flush:%s" % t for t in FLUSH] +
            ["stops", "thresholds"] + ["ragged:%dx%d" % wh for wh in RAGGED] + ["children"])


def policies(name):
    kind = name.partition(":")[0]
    return {"lengths": (0, 2), "survivors": (0, 2), "flush": (0, 2), "children": (2, 3)}.get(kind, (0, 1, 2, 3))


def dpix_for(sc, info, ref):
    """dL/dpixel of a family: unit normal, a hundred times larger on the pixels that stop (reference's decision)"""
    rng = np.random.default_rng(99)
    W, H = sc["W"], sc["H"]
    d = rng.normal(size=(3, H, W))
    if info.get("stops"):
        stopped = ref["final_T"] < 0.02
        d = d * np.where(stopped, 100.0, 1.0)[None]
    return d.astype(np.float32)


def check_preconditions(sc, info, fw, ref):
    """Every property the family relies on, on the oracle's preprocess / binning (fw = oracle_forward) and the float64 walk over them
    (ref = reference_of(fw)).  Returns the number of ambiguous pixels outside the named pairs."""
    W, H = sc["W"], sc["H"]
    geo, bins = fw["geo"], fw["bins"]
    P = sc["means"].shape[0]
    gx = (W + 15) // 16
    vis = geo["radii"] > 0
    assert vis.all() or info.get("ragged"), "%d of %d Gaussians culled" % ((~vis).sum(), P)
    z = geo["depths"].astype(np.float64)
    order = np.argsort(sc["rank"], kind="stable")
    order = order[vis[order]]
    assert (np.diff(z[order]) > 0).all(), "depths do not follow the ranks"
    for t in range(bins["ranges"].shape[0]):                       # list order = rank order
        r0, r1 = bins["ranges"][t]
        assert (np.diff(sc["rank"][bins["point_list"][r0:r1].astype(np.int64)]) > 0).all()
    for t, n in info.get("lengths", {}).items():
        r0, r1 = bins["ranges"][t]
        assert int(r1 - r0) == n, "tile %d: list of %d, %d wanted" % (t, r1 - r0, n)
    if "exact" in info:
        want = np.stack([sc["cx"], sc["cy"]], 1).astype(np.float32)
        assert np.array_equal(geo["xy"][info["exact"]], want[info["exact"]]), "a centre is not exactly on its pixel"
    for (x0, y0, x1, y1) in info.get("no_stop", ()):
        assert (ref["final_T"][y0:y1, x0:x1] > 10 * blend_ref.T_MIN).all() and (ref["n_contrib"][y0:y1, x0:x1] > 0).all()
    nc = ref["n_contrib"]
    for (x0, y0), want in info["waves"].items():
        g, takes, slack = reach(fw, W, H, x0, y0)
        if "survivors" in want or "taken" in want:
            assert (slack[~takes] > 0.1).all(), "an entry that no pixel of the wave takes is not surely culled"
        if "survivors" in want:
            got = [int(takes[b:b + 64].sum()) for b in range(0, g.size, 64)]
            assert got == list(want["survivors"]), (got, want["survivors"])
        blk = nc[y0:y0 + 8, x0:x0 + 8]
        if "taken" in want:
            assert int(takes.sum()) == want["taken"]
        if want.get("empty"):
            assert (blk == 0).all() and g.size > 0
        if want.get("all_stop"):
            assert (blk < g.size).all() and (ref["final_T"][y0:y0 + 8, x0:x0 + 8] < 1e-2).all() and (blk > 0).all()
        if "distinct" in want:
            vals = np.unique(blk)
            assert vals.size >= want["distinct"] and vals.min() <= want["lo"] and vals.max() >= want["hi"], vals
        if "first_own_beyond" in want:                               # (in rank order over ALL Gaussians: the 64-px parent's list)
            hits = np.zeros(P, bool)
            for (u, v) in ((x0 - 8, y0 - 8), (x0, y0 - 8), (x0 - 8, y0), (x0, y0)):              # the four waves of the wave's 16-px child
                hits |= _reaches_wave(geo, u, v)
            assert hits.any() and sc["late"][hits].all() and int((~sc["late"]).sum()) > want["first_own_beyond"]
    if "single" in info:
        s_ = info["single"]
        m = blend_ref.reference(W, H, blend_ref.records(geo), blend_ref.lists(bins["ranges"], bins["point_list"]), BG, keep_pairs=True)["margins"][0]
        col = int(np.nonzero(m["g"] == s_["gid"])[0][0])
        hit = m["take"][:, col]
        assert hit.sum() == 1 and (m["xs"][hit][0], m["ys"][hit][0]) == s_["pixel"]
    if info.get("ragged"):
        assert vis.sum() >= 60 and ((geo["xy"][:, 0] < 0) | (geo["xy"][:, 0] > W - 1) | (geo["xy"][:, 1] < 0) | (geo["xy"][:, 1] > H - 1)).sum() >= 10
    if info.get("children"):
        for sg, lo, hi in ((0.6, 1, 1), (2.0, 4, 4), (5.0, 16, 16), (BIG, 64, 64)):          # quadrants reached
            for i in np.nonzero(np.isclose(sc["sigma"], sg))[0][:: 7]:
                nq = _quadrants_reached(geo, int(i), W, H)
                assert lo <= nq <= hi, (sg, nq)
    # designated pairs: unambiguous unless named, and the reference decides what the family wants
    named = np.zeros((H, W), bool)
    for d in info["designated"]:
        x, y = d["pixel"]
        if d["ambiguous"]:
            named[y, x] = True
    for d in info["designated"]:
        x, y = d["pixel"]
        for mode in ("exact", "poly"):
            assert bool(ref["amb_" + mode][y, x]) == (mode in d["ambiguous"]), (d["name"], mode)
    stray = (ref["amb_poly"] | ref["amb_oracle"]) & ~named
    return int(stray.sum())


def _reaches_wave(geo, x0, y0):
    xy = geo["xy"].astype(np.float64); co = geo["conic_op"].astype(np.float64)
    ys, xs = np.mgrid[y0:y0 + 8, x0:x0 + 8]
    dx = xy[:, 0][:, None] - xs.reshape(1, -1); dy = xy[:, 1][:, None] - ys.reshape(1, -1)
    oG = co[:, 3:4] * np.exp(np.minimum(-0.5 * (co[:, 0:1] * dx * dx + co[:, 2:3] * dy * dy) - co[:, 1:2] * dx * dy, 0.0))
    return (oG >= blend_ref.A_MIN).any(axis=1)


def _quadrants_reached(geo, i, W, H):
    xy = geo["xy"][i].astype(np.float64); co = geo["conic_op"][i].astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    dx, dy = xy[0] - xs, xy[1] - ys
    hit = co[3] * np.exp(-0.5 * (co[0] * dx * dx + co[2] * dy * dy) - co[1] * dx * dy) >= blend_ref.A_MIN
    return int(np.unique((ys[hit] // 8) * 8 + xs[hit] // 8).size)
