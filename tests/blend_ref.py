"""Float64 reference of the blend stage (gm_render.hip: render_fwd_kernel / render_bwd_kernel and their aux variants).  numpy only.

It reads the float32 records the kernels read - per Gaussian xy, conic, opacity, rgb and view depth z, per parent tile a range into the
point list (and, under the culled emission policies, the child mask of every list entry) - and evaluates the blend in float64 with the
KERNELS' decision rules, which are the reference's (RAST/forward.cu:336-352) with `power` clamped at 0 instead of skipped:

    oG = opacity * exp(min(power, 0));   skip the entry when oG < 1/255;   alpha = min(0.99, oG);
    stop, WITHOUT applying the entry, when T (1 - alpha) < 1e-4        (the three constants are the float32 ones the kernels compare with).

A whole parent tile is evaluated at once as [pixels, entries] arrays (cumulative products along the entries), so a 64 x 64 image with
600-entry lists takes well under a second.

Ambiguity.  Two correct float32 evaluations can take another decision only where a threshold lies within rounding distance of the value
compared with it.  The distances are the ones of helpers.account_outlier_pixels, restated:
    mag   = |con.x| dx^2 / 2 + |con.z| dy^2 / 2 + |con.y dx dy|                the exponent's cancelling terms
    d_pow = 8 ulp (mag + 1)                                                     the per-pixel exponent form (GM_FWD_EXACT_EXPONENT, the backward)
    d_pol = d_pow + 8 ulp (mag' + 1),  mag' = mag at |dx| + 3.5, |dy| + 3.5     the matrix-core polynomial (formed about a point <= 3.5 px away)
    d_T   = ulp + sum over the accepted entries in front of (alpha / (1 - alpha) d + ulp)      log T at the stop test
An entry a pixel VISITS (it is the pixel's wave's own, and lies at or before the pixel's stop) is ambiguous when
    |log(255 oG)| <= d   (the alpha >= 1/255 skip),   or   it is accepted and |log(T (1 - alpha) / 1e-4)| <= d_T   (the stop),
and - for the comparison with the C oracle only, whose walk SKIPS power > 0 - when |power| <= d_pow, opacity >= 0.99 / 255 and mag > 0
(mag == 0 <=> dx == dy == 0 exactly: the exponent is then exactly 0 in every evaluation, nothing rounds).
The min(0.99, .) clamp is continuous: it is no decision.
TWO PLACES DIFFER FROM THE HELPER, both narrowing what counts as ambiguous (the tests get stricter, never laxer):
  * the helper accumulates alpha / (1 - alpha) d into d_T for every accepted entry; here an entry clamped at 0.99 beyond the reach of its
    distance (oG >= 0.99 e^d) adds its product's ulp only - its alpha is exactly 0.99 in every evaluation (the helper's own docstring:
    "entries clamped at 0.99 do not move").  Without this the two-clamped-entries stop, (1 - 0.99f)^2 against 1e-4, could not be designated.
  * the helper's power test has no `mag > 0` exemption; here a pixel exactly on a splat's centre is exempt (see above), or no splat
    centred on a pixel could be designated at all.
Per pixel the walk also returns `loud`: the largest |colour| among the entries the pixel can possibly blend (its own, within reach of
alpha >= 1/255 by the polynomial's distance, at or before its first DEFINITE stop), at least 1 - the scale of one flipped entry's weight.

Rounding budget of the backward (S_abs).  Every output element is a sum over (pixel, entry) pairs of products; S_abs is the same sum with
every product replaced by the product of the absolute values of its uncancelled parts:
    dL/dalpha = T cd - A / (1 - alpha)      ->   D = |T cd| + |A / (1 - alpha)|         (cd = colour . dL/dpixel, A = what is blended behind)
    h = oG dL/dalpha                         ->   |h| := oG D
    dopacity  += G dL/dalpha                 ->   G D
    dconic    += -1/2 h (dx^2, dx dy, dy^2)  ->   1/2 |h| (dx^2, |dx dy|, dy^2)
    dmean2D.x += W/2 h (-a dx - b dy)        ->   W/2 (|a| |h dx| + |b| |h dy|)           (the kernel sums MOMENTS of h: sum h dx and sum h dy
    dmean2D.y += H/2 h (-c dy - b dx)        ->   H/2 (|c| |h dy| + |b| |h dx|)            round separately before the conic multiplies them)
    dcolor    += alpha T dL/dpixel           ->   alpha T |dL/dpixel|;      dz += alpha T dL/ddepth   ->   alpha T |dL/ddepth|
A float32 evaluation of such a sum is off by a small multiple of 2^-23 S_abs whatever cancels inside it; the multiple is measured on the
C oracle in test_blend_ref_host.py (r_oracle), never on the HIP kernel.
The gradient flows through the 0.99 clamp exactly as in orc_render_bwd / backward.cu (dL/dG = opacity dL/dalpha, clamped or not)."""
import numpy as np

EPS = 2.0 ** -23
A_MIN = float(np.float32(1.0) / np.float32(255.0))
A_MAX = float(np.float32(0.99))
T_MIN = float(np.float32(0.0001))
CHUNK = 1024                          # pixels per block of a parent tile


def records(geo):
    """the oracle's preprocess output (or gpu_utils.forward_state's) as the dict of float32 records the walk reads"""
    return dict(xy=np.asarray(geo["xy"], np.float32), conic_op=np.asarray(geo["conic_op"], np.float32), rgb=np.asarray(geo["rgb"], np.float32),
                z=np.asarray(geo["depths"], np.float32))


def records_from_state(st):
    """gpu_utils.forward_state's splat records (x, y, conic xyz, opacity, rgb) + the depth keys"""
    sp = st["splat"]
    return dict(xy=sp[:, 0:2].copy(), conic_op=np.concatenate([sp[:, 2:5], sp[:, 5:6]], 1), rgb=sp[:, 6:9].copy(),
                z=st["depth_key"].astype(np.uint32).view(np.float32))


def lists(ranges, point_list, policy=0, child_mask=None):
    """policy 0 / 1: one list per 16-px tile; 2: per 32-px parent, mask bit qy * 4 + qx per 8-px quadrant; 3: per 64-px parent, mask bit
    cy * 4 + cx per 16-px child"""
    return dict(ranges=np.asarray(ranges, np.int64).reshape(-1, 2), point_list=np.asarray(point_list, np.int64), policy=int(policy),
                child_mask=None if child_mask is None else np.asarray(child_mask, np.int64))


def pixel_bit(policy, x, y):
    """the child-mask bit of pixel (x, y)'s wave"""
    if policy == 2:
        return 1 << (((y % 32) // 8) * 4 + (x % 32) // 8)
    if policy == 3:
        return 1 << (((y % 64) // 16) * 4 + (x % 64) // 16)
    return 1


def reference(W, H, rec, li, bg, dL_dpix=None, dL_ddepth=None, dL_dalpha=None, keep_pairs=False):
    """-> dict.  Forward, per pixel [H, W]: color [3, H, W], final_T, n_contrib, alpha, depth; the flags amb_exact / amb_poly / amb_oracle
    and the first-order rounding bounds bound_exact / bound_poly = dict(color, final_T, depth) (alpha's is final_T's); `pairs`: the
    ambiguous (y, x, list position, kind) tuples; with keep_pairs `margins`: per parent block the arrays (ys, xs, visited, log(255 oG),
    d_pow, d_pol, log(T (1 - alpha) / 1e-4), d_T).
    Backward (dL_dpix given), per Gaussian: dmean2D [P, 2], dconic [P, 3], dopacity [P], dcolor [P, 3], dz [P] and S_<name> of each."""
    xy = rec["xy"].astype(np.float64); co = rec["conic_op"].astype(np.float64); rgb = rec["rgb"].astype(np.float64); zz = rec["z"].astype(np.float64)
    P = xy.shape[0]
    bg = np.asarray(bg, np.float64).reshape(3)
    policy = li["policy"]
    s = max(policy - 1, 0)
    side = 16 << s
    pgx, pgy = -(-W // side), -(-H // side)
    out = dict(color=np.zeros((3, H, W)), final_T=np.ones((H, W)), n_contrib=np.zeros((H, W), np.int64), alpha=np.zeros((H, W)),
               depth=np.zeros((H, W)), front_bound=np.full((H, W), 2 * EPS), loud=np.ones((H, W)), pairs=[], margins=[])
    for k in ("amb_exact", "amb_poly", "amb_oracle"):
        out[k] = np.zeros((H, W), bool)
    for m in ("exact", "poly"):
        out["bound_" + m] = dict(color=np.zeros((H, W)), final_T=np.zeros((H, W)), depth=np.zeros((H, W)))
    out["color"] += bg[:, None, None]
    bwd = dL_dpix is not None
    if bwd:
        dp = np.asarray(dL_dpix, np.float64).reshape(3, H, W)
        dpd = np.zeros((H, W)) if dL_ddepth is None else np.asarray(dL_ddepth, np.float64).reshape(H, W)
        dpa = np.zeros((H, W)) if dL_dalpha is None else np.asarray(dL_dalpha, np.float64).reshape(H, W)
        names = dict(dmean2D=2, dconic=3, dopacity=1, dcolor=3, dz=1)
        for k, c in names.items():
            out[k] = np.zeros((P, c)); out["S_" + k] = np.zeros((P, c))
    for p in range(pgx * pgy):
        r0, r1 = li["ranges"][p]
        n = int(r1 - r0)
        if n <= 0:
            continue
        g = li["point_list"][r0:r1]
        cm = None if (s == 0 or li["child_mask"] is None) else li["child_mask"][r0:r1]
        X0, Y0 = (p % pgx) * side, (p // pgx) * side
        yy, xx = np.mgrid[Y0:min(Y0 + side, H), X0:min(X0 + side, W)]
        yy, xx = yy.reshape(-1), xx.reshape(-1)
        for c0 in range(0, yy.size, CHUNK):
            _block(out, yy[c0:c0 + CHUNK], xx[c0:c0 + CHUNK], g, cm, policy, xy, co, rgb, zz, bg, W, H,
                   (dp, dpd, dpa) if bwd else None, keep_pairs)
    if bwd:
        for k in ("dopacity", "dz", "S_dopacity", "S_dz"):
            out[k] = out[k][:, 0]
    return out


def _block(out, ys, xs, g, cm, policy, xy, co, rgb, zz, bg, W, H, grads, keep_pairs):
    n = g.size
    idx = np.arange(n)[None, :]
    if cm is None:
        mine = np.ones((ys.size, n), bool)
    else:
        bit = np.array([pixel_bit(policy, int(x), int(y)) for x, y in zip(xs, ys)], np.int64)
        mine = (cm[None, :] & bit[:, None]) != 0
    a, b, c, op = co[g, 0][None, :], co[g, 1][None, :], co[g, 2][None, :], co[g, 3][None, :]
    dx = xy[g, 0][None, :] - xs[:, None]; dy = xy[g, 1][None, :] - ys[:, None]
    t1 = 0.5 * a * dx * dx; t2 = 0.5 * c * dy * dy; t3 = b * dx * dy
    power = -(t1 + t2) - t3
    mag = np.abs(t1) + np.abs(t2) + np.abs(t3)
    G = np.exp(np.minimum(power, 0.0))
    oG = op * G
    take = mine & (oG >= A_MIN)
    alpha = np.where(take, np.minimum(A_MAX, oG), 0.0)
    keep = 1.0 - alpha
    Tb = np.concatenate([np.ones((ys.size, 1)), np.cumprod(keep, axis=1)[:, :-1]], axis=1)          # transmittance in FRONT of each entry (no stop yet)
    test = Tb * keep
    stopm = take & (test < T_MIN)
    has = stopm.any(axis=1)
    kstop = np.where(has, np.argmax(stopm, axis=1), n)                                                # the stopping entry (not applied)
    applied = take & (idx < kstop[:, None])
    visited = mine & (idx <= kstop[:, None])
    al = np.where(applied, alpha, 0.0)
    w = al * Tb
    T_fin = np.prod(1.0 - al, axis=1)
    ncon = np.where(applied, idx + 1, 0).max(axis=1)
    out["final_T"][ys, xs] = T_fin
    out["alpha"][ys, xs] = 1.0 - T_fin
    out["n_contrib"][ys, xs] = ncon
    # the backward's reconstruction final_T / prod(1 - alpha) of the transmittance in front of the list: per applied entry the forward's
    # T - alpha T (one rounding of the product, alpha / (1 - alpha) ulp of the difference, and the difference's own) and the backward's
    # 1 - alpha, v_rcp (one ulp) and product: (4 + alpha / (1 - alpha)) ulp, plus the two ends
    out["front_bound"][ys, xs] = EPS * (np.where(applied, 4.0 + al / (1.0 - al), 0.0).sum(axis=1) + 2.0)
    col = w @ rgb[g]                                                                                  # [Np, 3]
    out["color"][:, ys, xs] = (col + T_fin[:, None] * bg[None, :]).T
    out["depth"][ys, xs] = w @ zz[g]

    # ---- ambiguity and the forward's first-order rounding bounds
    d_pow = 8 * EPS * (mag + 1.0)
    U = np.abs(dx) + 3.5; V = np.abs(dy) + 3.5
    d_pol = d_pow + 8 * EPS * (0.5 * np.abs(a) * U * U + 0.5 * np.abs(c) * V * V + np.abs(b) * U * V + 1.0)
    with np.errstate(divide="ignore"):
        la = np.log(np.maximum(oG, 1e-300) / A_MIN)                                                 # log(oG / the float32 threshold)
        lt = np.log(np.maximum(test, 1e-300) / T_MIN)
    amb_power = visited & (np.abs(power) <= d_pow) & (op >= 0.99 / 255.0) & (mag > 0.0)
    flags = {}
    for mode, d in (("exact", d_pow), ("poly", d_pol)):
        # (an entry clamped at 0.99 beyond the reach of d does not move - helpers.account_outlier_pixels - and adds its product's rounding only)
        d_eff = np.where(oG >= A_MAX * np.exp(d), 0.0, d)
        d_T = np.cumsum(np.where(take, alpha / (1.0 - alpha) * d_eff + EPS, 0.0), axis=1) + EPS
        amb_a = visited & (np.abs(la) <= d)
        amb_s = visited & take & (np.abs(lt) <= d_T)
        flags[mode] = (amb_a, amb_s, d_T)
        if mode == "poly":
            definite = take & (lt < -d_T)
            kdef = np.where(definite.any(axis=1), np.argmax(definite, axis=1), n)
            can = mine & (idx <= kdef[:, None]) & (la >= -d)
            out["loud"][ys, xs] = np.maximum(1.0, np.where(can, np.abs(rgb[g]).max(axis=1)[None, :], 0.0).max(axis=1))
        out["amb_" + mode][ys, xs] = (amb_a | amb_s).any(axis=1)
        # rounding bound: alpha_i moves by alpha_i d_i (not at all once clamped beyond reach of d_i), T in front of entry i by
        # T_i rho_i with rho_i = sum_{j < i} (alpha_j / (1 - alpha_j) d_j + ulp) - the triangle inequality over the blend sum, plus the
        # float32 summation of the k applied terms ((k + 2) ulp sum |terms|) and four roundings per term (weight, product, and the
        # polynomial build's two scalings by 0.99)
        step = np.where(applied, al / (1.0 - al) * d_eff + EPS, 0.0)
        rho = np.concatenate([np.zeros((ys.size, 1)), np.cumsum(step, axis=1)[:, :-1]], axis=1)
        rho_fin = step.sum(axis=1) + EPS
        kk = applied.sum(axis=1) + 2.0
        wr = w * (rho + d_eff + 4 * EPS)
        cabs = np.abs(rgb[g])
        bc = (wr @ cabs).max(axis=1) + T_fin * rho_fin * np.abs(bg).max() + kk * EPS * ((w @ cabs).max(axis=1) + T_fin * np.abs(bg).max())
        bd = wr @ np.abs(zz[g]) + kk * EPS * (w @ np.abs(zz[g]))
        B = out["bound_" + mode]
        B["color"][ys, xs] = bc; B["final_T"][ys, xs] = T_fin * rho_fin + EPS; B["depth"][ys, xs] = bd
    out["amb_oracle"][ys, xs] = (flags["exact"][0] | flags["exact"][1] | amb_power).any(axis=1)
    for kind, m in (("alpha", flags["poly"][0]), ("stop", flags["poly"][1]), ("power", amb_power)):
        for i, j in zip(*np.nonzero(m)):
            out["pairs"].append((int(ys[i]), int(xs[i]), int(j), kind))
    if keep_pairs:
        out["margins"].append(dict(ys=ys, xs=xs, visited=visited, log_alpha=la, d_pow=d_pow, d_pol=d_pol, log_stop=lt, d_T=flags["exact"][2],
                                   d_T_pol=flags["poly"][2], take=take, g=g))
    if grads is None:
        return

    # ---- backward (orc_render_bwd's walk, driven by the decisions above)
    dp, dpd, dpa = grads
    dpx = dp[:, ys, xs]                                                    # [3, Np]
    pd, pa = dpd[ys, xs], dpa[ys, xs]
    cd = dpx[0][:, None] * rgb[g, 0][None, :] + dpx[1][:, None] * rgb[g, 1][None, :] + dpx[2][:, None] * rgb[g, 2][None, :]
    cd = cd + pd[:, None] * zz[g][None, :] + pa[:, None]
    wcd = w * cd
    behind = wcd.sum(axis=1)[:, None] - np.cumsum(wcd, axis=1) + (T_fin * (bg @ dpx))[:, None]      # A_i: everything blended behind entry i
    inv = 1.0 / (1.0 - al)
    dLda = np.where(applied, Tb * cd - behind * inv, 0.0)
    D = np.where(applied, np.abs(Tb * cd) + np.abs(behind * inv), 0.0)
    oGa = np.where(applied, oG, 0.0)
    h, habs = oGa * dLda, oGa * D
    Ga = np.where(applied, G, 0.0)
    adx, ady = np.abs(dx), np.abs(dy)
    a1, b1, c1 = a[0], b[0], c[0]

    def add(name, col, val):
        out[name][g, col] += val

    add("dopacity", 0, (Ga * dLda).sum(axis=0)); add("S_dopacity", 0, (Ga * D).sum(axis=0))
    hx, hy = (h * dx).sum(axis=0), (h * dy).sum(axis=0)
    hxa, hya = (habs * adx).sum(axis=0), (habs * ady).sum(axis=0)
    add("dmean2D", 0, 0.5 * W * (-a1 * hx - b1 * hy)); add("S_dmean2D", 0, 0.5 * W * (np.abs(a1) * hxa + np.abs(b1) * hya))
    add("dmean2D", 1, 0.5 * H * (-c1 * hy - b1 * hx)); add("S_dmean2D", 1, 0.5 * H * (np.abs(c1) * hya + np.abs(b1) * hxa))
    for col, (u, ua) in enumerate(((dx * dx, adx * adx), (dx * dy, adx * ady), (dy * dy, ady * ady))):
        add("dconic", col, -0.5 * (h * u).sum(axis=0)); add("S_dconic", col, 0.5 * (habs * ua).sum(axis=0))
    for ch in range(3):
        add("dcolor", ch, (w * dpx[ch][:, None]).sum(axis=0)); add("S_dcolor", ch, (w * np.abs(dpx[ch])[:, None]).sum(axis=0))
    add("dz", 0, (w * pd[:, None]).sum(axis=0)); add("S_dz", 0, (w * np.abs(pd)[:, None]).sum(axis=0))
