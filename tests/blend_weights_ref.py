"""float64 restatement of gm_blend_weights (include/gmesh_hip.h) on the oracle's lists, and the scenes its tests share.

From oracle.forward_full's `geo` (xy, conic_op) and `bins` (ranges, point_list: the reference's lists per 16-px tile, which every
emission policy walks in the same order) every pixel's list is walked with the rules of the GM_FWD_EXACT_EXPONENT blend:
  oG = opacity * min(1, exp(power)); skipped when oG < 1/255; alpha = min(0.99, oG); w = alpha T; stop WITHOUT applying the entry when
  T - w < 1e-4; T starts at 1.
Besides the sums it returns what the tests' bounds are made of, with exactly the rounding model of helpers.account_outlier_pixels:
  d_pow = 8 ulp (mag + 1)      distance of a float32 evaluation of an entry's exponent (and log alpha) from the exact one
  d_T   = the cumulative distance of log T (alpha / (1 - alpha) d_pow + ulp per accepted entry, + ulp)
so that a float32 weight w = alpha T lies within w (d_pow + d_T) of the float64 one, and the CENSUS of decisions at a threshold: the
pixels with an entry whose `alpha >= 1/255` or `T (1 - alpha) < 1e-4` decision lies within that distance (on such a pixel two correct
float32 walks may part ways; the scenes below have none, which every test asserts first).
"""
import numpy as np

EPS = 2.0 ** -23


def walk(fw, W, H, mask=None, P=None):
    """fw: oracle.forward_full(...).  mask: uint8 [H,W] or None (255 everywhere).  Returns a dict:
    total, inside, peak [P] float64 (inside in weight units: sum w k / 255), n_acc [P] accepted pixels, err [P] = sum over the accepted
    pixels of w (d_pow + d_T), err_max [P] = the largest such term, one_minus_T [H,W], accepted [H,W] entries accepted per pixel,
    stopped [H,W] bool, census = pixels with a decision within its rounding distance."""
    geo, bins = fw["geo"], fw["bins"]
    xy = geo["xy"].astype(np.float64); co = geo["conic_op"].astype(np.float64)
    P = len(xy) if P is None else P
    k = np.full((H, W), 255.0) if mask is None else np.asarray(mask, np.float64).reshape(H, W)
    total, inside, peak, err, err_max = (np.zeros(P) for _ in range(5))
    n_acc = np.zeros(P, np.int64)
    omt = np.zeros((H, W)); accepted = np.zeros((H, W), np.int64); stopped = np.zeros((H, W), bool)
    census = 0
    gx = (W + 15) // 16
    for y in range(H):
        for x in range(W):
            r0, r1 = bins["ranges"][(y // 16) * gx + (x // 16)]
            g = bins["point_list"][r0:r1].astype(np.int64)
            if len(g) == 0:
                continue
            dx = xy[g, 0] - x; dy = xy[g, 1] - y
            t1 = 0.5 * co[g, 0] * dx * dx; t2 = 0.5 * co[g, 2] * dy * dy; t3 = co[g, 1] * dx * dy
            power = np.minimum(-(t1 + t2) - t3, 0.0)
            d_pow = 8 * EPS * (np.abs(t1) + np.abs(t2) + np.abs(t3) + 1.0)
            oG = co[g, 3] * np.exp(power)
            acc = oG >= 1.0 / 255.0
            alpha = np.minimum(0.99, oG)
            keep = np.where(acc, 1.0 - alpha, 1.0)
            T_before = np.concatenate([[1.0], np.cumprod(keep)[:-1]])
            test_T = T_before * (1.0 - alpha)
            stop = acc & (test_T < 1e-4)
            n = int(np.argmax(stop)) if stop.any() else len(g)          # entries [0, n) are walked and applied where accepted
            d_T = np.cumsum(np.where(acc, alpha / (1.0 - alpha) * d_pow + EPS, 0.0)) + EPS
            # census: helpers.account_outlier_pixels' ambiguity tests over the entries a definite walk visits
            definite_stop = acc & (test_T < 1e-4 * np.exp(-d_T))
            n_vis = int(np.argmax(definite_stop)) + 1 if definite_stop.any() else len(g)
            v = slice(0, n_vis)
            amb_alpha = np.abs(np.log(np.maximum(co[g, 3][v] * np.exp(power[v]), 1e-300) * 255.0)) <= d_pow[v]
            amb_stop = acc[v] & (np.abs(np.log(np.maximum(test_T[v], 1e-300) / 1e-4)) <= d_T[v])
            census += int((amb_alpha | amb_stop).any())
            a = acc[:n]
            ids = g[:n][a]
            w = (alpha[:n] * T_before[:n])[a]
            e = w * (d_pow[:n] + d_T[:n])[a]
            np.add.at(total, ids, w); np.add.at(inside, ids, w * (k[y, x] / 255.0)); np.add.at(err, ids, e)
            np.maximum.at(peak, ids, w); np.maximum.at(err_max, ids, e)
            np.add.at(n_acc, ids, 1)
            omt[y, x] = w.sum()
            accepted[y, x] = len(w)
            stopped[y, x] = stop.any()
            T_final = T_before[n - 1] * keep[n - 1] if n else 1.0
            assert abs(w.sum() - (1.0 - T_final)) <= 1e-12, (y, x)      # sum_i w_i = 1 - T_final
    return dict(total=total, inside=inside, peak=peak, n_acc=n_acc, err=err, err_max=err_max, one_minus_T=omt, accepted=accepted,
                stopped=stopped, census=census)


def scene(name):
    """(scene, cam) of the shared test scenes: the smallest that reach every branch.
    s0..s3: 300 Gaussians on 48 x 40 (some behind the camera, partial edge tiles both ways); mid: 2000 on 70 x 50; sat: a saturating one
    (opacity 0.95, large splats: nearly every pixel stops, alpha clamps at 0.99); wide: 72 x 72 - 5 x 5 tiles, so that under policies 2
    and 3 the last parent tile of a row and of a column lacks children."""
    from helpers import small_scene
    if name in ("s0", "s1", "s2", "s3"):
        return small_scene(P=300, W=48, H=40, seed=int(name[1]))
    if name == "mid":
        return small_scene(P=2000, W=70, H=50, seed=5, scale_lo=0.02, scale_hi=0.2)
    if name == "sat":
        sc, cam = small_scene(P=1500, W=48, H=40, seed=7, scale_lo=0.3, scale_hi=0.9)
        sc["opac"][:] = 0.95
        return sc, cam
    if name == "wide":
        return small_scene(P=400, W=72, H=72, seed=11)
    raise KeyError(name)


SCENES = ("s0", "s1", "s2", "s3", "mid", "sat", "wide")
_CACHE = {}


def reference(oracle, name):
    """(scene, cam, oracle forward with background 0, mask uint8 [H,W] of random bytes, walk(...) with that mask), computed once."""
    if name not in _CACHE:
        sc, cam = scene(name)
        W, H = cam["W"], cam["H"]
        fw = oracle.forward_full(sc, cam, np.zeros(3, np.float32), use_precomp_color=True)
        mask = np.random.default_rng(1000 + len(name) + sum(map(ord, name))).integers(0, 256, size=(H, W)).astype(np.uint8)
        _CACHE[name] = (sc, cam, fw, mask, walk(fw, W, H, mask))
    return _CACHE[name]
