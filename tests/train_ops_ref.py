"""The fused training operators of csrc/gm_train.hip restated in numpy: float64 definitions of the mesh-bound and the plain activation
(forward and analytic adjoint), of Adam's rule and of the three densification statements, each with a PER-ELEMENT ERROR SCALE, plus
adam_ref32 - Adam's rule with float32 rounding after every operation, in the order the kernel spells it.  No project code in here.

The formulas are the reference's: scene/mesh_based_gaussian_model.py:122-152, 172-174 (get_xyz / get_scaling / get_rotation /
get_opacity), scene/gaussian_model.py:26-43 (the plain model), utils/loss_utils.py:86-108 (mesh_restrict_loss), jittor/optim.py Adam.step,
train_mesh_gaussian.py:119-126 + mesh_based_gaussian_model.py:587-589 (densification statistics).

ERROR SCALE: for every output element, the sum of the magnitudes of the terms that are ADDED to form it.  A float32 evaluation with K
rounded operations on its longest path is within about K 2^-24 scale of the exact value, whatever cancels; a tolerance that multiplies the
scale is therefore fair to a row with cancellation and does not hide a small row behind a large one.  Where the value goes through an
exponential, `exp` holds the extra term |d value / d x| |x| per unit of RELATIVE argument error: the fast exponential rounds x log2(e)
before it exponentiates, an error that grows with |x| and not with the number of operations (multiply by 2^-23 for that rounding).

Two choices the definition above forces:
  * the normal offset k n_c = alpha r (sigmoid(d) - 0.5) n_c of xyz is formed by adding sigmoid(d) and -0.5, so its share of the scale
    is alpha |r| (sigmoid(d) + 0.5) |n_c| - not |k n_c|, which vanishes at d = 0 where the rounding error of the sigmoid does not;
  * the sigmoid's derivative is formed as s (1 - s), as Jittor and torch do, so its scale is s (1 + s): beyond x ~ 5 a float32
    s (1 - s) is NOT accurate relative to its own value (1 - s carries half an ulp of 1), and beyond x ~ 16.64 it is exactly 0.  The
    tests pin that region by exact statements instead."""
import numpy as np

f32, f64 = np.float32, np.float64
EPS_NORMALIZE = 1e-12                     # jt.normalize / F.normalize: x / maximum(|x|, eps)
TINY32 = 1.1754944e-38                    # float32's smallest normal


def _sigmoid(x):
    x = np.asarray(x, f64)
    with np.errstate(over="ignore"):
        return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))


def _d(x):
    return np.asarray(x, f64)


# ------------------------------------------------------------------------------------------------------------ shared pieces
def _normalize(q):
    nrm = np.sqrt((q * q).sum(axis=1, keepdims=True))
    den = np.maximum(nrm, EPS_NORMALIZE)
    return q / den, nrm, den


def _normalize_adjoint(q, g):
    """(d_q, scale) of y = q / max(|q|, eps): |q| > eps: (g - y (y.g)) / |q|; the clamp active (|q| <= eps): g / eps - the maximum passes
    no gradient to |q| there."""
    y, nrm, den = _normalize(q)
    yg = (y * g).sum(axis=1, keepdims=True)
    live = nrm > EPS_NORMALIZE
    d_q = np.where(live, (g - y * yg) / den, g / den)
    scale = np.where(live, (np.abs(g) + np.abs(y) * np.abs(yg)) / den, np.abs(g) / den)
    return d_q, scale


def face_radius(v1, v2, v3):
    """(R, cond): sqrt(|AB x AC|) (circumradius(), utils/loss_utils.py:86-100) and the conditioning of the cross product, |c|_abs / |c|
    with c_abs built from the magnitudes of the two products of every component (1 where nothing cancels, and for a degenerate face)."""
    v1, v2, v3 = _d(v1), _d(v2), _d(v3)
    a, b = v2 - v1, v3 - v1
    c = np.cross(a, b)
    ca = np.stack([np.abs(a[:, 1] * b[:, 2]) + np.abs(a[:, 2] * b[:, 1]), np.abs(a[:, 2] * b[:, 0]) + np.abs(a[:, 0] * b[:, 2]),
                   np.abs(a[:, 0] * b[:, 1]) + np.abs(a[:, 1] * b[:, 0])], axis=1)
    n, na = np.sqrt((c * c).sum(axis=1)), np.sqrt((ca * ca).sum(axis=1))
    return np.sqrt(n), np.where(n > 0, na / np.where(n > 0, n, 1.0), 1.0)


# ------------------------------------------------------------------------------------------------------------ mesh-bound activation
def mesh_activate_ref(bc, dist, scaling, rot, opac, v1, v2, v3, normal, r, alpha=4.0, mr_weight=None):
    """Forward in float64 of the float32 inputs.  Returns a dict:
      out[k], scale[k], exp[k] for k in xyz [N,3], scales [N,3], rots [N,4], opac [N,1] and, with mr_weight, mr (scalar);
      w [N,3] (softmax), sd [N,1], k [N,1], R [N], term [N] (the signed smax - w R before the hinge), margin [N] = |term| / (smax + w R).
    mr_weight is rounded to float32 first, as the C ABI takes it."""
    bc, dist, scaling, rot, opac, v1, v2, v3, normal, r = (_d(x) for x in (bc, dist, scaling, rot, opac, v1, v2, v3, normal, r))
    N = bc.shape[0]
    dist, opac, r = dist.reshape(N, 1), opac.reshape(N, 1), r.reshape(N, 1)
    x = bc - bc.max(axis=1, keepdims=True)
    e = np.exp(x)
    w = e / e.sum(axis=1, keepdims=True)
    sd = _sigmoid(dist)
    k = alpha * r * (sd - 0.5)
    V = np.stack([v1, v2, v3], axis=1)                                             # [N, vertex, component]
    xyz = (w[:, :, None] * V).sum(axis=1) + k * normal
    out, scale, ex = {}, {}, {}
    out["xyz"] = xyz
    scale["xyz"] = (w[:, :, None] * np.abs(V)).sum(axis=1) + alpha * np.abs(r) * (sd + 0.5) * np.abs(normal)
    # d w_i / d(relative argument error) = w_i (|x_i| + sum_j w_j |x_j|); the offset goes through sigmoid(d): ds = s (1 - s) |d|.
    # The softmax's argument b_i - max b is itself a rounded difference (2^-24 |x| more, on top of the 2^-23 |x| of x log2(e)): its share
    # is entered 1.5-fold, so that ONE factor 2^-23 serves every `exp` entry.
    ew = 1.5 * w * (np.abs(x) + (w * np.abs(x)).sum(axis=1, keepdims=True))
    ex["xyz"] = (ew[:, :, None] * np.abs(V)).sum(axis=1) + alpha * np.abs(r) * sd * (1 - sd) * np.abs(dist) * np.abs(normal)
    out["scales"] = np.exp(scaling); scale["scales"] = out["scales"]; ex["scales"] = np.abs(scaling) * out["scales"]
    y, nrm, den = _normalize(rot)
    out["rots"] = y; scale["rots"] = np.abs(y); ex["rots"] = np.zeros_like(y)
    so = _sigmoid(opac)
    out["opac"] = so; scale["opac"] = so; ex["opac"] = np.abs(opac) * so * (1 - so)
    res = dict(out=out, scale=scale, exp=ex, w=w, sd=sd, k=k, so=so)
    if mr_weight is not None:
        wt = float(f32(mr_weight))
        R, cond = face_radius(v1, v2, v3)
        smax = out["scales"].max(axis=1)
        term = smax - wt * R
        live = term > 0
        mag = smax + abs(wt) * R * cond
        margin = np.abs(term) / np.maximum(smax + abs(wt) * R, 1e-300)
        out["mr"] = np.maximum(term, 0.0).sum()
        # rows within float32 rounding of the hinge may land on either side: their magnitudes belong to the scale too
        near = live | (margin < 2.0 ** -18)
        scale["mr"] = (mag * near).sum()
        ex["mr"] = (np.abs(scaling[np.arange(N), out["scales"].argmax(axis=1)]) * smax * near).sum()
        res.update(R=R, cond=cond, term=term, margin=margin, axis=out["scales"].argmax(axis=1), wt=wt)     # argmax: the FIRST largest
    return res


def mesh_activate_adjoint(bc, dist, scaling, rot, opac, v1, v2, v3, normal, r, g_xyz, g_scales, g_rots, g_opac, alpha=4.0, mr_weight=None,
                          g_mr=None):
    """The analytic adjoint in float64.  A missing upstream gradient (None) is a zero gradient.  Returns (grad, scale): dicts over bc,
    dist, scaling, rot, opac.  The mesh-restrict term sum max(0, max_c exp(s_c) - w sqrt(|AB x AC|)) sends g_mr to the FIRST largest axis
    of a row whose term is positive, as the kernel documents."""
    fw = mesh_activate_ref(bc, dist, scaling, rot, opac, v1, v2, v3, normal, r, alpha, mr_weight)
    bc, dist, scaling, rot, opac, v1, v2, v3, normal, r = (_d(x) for x in (bc, dist, scaling, rot, opac, v1, v2, v3, normal, r))
    N = bc.shape[0]
    shp_d, shp_o = dist.shape, opac.shape
    dist, opac, r = dist.reshape(N, 1), opac.reshape(N, 1), r.reshape(N, 1)
    z = lambda g, s: np.zeros(s) if g is None else _d(g).reshape(s)
    gx, gs, gr, go = z(g_xyz, (N, 3)), z(g_scales, (N, 3)), z(g_rots, (N, 4)), z(g_opac, (N, 1))
    w, sd, so = fw["w"], fw["sd"], fw["so"]
    V = np.stack([v1, v2, v3], axis=1)
    dw = (gx[:, None, :] * V).sum(axis=2)                                          # [N, vertex]
    dwa = (np.abs(gx[:, None, :] * V)).sum(axis=2)
    grad, scale = {}, {}
    grad["bc"] = w * (dw - (w * dw).sum(axis=1, keepdims=True))
    scale["bc"] = w * (dwa + (w * dwa).sum(axis=1, keepdims=True))
    gn = (gx * normal).sum(axis=1, keepdims=True)
    gna = np.abs(gx * normal).sum(axis=1, keepdims=True)
    grad["dist"] = (gn * alpha * r * sd * (1 - sd)).reshape(shp_d)
    scale["dist"] = (gna * alpha * np.abs(r) * sd * (1 + sd)).reshape(shp_d)
    sc = fw["out"]["scales"]
    hot = np.zeros((N, 3))
    if mr_weight is not None and g_mr is not None:
        hot[np.arange(N), fw["axis"]] = (fw["term"] > 0) * float(g_mr)
    grad["scaling"] = (gs + hot) * sc
    scale["scaling"] = (np.abs(gs) + np.abs(hot)) * sc
    grad["rot"], scale["rot"] = _normalize_adjoint(rot, gr)
    grad["opac"] = (go * so * (1 - so)).reshape(shp_o)
    scale["opac"] = (np.abs(go) * so * (1 + so)).reshape(shp_o)
    return grad, scale


# ------------------------------------------------------------------------------------------------------------ plain activation
def plain_activate_ref(xyz, scaling, rot, opac):
    """(out, scale, exp) dicts over xyz, scales, rots, opac: the plain model's map (scene/gaussian_model.py:26-43), xyz passing through."""
    xyz, scaling, rot, opac = (_d(x) for x in (xyz, scaling, rot, opac))
    so = _sigmoid(opac)
    y = _normalize(rot)[0]
    out = dict(xyz=xyz, scales=np.exp(scaling), rots=y, opac=so)
    scale = dict(xyz=np.abs(xyz), scales=out["scales"], rots=np.abs(y), opac=so)
    ex = dict(xyz=np.zeros_like(xyz), scales=np.abs(scaling) * out["scales"], rots=np.zeros_like(y), opac=np.abs(opac) * so * (1 - so))
    return out, scale, ex


def plain_activate_adjoint(xyz, scaling, rot, opac, g_xyz, g_scales, g_rots, g_opac):
    xyz, scaling, rot, opac = (_d(x) for x in (xyz, scaling, rot, opac))
    z = lambda g, like: np.zeros_like(like) if g is None else _d(g).reshape(like.shape)
    gx, gs, gr, go = z(g_xyz, xyz), z(g_scales, scaling), z(g_rots, rot), z(g_opac, opac)
    so = _sigmoid(opac)
    grad, scale = dict(xyz=gx), dict(xyz=np.abs(gx))
    grad["scaling"] = gs * np.exp(scaling); scale["scaling"] = np.abs(grad["scaling"])
    grad["rot"], scale["rot"] = _normalize_adjoint(rot, gr)
    grad["opac"] = go * so * (1 - so); scale["opac"] = np.abs(go) * so * (1 + so)
    return grad, scale


# ------------------------------------------------------------------------------------------------------------ Adam
def _rates(n, lr, lr_rest, period, split):
    """the learning rate of every element: period == 0: lr; else lr where (index % period) < split, lr_rest elsewhere"""
    idx = np.arange(n, dtype=np.int64)
    if not period:
        return np.full(n, float(lr)), idx
    return np.where(idx % period < split, float(lr), float(lr if lr_rest is None else lr_rest)), idx


def _live(n, period, active):
    """elements the step touches: all, or - 0 < active < period - those below the rounded-up granule 4 ceil(active / 4) of their period"""
    if not (period and active and active < period):
        return np.ones(n, bool)
    return (np.arange(n, dtype=np.int64) % period) < 4 * ((active + 3) // 4)


def adam_ref64(p, m, v, g, t, lr, b1=0.9, b2=0.999, eps=1e-8, lr_rest=None, period=0, split=0, active=0):
    """jittor.nn.Adam's rule in float64: m' = b1 m + (1-b1) g; v' = b2 v + (1-b2) g^2; p' = p - lr sqrt(1-b2^t)/(1-b1^t) m'/(sqrt(v')+eps).
    Returns (p', m', v', step) flat float64; untouched elements (see _live) keep their values, step 0."""
    p, m, v, g = (_d(x).reshape(-1) for x in (p, m, v, g))
    rate, _ = _rates(p.size, lr, lr_rest, period, split)
    live = _live(p.size, period, active)
    with np.errstate(all="ignore"):
        m1 = b1 * m + (1 - b1) * g
        v1 = b2 * v + (1 - b2) * g * g
        step = rate * (np.sqrt(1 - b2 ** t) / (1 - b1 ** t)) * m1 / (np.sqrt(v1) + eps)
    return np.where(live, p - step, p), np.where(live, m1, m), np.where(live, v1, v), np.where(live, step, 0.0)


def adam_param_from_moments(p, m1, v1, t, lr, b1=0.9, b2=0.999, eps=1e-8, lr_rest=None, period=0, split=0):
    """(p', step): the parameter line alone, in float64, from given (float32) new moments"""
    p, m1, v1 = (_d(x).reshape(-1) for x in (p, m1, v1))
    rate, _ = _rates(p.size, lr, lr_rest, period, split)
    with np.errstate(all="ignore"):
        step = rate * (np.sqrt(1 - b2 ** t) / (1 - b1 ** t)) * m1 / (np.sqrt(v1) + eps)
    return p - step, step


def _fma32(a, b, c):
    """fma(a, b, c) on float32 arrays: the product of two float32 is exact in float64; the sum is rounded to float64 and then to float32 -
    one rounding for all practical purposes (the double rounding differs from a true fma on a 2^-29 share of inputs, by one ulp)"""
    with np.errstate(all="ignore"):
        return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def adam_ref32(p, m, v, g, t, lr, b1=0.9, b2=0.999, eps=1e-8, lr_rest=None, period=0, split=0, active=0):
    """The same rule with float32 rounding after every operation, in the order adam_update (csrc/gm_common.h) spells it:
        m' = fma(b1, m, c1 g);  v' = fma(b2, v, (c2 g) g);  p' = p - st m' / (sqrt(v') + eps)
    c1 = float32(1 - b1), c2 = float32(1 - b2) and st = float32(lr sqrt(1 - b2^t) / (1 - b1^t)) formed in double.  Elements at or past the
    rounded-up granule 4 ceil(active / 4) of their period are returned unchanged.  Returns (p', m', v') flat float32."""
    p, m, v, g = (np.asarray(x, f32).reshape(-1) for x in (p, m, v, g))
    fb1, fb2, feps = f32(b1), f32(b2), f32(eps)
    c1, c2 = f32(1.0 - float(b1)), f32(1.0 - float(b2))
    corr = np.sqrt(1.0 - float(b2) ** t) / (1.0 - float(b1) ** t)
    rate, _ = _rates(p.size, f64(f32(lr)), None if lr_rest is None else f64(f32(lr_rest)), period, split)       # the ABI takes float rates
    st = (rate * corr).astype(f32)
    live = _live(p.size, period, active)
    with np.errstate(all="ignore"):
        m1 = _fma32(np.full_like(m, fb1), m, c1 * g)
        v1 = _fma32(np.full_like(v, fb2), v, (c2 * g) * g)
        p1 = p - (st * m1) / (np.sqrt(v1) + feps)
    assert m1.dtype == f32 and v1.dtype == f32 and p1.dtype == f32
    return np.where(live, p1, p), np.where(live, m1, m), np.where(live, v1, v)


def ulp32(x):
    """the spacing of float32 at |x| (float64 array), never below the subnormal spacing"""
    x = np.abs(np.asarray(x, f64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.maximum(x, 2.0 ** -126)))
    return 2.0 ** (np.maximum(e, -126) - 23)


# ------------------------------------------------------------------------------------------------------------ densification statistics
def densify_stats_ref(radii, grad, max_radii2D, grad_accum, denom):
    """The three statements over the visible rows (radii > 0), accumulators float32 in / out:
        max_radii2D[vis] = max(max_radii2D[vis], radii[vis].float())        float32, exact
        denom[vis] += 1                                                      float32
        grad_accum[vis] += |grad[vis, :2]|                                   (a) float64: acc + hypot(gx, gy)   (b) float32 statements
    Returns dict(vis, max_radii2D f32, denom f32, accum64 f64, accum32 f32, safe bool [N]); `safe` marks rows whose gx^2 + gy^2 neither
    overflows nor loses bits to underflow in float32 - elsewhere the reference's own float32 norm overflows / underflows and (b) is
    the statement to compare with."""
    radii = np.asarray(radii).reshape(-1)
    g = np.asarray(grad, f32)
    mr, acc, den = (np.asarray(x, f32).reshape(-1).copy() for x in (max_radii2D, grad_accum, denom))
    vis = radii > 0
    rf = radii.astype(f32)                                                  # rounds above 2^24 as radii.float() does
    mr[vis] = np.maximum(mr[vis], rf[vis])
    den[vis] = den[vis] + f32(1.0)
    gx, gy = g[:, 0], g[:, 1]
    acc64 = acc.astype(f64)
    acc64[vis] = acc64[vis] + np.hypot(gx[vis].astype(f64), gy[vis].astype(f64))
    with np.errstate(all="ignore"):
        s32 = gx * gx + gy * gy
        acc32 = acc.copy()
        acc32[vis] = acc32[vis] + np.sqrt(s32)[vis]
    big = np.maximum(np.abs(gx.astype(f64)), np.abs(gy.astype(f64)))
    # big^2 must stay a NORMAL float32 with all its bits (>= 2^-126 2^24 keeps the smaller square's bits relevant) and below the maximum
    safe = (big == 0) | ((big * big >= 2.0 ** -100) & (2 * big * big < 3.0e38))
    return dict(vis=vis, max_radii2D=mr, denom=den, accum64=acc64, accum32=acc32, safe=safe)


# ------------------------------------------------------------------------------------------------------------ the input classes of the tests
MR_WEIGHT = 0.7                           # the mesh-restrict weight the hinge rows below are built for
HINGE_DELTA = 2.0 ** -20                  # a hinge row's term is +-8 float32 ulp of its largest scale (see mesh_edge_inputs)

_DIST = ("benign", "0", "1e-3", "10", "16.6..16.7", "20", "100")
_BC = ("benign", "spread100", "two-equal", "three-equal", "spread10")
_SC = ("benign", "uniform[-12,4]", "two-axes-same-bits", "three-axes-same-bits")
_ROT = ("benign", "benign", "norm1e-7", "norm1e-11", "norm5e-13", "norm1e-14", "zero", "norm1e3", "benign")
_FACE = ("degenerate", "hinge+", "hinge-") + ("random",) * 8


def opacity_pool():
    """the dense opacity grid: [-104, 30] in steps of 0.1, and 2001 points in [16, 18]"""
    return np.concatenate([np.linspace(-104.0, 30.0, 1341), np.linspace(16.0, 18.0, 2001)])


def mesh_edge_inputs(N, seed=0, shift=0):
    """float32 inputs of mesh_activate built from named classes of rows.  Row i belongs to one class per input, chosen by (i + shift)
    modulo pairwise coprime periods (5, 7, 4, 9, 11, 13, 3), so that consecutive rows - one wave - hold a mix and every combination
    turns up.  Returns (dict of arrays, list of N class labels).  Hinge rows are built for mr_weight = MR_WEIGHT:
    v1 = 0, v2 = (a, 0, 0), v3 = (0, b, 0), so R = sqrt(a b) without cancellation, |scaling| <= 1, and a chosen so that
    max_c exp(s_c) - w R = +-HINGE_DELTA max_c exp(s_c): 8 ulp, twice what the kernel's roundings can move it by
    ((|s| + 2) 2^-24 on the exponential, 4 2^-24 on w R: at most 7 2^-24 = 3.5 ulp together)."""
    rng = np.random.default_rng(seed)
    j = np.arange(N, dtype=np.int64) + shift
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)
    # barycentric logits
    cb = j % 5
    bc = rng.standard_normal((N, 3)) * 2
    bc = np.where((cb == 1)[:, None], rng.uniform(-100, 100, (N, 3)), bc)
    bc = np.where((cb == 4)[:, None], rng.uniform(-10, 10, (N, 3)), bc)
    pair = (j // 5) % 3
    two = bc.copy(); two[np.arange(N), pair] = two[np.arange(N), (pair + 1) % 3]
    bc = np.where((cb == 2)[:, None], two, bc)
    bc = np.where((cb == 3)[:, None], bc[:, :1], bc)
    # distance
    cd = j % 7
    sign = np.where((j // 7) % 2 == 0, 1.0, -1.0)
    dist = rng.standard_normal(N)
    for c, val in ((1, 0.0), (2, 1e-3), (3, 10.0), (5, 20.0), (6, 100.0)):
        dist = np.where(cd == c, sign * val, dist)
    dist = np.where(cd == 4, sign * rng.uniform(16.6, 16.7, N), dist)
    # scaling
    cs = j % 4
    scaling = rng.standard_normal((N, 3)) - 2
    uni = rng.uniform(-12, 4, (N, 3))
    scaling = np.where((cs >= 1)[:, None], uni, scaling)
    pair = (j // 4) % 3
    two = scaling.copy(); two[np.arange(N), pair] = two[np.arange(N), (pair + 1) % 3]
    scaling = np.where((cs == 2)[:, None], two, scaling)
    scaling = np.where((cs == 3)[:, None], scaling[:, :1], scaling)
    # rotation
    cr = j % 9
    rot = rng.standard_normal((N, 4))
    d = unit(rng.standard_normal((N, 4)))
    for c, nrm in ((2, 1e-7), (3, 1e-11), (4, 5e-13), (5, 1e-14), (6, 0.0), (7, 1e3)):
        rot = np.where((cr == c)[:, None], d * nrm, rot)
    # opacity: two rows of three from the dense grid, the third benign
    pool = opacity_pool()
    pool = pool[np.random.default_rng(12345).permutation(len(pool))]
    opac = np.where(j % 3 == 0, rng.standard_normal(N) * 2, pool[(j - j // 3) % len(pool)])
    # faces
    cf = j % 11
    v1, v2, v3 = (rng.standard_normal((N, 3)) for _ in range(3))
    deg = (cf == 0)[:, None]
    v2, v3 = np.where(deg, v1, v2), np.where(deg, v1, v3)
    hinge = (cf == 1) | (cf == 2)
    scaling = np.where(hinge[:, None], scaling / 12.0, scaling).astype(f32)                       # |s| <= 1, ties kept
    smax = np.exp(scaling.astype(f64).max(axis=1))
    wt = float(f32(MR_WEIGHT))
    b = rng.uniform(0.5, 2.0, N).astype(f32).astype(f64)
    a = ((smax * (1.0 - np.where(cf == 1, HINGE_DELTA, -HINGE_DELTA)) / wt) ** 2 / b)
    zero = np.zeros(N)
    h = hinge[:, None]
    v1 = np.where(h, 0.0, v1); v2 = np.where(h, np.stack([a, zero, zero], 1), v2); v3 = np.where(h, np.stack([zero, b, zero], 1), v3)
    normal = unit(rng.standard_normal((N, 3)))
    r = np.where(j % 13 == 5, 0.0, rng.random(N) + 0.1)
    ins = dict(bc=bc, dist=dist.reshape(N, 1), scaling=scaling, rot=rot, opac=opac.reshape(N, 1), v1=v1, v2=v2, v3=v3, normal=normal,
               r=r.reshape(N, 1))
    ins = {k: np.ascontiguousarray(v, f32) for k, v in ins.items()}
    labels = ["bc=%s|dist=%s%s|sc=%s|q=%s|opac=%s|face=%s|r=%s" % (_BC[cb[i]], "-" if sign[i] < 0 and cd[i] else "", _DIST[cd[i]], _SC[cs[i]],
                                                                    _ROT[cr[i]], "benign" if j[i] % 3 == 0 else "grid", _FACE[cf[i]],
                                                                    "0" if j[i] % 13 == 5 else "pos") for i in range(N)]
    return ins, labels


def upstream(N, seed, which=(True, True, True, True)):
    """N(0,1) upstream gradients for (xyz, scales, rots, opac), float32; None where `which` is False"""
    rng = np.random.default_rng(seed + 977)
    gs = [rng.standard_normal((N, k)).astype(f32) for k in (3, 3, 4, 1)]
    return [g if w else None for g, w in zip(gs, which)]


def report(name, got, want, bound, labels, scale=None, cols=1):
    """'' if |got - want| <= bound everywhere, else the worst offenders: input class, element index, got, want, scale, bound"""
    got, want, bound = np.asarray(got, f64), np.asarray(want, f64), np.asarray(bound, f64)
    err = np.abs(got - want)
    bad = ~(err <= bound)                                                          # (a NaN is bad)
    if not bad.any():
        return ""
    flat = np.flatnonzero(bad.reshape(-1))
    order = flat[np.argsort(-(err.reshape(-1)[flat] / np.maximum(bound.reshape(-1)[flat], 1e-300)))][:8]
    sc = None if scale is None else np.broadcast_to(np.asarray(scale, f64), got.shape).reshape(-1)
    lines = ["%s: %d of %d elements outside the bound" % (name, int(bad.sum()), bad.size)]
    for e in order:
        row = int(e) // cols
        lines.append("  element %d (row %d, col %d) class [%s]: got %.9g want %.9g err %.3g bound %.3g scale %s" % (
            e, row, int(e) % cols, labels[row] if labels is not None else "-", got.reshape(-1)[e], want.reshape(-1)[e], err.reshape(-1)[e],
            bound.reshape(-1)[e], "-" if sc is None else "%.9g" % sc[e]))
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------------------ the gates (host and GPU tests share them)
U = 2.0 ** -24                            # half an ulp: the relative error of one correctly rounded float32 operation
FWD_FIGURE = 2e-6                         # the project's forward figure (test_mesh_activate_forward_and_backward), here per element
BWD_FIGURE = 1e-5                         # the project's backward figure, here times the per-element scale
BAND = (16.6, 16.7)                       # where float32 1 + exp(-x) stops seeing exp(-x): below, s (1 - s) > 0; above, exactly 0
BAND_FIGURE = 1.2e-7                      # the project's figure for s (1 - s) where s is within an ulp of 1 (test_plain_activate_...)

# K: rounded operations on the longest path to an output of mesh_activate_fwd_kernel, each worth U of the scale (the instruction behind
# __expf is good to 1 ulp = 2 U; 1.0f / x and sqrtf are correctly rounded: 1 U; a contracted multiply-add only removes a rounding).
#   scales = __expf(s)                                  : the exponential 2                                                          =  2
#   opac   = 1 / (1 + __expf(-x))                       : exponential 2, sum 1, division 1                                           =  4
#   rots   = q * (1 / max(sqrt(sum q^2), eps))          : 4 products + 3 sums of positive terms <= 4 on the sum, halved by the root
#                                                         2, root 1, division 1, product 1                                          =  5
#   xyz    = (w0 v1 + w1 v2 + w2 v3) + k n              : e_i 2; S = (e0 + e1) + e2: 2 + 2 sums 4; 1 / S 5; w_i = e_i inv: 2 + 5 + 1 = 8;
#                                                         product 9, two sums 11, the sum with k n 12.  The other path, k n with
#                                                         k = (alpha r)(sigmoid(d) - 0.5): sigmoid 4, difference 5, alpha r 1, product 7,
#                                                         times n 8, final sum 9, is shorter                                         = 12
#   (the argument roundings of the exponentials are not in K: they grow with |x| and sit in the `exp` term, times 2^-23)
K_FWD = dict(scales=2, opac=4, rots=5, xyz=12)
# mr: per row, smax carries 2 (+ its `exp` term); w R: the edge differences 1 each and the product 1 and the difference of products 1 give
# 4 on a cross-product component RELATIVE TO THE MAGNITUDES OF ITS PRODUCTS (hence `cond` in the scale), squares and their sums 3 more,
# two roots quarter that and add 1.5, times w 1: below 6; the difference smax - w R 1: 7 per row at most.  The reduction: 6 levels of the
# shuffle tree, 2 for the four wave partials, then part.sum() over nb = ceil(N / 256) partials in an order torch does not promise: nb - 1.
# K = 15 + nb - 1, and never above the project's figure for this output, 1e-5 (test_mesh_restrict_term_fused_into_the_activation).
def k_mr(N):
    return min(15 + (N + 255) // 256 - 1, 1e-5 / U)


def forward_bounds(fw, N):
    """per-element bound of every forward output: K U scale + 2^-23 exp, never above FWD_FIGURE max(1, |ref|) (mr: see k_mr), plus
    float32's smallest normal for outputs whose exact value underflows float32 (sigmoid(-104) = 7e-46 is stored as 0)."""
    b = {}
    for k, K in K_FWD.items():
        derived = K * U * fw["scale"][k] + 2.0 ** -23 * fw["exp"][k]
        b[k] = np.minimum(derived, FWD_FIGURE * np.maximum(1.0, np.abs(fw["out"][k]))) + TINY32
    if "mr" in fw["out"]:
        b["mr"] = k_mr(N) * U * fw["scale"]["mr"] + 2.0 ** -23 * fw["exp"]["mr"] + TINY32
    return b


def check_mesh_forward(got, fw, labels, N):
    """got: dict xyz / scales / rots / opac (/ mr) of float32 arrays.  Returns the text of all failures ('' = pass)."""
    b = forward_bounds(fw, N)
    msgs = [report("forward " + k, got[k], fw["out"][k], b[k], labels, fw["scale"][k], cols=np.asarray(got[k]).shape[1]) for k in K_FWD]
    if "mr" in got:
        err = abs(float(got["mr"]) - fw["out"]["mr"])
        if not err <= b["mr"]:
            msgs.append("forward mr: got %.9g want %.9g err %.3g bound %.3g scale %.9g (K = %g)" % (float(got["mr"]), fw["out"]["mr"], err,
                                                                                                  b["mr"], fw["scale"]["mr"], k_mr(N)))
    # the zero quaternion gives a forward of exactly 0
    zero = ~np.asarray(fw["scale"]["rots"]).any(axis=1) & (np.asarray(fw["out"]["rots"]) == 0).all(axis=1)
    if zero.any() and np.asarray(got["rots"])[zero].any():
        msgs.append("forward rots: a zero quaternion did not give exact zeros (rows %s)" % np.flatnonzero(zero)[:8])
    return "\n".join(m for m in msgs if m)


def check_mesh_backward(got, ins, ups, labels, alpha=4.0, mr_weight=None, g_mr=None, hinge_exempt=None):
    """got: dict bc / dist / scaling / rot / opac of float32 arrays; ups: the four upstream gradients (None = missing).
    Every element within BWD_FIGURE scale + TINY32 of the float64 adjoint, except the derived exact statements:
      * x >= 16.7 (dist, opac): the sigmoid factor s (1 - s) is exactly 0 - once exp(-x) < 2^-24, 1 + exp(-x) rounds to 1 in float32;
        exp(-16.7) = 5.59e-8 against 2^-24 = 5.96e-8, a 6 % margin over any fast-exp error;
      * BAND[0] < x < BAND[1]: exactly 0 or at most BAND_FIGURE |upstream factor|;
      * a missing upstream gradient: exact zeros;  * the zero quaternion: d_rotation = g 1e12 (inside the ordinary bound).
    hinge_exempt: rows (bool) whose mesh-restrict term is within rounding of the hinge WITHOUT having been built there: either side of
    the subgradient is accepted for them (the caller bounds their number)."""
    grad, scale = mesh_activate_adjoint(ins["bc"], ins["dist"], ins["scaling"], ins["rot"], ins["opac"], ins["v1"], ins["v2"], ins["v3"],
                                        ins["normal"], ins["r"], *ups, alpha=alpha, mr_weight=mr_weight, g_mr=g_mr)
    N = ins["bc"].shape[0]
    msgs = []
    for k in ("bc", "dist", "scaling", "rot", "opac"):
        g, want, sc = np.asarray(got[k], f64).reshape(grad[k].shape), grad[k], scale[k]
        bound = BWD_FIGURE * sc + TINY32
        if k in ("dist", "opac"):
            x = np.asarray(ins[k], f64).reshape(want.shape)
            if k == "dist":
                factor = np.zeros((N, 1)) if ups[0] is None else np.abs((np.asarray(ups[0], f64) * np.asarray(ins["normal"], f64)).sum(
                    axis=1, keepdims=True) * alpha * np.asarray(ins["r"], f64).reshape(N, 1))
            else:
                factor = np.zeros((N, 1)) if ups[3] is None else np.abs(np.asarray(ups[3], f64).reshape(N, 1))
            factor = factor.reshape(want.shape)
            hi, band = x >= BAND[1], (x > BAND[0]) & (x < BAND[1])
            want = np.where(hi | band, 0.0, want)
            bound = np.where(hi, 0.0, np.where(band, BAND_FIGURE * factor, bound))
        if k == "scaling" and hinge_exempt is not None and hinge_exempt.any():
            other, _ = mesh_activate_adjoint(ins["bc"], ins["dist"], ins["scaling"], ins["rot"], ins["opac"], ins["v1"], ins["v2"], ins["v3"],
                                             ins["normal"], ins["r"], *ups, alpha=alpha, mr_weight=None)
            closer = np.abs(g - other["scaling"]) < np.abs(g - want)
            want = np.where(hinge_exempt[:, None] & closer, other["scaling"], want)
        msgs.append(report("backward d_" + k, g, want, bound, labels, sc, cols=want.shape[1] if want.ndim > 1 else 1))
    miss = dict(bc=ups[0] is None, dist=ups[0] is None, scaling=ups[1] is None and g_mr is None, rot=ups[2] is None, opac=ups[3] is None)
    for k, m in miss.items():
        if m and np.asarray(got[k]).any():
            msgs.append("backward d_%s: a missing upstream gradient did not give exact zeros" % k)
    return "\n".join(m for m in msgs if m)
