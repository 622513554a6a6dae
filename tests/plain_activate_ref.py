"""The plain model's activation and its adjoint (csrc/gm_train.hip: plain_activate_fwd_kernel / _bwd_kernel), in numpy, per element.

    forward(xyz, scaling, rot, opac, dtype)                                   -> {"xyz", "scales", "rots", "opac"}
    backward(scaling, rot, opac, g_xyz, g_scales, g_rots, g_opac, dtype, ...) -> {"d_xyz", "d_scaling", "d_rotation", "d_opacity"}
    abs_sums(...)                                                             -> S_abs of all eight tensors, float64

The definition is the kernel's header comment on float32 inputs: xyz copied, exp(scaling), q / max(|q|, eps), 1 / (1 + exp(-x)); the rotation's
adjoint (g - y (y.g)) / |q| where the FLOAT32 |q| exceeds eps and g / eps where not; the opacity's g (1 - s) s; a missing upstream gradient is zero.
eps is the float32 literal 1e-12f (an exact operand of the kernel, as of F.normalize on float32), also in the float64 chain.  dtype=float64 is the
reference; dtype=float32 restates the kernel line by line with one rounding per operation (sum of squares left to right, one reciprocal of
max(|q|, eps) that y and the adjoint are multiplied with, (g (1 - s)) s) - what a correct float32 evaluator reaches.

S_abs of an element is the sum of the absolute values of the terms of its formula: a forward element's magnitude; |g| for d_xyz; |g| exp(s) for
d_scaling; (|g_c| + |y_c| sum_k |y_k g_k|) / |q| for d_rotation_c (|g_c| / eps under the clamp); |g| s (1 + s) for d_opacity (g s - g s s).
ratio = |got - ref64| / (2^-24 S_abs); R_F32 holds what the float32 restatement reaches (test_plain_activate_ref_host.py measures it).

The gate of the device tests (check()):   ratio <= 2 max(r_f32, 2)   for every element of every tensor.
  The floor of 2 units: the device's expf and divisions may err one ulp more than numpy's correctly rounded ones (1 ulp is the math library's
  documented bound for expf); the factor 2 is the project's margin over the float32 restatement.  The gate is purely relative - it has no
  term for underflow - so every gated reference value of the cases below is zero or a normal float32 (asserted on the CPU).
  d_opacity at x > 17, where the float32 s is within an ulp of 1 and g (1 - s) s is a multiple of 2^-24 g, keeps the project's convention
  |got| <= 1.2e-7 |g| (the kernel's comment: the reference's optimizer never sees the ~1e-13 gradients an exact e / (1 + e)^2 would give);
  from x >= 18 on the element must be exactly 0 (a rule of this module, beyond the band): exp(-18) = 1.52e-8 is below 2^-25 = 2.98e-8, also
  when an expf returns it an ulp off; 1 + e rounds to 1 in float32 for every e <= 2^-24, so s is 1, 1 - s is 0 and so is the product.

Upstream gradients and outputs are rows [row0, row0 + N) of buffers of `capacity` rows: backward(..., row0=r) reads g_*[r : r + N].
"""
import numpy as np

U = 2.0 ** -24
EPS32 = np.float32(1e-12)
FWD = ("xyz", "scales", "rots", "opac")
BWD = ("d_xyz", "d_scaling", "d_rotation", "d_opacity")
TENSORS = FWD + BWD
UPSTREAM = ("g_xyz", "g_scales", "g_rots", "g_opac")
NS = (1, 255, 256, 257, 1025)
NMAX = 1025
BAND_X, BAND, ZERO_X = 17.0, 1.2e-7, 18.0
VARIANTS = ("no_projection", "clamp_at_1e-6", "exp_rel_1e-5", "accurate_one_minus_s", "no_row0")
MIN_NORMAL = 2.0 ** -126

# worst ratio of the float32 restatement against float64 per tensor over case() (all 1025 rows; the smaller N are its prefixes) - measured by
# test_plain_activate_ref_host.py::test_r_f32_is_measured, rounded up to one decimal
R_F32 = {"xyz": 0.0, "scales": 1.0, "rots": 2.3, "opac": 1.7, "d_xyz": 0.0, "d_scaling": 1.8, "d_rotation": 4.9, "d_opacity": 2.6}


def bar(tensor):
    return 2.0 * max(R_F32[tensor], 2.0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the two chains

def _len(q, dtype):
    q = np.asarray(q).astype(dtype)
    with np.errstate(over="ignore"):
        return np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])[:, None]


def clamp_free(rot):
    """[N,1] bool: the float32 |q| exceeds eps - the branch the kernel takes, and the one the float64 adjoint is defined with"""
    return _len(rot, np.float32) > EPS32


def _exp(a, dtype):
    """exp with ONE rounding: numpy's float32 exp is a vector routine some ulps off at large arguments, so the float32 chain rounds the
    float64 value"""
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(np.asarray(a).astype(np.float64)).astype(dtype)


def _sigmoid(x, dtype):
    one = np.ones((), dtype)
    with np.errstate(over="ignore"):
        return one / (one + _exp(-np.asarray(x).astype(dtype), dtype))


def forward(xyz, scaling, rot, opac, dtype):
    dtype = np.dtype(dtype)
    q = np.asarray(rot).astype(dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        out = {"xyz": np.asarray(xyz).astype(dtype), "scales": _exp(np.asarray(scaling).astype(dtype), dtype),
               "rots": q / np.maximum(_len(q, dtype), EPS32.astype(dtype)), "opac": _sigmoid(opac, dtype)}
    return out


def _rows(g, like, row0, dtype, variant):
    """rows [row0, row0 + N) of an upstream buffer as `like`'s shape; None: zeros"""
    n = like.shape[0]
    if g is None:
        return np.zeros(like.shape, dtype)
    r = 0 if variant == "no_row0" else row0
    return np.asarray(g)[r:r + n].reshape(like.shape).astype(dtype)


def backward(scaling, rot, opac, g_xyz, g_scales, g_rots, g_opac, dtype, variant=None, row0=0, absolute=False):
    """absolute: every operand by its magnitude and the subtractions as additions, in float64 (S_abs)"""
    dtype = np.dtype(dtype)
    assert variant in (None,) + VARIANTS and not (absolute and (variant or dtype != np.float64))
    s, q, x = (np.asarray(a).astype(dtype) for a in (scaling, rot, opac))
    n = s.shape[0]
    gx, gs, gr, go = (_rows(g, like, row0, dtype, variant) for g, like in ((g_xyz, s), (g_scales, s), (g_rots, q), (g_opac, x)))
    free = clamp_free(rot)
    if variant == "clamp_at_1e-6":
        free = _len(rot, np.float32) > np.float32(1e-6)
    eps = EPS32.astype(dtype)
    one = np.ones((), dtype)
    if absolute:
        gx, gs, gr, go, q = np.abs(gx), np.abs(gs), np.abs(gr), np.abs(go), np.abs(q)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        e = _exp(s, dtype)
        if variant == "exp_rel_1e-5":
            e = e * dtype.type(1.0 + 1e-5)
        qn = one / np.maximum(_len(q, dtype), eps)
        y = q * qn
        yd = (((y[:, 0] * gr[:, 0] + y[:, 1] * gr[:, 1]) + y[:, 2] * gr[:, 2]) + y[:, 3] * gr[:, 3])[:, None]
        proj = y * yd
        if variant == "no_projection":
            proj = proj * dtype.type(0.0)
        d_rot = np.where(free, ((gr + proj) if absolute else (gr - proj)) * qn, gr * qn)
        sg = _sigmoid(opac, dtype)
        one_minus = (one + sg) if absolute else (one - sg)
        if variant == "accurate_one_minus_s":
            em = _exp(-x, dtype)
            one_minus = np.where(sg == one, em / (one + em), one_minus)
        d_op = (go * one_minus) * sg
        d_s = gs * e
    return {"d_xyz": gx, "d_scaling": d_s, "d_rotation": d_rot, "d_opacity": d_op}


def abs_sums(xyz, scaling, rot, opac, g_xyz, g_scales, g_rots, g_opac, row0=0):
    out = {k: np.abs(v) for k, v in forward(xyz, scaling, rot, opac, np.float64).items()}
    out.update(backward(scaling, rot, opac, g_xyz, g_scales, g_rots, g_opac, np.float64, row0=row0, absolute=True))
    return out


def reference(xyz, scaling, rot, opac, g_xyz, g_scales, g_rots, g_opac, row0=0):
    """(ref64, S_abs) over all eight tensors"""
    ref = forward(xyz, scaling, rot, opac, np.float64)
    ref.update(backward(scaling, rot, opac, g_xyz, g_scales, g_rots, g_opac, np.float64, row0=row0))
    return ref, abs_sums(xyz, scaling, rot, opac, g_xyz, g_scales, g_rots, g_opac, row0)


def restatement(xyz, scaling, rot, opac, g_xyz, g_scales, g_rots, g_opac, variant=None, row0=0):
    """the float32 restatement (or a wrong variant of its backward) over all eight tensors"""
    out = forward(xyz, scaling, rot, opac, np.float32)
    out.update(backward(scaling, rot, opac, g_xyz, g_scales, g_rots, g_opac, np.float32, variant=variant, row0=row0))
    assert all(v.dtype == np.float32 for v in out.values())
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the gate

def ratio(got, ref64, s_abs):
    """per element |got - ref64| / (2^-24 S_abs); an exact element is 0 whatever S_abs, a NaN or a miss where S_abs == 0 is inf"""
    got, ref64 = np.asarray(got, np.float64).reshape(np.shape(ref64)), np.asarray(ref64, np.float64)
    err = np.abs(got - ref64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(err == 0, 0.0, err / (U * s_abs))
    return np.where(np.isnan(out), np.inf, out)


def check(got, ref64, s_abs, opac, g_opac, row0=0):
    """dict tensor -> per-element (ratio / bar) for the tensors present in `got`: an element passes where the figure is <= 1.
    d_opacity at x > BAND_X: |got| / (BAND |g|) instead, and inf where x >= ZERO_X and got != 0."""
    out = {}
    for t in TENSORS:
        if got.get(t) is None:
            continue
        r = ratio(got[t], ref64[t], s_abs[t]) / bar(t)
        if t == "d_opacity":
            x = np.asarray(opac, np.float64).reshape(r.shape)
            g = np.abs(_rows(g_opac, x, row0, np.float64, None))
            v = np.abs(np.asarray(got[t], np.float64).reshape(r.shape))
            with np.errstate(divide="ignore", invalid="ignore"):
                band = np.where(v == 0, 0.0, v / (BAND * g))
            band = np.where(np.isnan(band) | ((x >= ZERO_X) & (v != 0)), np.inf, band)
            r = np.where(x > BAND_X, band, r)
        out[t] = r
    return out


def failures(figures):
    """[(tensor, number of failing elements, worst figure, its flat index)] of check()'s result"""
    return [(t, int((~(f <= 1.0)).sum()), float(f.max()), int(f.argmax())) for t, f in figures.items() if not (f <= 1.0).all()]


def worst(figures):
    return {t: (float(f.max()) if f.size else 0.0) for t, f in figures.items()}


def table(figures):
    return "  ".join("%s %.3f" % (t, v) for t, v in worst(figures).items())


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases

SCALING_EDGES = (-80.0, 0.0, 80.0, 88.0)        # with -87: the range where exp is a normal float32
ROWS = {"scaling_edges": (1, 2, 3, 4), "rot_1e-7": (6, 7, 255), "rot_1e-11": (8, 9, 1024), "rot_above_clamp": 10, "rot_below_clamp": (11, 256),
        "rot_zero": 12, "rot_one_component": 13, "rot_1e3": 14, "opac_linspace": 20, "opac_17": (61, 62), "opac_80": (63, 64)}
_cache = {}


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _scaled_to(q, length):
    q = q.astype(np.float64)
    return (q * (length / np.sqrt((q * q).sum()))).astype(np.float32)


def case():
    """the gated case: 1025 rows, float32, read-only; the smaller N are prefixes (inputs(n)).  Keys: xyz, scaling, rot, opac, g_xyz, g_scales,
    g_rots, g_opac, and row_m87 - the row whose scaling is -87."""
    if "case" in _cache:
        return _cache["case"]
    rng = np.random.default_rng(20240607)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    c = {"xyz": f(rng.normal(0, 3, (NMAX, 3))), "scaling": f(rng.normal(-3, 2, (NMAX, 3))), "rot": f(rng.normal(0, 1, (NMAX, 4))),
         "opac": f(rng.normal(0, 10, (NMAX, 1)))}
    for k, w in zip(UPSTREAM, (3, 3, 4, 1)):
        c[k] = f(rng.normal(0, 1, (NMAX, w)))
    for r, v in zip(ROWS["scaling_edges"], SCALING_EDGES):
        c["scaling"][r] = v
    # exp(-87) = 1.6e-38 is normal, its product with |g| < 0.72 is not, and the gate has no term for underflow: the row sits where the
    # seeded upstream gradient keeps g exp(-87) normal
    ok = np.flatnonzero((np.abs(c["g_scales"]) >= 0.75).all(axis=1))
    c["row_m87"] = int(ok[(ok >= 15) & (ok < 20) | (ok >= 65)][0])
    c["scaling"][c["row_m87"]] = -87.0
    c["scaling"][1023] = (-80.0, 0.0, 88.0)                                    # (a mixed row in the last full wave)
    for r in ROWS["rot_1e-7"]:
        c["rot"][r] *= np.float32(1e-7)
    for r in ROWS["rot_1e-11"]:
        c["rot"][r] *= np.float32(1e-11)
    c["rot"][ROWS["rot_above_clamp"]] = _scaled_to(c["rot"][ROWS["rot_above_clamp"]], 2e-12)
    for r in ROWS["rot_below_clamp"]:
        c["rot"][r] = _scaled_to(c["rot"][r], 5e-13)
    c["rot"][ROWS["rot_zero"]] = 0.0
    c["rot"][ROWS["rot_one_component"]] = (0.0, 0.0, -0.7, 0.0)
    c["rot"][ROWS["rot_1e3"]] *= np.float32(1e3)
    r0 = ROWS["opac_linspace"]
    c["opac"][r0:r0 + 41, 0] = np.linspace(-30, 30, 41)
    c["opac"][list(ROWS["opac_17"]), 0] = (17.0, -17.0)
    c["opac"][list(ROWS["opac_80"]), 0] = (80.0, -80.0)
    _cache["case"] = _freeze(c)
    return c


def inputs(n=NMAX):
    """(xyz, scaling, rot, opac) of the first n rows"""
    c = case()
    return tuple(c[k][:n] for k in ("xyz", "scaling", "rot", "opac"))


def upstream(n=NMAX):
    c = case()
    return tuple(c[k][:n] for k in UPSTREAM)


def case_reference(n=NMAX):
    """(ref64, S_abs) of the first n rows, computed once per n and read-only"""
    key = ("ref", n)
    if key not in _cache:
        ref, s_abs = reference(*inputs(n), *upstream(n))
        _cache[key] = (_freeze(ref), _freeze(s_abs))
    return _cache[key]


SPECIAL_ROWS = {"scaling_89": 1, "scaling_-inf": 2, "nan_xyz": 4, "nan_scaling": 5, "nan_rot": 6, "nan_opac": 7, "nan_g_rots": 9, "rot_1e20": 11}


def special_case():
    """16 rows kept out of the gate (SPECIAL_ROWS; the other rows are ordinary), with N(0, 1) upstream gradients.  What is asserted of them:
      scaling 89 -> scales +inf, scaling -inf -> scales 0 (and d_scaling 0);
      a NaN in one input (or one upstream gradient) of a row reaches that row's outputs / gradients, and only them; a NaN component of a
      rotation makes |q| NaN and with it all four rots and all four d_rotation of the row, as F.normalize does (clamp_min keeps a NaN);
      rot * 1e20: |q|^2 overflows to +inf in float32, |q| = inf, rots = q / inf = +-0, the reciprocal is 0, y = 0, y.g = 0 and
      d_rotation = (g - 0) 0 = +-0 - the float32 formula's answer (the float64 one is the unit quaternion)."""
    if "special" in _cache:
        return _cache["special"]
    rng = np.random.default_rng(77)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    n = 16
    c = {"xyz": f(rng.normal(0, 3, (n, 3))), "scaling": f(rng.normal(-3, 2, (n, 3))), "rot": f(rng.normal(0, 1, (n, 4))),
         "opac": f(rng.normal(0, 3, (n, 1)))}
    for k, w in zip(UPSTREAM, (3, 3, 4, 1)):
        c[k] = f(rng.normal(0, 1, (n, w)))
    R = SPECIAL_ROWS
    c["scaling"][R["scaling_89"]] = 89.0
    c["scaling"][R["scaling_-inf"]] = -np.inf
    c["xyz"][R["nan_xyz"], 1] = np.nan
    c["scaling"][R["nan_scaling"], 2] = np.nan
    c["rot"][R["nan_rot"], 3] = np.nan
    c["opac"][R["nan_opac"], 0] = np.nan
    c["g_rots"][R["nan_g_rots"], 0] = np.nan
    c["rot"][R["rot_1e20"]] *= np.float32(1e20)
    _cache["special"] = _freeze(c)
    return c


def special_failures(got, c=None):
    """what is asserted of special_case(), on any evaluator's eight tensors `got`; returns a list of complaints (empty: all holds)"""
    c = special_case() if c is None else c
    R = SPECIAL_ROWS
    g = {t: np.asarray(got[t], np.float32).reshape(16, -1) for t in TENSORS}
    bad = []
    if not (np.isposinf(g["scales"][R["scaling_89"]]).all() and np.isposinf(np.abs(g["d_scaling"][R["scaling_89"]])).all()):
        bad.append("scaling 89: scales %s d_scaling %s" % (g["scales"][R["scaling_89"]], g["d_scaling"][R["scaling_89"]]))
    if not ((g["scales"][R["scaling_-inf"]] == 0).all() and (g["d_scaling"][R["scaling_-inf"]] == 0).all()):
        bad.append("scaling -inf: scales %s d_scaling %s" % (g["scales"][R["scaling_-inf"]], g["d_scaling"][R["scaling_-inf"]]))
    # where a NaN must be, and nowhere else: {tensor: rows}
    want = {"xyz": [R["nan_xyz"]], "scales": [R["nan_scaling"]], "d_scaling": [R["nan_scaling"]], "rots": [R["nan_rot"]],
            "d_rotation": [R["nan_rot"], R["nan_g_rots"]], "opac": [R["nan_opac"]], "d_opacity": [R["nan_opac"]], "d_xyz": []}
    for t in TENSORS:
        rows = sorted(np.flatnonzero(np.isnan(g[t]).any(axis=1)).tolist())
        if rows != sorted(want[t]):
            bad.append("%s: NaN in rows %s, expected %s" % (t, rows, sorted(want[t])))
    if not (np.isnan(g["xyz"][R["nan_xyz"]]).tolist() == [False, True, False] and np.isnan(g["scales"][R["nan_scaling"]]).tolist() == [False, False, True]):
        bad.append("a NaN of one component of xyz / scaling spread within its row")
    if not (np.isnan(g["rots"][R["nan_rot"]]).all() and np.isnan(g["d_rotation"][R["nan_rot"]]).all()):
        bad.append("a NaN component of a rotation: |q| is NaN and so are all of the row's rots %s and d_rotation %s (torch's clamp_min keeps a NaN; "
                   "fmaxf would drop it)" % (g["rots"][R["nan_rot"]], g["d_rotation"][R["nan_rot"]]))
    if not ((g["rots"][R["rot_1e20"]] == 0).all() and (g["d_rotation"][R["rot_1e20"]] == 0).all()):
        bad.append("rot * 1e20: rots %s d_rotation %s" % (g["rots"][R["rot_1e20"]], g["d_rotation"][R["rot_1e20"]]))
    return bad


def ordinary_special_rows():
    return [r for r in range(16) if r not in SPECIAL_ROWS.values()]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the inputs of test_gpu_bg_train.py::test_plain_activate_matches_float64_autograd

def present_test_inputs(extra=0):
    """(xyz, scaling, rot, opac, ups) as torch CPU tensors; ups = the four upstream gradients, of 5000 + extra rows (that test's joint
    buffers have 37 rows more than the model).  The test itself draws its inputs here, so the host test cannot drift from it."""
    import torch
    g = torch.Generator().manual_seed(1)
    n = 5000
    xyz = torch.randn(n, 3, generator=g)
    scaling = torch.randn(n, 3, generator=g) * 2 - 3
    rot = torch.randn(n, 4, generator=g)
    rot[:7] *= 1e-7
    rot[7] = 0.0
    rot[8] = torch.tensor([1e-14, 0.0, -1e-14, 0.0])
    opac = torch.randn(n, 1, generator=g) * 10
    opac[:20, 0] = torch.linspace(-30, 30, 20)
    ups = [torch.randn((n + extra, w), generator=g) for w in (3, 3, 4, 1)]
    return xyz, scaling, rot, opac, ups


def present_rel(a, b):
    """test_gpu_bg_train._rel: max |a - b| / max |b|"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-30))
