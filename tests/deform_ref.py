"""The row body of the deform / shade kernels (gm_deform.hip: gather_blend, deform_cov, shade_rotated; gm_sh.h: sh_channel), in numpy.

    stage1(tri, w, dV, Rv, Sv, cov, pos, dtype)  -> npos [N,3], O [N,9], Rt [N,9]
    stage2(deg, npos, Rt, campos, shs, dtype)    -> rgb [N,3]

One operation per line, in the kernels' parenthesisation: with dtype=float64 this is the reference, with dtype=float32 a step-by-step
emulation of a correct float32 evaluator (numpy rounds every float32 operation once and contracts nothing, like the kernels under
`#pragma clang fp contract(off)`).  The inputs are float32 values and exact in either; the kernels' constants are their float32 literals.

stage1_abs / stage2_abs are the same chains with every operand and constant replaced by its absolute value and every subtraction by an
addition, in float64: S_abs, the magnitude a result's rounding errors scale with.  One step is not propagated: the view direction
d = (npos - campos) / |npos - campos| enters stage2_abs as |d|.  Its operands are exact, so its subtraction, squares, sum of squares, square
root and division all err RELATIVE to their results (no cancellation of rounded quantities): d's own magnitude is its error scale, and the
colour bar gets no term for the camera's distance - stage 2 is compared from the evaluator's OWN float32 npos and Rt.

    ratio = |got - ref64| / (2^-24 S_abs)          per element

First-order rounding counts (the most roundings of relative size u = 2^-24 that reach an element, each weighted by |operands|, so
ratio <= count up to O(u)); a product of factors carrying a and b roundings carries a + b + 1, a sum of n terms the worst term's plus n - 1:
    blend (w0 a + w1 b) + w2 c: 1 + 2 = 3            -> Rt: 3;  npos = p + d: 3 + 1 = 4
    RS = Rt Sb: (3 + 3 + 1) + 2 = 9;  A = RS C: (9 + 0 + 1) + 2 = 12;  O = A RS^T: (12 + 9 + 1) + 2 = 24
    d: dx 1; dx dx 3; the sum 5; the root 2.5 + 1; the quotient 1 + 3.5 + 1 = 5.5;  x = (Rt d): (0 + 5.5 + 1) + 2 = 8.5
    degree 0: C0 S0 1, + 0.5 1                                                          -> 2
    degree 1: worst term (C1 y) S: 8.5 + 2 = 10.5; 3 sums and the + 0.5                 -> 14.5
    degree 2: xy, zz: 18; (2 zz - xx) - yy: 20; (C (..)) S: 22; 8 sums and the + 0.5    -> 31
    degree 3: (C z) ((2 zz - 3 xx) - 3 yy): 9.5 + 21 + 1, times S: 32.5; 15 sums, + 0.5 -> 48.5
The clamp max(., 0) is 1-Lipschitz and adds nothing.  These are ceilings, not expectations: roundings do not align.  What a correct
float32 evaluator really reaches on the cases of deform_cases.py is R_F32 below, measured by test_deform_ref_host.py; the GPU test holds
every element to 2 R_F32.
"""
import numpy as np

U = 2.0 ** -24
TENSORS = ("pos", "rot", "cov", "colour")
COUNT = {"pos": 4.0, "rot": 3.0, "cov": 24.0, "colour": (2.0, 14.5, 31.0, 48.5)}        # colour: per degree

# worst ratio of the float32 emulation against float64 per kind and tensor, over all 257 rows, degrees 0..3 and both cameras of
# deform_cases (measured by test_deform_ref_host.py::test_r_f32_is_measured_and_under_its_rounding_count, rounded up to one decimal)
R_F32 = {
    "twist": {"pos": 1.6, "rot": 2.2, "cov": 5.8, "colour": 1.6},
    "needle": {"pos": 2.3, "rot": 2.0, "cov": 3.7, "colour": 1.7},
    "outside": {"pos": 1.2, "rot": 1.8, "cov": 4.6, "colour": 1.5},
    "onehot": {"pos": 1.0, "rot": 0.0, "cov": 3.4, "colour": 1.6},
    "clamp": {"pos": 1.5, "rot": 1.8, "cov": 4.9, "colour": 1.8},
}

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
         -0.5900435899266435)

STAGE1_VARIANTS = ("swap_w", "rt_not_transposed", "s_rt", "s78_first_vertex", "w_half", "tables_10bit", "flush_O")
STAGE2_VARIANTS = ("dir_not_normalised", "dir_rt", "deg_plus", "deg_minus", "clamp_before")


class _Arith:
    """dtype arithmetic, or (absolute) the float64 magnitude chain"""

    def __init__(self, dtype, absolute=False):
        self.dtype, self.absolute = np.dtype(dtype), absolute

    def lift(self, a):
        a = np.asarray(a).astype(self.dtype)
        return np.abs(a) if self.absolute else a

    def c(self, v):                                     # a constant of the kernels: the float32 literal
        x = np.float32(v).astype(self.dtype)
        return np.abs(x) if self.absolute else x

    def sub(self, a, b):
        return a + b if self.absolute else a - b


def round_mantissa(a, bits):
    """float32 values rounded to `bits` explicit mantissa bits (round half up in magnitude)"""
    i = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    drop = 23 - bits
    i = ((i + (1 << (drop - 1))) >> drop) << drop
    return i.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def _stage1(ar, tri, w, dV, Rv, Sv, cov, pos, variant=None):
    tri = np.asarray(tri)
    t0, t1, t2 = tri[:, 0], tri[:, 1], tri[:, 2]
    if variant == "w_half":
        w = np.asarray(w, np.float32).astype(np.float16).astype(np.float32)
    if variant == "tables_10bit":
        dV, Rv, Sv = (round_mantissa(np.asarray(t, np.float32), 10) for t in (dV, Rv, Sv))
    w = ar.lift(w)
    dV, Rv, Sv = ar.lift(dV).reshape(-1, 3), ar.lift(Rv).reshape(-1, 9), ar.lift(Sv).reshape(-1, 9)
    C, p = ar.lift(cov).reshape(-1, 9), ar.lift(pos)
    w0, w1, w2 = w[:, 0:1], w[:, 1:2], w[:, 2:3]
    if variant == "swap_w":
        w1, w2 = w2, w1
    blend = lambda tab: (w0 * tab[t0] + w1 * tab[t1]) + w2 * tab[t2]            # gather_blend
    d, Rb, Sb = blend(dV), blend(Rv), blend(Sv)
    if variant == "s78_first_vertex":
        Sb = Sb.copy()
        Sb[:, 7:9] = Sv[t0][:, 7:9]
    Rt = Rb if variant == "rt_not_transposed" else Rb.reshape(-1, 3, 3).transpose(0, 2, 1).reshape(-1, 9)       # deform_cov
    if variant == "s_rt":
        RS = [(Sb[:, 3 * a] * Rt[:, b] + Sb[:, 3 * a + 1] * Rt[:, 3 + b]) + Sb[:, 3 * a + 2] * Rt[:, 6 + b] for a in range(3) for b in range(3)]
    else:
        RS = [(Rt[:, 3 * a] * Sb[:, b] + Rt[:, 3 * a + 1] * Sb[:, 3 + b]) + Rt[:, 3 * a + 2] * Sb[:, 6 + b] for a in range(3) for b in range(3)]
    A = [(RS[3 * a] * C[:, b] + RS[3 * a + 1] * C[:, 3 + b]) + RS[3 * a + 2] * C[:, 6 + b] for a in range(3) for b in range(3)]
    O = [(A[3 * a] * RS[3 * b] + A[3 * a + 1] * RS[3 * b + 1]) + A[3 * a + 2] * RS[3 * b + 2] for a in range(3) for b in range(3)]
    O = np.stack(O, axis=1)
    if variant == "flush_O":
        O = np.where(np.abs(O) < 1e-6 * np.abs(O).max(), 0, O).astype(O.dtype)
    npos = p + d
    return npos, O, np.ascontiguousarray(Rt)


def _direction(dtype, npos, campos, normalise=True):
    npos, campos = np.asarray(npos).astype(dtype), np.asarray(campos).astype(dtype).reshape(3)
    dx, dy, dz = (npos[:, k:k + 1] - campos[k] for k in range(3))
    if normalise:
        ln = np.sqrt(dx * dx + dy * dy + dz * dz)
        dx, dy, dz = dx / ln, dy / ln, dz / ln
    return dx, dy, dz


def _stage2(ar, deg, npos, Rt, campos, shs, variant=None):
    if variant == "deg_plus":
        deg = min(deg + 1, 3)
    if variant == "deg_minus":
        deg = max(deg - 1, 0)
    if ar.absolute:
        dx, dy, dz = (np.abs(v) for v in _direction(np.float64, npos, campos))
    else:
        dx, dy, dz = _direction(ar.dtype, npos, campos, normalise=variant != "dir_not_normalised")
    R = [ar.lift(Rt).reshape(-1, 9)[:, k:k + 1] for k in range(9)]
    if variant == "dir_rt":
        x, y, z = ((R[3 * k] * dx + R[3 * k + 1] * dy) + R[3 * k + 2] * dz for k in range(3))
    else:                                                                       # shade_rotated: dir_rot = rot^T dir
        x, y, z = ((R[k] * dx + R[3 + k] * dy) + R[6 + k] * dz for k in range(3))
    shs = np.asarray(shs)
    S = lambda k: ar.lift(shs[:, k, :])                                         # [N,3]: the three channels at once
    c, sub = ar.c, ar.sub
    r = c(SH_C0) * S(0)                                                         # sh_channel
    if deg > 0:
        r = sub(sub(r, c(SH_C1) * y * S(1)) + c(SH_C1) * z * S(2), c(SH_C1) * x * S(3))
        if deg > 1:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            r = (r + c(SH_C2[0]) * xy * S(4) + c(SH_C2[1]) * yz * S(5) + c(SH_C2[2]) * sub(sub(c(2.0) * zz, xx), yy) * S(6) +
                 c(SH_C2[3]) * xz * S(7) + c(SH_C2[4]) * sub(xx, yy) * S(8))
            if deg > 2:
                r = (r + c(SH_C3[0]) * y * sub(c(3.0) * xx, yy) * S(9) + c(SH_C3[1]) * xy * z * S(10) +
                     c(SH_C3[2]) * y * sub(sub(c(4.0) * zz, xx), yy) * S(11) +
                     c(SH_C3[3]) * z * sub(sub(c(2.0) * zz, c(3.0) * xx), c(3.0) * yy) * S(12) +
                     c(SH_C3[4]) * x * sub(sub(c(4.0) * zz, xx), yy) * S(13) + c(SH_C3[5]) * z * sub(xx, yy) * S(14) +
                     c(SH_C3[6]) * x * sub(xx, c(3.0) * yy) * S(15))
    if ar.absolute:
        return r + c(0.5)
    if variant == "clamp_before":
        return np.maximum(r, c(0.0)) + c(0.5)
    return np.maximum(r + c(0.5), c(0.0))


def stage1(tri, w, dV, Rv, Sv, cov, pos, dtype, variant=None):
    return _stage1(_Arith(dtype), tri, w, dV, Rv, Sv, cov, pos, variant)


def stage1_abs(tri, w, dV, Rv, Sv, cov, pos):
    return _stage1(_Arith(np.float64, True), tri, w, dV, Rv, Sv, cov, pos)


def stage2(deg, npos, Rt, campos, shs, dtype, variant=None):
    return _stage2(_Arith(dtype), deg, npos, Rt, campos, shs, variant)


def stage2_abs(deg, npos, Rt, campos, shs):
    return _stage2(_Arith(np.float64, True), deg, npos, Rt, campos, shs)


def ratio(got, ref64, s_abs):
    """per element |got - ref64| / (2^-24 S_abs); an exact element is 0 whatever S_abs, a NaN or a miss where S_abs == 0 is inf"""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    err = np.abs(got - ref64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(err == 0, 0.0, err / (U * s_abs))
    return np.where(np.isnan(out), np.inf, out)


def stage1_inputs(case, n=None):
    return tuple(case[k][:n] if k in ("tri", "w", "cov", "pos") else case[k] for k in ("tri", "w", "dV", "Rv", "Sv", "cov", "pos"))


_REF1 = {}


def stage1_reference(case):
    """float64 stage 1 of a case and its S_abs, once per case (shared, read-only): dict(pos, cov, rot) -> (ref, s_abs)"""
    key = id(case)
    if key not in _REF1:
        p, O, Rt = stage1(*stage1_inputs(case), np.float64)
        pa, Oa, Rta = stage1_abs(*stage1_inputs(case))
        for a in (p, O, Rt, pa, Oa, Rta):
            a.setflags(write=False)
        _REF1[key] = (case, {"pos": (p, pa), "cov": (O, Oa), "rot": (Rt, Rta)})
    return _REF1[key][1]


def row_ratios(case, deg, campos, shs, pos, cov, rot, rgb):
    """Ratios of an evaluator's float32 results on the first len(pos) rows of a case, per tensor: stage 1 from the inputs, stage 2 from
    the evaluator's own pos and rot.  dict tensor -> [n, width] array of ratios."""
    n = np.shape(pos)[0]
    ref1 = stage1_reference(case)
    out = {}
    for name, got in (("pos", pos), ("cov", np.reshape(cov, (n, 9))), ("rot", np.reshape(rot, (n, 9)))):
        ref, s_abs = ref1[name]
        out[name] = ratio(got, ref[:n], s_abs[:n])
    rot32, pos32 = np.asarray(rot, np.float32).reshape(n, 9), np.asarray(pos, np.float32)
    out["colour"] = ratio(rgb, stage2(deg, pos32, rot32, campos, shs[:n], np.float64), stage2_abs(deg, pos32, rot32, campos, shs[:n]))
    return out


def worst(ratios):
    """dict tensor -> (worst ratio, row, element)"""
    out = {}
    for name, r in ratios.items():
        i = int(np.argmax(r))
        out[name] = (float(r.reshape(-1)[i]), i // r.shape[1], i % r.shape[1])
    return out


def old_gate_passes(case, deg, campos, shs, pos, cov, rot, rgb):
    """the tensor max-norm gate of test_gpu_parity.py::test_deform_and_sh_colors on the same results"""
    n = np.shape(pos)[0]
    ref1 = stage1_reference(case)
    p_ref, c_ref, r_ref = (ref1[k][0][:n] for k in ("pos", "cov", "rot"))
    rgb_ref = stage2(deg, p_ref, r_ref, campos, shs[:n], np.float64)
    with np.errstate(invalid="ignore"):
        return bool(np.abs(pos - p_ref).max() <= 1e-5 * np.abs(p_ref).max() and
                    np.abs(np.reshape(cov, (n, 9)) - c_ref).max() <= 1e-5 * np.abs(c_ref).max() and
                    np.abs(np.reshape(rot, (n, 9)) - r_ref).max() <= 1e-5 and np.abs(rgb - rgb_ref).max() <= 1e-5)
