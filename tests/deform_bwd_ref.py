"""The backward of the deform / shade row body (csrc/gm_deform_bwd.hip: gm_deform_shade_bwd), in numpy.

    backward(deg, tri, w, dV, Rv, Sv, cov, pos, shs, campos, g_pos, g_cov6, g_rgb, gate, dtype) -> dict of the six gradients
        g_dV [Vm,3], g_Rv [Vm,9], g_Sv [Vm,9]  (the vertex sums),  g_shs [N,M,3], g_cov [N,9], g_rest_pos [N,3]  (per row)

One operation per line, in the kernel's parenthesisation (deform_ref.py states the forward half the same way): dtype=float64 is the
reference, dtype=float32 the emulation of a correct float32 evaluator.  The emulation accumulates each vertex's incidence list
SEQUENTIALLY in list order - the least accurate of the reasonable orders (the kernel runs 64 strided partial sums and a tree).  The list is
the one deform.DeformBinding builds: the entries 3 row + corner of a vertex, ascending.

gate [N,3] bool is an input: where the forward's r + 0.5 > 0.  A device test passes the device forward's own rgb > 0 (the +-4 ulp rows of the
`clamp` case may fall either side in float32); the host tests pass the float64 forward's.

The view direction is formed from npos_dir when given - the EVALUATOR'S OWN float32 deformed positions - as deform_ref.py compares the colour
from the evaluator's own position: float32 positions are exact operands, so dir = (npos - cam) / |npos - cam| errs relative to its own
magnitude and the bars get no term for the camera's distance (a camera 1e-3 from a Gaussian would otherwise turn the position's 4 roundings
into a relative error of 1e-3 in dir).  With npos_dir=None the chain is closed: that is what autograd differentiates.

backward_abs is the same chain with every operand and constant replaced by its absolute value and every subtraction by an addition, in
float64 (S_abs, deform_ref.py's convention: the direction enters as |dir|, the length as itself); ratio = |got - ref64| / (2^-24 S_abs).

First-order rounding counts (deform_ref.py's rules; degree 3, the worst): blend 3; RS 9; dir 5.5, len 3.5; x = Rb dir: (3 + 5.5 + 1) + 2 = 11.5;
  covariance route: RS C^T, RS C: 12; G (..): 15; g_RS 16; g_Rt = g_RS Sb^T, g_Sb = Rt^T g_RS: (16 + 3 + 1) + 2 = 22; g_C = RS^T (G RS): (9 + 12 + 1) + 2 = 24
  basis: (C z) ((2 zz - 3 xx) - 3 yy): 12.5 + 27 + 1 = 40.5, g_shs = basis g_r: 41.5
  dSH/dx: worst term (C S) ((-3 xx + 4 zz) - yy): 1 + 27 + 1 = 29, seven terms and the += : 36; g_xyz: (36 + 0 + 1) + 2 = 39
  g_Rb = g_Rt^T + g_xyz dir: max(22, 39 + 5.5 + 1) + 1 = 46.5
  g_dir = Rb^T g_xyz: 45; s = g_dir . dir: 53.5; dir s: 60; g_dir - dir s: 61; / len: 65.5; g_pos + ..: 66.5
  a vertex sum over a list of L entries: the row's count + 1 (times w) + L - 1
Ceilings, not expectations; what the emulation reaches is R_F32 below (measured by test_deform_bwd_ref_host.py); the device test holds every
element to 2 R_F32.
"""
import numpy as np

import deform_ref as ref

U = ref.U
ROW_TENSORS = ("g_shs", "g_cov", "g_rest_pos")
VERTEX_TENSORS = ("g_dV", "g_Rv", "g_Sv")
TENSORS = VERTEX_TENSORS + ROW_TENSORS
COUNT_ROW = {"g_dV": 66.5, "g_Rv": 46.5, "g_Sv": 22.0, "g_shs": 41.5, "g_cov": 24.0, "g_rest_pos": 66.5}
VARIANTS = ("no_direction_term", "no_gt_term", "grt_not_transposed", "corners_swapped", "gate_ignored", "degree_off_by_one")


def count(tensor, longest_list):
    """the rounding count of a tensor's elements: a vertex sum adds the weight's product and the list's additions"""
    return COUNT_ROW[tensor] + (longest_list if tensor in VERTEX_TENSORS else 0.0)


# worst ratio of the float32 emulation against float64 per kind (deform_bwd_cases.KINDS) and tensor, over N in deform_bwd_cases.NS, degrees 0..3 and both
# cameras (measured by test_deform_bwd_ref_host.py::test_r_f32_is_measured_and_under_its_rounding_count, rounded up to one decimal)
R_F32 = {
    "twist": {"g_dV": 2.3, "g_Rv": 3.8, "g_Sv": 2.7, "g_shs": 7.2, "g_cov": 5.1, "g_rest_pos": 2.1},
    "needle": {"g_dV": 2.0, "g_Rv": 3.3, "g_Sv": 1.8, "g_shs": 5.2, "g_cov": 4.2, "g_rest_pos": 1.4},
    "outside": {"g_dV": 2.6, "g_Rv": 2.4, "g_Sv": 2.7, "g_shs": 5.6, "g_cov": 4.6, "g_rest_pos": 1.0},
    "onehot": {"g_dV": 2.1, "g_Rv": 2.5, "g_Sv": 1.9, "g_shs": 6.4, "g_cov": 3.3, "g_rest_pos": 1.4},
    "clamp": {"g_dV": 2.6, "g_Rv": 3.2, "g_Sv": 3.1, "g_shs": 6.9, "g_cov": 4.8, "g_rest_pos": 1.2},
    "edges": {"g_dV": 2.5, "g_Rv": 2.8, "g_Sv": 2.5, "g_shs": 8.2, "g_cov": 5.0, "g_rest_pos": 1.3},
    "hub": {"g_dV": 3.8, "g_Rv": 4.2, "g_Sv": 3.3, "g_shs": 5.7, "g_cov": 4.2, "g_rest_pos": 2.0},
    "last_unused": {"g_dV": 2.7, "g_Rv": 3.9, "g_Sv": 3.4, "g_shs": 6.8, "g_cov": 6.5, "g_rest_pos": 1.6},
}


def incidence(tri, Vm):
    """(offsets int64 [Vm+1], entries int64 [3N]) as deform.DeformBinding builds them: a stable sort of tri.reshape(-1)"""
    flat = np.asarray(tri, np.int64).reshape(-1)
    entries = np.argsort(flat, kind="stable")
    offsets = np.zeros(Vm + 1, np.int64)
    np.cumsum(np.bincount(flat, minlength=Vm), out=offsets[1:])
    return offsets, entries


def _mm(A, B):          # c[a][b] = sum_k a[a][k] b[k][b]
    return [(A[3 * a] * B[b] + A[3 * a + 1] * B[3 + b]) + A[3 * a + 2] * B[6 + b] for a in range(3) for b in range(3)]


def _mm_nt(A, B):       # c[a][b] = sum_k a[a][k] b[b][k]
    return [(A[3 * a] * B[3 * b] + A[3 * a + 1] * B[3 * b + 1]) + A[3 * a + 2] * B[3 * b + 2] for a in range(3) for b in range(3)]


def _mm_tn(A, B):       # c[a][b] = sum_k a[k][a] b[k][b]
    return [(A[a] * B[b] + A[3 + a] * B[3 + b]) + A[6 + a] * B[6 + b] for a in range(3) for b in range(3)]


def _cols(a, n):
    return [a[:, k] for k in range(n)]


def _sh_derivatives(ar, deg, x, y, z, S):
    """basis [16] of [N,1] (None beyond the degree) and dSH/dx, dSH/dy, dSH/dz [N,3] per channel, as the kernel (and gm_preprocess.hip) state them"""
    c, sub = ar.c, ar.sub
    neg = (lambda a: a) if ar.absolute else (lambda a: -a)
    zero = x * c(0.0)
    basis = [None] * 16
    basis[0] = c(ref.SH_C0) + zero
    ddx = ddy = ddz = c(0.0) * S(0)
    C1, C2, C3 = c(ref.SH_C1), [c(v) for v in ref.SH_C2], [c(v) for v in ref.SH_C3]
    two, three, four = c(2.0), c(3.0), c(4.0)
    if deg > 0:
        basis[1], basis[2], basis[3] = neg(C1) * y, C1 * z, neg(C1) * x
        ddx, ddy, ddz = neg(C1) * S(3), neg(C1) * S(1), C1 * S(2)
        if deg > 1:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            basis[4], basis[5], basis[6] = C2[0] * xy, C2[1] * yz, C2[2] * sub(sub(two * zz, xx), yy)
            basis[7], basis[8] = C2[3] * xz, C2[4] * sub(xx, yy)
            ddx = ddx + (C2[0] * y * S(4) + C2[2] * two * neg(x) * S(6) + C2[3] * z * S(7) + C2[4] * two * x * S(8))
            ddy = ddy + (C2[0] * x * S(4) + C2[1] * z * S(5) + C2[2] * two * neg(y) * S(6) + C2[4] * two * neg(y) * S(8))
            ddz = ddz + (C2[1] * y * S(5) + C2[2] * two * two * z * S(6) + C2[3] * x * S(7))
            if deg > 2:
                basis[9], basis[10] = C3[0] * y * sub(three * xx, yy), C3[1] * xy * z
                basis[11], basis[12] = C3[2] * y * sub(sub(four * zz, xx), yy), C3[3] * z * sub(sub(two * zz, three * xx), three * yy)
                basis[13], basis[14] = C3[4] * x * sub(sub(four * zz, xx), yy), C3[5] * z * sub(xx, yy)
                basis[15] = C3[6] * x * sub(xx, three * yy)
                ddx = ddx + (C3[0] * S(9) * three * two * xy + C3[1] * S(10) * yz + C3[2] * S(11) * neg(two) * xy +
                             C3[3] * S(12) * neg(three) * two * xz + C3[4] * S(13) * sub(neg(three) * xx + four * zz, yy) +
                             C3[5] * S(14) * two * xz + C3[6] * S(15) * three * sub(xx, yy))
                ddy = ddy + (C3[0] * S(9) * three * sub(xx, yy) + C3[1] * S(10) * xz +
                             C3[2] * S(11) * sub(neg(three) * yy + four * zz, xx) + C3[3] * S(12) * neg(three) * two * yz +
                             C3[4] * S(13) * neg(two) * xy + C3[5] * S(14) * neg(two) * yz + C3[6] * S(15) * neg(three) * two * xy)
                ddz = ddz + (C3[1] * S(10) * xy + C3[2] * S(11) * four * two * yz +
                             C3[3] * S(12) * three * sub(sub(two * zz, xx), yy) + C3[4] * S(13) * four * two * xz +
                             C3[5] * S(14) * sub(xx, yy))
    return basis, ddx, ddy, ddz


def _backward(ar, deg, tri, w, dV, Rv, Sv, cov, pos, shs, campos, g_pos, g_cov6, g_rgb, gate, variant=None, npos_dir=None, Vm=None):
    tri = np.asarray(tri)
    N, M = tri.shape[0], np.shape(shs)[1]
    Vm = np.shape(dV)[0] if Vm is None else Vm
    t0, t1, t2 = tri[:, 0], tri[:, 1], tri[:, 2]
    w_ = ar.lift(w)
    dV, Rv, Sv = ar.lift(dV).reshape(-1, 3), ar.lift(Rv).reshape(-1, 9), ar.lift(Sv).reshape(-1, 9)
    C, p = _cols(ar.lift(cov).reshape(-1, 9), 9), ar.lift(pos)
    w0, w1, w2 = w_[:, 0:1], w_[:, 1:2], w_[:, 2:3]
    blend = lambda tab: (w0 * tab[t0] + w1 * tab[t1]) + w2 * tab[t2]
    d, Rb, Sb = blend(dV), _cols(blend(Rv), 9), _cols(blend(Sv), 9)
    npos = p + d
    # ---- the view direction
    if ar.absolute:
        dx, dy, dz = ref._direction(np.float64, npos_dir, campos, normalise=False)
        ln = np.sqrt(dx * dx + dy * dy + dz * dz)
        dirs = [np.abs(v / ln)[:, 0] for v in (dx, dy, dz)]
    else:
        dx, dy, dz = ref._direction(ar.dtype, npos if npos_dir is None else npos_dir, campos, normalise=False)
        ln = np.sqrt(dx * dx + dy * dy + dz * dz)
        dirs = [(v / ln)[:, 0] for v in (dx, dy, dz)]
    ln = ln[:, 0]
    x = ((Rb[0] * dirs[0] + Rb[1] * dirs[1]) + Rb[2] * dirs[2])[:, None]
    y = ((Rb[3] * dirs[0] + Rb[4] * dirs[1]) + Rb[5] * dirs[2])[:, None]
    z = ((Rb[6] * dirs[0] + Rb[7] * dirs[1]) + Rb[8] * dirs[2])[:, None]
    # ---- colour route
    if variant == "degree_off_by_one":
        deg = deg - 1 if deg > 0 else 1
    ncoef = (deg + 1) ** 2
    shs = np.asarray(shs)
    S = lambda k: ar.lift(shs[:, k, :])
    g_rgb = ar.lift(np.zeros((N, 3), np.float32) if g_rgb is None else g_rgb)
    gr = g_rgb if variant == "gate_ignored" else np.where(np.asarray(gate, bool), g_rgb, ar.c(0.0))
    basis, ddx, ddy, ddz = _sh_derivatives(ar, deg, x, y, z, S)
    gxyz = [(gr[:, 0] * dd[:, 0] + gr[:, 1] * dd[:, 1]) + gr[:, 2] * dd[:, 2] for dd in (ddx, ddy, ddz)]
    g_shs = np.zeros((N, M, 3), ar.dtype)
    for k in range(ncoef):
        g_shs[:, k, :] = basis[k] * gr
    # ---- covariance route
    g6 = _cols(ar.lift(np.zeros((N, 6), np.float32) if g_cov6 is None else g_cov6), 6)
    zero = g6[0] * ar.c(0.0)
    G = [g6[0], g6[1], g6[2], zero, g6[3], g6[4], zero, zero, g6[5]]
    Rt = [Rb[3 * b + a] for a in range(3) for b in range(3)]
    RS = _mm(Rt, Sb)
    P = _mm_nt(RS, C)
    Q = _mm(RS, C)
    T1 = _mm(G, P)
    T2 = _mm_tn(G, Q)
    gRS = T1 if variant == "no_gt_term" else [a + b for a, b in zip(T1, T2)]
    g_cov = np.stack(_mm_tn(RS, _mm(G, RS)), axis=1)
    gRt = _mm_nt(gRS, Sb)
    gSb = _mm_tn(Rt, gRS)
    if variant == "grt_not_transposed":
        gRb = [gRt[3 * a + b] + gxyz[a] * dirs[b] for a in range(3) for b in range(3)]
    else:
        gRb = [gRt[3 * b + a] + gxyz[a] * dirs[b] for a in range(3) for b in range(3)]
    gdir = [(Rb[b] * gxyz[0] + Rb[3 + b] * gxyz[1]) + Rb[6 + b] * gxyz[2] for b in range(3)]
    s = (gdir[0] * dirs[0] + gdir[1] * dirs[1]) + gdir[2] * dirs[2]
    gp = ar.lift(g_pos)
    if variant == "no_direction_term":
        gn = [gp[:, k] for k in range(3)]
    else:
        gn = [gp[:, k] + ar.sub(gdir[k], dirs[k] * s) / ln for k in range(3)]
    rows = np.stack(gn + gRb + gSb, axis=1)                                     # [N,21]: g_d | g_Rb | g_Sb
    # ---- the vertex sums: each list sequentially, in list order
    scatter_tri = tri[:, [0, 2, 1]] if variant == "corners_swapped" else tri
    offsets, entries = incidence(scatter_tri, Vm)
    wf = w_.reshape(-1)
    acc = np.zeros((Vm, 21), ar.dtype)
    for v in range(Vm):
        for e in entries[offsets[v]:offsets[v + 1]]:
            acc[v] = acc[v] + wf[e] * rows[e // 3]
    return {"g_dV": acc[:, 0:3], "g_Rv": acc[:, 3:12], "g_Sv": acc[:, 12:21], "g_shs": g_shs, "g_cov": g_cov, "g_rest_pos": np.stack(gn, axis=1)}, npos


def backward(deg, tri, w, dV, Rv, Sv, cov, pos, shs, campos, g_pos, g_cov6, g_rgb, gate, dtype, variant=None, npos_dir=None, want_npos=False):
    out, npos = _backward(ref._Arith(dtype), deg, tri, w, dV, Rv, Sv, cov, pos, shs, campos, g_pos, g_cov6, g_rgb, gate, variant, npos_dir)
    return (out, npos) if want_npos else out


def backward_abs(deg, tri, w, dV, Rv, Sv, cov, pos, shs, campos, g_pos, g_cov6, g_rgb, gate, npos_dir):
    return _backward(ref._Arith(np.float64, True), deg, tri, w, dV, Rv, Sv, cov, pos, shs, campos, g_pos, g_cov6, g_rgb, gate, None, npos_dir)[0]


def ratios(got, ref64, s_abs):
    """dict tensor -> per-element ratio for the tensors present in got"""
    return {t: ref.ratio(np.reshape(got[t], np.shape(ref64[t])), ref64[t], s_abs[t]) for t in TENSORS if got.get(t) is not None}
