"""Topology edits of bg_model.PlainGaussians (densify_and_prune, reset_opacity) restated in float64 numpy on the float32 states of
tests/golden/bg_densify.npz: which row of the result is which row of the input (kept, cloned, split), the float64 value and the absolute
sum of every COMPUTED element, and the margin of every decision.  Shared by test_bg_model_host.py (CPU torch against it) and
test_gpu_bg_topology.py (the device model against it and, for everything copied, against the CPU model bit for bit).

Computed elements and their absolute sums S_abs (the sum of the magnitudes of the terms of the formula):
  a split row's xyz_c  = sum_k R_ck (exp(scaling_k) Z_k) + xyz_c : sum_k |R|_ck exp(scaling_k) |Z_k| + |xyz_c|, |R| being build_rotation's
                         polynomial in q / |q| with every operand by its magnitude and every subtraction as an addition;
  a split row's scaling = log(exp(scaling) / 1.6) and the opacity after a reset, log(p / (1 - p)) with p = min(sigmoid(x), 0.01):
                         1 + |result| - a logarithm hands the relative rounding of its argument on as an absolute one, the term of magnitude 1.
BOUND = 8 x 2^-24 S_abs: four float32 roundings in the longest chain (exp, the product with the sample, the three-term rotation product,
the add), doubled.  test_bg_model_host.py measures CPU torch against this restatement at under half of it."""
import os
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "bg_densify.npz")
U = 2.0 ** -24
FACTOR = 8.0
MARGIN = 1e-4
PERCENT_DENSE, EXTENT, MIN_OPACITY, SPLIT_N = 0.01, 1.0, 0.005, 2
GROUPS = ("xyz", "f_dc+f_rest", "opacity", "scaling", "rotation")


def model_from(d, prefix, device="cpu"):
    """a PlainGaussians holding the fixture's state `prefix`: parameters, both Adam moments, densification statistics"""
    import torch
    from gaussianmesh_amd.bg_model import PlainGaussians
    from gaussianmesh_amd.bg_train import BG_DEFAULT_OPT
    g = PlainGaussians(3, device=device)
    t = lambda k: torch.as_tensor(d["%s_%s" % (prefix, k)]).to(device)
    g._set_params(t("p_xyz"), torch.cat([t("p_f_dc"), t("p_f_rest")], dim=1), t("p_scaling"), t("p_rotation"), t("p_opacity"))
    g.spatial_lr_scale = 1.0
    g.training_setup(SimpleNamespace(**BG_DEFAULT_OPT))
    for grp in g.optimizer.param_groups:
        for slot, key in (("m", "m"), ("values", "v")):
            if grp["name"] == PlainGaussians.SH_GROUP:
                grp[slot][0] = torch.cat([t("%s_f_dc" % key), t("%s_f_rest" % key)], dim=1).contiguous()
            else:
                grp[slot][0] = t("%s_%s" % (key, grp["name"])).clone()
    g.max_radii2D, g.xyz_gradient_accum, g.denom = t("b_max_radii2D").clone(), t("b_xyz_gradient_accum").clone(), t("b_denom").clone()
    return g


def _rel_margin(a, threshold):
    return np.abs(a - threshold) / abs(threshold)


def _rotation(q, absolute=False):
    """build_rotation: [n,3,3] of q / |q|; absolute: the magnitude chain"""
    q = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    if absolute:
        q = np.abs(q)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    s = (lambda a, b: a + b) if absolute else (lambda a, b: a - b)
    return np.stack([s(1, 2 * (y * y + z * z)), 2 * s(x * y, w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), s(1, 2 * (x * x + z * z)), 2 * s(y * z, w * x),
                     2 * s(x * z, w * y), 2 * (y * z + w * x), s(1, 2 * (x * x + y * y))], axis=1).reshape(-1, 3, 3)


def densify_plan(d, case):
    """densify_and_prune(threshold, 0.005, 1.0, None, samples=Z) on state <case>0.  Returns a dict:
      src [n1] int      the input row each result row comes from
      kind [n1] '<U5'   "kept", "clone" or "split"
      xyz, scaling      float64 [n1,3] values of the split rows (NaN elsewhere), xyz_abs / scaling_abs their S_abs
      margin            the smallest relative distance of any decision from its threshold"""
    f = lambda k: d["%s0_%s" % (case, k)].astype(np.float64)
    xyz, scaling, rot, opac = f("p_xyz"), f("p_scaling"), f("p_rotation"), f("p_opacity")
    n0 = xyz.shape[0]
    thr = float(d[case + "_threshold"])
    with np.errstate(divide="ignore", invalid="ignore"):
        grads = f("b_xyz_gradient_accum")[:, 0] / f("b_denom")[:, 0]
    grads[np.isnan(grads)] = 0.0
    smax = np.exp(scaling).max(axis=1)
    big = smax > PERCENT_DENSE * EXTENT
    hot = np.abs(grads) >= thr
    clone, split = hot & ~big, (grads >= thr) & big
    src = np.concatenate([np.arange(n0), np.flatnonzero(clone)] + [np.flatnonzero(split)] * SPLIT_N)
    kind = np.array(["kept"] * n0 + ["clone"] * int(clone.sum()) + ["split"] * (SPLIT_N * int(split.sum())))
    keep = np.ones(src.size, bool)
    keep[:n0] = ~split                                           # the split rows' originals go
    sig = 1.0 / (1.0 + np.exp(-opac[:, 0]))
    keep &= ~(sig[src] < MIN_OPACITY)
    margin = min(_rel_margin(smax, PERCENT_DENSE * EXTENT).min(), _rel_margin(np.abs(grads), thr).min(), _rel_margin(sig, MIN_OPACITY).min())
    # the split rows, block after block
    sel = np.flatnonzero(split)
    Z = d[case + "_Z"].astype(np.float64)
    assert Z.shape == (SPLIT_N * sel.size, 3)
    rep = np.concatenate([sel] * SPLIT_N)
    s = np.exp(scaling[rep]) * Z
    new_xyz = np.einsum("nck,nk->nc", _rotation(rot[rep]), s) + xyz[rep]
    new_xyz_abs = np.einsum("nck,nk->nc", _rotation(rot[rep], True), np.abs(s)) + np.abs(xyz[rep])
    new_scaling = np.log(np.exp(scaling[rep]) / float(np.float32(0.8 * SPLIT_N)))
    out = {"src": src[keep], "kind": kind[keep], "margin": float(margin), "n_clone": int(clone.sum()), "n_split": int(split.sum())}
    nan = np.full((src.size, 3), np.nan)
    for name, val in (("xyz", new_xyz), ("xyz_abs", new_xyz_abs), ("scaling", new_scaling), ("scaling_abs", 1.0 + np.abs(new_scaling))):
        a = nan.copy()
        a[kind == "split"] = val
        out[name] = a[keep]
    return out


def reset_opacity_ref(opacity):
    """(float64 value, S_abs) of inverse_sigmoid(min(sigmoid(x), 0.01)) on float32 opacities [n,1]"""
    x = np.asarray(opacity, np.float64)
    p = np.minimum(1.0 / (1.0 + np.exp(-x)), float(np.float32(0.01)))
    v = np.log(p / (1.0 - p))
    return v, 1.0 + np.abs(v)


def ratio(got, ref64, s_abs):
    """|got - ref64| / (2^-24 S_abs) per element"""
    return np.abs(np.asarray(got, np.float64) - ref64) / (U * s_abs)
