"""Host side of the background stage: the new C entry points (declared, typed, validated before any GPU work), the PLY round trip of
bg_model.PlainGaussians, and its densification against the reference's GaussianModel (tests/golden/bg_densify.npz)."""
import os
import re

import numpy as np
import pytest
import torch

import bg_topology_ref as topo
from gaussianmesh_amd import _lib
from gaussianmesh_amd import io as gio
from gaussianmesh_amd.bg_model import PlainGaussians

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "bg_densify.npz")


def _declared_args(name, ret="int"):
    text = open(os.path.join(ROOT, "include", "gmesh_hip.h")).read()
    m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, name), text)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name, ret, n", [("gm_plain_activate_fwd", "int", 12), ("gm_plain_activate_bwd", "int", 15),
                                          ("gm_knn_nearest", "int", 9), ("gm_knn_nearest_workspace_bytes", "size_t", 2)])
def test_header_declares_and_lib_types_the_new_entry_points(name, ret, n):
    args = _declared_args(name, ret)
    assert name in _lib.header_symbols()
    assert len(args) == n
    assert len(_lib.SIGNATURES[name][1]) == n
    assert hasattr(_lib.lib(), name)


def test_abi_version_unchanged():
    assert _lib.lib().gm_abi_version() == 3


def test_knn_nearest_refuses_before_any_gpu_work():
    l = _lib.lib()
    one = 1 << 24
    assert l.gm_knn_nearest(10, one, 0, one, one, one, one, 1 << 20, None) == 1 and b"Pr == 0" in l.gm_last_error()
    assert l.gm_knn_nearest(-1, one, 5, one, one, one, one, 1 << 20, None) == 1
    assert l.gm_knn_nearest(10, None, 5, one, one, one, one, 1 << 20, None) == 1 and b"null" in l.gm_last_error()
    need = l.gm_knn_nearest_workspace_bytes(10, 5)
    assert need > 0
    assert l.gm_knn_nearest(10, one, 5, one, one, one, one, need - 1, None) == 3 and b"workspace" in l.gm_last_error()
    assert l.gm_knn_nearest(0, None, 5, None, None, None, None, 0, None) == 0          # nothing to do
    # the sort's block count is not monotonic in n: the workspace covers whichever set needs more
    assert l.gm_knn_nearest_workspace_bytes(1600000, 1500000) >= l.gm_knn_nearest_workspace_bytes(1500000, 1500000)


def test_knn_nearest_python_refusals():
    from gaussianmesh_amd.simple_knn import knn_nearest
    with pytest.raises(ValueError, match="empty"):
        knn_nearest(torch.zeros((4, 3)), torch.zeros((0, 3)))
    with pytest.raises(ValueError, match=r"\[P,3\]"):
        knn_nearest(torch.zeros((4, 2)), torch.zeros((3, 3)))
    with pytest.raises(_lib.GmeshError):
        knn_nearest(torch.zeros((4, 3)), torch.zeros((3, 3)))                         # CPU tensors: no CPU path


def test_plain_activate_refuses_before_any_gpu_work():
    l = _lib.lib()
    a = 1 << 24
    fwd = lambda N=10, row0=0, cap=10, rot=a, orot=a: l.gm_plain_activate_fwd(N, a, a, rot, a, a, a, orot, a, row0, cap, None)
    assert fwd(cap=9) == 1 and b"capacity" in l.gm_last_error()
    assert fwd(row0=5, cap=14) == 1
    assert fwd(N=-1) == 1
    assert fwd(rot=a + 4) == 1 and b"aligned" in l.gm_last_error()
    assert fwd(orot=a + 8) == 1
    assert l.gm_plain_activate_fwd(10, a, None, a, a, a, a, a, a, 0, 10, None) == 1 and b"null" in l.gm_last_error()
    assert fwd(N=0, cap=0) == 0
    bwd = lambda N=10, row0=0, cap=10, grot=a: l.gm_plain_activate_bwd(N, a, a, a, None, None, grot, None, row0, cap, a, a, a, a, None)
    assert bwd(cap=5) == 1 and b"capacity" in l.gm_last_error()
    assert bwd(grot=a + 4) == 1 and b"aligned" in l.gm_last_error()
    assert l.gm_plain_activate_bwd(10, a, a, a, None, None, None, None, 0, 10, a, None, a, a, None) == 1


def test_plain_gaussians_has_no_activated():
    assert not hasattr(PlainGaussians(3, device="cpu"), "activated")


def test_ply_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    N = 37
    g = PlainGaussians(3, device="cpu")
    r = lambda *s: torch.as_tensor(rng.normal(size=s).astype(np.float32))
    g._set_params(r(N, 3), r(N, 16, 3), r(N, 3), r(N, 4), r(N, 1))
    p = str(tmp_path / "pc" / "point_cloud.ply")
    g.save_ply(p)
    m = gio.load_plain_gaussians(p)
    assert np.array_equal(m["xyz"], g._xyz.detach().numpy())
    assert np.array_equal(m["features_dc"], g._features_dc.detach().numpy())
    assert np.array_equal(m["features_rest"], g._features_rest.detach().numpy())
    names, _ = gio.read_ply(p)
    assert names[:9] == ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] and names[-8:] == [
        "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    h = PlainGaussians(3, device="cpu")
    h.load_ply(p)
    for a in ("_xyz", "_features", "_scaling", "_rotation", "_opacity"):
        assert torch.equal(getattr(h, a), getattr(g, a)), a
    assert h.active_sh_degree == 3 and h._opacity.shape == (N, 1)


# ---- densification against the reference (tests/golden/make_golden_bg_model.py)
def _model_from(d, prefix):
    return topo.model_from(d, prefix, "cpu")


def _assert_matches(g, d, prefix, atol=0.0):
    t = lambda k: d["%s_%s" % (prefix, k)]
    grp = {x["name"]: x for x in g.optimizer.param_groups}
    for name in ("xyz", "opacity", "scaling", "rotation"):
        for slot, key in (("params", "p"), ("m", "m"), ("values", "v")):
            np.testing.assert_allclose(grp[name][slot][0].detach().numpy(), t("%s_%s" % (key, name)), rtol=0, atol=atol, err_msg=prefix + name + key)
    sh = grp[PlainGaussians.SH_GROUP]
    for slot, key in (("params", "p"), ("m", "m"), ("values", "v")):
        v = sh[slot][0].detach().numpy()
        assert np.array_equal(v[:, :1], t(key + "_f_dc")) and np.array_equal(v[:, 1:], t(key + "_f_rest")), prefix + key
    for b in ("max_radii2D", "xyz_gradient_accum", "denom"):
        assert np.array_equal(getattr(g, b).numpy(), t("b_" + b)), prefix + b
    assert g._xyz is grp["xyz"]["params"][0] and g._features is sh["params"][0]


@pytest.mark.parametrize("case", ["A", "B"])
def test_densify_and_prune_matches_reference(case):
    d = np.load(GOLD)
    g = _model_from(d, case + "0")
    n0 = g._xyz.shape[0]
    g.densify_and_prune(float(d[case + "_threshold"]), 0.005, 1.0, None, samples=torch.as_tensor(d[case + "_Z"]))
    assert g._xyz.shape[0] == d[case + "1_p_xyz"].shape[0] != n0
    _assert_matches(g, d, case + "1")
    assert g.screenspace_points.shape == (g._xyz.shape[0], 3)


def test_prune_points_and_reset_opacity_match_reference():
    d = np.load(GOLD)
    g = _model_from(d, "C0")
    g.prune_points(torch.as_tensor(d["C_mask"]))
    _assert_matches(g, d, "C1")
    g.reset_opacity()
    _assert_matches(g, d, "C2", atol=0.0)


# ---- the computed rows against a float64 restatement (bg_topology_ref.py): the bound test_gpu_bg_topology.py holds the device to
def _src_rows_pruned_by_opacity(plan, d, case):
    n0 = d[case + "0_p_xyz"].shape[0]
    return n0 + plan["n_clone"] + topo.SPLIT_N * plan["n_split"] - plan["n_split"] - plan["src"].size


@pytest.mark.parametrize("case", ["A", "B"])
def test_split_rows_against_the_float64_restatement(case):
    """Measured here (x86-64, CPU torch): the worst |value - float64| / (2^-24 S_abs) over the split rows of A and B is 1.10 for xyz and
    0.93 for scaling; asserted: under half of bg_topology_ref.FACTOR = 8, so the device test's bound stands as the issue states it."""
    d = np.load(GOLD)
    plan = topo.densify_plan(d, case)
    assert plan["margin"] >= topo.MARGIN, plan["margin"]        # no decision within 1e-4 of its threshold: an ulp cannot flip a selection
    assert plan["n_split"] > 0 and (plan["n_clone"] > 0 or case == "A")       # (A: 32 rows split, none cloned; B: 69 split, 3 cloned)
    assert _src_rows_pruned_by_opacity(plan, d, case) > 0
    g = _model_from(d, case + "0")
    src0 = {k: getattr(g, k).detach().numpy().copy() for k in ("_xyz", "_features", "_scaling", "_rotation", "_opacity")}
    g.densify_and_prune(float(d[case + "_threshold"]), 0.005, 1.0, None, samples=torch.as_tensor(d[case + "_Z"]))
    src, split = plan["src"], plan["kind"] == "split"
    assert g._xyz.shape[0] == src.size
    for k in ("_features", "_rotation", "_opacity"):            # copied on every row
        assert np.array_equal(getattr(g, k).detach().numpy(), src0[k][src]), k
    for k, name in (("_xyz", "xyz"), ("_scaling", "scaling")):
        got = getattr(g, k).detach().numpy()
        assert np.array_equal(got[~split], src0[k][src][~split]), k
        r = topo.ratio(got[split], plan[name][split], plan[name + "_abs"][split])
        print("CPU torch against float64, case %s, split rows' %s: worst %.3f units of 2^-24 S_abs (bound %g)" % (case, name, r.max(), topo.FACTOR))
        assert r.max() <= topo.FACTOR / 2, (k, float(r.max()))


def test_reset_opacity_against_the_float64_restatement():
    """Measured here: 0.24 units of 2^-24 S_abs at worst; asserted: under half of bg_topology_ref.FACTOR"""
    d = np.load(GOLD)
    g = _model_from(d, "C0")
    g.prune_points(torch.as_tensor(d["C_mask"]))
    x = g._opacity.detach().numpy().copy()
    g.reset_opacity()
    want, s_abs = topo.reset_opacity_ref(x)
    r = topo.ratio(g._opacity.detach().numpy(), want, s_abs)
    print("CPU torch against float64, reset opacities: worst %.3f units of 2^-24 S_abs (bound %g)" % (r.max(), topo.FACTOR))
    assert r.max() <= topo.FACTOR / 2
    assert (x > -4.0).any() and (x < -4.7).any()                 # both sides of logit(0.01) = -4.595
