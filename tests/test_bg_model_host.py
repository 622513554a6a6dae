"""Host side of the background stage: the new C entry points (declared, typed, validated before any GPU work), the PLY round trip of
bg_model.PlainGaussians, and its densification against the reference's GaussianModel (tests/golden/bg_densify.npz)."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gaussianmesh_amd import _lib
from gaussianmesh_amd import io as gio
from gaussianmesh_amd.bg_model import PlainGaussians
from gaussianmesh_amd.bg_train import BG_DEFAULT_OPT

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
    g = PlainGaussians(3, device="cpu")
    t = lambda k: torch.as_tensor(d["%s_%s" % (prefix, k)])
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
