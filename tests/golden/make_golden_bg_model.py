"""Generates tests/golden/bg_densify.npz by EXECUTING the reference's plain GaussianModel (scene/gaussian_model.py) on this
package's torch-backed `jittor` subset (gaussianmesh_amd.compat), as make_golden_model.py does for the mesh-bound model.

Runs only where the reference tree is available, GM_REFERENCE_TREE=<its path> (the fixture is committed; the tests never read it).
jt.normal - the only random draw, densify_and_split's position samples - is pinned: it returns mean + std * Z with Z drawn here
from a seeded numpy generator and recorded ("<case>_Z"), so a test can hand the same standard-normal samples to
bg_model.PlainGaussians.densify_and_split.  What the fixture pins is the reference's ORDER of rows and optimizer-state edits:
clone before split, the split's zero-padded gradient, the 1/(0.8 N) scale, the opacity-only prune, reset_opacity's zeroed moments.

Reference code executed (file:line):
  scene/gaussian_model.py:172-190   training_setup (+ two Adam steps of a synthetic loss, so that the moments are not zero)
  scene/gaussian_model.py:298-421   replace_tensor_to_optimizer, _prune_optimizer, prune_points, cat_tensors_to_optimizer,
                                    densification_postfix, densify_and_split, densify_and_clone, densify_and_prune
  scene/gaussian_model.py:246-251   reset_opacity
  scene/gaussian_model.py:423-427   add_densification_stats
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = os.environ.get("GM_REFERENCE_TREE", "")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


def _load(name, relpath):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_model(jt, gm, rng, n):
    g = gm.GaussianModel(3)
    f = lambda *s: jt.array(rng.normal(size=s).astype(np.float32))
    g._xyz = f(n, 3)
    g._features_dc = f(n, 1, 3)
    g._features_rest = f(n, 15, 3) * 0.2
    g._scaling = jt.log(jt.array(rng.uniform(0.002, 0.03, (n, 3)).astype(np.float32)))
    g._rotation = f(n, 4)
    g._opacity = f(n, 1) * 3.0
    g.max_radii2D = jt.zeros((n,))
    args = types.SimpleNamespace(percent_dense=0.01, position_lr_init=1.6e-4, position_lr_final=1.6e-6, position_lr_delay_mult=0.01,
                                 position_lr_max_steps=30000, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001)
    g.spatial_lr_scale = 1.0
    g.training_setup(args)
    for it in range(2):
        w = jt.array(rng.normal(size=(n, 3)).astype(np.float32))
        loss = ((g.get_xyz * w).sum() + (g.get_opacity ** 2).sum() + (g.get_scaling * w).sum() + (g.get_rotation ** 2 * w[:, :1]).sum() +
                (g.get_features ** 2).sum() * 0.1)
        g.optimizer.backward(loss)
        g.update_learning_rate(it + 1)
        g.optimizer.step(); g.optimizer.zero_grad()
    return g


def snapshot(g, prefix, out):
    t = lambda x: np.ascontiguousarray(x.detach().cpu().numpy())
    for grp in g.optimizer.param_groups:
        out["%s_p_%s" % (prefix, grp["name"])] = t(grp["params"][0])
        out["%s_m_%s" % (prefix, grp["name"])] = t(grp["m"][0])
        out["%s_v_%s" % (prefix, grp["name"])] = t(grp["values"][0])
    for b in ("max_radii2D", "xyz_gradient_accum", "denom"):
        out["%s_b_%s" % (prefix, b)] = t(getattr(g, b))


def main():
    assert os.path.isdir(REF), "set GM_REFERENCE_TREE to the reference checkout; the fixture can only be regenerated there"
    import gaussianmesh_amd.compat as compat
    jt = compat.install(force=True, operators=True)
    for name in ("plyfile",):
        m = types.ModuleType(name)
        m.PlyData = m.PlyElement = None
        sys.modules[name] = m
    pkg = types.ModuleType("scene"); pkg.__path__ = [os.path.join(REF, "scene")]      # keep scene/__init__.py (dataset readers) out
    sys.modules["scene"] = pkg
    knn = types.ModuleType("scene.simple_knn"); knn.distCUDA2 = None                    # (create_from_pcd only; not executed)
    sys.modules["scene.simple_knn"] = knn
    sys.path.insert(0, REF)
    gm = _load("ref_gaussian_model", "scene/gaussian_model.py")

    zs = {}
    rng_z = np.random.default_rng(11)

    def pinned_normal(mean, std, *a, **k):
        z = rng_z.normal(size=tuple(std.shape)).astype(np.float32)
        zs["last"] = z
        return mean + std * jt.array(z)
    jt.normal = pinned_normal
    gm.jt.normal = pinned_normal

    t = lambda x: np.ascontiguousarray(x.detach().cpu().numpy())
    out = {}
    rng = np.random.default_rng(20261015)
    # A, B: densify_and_prune (clone + split + opacity prune) at two thresholds; C: prune_points then reset_opacity
    for case, n, q, vis in (("A", 64, 0.5, 0.8), ("B", 96, 0.25, 1.0)):
        g = build_model(jt, gm, rng, n)
        with jt.no_grad():
            g.add_densification_stats(jt.array(rng.normal(size=(n, 3)).astype(np.float32) * 1e-3), jt.array(rng.random(n) < vis))
            g.max_radii2D = jt.array((rng.random(n) * 30).astype(np.float32))
        snapshot(g, case + "0", out)
        grads = t(g.xyz_gradient_accum) / np.maximum(t(g.denom), 1)
        thr = float(np.quantile(grads, q))
        out[case + "_threshold"] = np.float64(thr)
        zs.pop("last", None)
        with jt.no_grad():
            g.densify_and_prune(thr, 0.005, 1.0, None)
        out[case + "_Z"] = zs.get("last", np.zeros((0, 3), np.float32))
        snapshot(g, case + "1", out)
    g = build_model(jt, gm, rng, 48)
    n = 48
    with jt.no_grad():
        g.add_densification_stats(jt.array(rng.normal(size=(n, 3)).astype(np.float32)), jt.array(rng.random(n) < 0.5))
        g.max_radii2D = jt.array((rng.random(n) * 30).astype(np.float32))
    snapshot(g, "C0", out)
    mask = rng.random(n) < 0.3
    out["C_mask"] = mask
    with jt.no_grad():
        g.prune_points(jt.array(mask))
    snapshot(g, "C1", out)
    with jt.no_grad():
        g.reset_opacity()
    snapshot(g, "C2", out)
    np.savez_compressed(os.path.join(OUT, "bg_densify.npz"), **out)
    print("wrote bg_densify.npz (%d arrays; A: %d -> %d rows, B: %d -> %d rows)" % (
        len(out), out["A0_p_xyz"].shape[0], out["A1_p_xyz"].shape[0], out["B0_p_xyz"].shape[0], out["B1_p_xyz"].shape[0]))


if __name__ == "__main__":
    main()
