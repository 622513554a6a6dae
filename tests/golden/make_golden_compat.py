"""Generates tests/golden/compat_ref.npz by EXECUTING the reference's own utility python on this package's torch-backed `jittor`
subset (gaussianmesh_amd.compat), with the inputs tests/test_compat_jittor.py uses.

Runs only where the reference tree is available: GM_REFERENCE_TREE=<path to the reference checkout> python tests/golden/make_golden_compat.py
(the fixture is committed; the tests never read the reference tree).

Reference code executed:
  utils/general_utils.py  build_scaling_rotation, strip_symmetric, inverse_sigmoid, get_expon_lr_func
  utils/loss_utils.py     ssim, l1_loss, gaussian, mesh_restrict_loss, circumradius
and records which modules (and names) the import block at the top of edit.py asks for: "module" or "module:name,name".
"""
import importlib.util
import os
import sys

import numpy as np

REF = os.environ.get("GM_REFERENCE_TREE", "")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))


def _load(name, relpath):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    assert REF and os.path.isdir(REF), "set GM_REFERENCE_TREE to the reference checkout; the fixture can only be regenerated there"
    import gaussianmesh_amd.compat as compat
    jt = compat.install(operators=True)
    sys.path.insert(0, REF)
    gu = _load("ref_general_utils", "utils/general_utils.py")
    lu = _load("ref_loss_utils", "utils/loss_utils.py")
    out = {}
    # utils: covariance from (scale, quaternion), inverse sigmoid, learning-rate schedule
    rng = np.random.default_rng(0)
    q = rng.standard_normal((7, 4)).astype(np.float32); s = np.exp(rng.standard_normal((7, 3))).astype(np.float32)
    L = gu.build_scaling_rotation(jt.array(s), jt.array(q))
    out.update(utils_q=q, utils_s=s, utils_cov6=gu.strip_symmetric(L @ L.transpose(1, 2)).numpy())
    out["sig_x"] = np.array([0.1, 0.5, 0.9], np.float32)
    out["sig_inv"] = gu.inverse_sigmoid(jt.array(out["sig_x"])).numpy()
    f = gu.get_expon_lr_func(1e-2, 1e-4, max_steps=100)
    out["lr_steps"] = np.arange(0, 101, 5, dtype=np.int64)
    out["lr"] = np.array([f(int(k)) for k in out["lr_steps"]], np.float64)
    # SSIM / L1 / window
    rng = np.random.default_rng(1)
    a = rng.random((3, 40, 36)).astype(np.float32); b = np.clip(a + 0.1 * rng.standard_normal(a.shape), 0, 1).astype(np.float32)
    out.update(ssim_a=a, ssim_b=b, ssim=np.float64(float(lu.ssim(jt.array(a), jt.array(b)))),
               l1=np.float64(float(lu.l1_loss(jt.array(a), jt.array(b)))), window=lu.gaussian(11, 1.5).numpy())
    # mesh restriction loss and circumradius
    rng = np.random.default_rng(5)
    sc = np.exp(rng.standard_normal((50, 3))).astype(np.float32) * 0.3
    p1, p2, p3 = (rng.standard_normal((50, 3)).astype(np.float32) for _ in range(3))
    out.update(mr_scale=sc, mr_p1=p1, mr_p2=p2, mr_p3=p3, mr_weight=np.float64(0.4),
               mr_loss=np.float64(float(lu.mesh_restrict_loss(jt.array(sc), jt.array(p1), jt.array(p2), jt.array(p3), weight=0.4))),
               mr_circumradius=lu.circumradius(jt.array(p1), jt.array(p2), jt.array(p3)).detach().numpy())
    # the import block of edit.py, as the modules and names it imports (not its text)
    import ast
    imports = []
    for n in ast.parse(open(os.path.join(REF, "edit.py")).read()).body:
        if isinstance(n, ast.Import):
            imports += [a.name for a in n.names]
        elif isinstance(n, ast.ImportFrom):
            imports.append("%s:%s" % (n.module, ",".join(a.name for a in n.names)))
    out["edit_imports"] = np.array(imports)
    np.savez_compressed(os.path.join(OUT, "compat_ref.npz"), **out)
    print("wrote compat_ref.npz (%d arrays)" % len(out))


if __name__ == "__main__":
    main()
