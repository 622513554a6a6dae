"""Host side of baking an edit into a plain cloud: the float64 definition of tests/sh_rotate_ref.py is exact (so the device can be held to
it in test_gpu_sh_rotate.py), gm_sh_rotate's declaration, typing and refusals (before any GPU work), the constant tables of
csrc/gm_shrot.hip against the computation that makes them, and the Python refusals."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from gaussianmesh_amd import _lib

import sh_rotate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gaussianmesh_amd", "csrc", "gm_shrot.hip")


def _matrices(kind, n, rng):
    if kind == "blend":
        return ref.blended_matrices(n, rng)
    if kind == "2R":
        return 2.0 * ref.random_rotations(n, rng)
    return np.zeros((n, 3, 3))


@pytest.mark.parametrize("deg", [1, 2, 3])
@pytest.mark.parametrize("kind", ["blend", "2R", "zero"])
def test_the_reference_is_exact(deg, kind):
    """|SH(d) . c' - SH(A^T d) . c| <= 1e-12 at 500 random unit directions; the zero matrix leaves the DC term alone"""
    rng = np.random.default_rng(10 * deg + len(kind))
    n = (deg + 1) ** 2
    A, c = _matrices(kind, 200, rng), ref.random_coefficients(200, rng)
    out = ref.rotate_sh_ref(c, A, deg)
    d = ref.unit_directions(500, rng)
    err = np.abs(ref.eval_sh(d, out, deg) - ref.eval_sh_rotated(d, A, c, deg)).max()
    print("deg %d %s: max |SH(d).c' - SH(A^T d).c| = %.3g" % (deg, kind, err))
    assert err <= 1e-12
    assert np.array_equal(out[:, n:], c[:, n:])                                   # coefficients beyond the degree: copied
    if kind == "zero":
        assert np.abs(out[:, 0] - c[:, 0]).max() <= 1e-13 and np.abs(out[:, 1:n]).max() <= 1e-13


def test_rotations_keep_each_band_and_identity_keeps_the_row():
    rng = np.random.default_rng(3)
    c = ref.random_coefficients(300, rng)
    c[:, 4:9] = 0.0                                                               # an empty band stays empty
    out = ref.rotate_sh_ref(c, ref.random_rotations(300, rng), 3)
    for lo, hi in ref.BANDS:
        assert np.abs(np.linalg.norm(out[:, lo:hi], axis=1) - np.linalg.norm(c[:, lo:hi], axis=1)).max() <= 1e-12, (lo, hi)
    assert np.abs(out[:, 4:9]).max() <= 1e-12
    assert np.abs(out[:, 1:4] - c[:, 1:4]).max() > 1e-2                           # (and the rows did turn)
    c = ref.random_coefficients(50, rng)
    for deg in (0, 1, 2, 3):
        assert np.abs(ref.rotate_sh_ref(c, np.tile(np.eye(3), (50, 1, 1)), deg) - c).max() <= 1e-13, deg


def test_header_declares_and_lib_types_the_entry_point():
    assert "gm_sh_rotate" in _lib.header_symbols()
    text = open(os.path.join(ROOT, "include", "gmesh_hip.h")).read()
    m = re.search(r"\bint\s+gm_sh_rotate\s*\(([^;]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 7 == len(_lib.SIGNATURES["gm_sh_rotate"][1])
    assert hasattr(_lib.lib(), "gm_sh_rotate")
    assert re.search(r"#define\s+GM_ABI_VERSION\s+3\b", text) and _lib.lib().gm_abi_version() == 3


def test_refuses_before_any_gpu_work():
    l = _lib.lib()
    a, b, r = 1 << 24, 1 << 26, 1 << 28                       # non-null "pointers", far apart: never dereferenced, every call is refused first
    call = lambda N=10, deg=3, M=16, shs=a, rot=r, out=b: l.gm_sh_rotate(N, deg, M, shs, rot, out, None)
    assert call(N=-1) == 1 and b"negative" in l.gm_last_error()
    for deg in (-1, 4, 100):
        assert call(deg=deg) == 1 and b"degree" in l.gm_last_error(), deg
    for deg, M in ((3, 15), (2, 8), (1, 3), (0, 0), (3, 0), (3, -16)):
        assert call(deg=deg, M=M) == 1 and b"coefficients" in l.gm_last_error(), (deg, M)
    for kw in (dict(shs=None), dict(rot=None), dict(out=None)):
        assert call(**kw) == 1 and b"null" in l.gm_last_error(), kw
    n = 10 * 16 * 3 * 4                                       # bytes of the rows
    for out in (a + 4, a - 4, a + n - 4, a - n + 4, a + 192):
        assert call(out=out) == 1 and b"overlaps shs" in l.gm_last_error(), out - a
    for out in (r, r + 4, r + 10 * 36 - 4, r - n + 4):
        assert call(out=out) == 1 and b"overlaps rot" in l.gm_last_error(), out - r
    assert call(N=0) == 0 and call(N=0, shs=None, rot=None, out=None) == 0      # N == 0: nothing launched


def test_the_kernel_file_waits_for_nothing_and_allocates_nothing():
    """gm_sh_rotate's "no workspace, no device allocation, no host wait": its translation unit names no such runtime call"""
    text = open(SRC).read()
    assert "gm_shrot.hip" in open(os.path.join(ROOT, "gaussianmesh_amd", "csrc", "Makefile")).read()
    hits = re.findall(r"hipMemcpy\w*|hipMemset\w*|hip\w*Synchronize|hipMalloc\w*|hipFree\w*|GM_LAUNCH_CHECK", text)
    assert not hits, hits
    assert "#pragma clang fp contract(off)" in text


def _source_table(name, shape):
    text = open(SRC).read()
    m = re.search(r"%s\[%d\]\[%d\]\s*=\s*\{(.*?)\};" % (name, shape[0], shape[1]), text, flags=re.S)
    assert m, name
    vals = [float(v.rstrip("f")) for v in re.findall(r"[-+]?[0-9][0-9.eE+-]*f", m.group(1))]
    return np.array(vals, np.float64).astype(np.float32).reshape(shape)


def _generator():
    spec = importlib.util.spec_from_file_location("sh_rotate_table", os.path.join(ROOT, "tools", "sh_rotate_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_tables_in_the_source_are_the_pseudo_inverse_of_the_basis_at_their_directions():
    D, P, cond = _generator().tables()
    assert cond < 1.2
    src_d, src_p = _source_table("SHROT_DIR", (32, 4)), _source_table("SHROT_PINVT", (32, 16))
    assert np.array_equal(src_d[:, :3], D) and not src_d[:, 3].any()
    assert np.array_equal(src_p, P.T)
    assert np.abs(np.linalg.norm(D.astype(np.float64), axis=1) - 1).max() <= 1e-7
    # the float64 tables invert the basis: P B = I
    assert np.abs(P.astype(np.float64) @ ref.basis(D.astype(np.float64)) - np.eye(16)).max() <= 1e-6


@pytest.mark.parametrize("deg", [1, 2, 3])
def test_the_kernels_method_in_float32_numpy_meets_the_device_bar(deg):
    """csrc/gm_shrot.hip's method restated in float32 numpy (sample at SHROT_DIR, multiply by SHROT_PINVT) against the float64
    reference, under the bar of test_gpu_sh_rotate.py: 1e-5 max(1, |A|_F)^deg max_k |c_k|"""
    rng = np.random.default_rng(deg)
    n = (deg + 1) ** 2
    D, P = _source_table("SHROT_DIR", (32, 4))[:, :3], _source_table("SHROT_PINVT", (32, 16))
    worst = 0.0
    for kind in ("blend", "2R", "zero"):
        A, c = _matrices(kind, 500, rng).astype(np.float32), ref.random_coefficients(500, rng).astype(np.float32)
        dr = np.einsum("nji,kj->nki", A, D).astype(np.float32)
        f = np.einsum("nkj,njc->nkc", ref.basis(dr)[..., :n].astype(np.float32), c[:, :n]).astype(np.float32)
        got = np.einsum("kj,nkc->njc", P[:, :n], f).astype(np.float32)
        exp = ref.rotate_sh_ref(c, A, deg)[:, :n]
        bar = 1e-5 * np.maximum(1.0, np.linalg.norm(A.astype(np.float64), axis=(1, 2))) ** deg * np.abs(c).max(axis=(1, 2))
        worst = max(worst, float((np.abs(got - exp).max(axis=(1, 2)) / bar).max()))
    print("deg %d: worst error / bar = %.3g" % (deg, worst))
    assert worst <= 1.0


def test_python_refusals_and_surface():
    from gaussianmesh_amd import deform, edittool
    with pytest.raises(_lib.GmeshError, match="no CPU path"):
        deform.rotate_sh(torch.zeros((4, 16, 3)), torch.eye(3).expand(4, 3, 3))
    assert hasattr(deform.SingleObjectDeform, "bake")
    for cls in (edittool.SingleObjectDeform, edittool.ObjectVisualTool, edittool.SceneVisualTool):
        assert hasattr(cls, "save_baked"), cls
    with pytest.raises(ValueError, match="no object named"):
        edittool.ObjectVisualTool(device="cpu").save_baked("unused.ply", name="nobody")
    with pytest.raises(ValueError, match="nothing to save"):
        edittool.ObjectVisualTool(device="cpu").save_baked("unused.ply")
