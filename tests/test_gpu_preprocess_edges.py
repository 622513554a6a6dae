"""-m gpu: the preprocess kernels (gm_pre_body.h pre_project / cov2d_T, the SH colour body, gm_preprocess.hip preprocess_bwd_body) on the
edge scene of tests/preprocess_edge_scene.py: Gaussians ON the near plane, the frustum clamp, the colour clamp, the empty tile rectangle,
the 0.1 floor of the radius and the denom2inv == 0 guard.

Forward: bit-identical to the C oracle (helpers._check_geometry), both input modes, D = 0 and 3, with and without tile culling.
Backward, stage level: HIP's own blend-stage gradients (dL/dmean2D, dL/dconic, dL/dcolour) go through the C oracle's preprocess backward
and through the float64 stage reference with float32 decisions (oracle/torch_dense.py stage_vjp), so blend noise cancels; every visible
row of every tensor must satisfy  err_hip <= 2 err_orc + floor  (both errors against the float64 reference, relative to the row's largest
entry; floor: the oracle's own 99.9th-percentile error on ordinary rows, measured on the CPU by tests/test_preprocess_edges_host.py), with the float32
conic -> cov2D block (gm_debug_backward_cov2d_float32) and with the binary64 block of the product.  Culled rows are written and zero.
The host test shows that this gate rejects the wrong kernels (clamp mask ignored, clamp decided one ulp off, ...) that the tensor max-norm
gate lets through on this scene.  Measured on the MI355X: worst err_hip / (2 err_orc + floor) 0.43 with the float32 block, 0.52 with the
binary64 block (NOTEBOOK.md "Preprocess kernels at their decision edges").
"""
import ctypes as C

import numpy as np
import pytest
import torch

import preprocess_edge_scene as es
from helpers import _check_geometry, _check_per_gaussian

pytestmark = pytest.mark.gpu

BG = np.array([0.2, 0.5, 0.7], np.float32)
_FW = {}


@pytest.fixture(autouse=True)
def _default_emission_policy():
    from gaussianmesh_amd import rasterizer
    rasterizer.set_default_emission_policy(2)
    yield
    rasterizer.set_default_emission_policy(2)


def _scene(M=16):
    sc, cam, groups = es.cached_edge_scene()
    if M != 16:
        from test_gpu_sh_layouts import _rows
        sc = dict(sc, shs=_rows(sc["shs"], M))
    return sc, cam, groups


def _oracle_forward(oracle, D, pre_cov, pre_col, M=16):
    """oracle.forward_full of the edge scene, once per configuration (shared, never modified)"""
    key = (D, pre_cov, pre_col, M)
    if key not in _FW:
        sc, cam, _ = _scene(M)
        _FW[key] = oracle.forward_full(sc, cam, BG, D=D, use_precomp_cov=pre_cov, use_precomp_color=pre_col)
    return _FW[key]


@pytest.mark.parametrize("tile_cull", [False, True], ids=["reference_lists", "tile_cull"])
@pytest.mark.parametrize("D,pre_cov,pre_col", [(0, False, False), (3, False, False), (0, True, True), (3, True, False)])
def test_forward_on_the_edge_scene_is_bit_identical_to_the_oracle(oracle, D, pre_cov, pre_col, tile_cull):
    from gpu_utils import forward_state
    sc, cam, groups = _scene()
    fw = _oracle_forward(oracle, D, pre_cov, pre_col)
    st = forward_state(sc, cam, BG, D=D, use_precomp_cov=pre_cov, use_precomp_color=pre_col, tile_cull=tile_cull)
    assert (fw["geo"]["radii"][groups["culled_block"]] == 0).all() and (fw["geo"]["radii"] > 0).sum() > 250
    if tile_cull:                                   # fewer instances than the reference emits: radii and per-Gaussian geometry
        _check_per_gaussian(st, fw["geo"], pre_col)
        assert 0 < st["R"] <= fw["bins"]["R"]
    else:
        _check_geometry(oracle, st, fw, sc, pre_col)


def _float32_block(on):
    from gaussianmesh_amd import _lib
    C.CDLL(_lib.lib()._name).gm_debug_backward_cov2d_float32(int(on))


def _operand(sc, layout):
    from test_gpu_sh_layouts import _operand as op
    return None if layout is None else op(sc["shs"], aligned=layout != "offset4")


# (D, pre_cov, pre_col, M, layout of the SH operand): M = 16 aligned takes the staged / DMA kernel (64-row blocks: nine full, one of 24),
# everything else the generic one (256-row blocks: two full - one of them all culled - and one of 88)
BACKWARD_CASES = ([(D, pre_cov, False, 16, "aligned") for pre_cov in (False, True) for D in (0, 1, 2, 3)]
                  + [(3, False, False, 16, "offset4"), (3, False, False, 20, "aligned"), (3, False, True, 16, None)])


@pytest.mark.parametrize("D,pre_cov,pre_col,M,layout", BACKWARD_CASES)
def test_backward_stage_per_row_against_float64_with_float32_decisions(oracle, D, pre_cov, pre_col, M, layout):
    from gpu_utils import stage_grads_gpu
    from poison import poisoned
    sc, cam, groups = _scene(M)
    fw = _oracle_forward(oracle, D, pre_cov, pre_col, M)
    geo = fw["geo"]
    vis = geo["radii"] > 0
    dec = es.decisions(sc, cam, geo, pre_cov)
    dpix = np.random.default_rng(1).normal(size=(3, es.H, es.W)).astype(np.float32)
    shs = None if pre_col else _operand(sc, layout)
    problems = []
    for on in (1, 0):
        what = "D=%d cov=%s col=%s M=%d %s, %s block" % (D, pre_cov, pre_col, M, layout, "float32" if on else "binary64")
        _float32_block(on)
        try:
            with poisoned(0xFF):                    # every gradient output starts as NaN: a row the kernel skips stays NaN
                g = stage_grads_gpu(sc, cam, BG, dpix, D, pre_cov, pre_col, shs=shs)
        finally:
            _float32_block(0)
        assert np.array_equal(g["radii"], geo["radii"]), what
        ins = (g["dmean2D"], g["dconic"].reshape(-1, 4), g["dcolor"])
        for k, x in zip(("dmean2D", "dconic", "dcolor"), ins):
            assert np.isfinite(x).all() and (x[~vis] == 0).all(), (what, k)
        assert np.isfinite(g["dopacity"]).all() and (g["dopacity"].reshape(-1)[~vis] == 0).all(), what
        live = np.abs(ins[1]).max(1) > 0
        assert (live & vis).sum() >= 0.9 * vis.sum(), what                    # the rows are reached: the gate is not vacuous
        ref = es.stage_reference(sc, cam, dec, *ins, D, pre_cov, pre_col)
        orc = es.stage_oracle(oracle, sc, cam, geo, *ins, D, pre_cov, pre_col)
        got = dict(means=g["dmean3D"])
        got.update(dict(cov=g["dcov3D"]) if pre_cov else dict(scales=g["dscale"], rots=g["drot"]))
        if not pre_col:
            got["shs"] = g["dsh"]
            assert g["dsh"].shape == (es.P, M, 3) and (g["dsh"][:, (D + 1) ** 2:] == 0).all(), what
        bad, worst = es.gate_failures(got, orc, ref, vis, groups)
        print("%s: worst err_hip / (2 err_orc + floor) per tensor: %s" % (what, "  ".join("%s %.3g" % kv for kv in worst.items() if isinstance(kv[0], str))))
        print("   per group: " + "  ".join("%s/%s %.2g" % (k[0], k[1], v) for k, v in worst.items() if not isinstance(k, str)))
        problems += [(what,) + b for b in bad[:20]]
        # rows whose gradient must be EXACTLY zero
        if not pre_col:
            cl = geo["clamped"].astype(bool) & vis[:, None]
            assert cl.sum() >= 20 and all((g["dsh"][cl[:, ch], :, ch] == 0).all() for ch in range(3)), what
        ovf = dec["overflow"] & vis
        assert ovf.sum() >= 3 and all((got[k][ovf] == 0).all() for k in (("cov",) if pre_cov else ("scales", "rots"))), what
    assert not problems, problems


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("D", [1, 3])
def test_backward_routes_agree_bit_for_bit_on_the_edge_scene(D):
    """dL/dpix on two pixels (no sum depends on its order): the staged / DMA kernel (M = 16 aligned), the generic kernel (M = 16 at a 4-byte
    offset, M = 20) and the staged kernel with the fused SH Adam step (gm_backward_sh_step) give the same bits in every output they share.
    (gm_backward_sh_step refuses a call without moments - tests/test_abi.py - so the step runs, on a copy of the rows.)"""
    from gpu_utils import stage_grads_gpu
    from gaussianmesh_amd import rasterizer as R
    from test_gpu_sh_layouts import _two_pixel_gradient
    sc, cam, _ = _scene()
    dpix = _two_pixel_gradient(D, es.W, es.H)
    base = stage_grads_gpu(sc, cam, BG, dpix, D, False, False, shs=_operand(sc, "aligned"))
    assert np.abs(base["dmean3D"]).max() > 0 and np.abs(base["dsh"]).max() > 0
    shared = ("radii", "dmean2D", "dcolor", "dopacity", "dmean3D", "dcov3D", "dscale", "drot", "dconic")
    for M, layout in ((16, "offset4"), (20, "aligned")):
        scM = _scene(M)[0]
        g = stage_grads_gpu(scM, cam, BG, dpix, D, False, False, shs=_operand(scM, layout))
        for k in shared:
            assert np.array_equal(_bits(g[k]), _bits(base[k])), (M, layout, k)
        assert np.array_equal(_bits(g["dsh"][:, :16]), _bits(base["dsh"])) and (g["dsh"][:, 16:] == 0).all(), (M, layout)
    p = _operand(sc, "aligned")
    ss = R.ShStep(p, torch.zeros_like(p), torch.zeros_like(p), 2.5e-3, 1.25e-4, (0.9, 0.999), 1e-15, 1)
    g = stage_grads_gpu(sc, cam, BG, dpix, D, False, False, shs=p, sh_step=ss)
    assert ss.applied and g["dsh"] is None
    for k in ("radii", "dmean2D", "dopacity", "dmean3D", "dscale", "drot"):
        assert np.array_equal(_bits(g[k]), _bits(base[k])), ("sh_step", k)
    moved = np.abs(p.cpu().numpy() - sc["shs"]).max(axis=(1, 2)) > 0              # the step ran, and only on rows that have a gradient
    assert moved.any() and not moved[np.abs(base["dsh"]).max(axis=(1, 2)) == 0].any()
