"""Inputs of the row tests of the deform / shade kernels (test_deform_ref_host.py, test_gpu_deform_rows.py): a 12 x 8 torus under the
twist-bend frame t = 9 and, per kind, 257 Gaussians bound to it.  A smaller N is the PREFIX [:N] of the same arrays, so a row keeps
its inputs - and must keep its bits - whatever the block it falls in.  Everything is cached and read-only.

  twist    the bound cloud as it comes
  needle   scales times exp(U(ln 1e-3, 0)) per axis (covariances over many orders of magnitude), per-vertex S = Q diag(sigma) Q^T with sigma
           log-uniform in [0.05, 20], and rows (SKEW_ROWS) whose rest covariance is one ulp off bit-symmetry: 9-entry route only
  outside  barycentric weights plus N(0, 0.6), renormalised to sum 1: many negative or above 1
  onehot   weights are rows of the identity (all three corners): the blend must be exact
  clamp    DC coefficients set so that, evaluated at degree D, rows CLAMP_ROWS[D] have r + 0.5 = -0.3, -4 ulp, +4 ulp, +0.3 (ulp = 2^-24)
shs(kind, deg) poisons the inactive coefficients k >= (deg + 1)^2 of every row with NaN.
"""
import functools
import math

import numpy as np

import deform_ref as ref
from gaussianmesh_amd import scenes

KINDS = ("twist", "needle", "outside", "onehot", "clamp")
NS = (1, 63, 64, 65, 128, 129, 255, 256, 257)           # edges of the 64-row fused blocks and of the 256-thread deform / sh_colors blocks
NMAX = 257
CAMPOS = np.array([4.0, 1.0, -3.0], np.float32)
NEAR_ROW = 70                                           # the second camera sits 1e-3 from this row's deformed centre
SKEW_ROWS = (3, 64, 130, 256)
CLAMP_TARGETS = (-0.3, -4.0 * ref.U, 4.0 * ref.U, 0.3)
CLAMP_ROWS = {D: tuple(2 + 5 * D + j for j in range(4)) + tuple(240 + 4 * D + j for j in range(4)) for D in range(4)}
W, H = 96, 64


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def mesh():
    verts, faces = scenes.torus_mesh(12, 8)
    V1, Rv, Sv = scenes.twist_bend_frame(verts, t=9)
    return verts, faces, V1, Rv, Sv


def _table(verts, V1, Rv, Sv):
    """what the device sees of a mesh frame: float32 state [Vm,21] = V1 | R | S, and dV as pack_mesh_state forms it (float32 V1 - verts)"""
    v32, V32 = verts.astype(np.float32), V1.astype(np.float32)
    R32, S32 = Rv.reshape(-1, 9).astype(np.float32), Sv.reshape(-1, 9).astype(np.float32)
    return dict(verts=_ro(v32), state=_ro(np.concatenate([V32, R32, S32], axis=1)), dV=_ro(V32 - v32), Rv=_ro(R32), Sv=_ro(S32))


@functools.lru_cache(maxsize=None)
def case(kind):
    """dict: tri [257,3] int32, w [257,3], cov [257,3,3], pos [257,3], shs [257,16,3] (no poison), opac [257,1]; the table: verts [Vm,3],
    state [Vm,21], dV [Vm,3], Rv / Sv [Vm,9]"""
    verts, faces, V1, Rv, Sv = mesh()
    i = KINDS.index(kind)
    rng = np.random.default_rng(100 + i)
    cl = scenes.bind_cloud_to_mesh(NMAX, verts, faces, seed=20 + i)
    scales, w, shs = cl["scales"], cl["weights"], cl["shs"].copy()
    if kind == "needle":
        scales = (scales * np.exp(rng.uniform(math.log(1e-3), 0.0, size=scales.shape))).astype(np.float32)
        Q = np.linalg.qr(rng.normal(size=(verts.shape[0], 3, 3)))[0]
        sigma = np.exp(rng.uniform(math.log(0.05), math.log(20.0), size=(verts.shape[0], 3)))
        Sv = Q @ (sigma[:, :, None] * Q.transpose(0, 2, 1))
    cov = scenes.cov3d_from_scale_rot(scales, cl["rots"]).astype(np.float32)
    assert np.array_equal(cov, cov.transpose(0, 2, 1))
    if kind == "needle":
        for r in SKEW_ROWS:
            cov[r, 0, 1] = np.nextafter(cov[r, 0, 1], cov[r, 0, 1] + np.float32(1))
    if kind == "outside":
        noise = rng.normal(0.0, 0.6, size=w.shape)
        for _ in range(100):
            weak = np.abs((w + noise).sum(1)) < 0.25                            # (a sum near 0 would renormalise to huge weights)
            if not weak.any():
                break
            noise[weak] = rng.normal(0.0, 0.6, size=(int(weak.sum()), 3))
        w = w + noise
        w = (w / w.sum(1, keepdims=True)).astype(np.float32)
    if kind == "onehot":
        w = np.eye(3, dtype=np.float32)[np.arange(NMAX) % 3]
    c = dict(kind=kind, tri=_ro(cl["tri"].astype(np.int32)), w=_ro(w.astype(np.float32)), cov=_ro(cov), pos=_ro(cl["means"].astype(np.float32)),
             opac=_ro(cl["opac"].astype(np.float32)))
    c.update(_table(verts, V1, Rv, Sv))
    if kind == "clamp":
        # the DC coefficient that puts r + 0.5 on its target at the row's degree: r is C0 S0 plus terms that do not involve S0
        npos, _, Rt = ref.stage1(*ref.stage1_inputs(c), np.float64)
        shs = _clamp_dc(shs, npos, Rt)
    c["shs"] = _ro(shs.astype(np.float32))
    return c


def _clamp_dc(shs, npos, Rt):
    shs = shs.copy()
    c0 = float(np.float32(ref.SH_C0))
    for D, rows in CLAMP_ROWS.items():
        rows = np.array(rows)
        # r without its DC term, from the float64 reference: stage2 returns max(r + 0.5, 0), so a DC of 8 / C0 lifts r clear of the clamp
        lifted = shs[rows].astype(np.float64)
        lifted[:, 0, :] = 8.0 / c0
        rest = ref.stage2(D, npos[rows], Rt[rows], CAMPOS, lifted, np.float64) - 0.5 - c0 * (8.0 / c0)
        target = np.tile(np.array(CLAMP_TARGETS), 2)[:, None]
        shs[rows, 0, :] = ((target - 0.5 - rest) / c0).astype(np.float32)
    return shs


@functools.lru_cache(maxsize=None)
def shs(kind, deg):
    """the case's SH rows [257,16,3] with the coefficients the degree does not use set to NaN"""
    s = case(kind)["shs"].copy()
    s[:, (deg + 1) ** 2:, :] = np.nan
    return _ro(s)


@functools.lru_cache(maxsize=None)
def near_camera(kind):
    npos = ref.stage1_reference(case(kind))["pos"][0]
    return _ro((npos[NEAR_ROW] + 1e-3 * np.array([0.6, 0.0, 0.8])).astype(np.float32))


def colour_cameras(kind):
    return (("far", CAMPOS), ("near", near_camera(kind)))


@functools.lru_cache(maxsize=None)
def frame_camera(k=1):
    return scenes.orbit_camera(k, 7, W, H, radius=6.0)


@functools.lru_cache(maxsize=None)
def identity_table():
    """R = S = I, dV = 0"""
    verts = mesh()[0]
    eye = np.tile(np.eye(3)[None], (verts.shape[0], 1, 1))
    return _table(verts, verts, eye, eye)
