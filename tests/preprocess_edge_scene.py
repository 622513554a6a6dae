"""A scene that puts Gaussians ON the discrete decisions of the preprocess kernels (gm_pre_body.h pre_project / cov2d_T, the SH colour
body, gm_preprocess.hip preprocess_bwd_body), and the float32 restatement of those decisions.  numpy only, deterministic.

edge_scene() -> (scene, cam, groups); groups maps a name to row indices:
  near      on the optical axis at view depths 0.2f + {0, +-1, +-2, +-8} ulp, 0.19 and 0.21          (`pv.z <= 0.2f`)
  clamp_x   t.x / t.z at +-lim {1 - 1e-6, 1, 1 + 1e-6, 1.2, 1.6, 2}, lim = 1.3 tan(fov/2); of the rows at lim itself one is nudged by a few
  clamp_y   ulps until float32 and float64 disagree about the clamp and one until the float32 quotient EQUALS the float32 limit
  clamp_xy  both axes at once, every sign combination                                                 (xmul / ymul, the clamped t in dtz)
  colour    SH_C0 dc + 0.5 at 0, one ulp either side and far either side, in one, two and three channels (the clamp bits; the other
            coefficients of the rows at the threshold are zero, so the bracket holds at every degree)
  rect      centres outside each image border at distances around radius and radius + 15 px          (the empty tile rectangle)
  iso       isotropic on-axis splats, zero scales included, and a sweep of slightly anisotropic ones  (`fmaxf(0.1f, mid*mid - det)`)
  overflow  scales ~1e4 (denom * denom = inf, denom2inv == 0) and ~3.3e3 (a factor 10 in denom on the safe side); radius < 2^24
  nonunit   quaternions of norm 0.5 and 2 (the rasterizer does not normalise)
  ordinary  a background of ordinary rows
  culled_block  rows 256..511: a whole 256-row block (four 64-row blocks) of culled Gaussians
P = 600 = 2 * 256 + 88 = 9 * 64 + 24: a full block, a culled block and a partial last block for both block widths.
Rows are built in view space and mapped back through the inverse view matrix in float64; the camera sits next to the world origin so that
a float32 world coordinate of a near-plane row resolves one ulp of 0.2.
"""
import numpy as np

from gaussianmesh_amd import scenes

F = np.float32
W, H = 64, 48
P = 600
SH_C0 = 0.28209479177387814
CLAMP_FACTORS = (1.0 - 1e-6, 1.0, 1.0 + 1e-6, 1.2, 1.6, 2.0)


def camera():
    return scenes.look_at_camera((-0.03, -0.02, -0.05), (1.0, 0.35, 2.0), W, H)


# ---------------------------------------------------------------------------------------------- float32 restatement of the decisions
def view_f32(means, view):
    """xform4x3 (gm_pre_body.h) in numpy float32: one rounding per operation, the kernel's association order."""
    v = np.asarray(view, F).reshape(-1)
    m = np.asarray(means, F)
    x, y, z = m[:, 0], m[:, 1], m[:, 2]
    return [((v[k] * x + v[4 + k] * y) + v[8 + k] * z) + v[12 + k] for k in range(3)]


def decisions_f32(means, cam, cov3D=None):
    """The clamp decisions of cov2d_T and (with the float32 cov3D rows) the denom2inv == 0 decision of the backward, statement by
    statement in numpy float32.  Returns dict(depth, txtz, tytz, limx, limy, inx, iny[, overflow, mid2_minus_det])."""
    with np.errstate(all="ignore"):
        v = np.asarray(cam["view"], F).reshape(-1)
        t0, t1, t2 = view_f32(means, cam["view"])
        tanx, tany = F(cam["tanx"]), F(cam["tany"])
        limx, limy = F(1.3) * tanx, F(1.3) * tany
        txtz, tytz = t0 / t2, t1 / t2
        out = dict(depth=t2, txtz=txtz, tytz=tytz, limx=limx, limy=limy,
                   inx=~((txtz < -limx) | (txtz > limx)), iny=~((tytz < -limy) | (tytz > limy)))
        if cov3D is None:
            return out
        fx, fy = F(cam["W"]) / (F(2.0) * tanx), F(cam["H"]) / (F(2.0) * tany)
        tx = np.minimum(limx, np.maximum(-limx, txtz)) * t2
        ty = np.minimum(limy, np.maximum(-limy, tytz)) * t2
        j00, j02 = fx / t2, -(fx * tx) / (t2 * t2)
        j11, j12 = fy / t2, -(fy * ty) / (t2 * t2)
        T0 = [(v[4 * i] * j00 + v[4 * i + 1] * F(0)) + v[4 * i + 2] * j02 for i in range(3)]
        T1 = [(v[4 * i] * F(0) + v[4 * i + 1] * j11) + v[4 * i + 2] * j12 for i in range(3)]
        c = np.asarray(cov3D, F)
        V = [c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]]
        A0 = [(T0[0] * V[k] + T0[1] * V[3 + k]) + T0[2] * V[6 + k] for k in range(3)]
        A1 = [(T1[0] * V[k] + T1[1] * V[3 + k]) + T1[2] * V[6 + k] for k in range(3)]
        a = (A0[0] * T0[0] + A0[1] * T0[1]) + A0[2] * T0[2]
        b = (A1[0] * T0[0] + A1[1] * T0[1]) + A1[2] * T0[2]
        cc = (A1[0] * T1[0] + A1[1] * T1[1]) + A1[2] * T1[2]
        a = a + F(0.3); cc = cc + F(0.3)
        denom = a * cc - b * b
        out["overflow"] = (F(1.0) / ((denom * denom) + F(0.0000001))) == 0
        mid = F(0.5) * (a + cc)
        out["mid2_minus_det"] = mid * mid - denom
        out["denom"] = denom
    return out


def decisions_f64(means, cam):
    """The clamp decisions in float64 arithmetic on the same float32 inputs."""
    m = np.asarray(means, np.float64)
    t = np.concatenate([m, np.ones((m.shape[0], 1))], 1) @ np.asarray(cam["view"], np.float64)
    rx, ry = t[:, 0] / t[:, 2], t[:, 1] / t[:, 2]
    return dict(depth=t[:, 2], inx=np.abs(rx) <= 1.3 * cam["tanx"], iny=np.abs(ry) <= 1.3 * cam["tany"])


def cov3d_unnormalised(scales, rots):
    """Sigma = R diag(s)^2 R^T with the quaternion NOT normalised (forward.cu:118-152), float64 -> the six float32 entries."""
    q = np.asarray(rots, np.float64); s = np.asarray(scales, np.float64)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    L = R * s[:, None, :]
    return scenes.strip_symmetric(L @ L.transpose(0, 2, 1))


# ---------------------------------------------------------------------------------------------- builder
def _nudges(p, n=6):
    """Every point whose float32 coordinates lie within n ulps of p's: [(2n+1)^3, 3], nearest first."""
    axes = []
    for k in range(3):
        up = [F(p[k])]; dn = [F(p[k])]
        for _ in range(n):
            up.append(np.nextafter(up[-1], F(np.inf))); dn.append(np.nextafter(dn[-1], F(-np.inf)))
        axes.append(np.array(dn[:0:-1] + up, F))
    steps = np.arange(-n, n + 1)
    g = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    d = np.abs(np.stack(np.meshgrid(steps, steps, steps, indexing="ij"), -1).reshape(-1, 3)).sum(1)
    return g[np.argsort(d, kind="stable")]


def _search(p, ok):
    """the point nearest p (in ulps) for which ok(points [K,3]) -> bool [K] holds; p itself if there is none"""
    c = _nudges(p)
    hit = np.nonzero(ok(c))[0]
    return c[hit[0]] if hit.size else np.asarray(p, F)


def _radius_iso(tv, s, cam):
    """radius of an isotropic splat of scale s at view position tv (float64; Sigma = s^2 I, so cov2D = s^2 J J^T)"""
    fx, fy = cam["W"] / (2.0 * cam["tanx"]), cam["H"] / (2.0 * cam["tany"])
    tz = tv[2]
    tx = np.clip(tv[0] / tz, -1.3 * cam["tanx"], 1.3 * cam["tanx"]) * tz
    ty = np.clip(tv[1] / tz, -1.3 * cam["tany"], 1.3 * cam["tany"]) * tz
    j00, j02, j11, j12 = fx / tz, -fx * tx / tz ** 2, fy / tz, -fy * ty / tz ** 2
    a, b, c = s * s * (j00 ** 2 + j02 ** 2) + 0.3, s * s * j02 * j12, s * s * (j11 ** 2 + j12 ** 2) + 0.3
    mid = 0.5 * (a + c)
    return float(np.ceil(3.0 * np.sqrt(mid + np.sqrt(max(0.1, mid * mid - (a * c - b * b))))))


def edge_scene():
    cam = camera()
    rng = np.random.default_rng(20250)
    view64 = np.asarray(cam["view"], np.float64)
    inv = np.linalg.inv(view64)
    tanx, tany = cam["tanx"], cam["tany"]
    limx, limy = 1.3 * tanx, 1.3 * tany
    world = lambda tv: (np.append(np.asarray(tv, np.float64), 1.0) @ inv)[:3].astype(F)
    pix2view = lambda px, py, z: np.array([((2 * px + 1) / W - 1) * tanx * z, ((2 * py + 1) / H - 1) * tany * z, z])
    rows = []                      # (group, mean, scale[3], quaternion or None, opacity or None, dc or None)

    def add(group, mean, scale, quat=None, opac=None, dc=None, keep_rest=False):
        rows.append((group, np.asarray(mean, F), np.broadcast_to(np.asarray(scale, F), (3,)).copy(), quat, opac, dc, keep_rest))

    # near: the float32 view depth EXACTLY at 0.2f + k ulp
    for k in (0, 1, -1, 2, -2, 8, -8):
        target = F(0.2)
        for _ in range(abs(k)):
            target = np.nextafter(target, F(np.inf if k > 0 else -np.inf))
        p = _search(world((0, 0, float(target))), lambda c: view_f32(c, cam["view"])[2] == target)
        assert view_f32(p[None], cam["view"])[2][0] == target, "no float32 mean reaches view depth 0.2f %+d ulp" % k
        add("near", p, 0.004, opac=0.8)
    for z in (0.19, 0.21):
        add("near", world((0, 0, z)), 0.004, opac=0.8)

    # frustum clamp
    def clamp_rows(group, axes_signs):
        for signs in axes_signs:
            j = 0
            which_axes = [k for k in (0, 1) if signs[k]]
            for f in CLAMP_FACTORS:
                for variant in ((0, 1, 2) if f == 1.0 else (0,)):
                    z = 3.0 + 3.0 * ((j * 0.37) % 1.0)
                    s = 0.8 + 0.7 * ((j * 0.61) % 1.0) if f < 1.1 else 1.5        # (a far row's tail must reach the image)
                    z = z if f < 1.5 else 3.0 + 0.5 * (j % 2)
                    rx = signs[0] * limx * f if signs[0] else rng.uniform(-0.5, 0.5) * limx
                    ry = signs[1] * limy * f if signs[1] else rng.uniform(-0.5, 0.5) * limy
                    p = world((rx * z, ry * z, z))
                    which = which_axes

                    def differ(c):
                        d32, d64 = decisions_f32(c, cam), decisions_f64(c, cam)
                        return np.all([d32[("inx", "iny")[k]] != d64[("inx", "iny")[k]] for k in which], 0)

                    def at_limit(c):
                        d32 = decisions_f32(c, cam)
                        return np.all([np.abs(d32[("txtz", "tytz")[k]]) == d32[("limx", "limy")[k]] for k in which], 0)
                    if variant:
                        p = _search(p, differ if variant == 1 else at_limit)
                    add(group, p, (s, 0.6 * s, 0.8 * s), opac=(0.2 if f > 1.8 and len(which_axes) == 2 else 0.05) if f > 1.1 else 0.02 + 0.06 * ((j * 0.43) % 1.0))
                    j += 1
    clamp_rows("clamp_x", [(1, 0), (-1, 0)])
    clamp_rows("clamp_y", [(0, 1), (0, -1)])
    clamp_rows("clamp_xy", [(1, -1), (-1, 1), (1, 1), (-1, -1)])

    # colour clamp bits: float32(SH_C0 * dc) at -0.5, one ulp either side, and far either side
    def dc_for(target):
        c0 = F(SH_C0); d = F(float(target) / SH_C0)
        for _ in range(64):
            if c0 * d == target:
                return d
            d = np.nextafter(d, F(-np.inf) if c0 * d > target else F(np.inf))
        raise AssertionError("no float32 dc gives SH_C0 * dc == %r" % target)
    half = F(-0.5)
    levels = [dc_for(half), dc_for(np.nextafter(half, F(-1))), dc_for(np.nextafter(half, F(0))), F(-3.0), F(1.0)]
    for chans in ((0,), (1,), (2,), (0, 1), (1, 2), (0, 1, 2)):
        for n_lv, lv in enumerate(levels):
            dc = np.full(3, 0.6, F); dc[list(chans)] = lv
            # (far from the threshold the higher coefficients stay: the SH direction term of dL/dmean under a clamped channel)
            add("colour", world(pix2view(rng.uniform(8, 56), rng.uniform(8, 40), rng.uniform(2.5, 6))), rng.uniform(0.1, 0.3, 3), dc=dc,
                keep_rest=n_lv >= 3)

    # empty tile rectangle: centres outside each border, around radius and radius + 15 px beyond it
    s_rect, z_rect = 0.12, 4.0
    for border in range(4):
        for off in (-3.0, -1.5, -0.5, 0.5, 1.5, 3.0, 12.0, 14.5, 15.5, 17.0):
            r = 6.0
            for _ in range(4):
                d = r + off
                px, py = [(-d, 20.3), (W - 1 + d, 27.6), (30.2, -d), (37.7, H - 1 + d)][border]
                tv = pix2view(px, py, z_rect)
                r = _radius_iso(tv, s_rect, cam)
            add("rect", world(tv), s_rect, quat=np.array([1, 0, 0, 0], F), opac=0.95)

    # the 0.1 floor of mid^2 - det: isotropic on-axis (zero scales included), and a sweep through the floor
    for z in (1.0, 2.5, 5.0, 9.0):
        for s in (0.0, 1e-3, 0.05, 0.3):
            add("iso", world((0, 0, z)), s, quat=np.array([1, 0, 0, 0], F))
    for ratio in (1.0, 0.9, 0.8, 0.7, 0.6, 0.5):
        add("iso", world((0, 0, 2.5)), (0.05, 0.05 * ratio, 0.05), quat=np.array([1, 0, 0, 0], F))

    # denom * denom overflows float32 (denom ~ (fx s / z)^4 > 1.8e19 from s ~ 5.9e3 at z = 5); a factor 10 in denom on the safe side
    for s in (1.0e4, 0.9e4, 1.2e4, 3.3e3, 3.0e3, 3.2e3):
        add("overflow", world(pix2view(rng.uniform(20, 44), rng.uniform(16, 32), 5.0)), (s, 0.9 * s, 1.1 * s), opac=0.01)

    for norm in (0.5, 2.0):
        for _ in range(4):
            q = rng.normal(size=4); q *= norm / np.linalg.norm(q)
            add("nonunit", world(pix2view(rng.uniform(4, 60), rng.uniform(4, 44), rng.uniform(2.5, 6))), rng.uniform(0.05, 0.4, 3), quat=q.astype(F))

    n_edge = len(rows)
    n_ord = P - 256 - n_edge
    assert n_ord >= 64, n_edge
    ordinary = []
    for _ in range(n_ord):
        ordinary.append(("ordinary", world(pix2view(rng.uniform(-4, W + 4), rng.uniform(-4, H + 4), rng.uniform(2.5, 7.0))),
                         np.exp(rng.uniform(np.log(0.05), np.log(0.4), 3)).astype(F), None, None, None, False))
    # a block of culled rows: behind the camera, inside the near plane, far outside the frustum
    culled = []
    for i in range(256):
        kind = i % 3
        tv = [(rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-6, -0.5)), (rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(0.0, 0.19)),
              (rng.choice([-1, 1]) * rng.uniform(40, 80), rng.uniform(-3, 3), rng.uniform(3, 6))][kind]
        culled.append(("culled_block", world(tv), np.full(3, 0.02, F), None, None, None, False))
    live = ordinary + rows                                # the edge rows fill the end of block 0 and the partial last block
    rows = live[:256] + culled + live[256:]
    assert len(rows) == P

    means = np.stack([r[1] for r in rows]).astype(F)
    scales = np.stack([r[2] for r in rows]).astype(F)
    q = rng.normal(size=(P, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    rots = q.astype(F)
    opac = rng.uniform(0.02, 0.2, size=(P, 1)).astype(F)
    shs = np.empty((P, 16, 3), F)
    shs[:, 0] = rng.normal(0, 0.5, size=(P, 3)); shs[:, 1:] = rng.normal(0, 0.1, size=(P, 15, 3))
    groups = {}
    for i, (g, _, _, quat, op, dc, keep_rest) in enumerate(rows):
        groups.setdefault(g, []).append(i)
        if quat is not None:
            rots[i] = quat
        if op is not None:
            opac[i] = op
        if dc is not None:
            if not keep_rest:
                shs[i] = 0
            shs[i, 0] = dc
    groups = {k: np.array(v, np.int64) for k, v in groups.items()}
    scene = dict(means=means, scales=scales, rots=rots, opac=opac, shs=shs, D=3)
    scene["cov3D_precomp"] = cov3d_unnormalised(scales, rots)
    scene["colors_precomp"] = rng.uniform(0, 1, size=(P, 3)).astype(F)
    return scene, cam, groups


_CACHE = []


def cached_edge_scene():
    """edge_scene() built once per process (the tests share it and leave it unchanged)"""
    if not _CACHE:
        _CACHE.append(edge_scene())
    return _CACHE[0]


# ---------------------------------------------------------------------------------------------- the per-row gate (host and GPU tests)
# floor of the gate, per tensor: the 99.9th percentile of the C oracle's own per-row distance from float64 over the `ordinary` rows of the
# edge scene, measured on the CPU with the oracle's blend-stage gradients of eight random image gradients (NOTEBOOK.md "Preprocess kernels
# at their decision edges"; tests/test_preprocess_edges_host.py repeats the measurement and asserts that these are its figures rounded
# up).  Never tuned on the HIP kernels' output.
FLOOR = dict(means=1.1e-6, scales=7.6e-6, rots=7.2e-6, cov=4.1e-6, shs=3.8e-7)     # measured: 1.08e-6, 7.55e-6, 7.16e-6, 4.07e-6, 3.75e-7


def decisions(scene, cam, geo, pre_cov=False):
    """The discrete decisions the float32 kernels took on this scene: visibility and colour-clamp bits from the C oracle's forward (geo),
    clamp and denom2inv == 0 from the numpy float32 restatement - what torch_dense.stage_vjp needs to branch where they branch."""
    d = decisions_f32(scene["means"], cam, scene["cov3D_precomp"] if pre_cov else geo["cov3D"])
    return dict(inx=d["inx"], iny=d["iny"], overflow=d["overflow"], clamped=geo["clamped"].astype(bool), visible=geo["radii"] > 0)


def mode_kw(scene, pre_cov, pre_col):
    kw = dict(colors_precomp=scene["colors_precomp"]) if pre_col else dict(shs=scene["shs"])
    kw.update(dict(cov3D_precomp=scene["cov3D_precomp"]) if pre_cov else dict(scales=scene["scales"], rots=scene["rots"]))
    return kw


def stage_reference(scene, cam, dec, dmean2D, dconic, dcolor, D, pre_cov=False, pre_col=False):
    """float64 stage VJP with the float32 decisions `dec`; the precomputed-colour gradient is the identity and is left out"""
    from oracle import torch_dense as td
    out = td.stage_vjp(dmean2D, np.asarray(dconic).reshape(-1, 4), dcolor, scene["means"], cam, D=D, decisions=dec, **mode_kw(scene, pre_cov, pre_col))
    out.pop("colors", None)
    return out


def stage_oracle(orc, scene, cam, geo, dmean2D, dconic, dcolor, D, pre_cov=False, pre_col=False):
    """the C oracle's preprocess backward (the float32 statements of backward.cu) on the same blend-stage gradients"""
    g = dict(geo, cov3D=scene["cov3D_precomp"]) if pre_cov else geo
    dmean3D, dcov, dsh, dscale, drot = orc.preprocess_bwd(
        scene["means"], g, cam["view"], cam["proj"], cam["campos"], cam["W"], cam["H"], cam["tanx"], cam["tany"], dmean2D,
        np.asarray(dconic).reshape(-1, 4), dcolor, D=D, shs=None if pre_col else scene["shs"], scales=None if pre_cov else scene["scales"],
        rots=None if pre_cov else scene["rots"])
    out = dict(means=dmean3D)
    out.update(dict(cov=dcov) if pre_cov else dict(scales=dscale, rots=drot))
    if not pre_col:
        out["shs"] = dsh
    return out


def row_errors(got, ref):
    """[P]: the largest error of a row relative to the row's largest float64 entry; a row whose reference is all zero must BE zero
    (error 0, else inf); a row holding a NaN / inf has error inf"""
    got = np.asarray(got, np.float64).reshape(len(ref), -1); ref = np.asarray(ref, np.float64).reshape(len(ref), -1)
    with np.errstate(all="ignore"):
        num = np.abs(got - ref).max(1); den = np.abs(ref).max(1)
        err = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num == 0, 0.0, np.inf))
    return np.where(np.isfinite(got).all(1), err, np.inf)


def gate_failures(got, orc_out, ref, visible, groups=None):
    """The per-row gate: err_got[i] <= 2 err_orc[i] + floor for every visible row of every tensor (both errors against the float64 stage
    reference `ref`), every culled row exactly zero.  Returns (failures: [(tensor, row, err_got, err_orc)], worst ratio err_got /
    (2 err_orc + floor) per tensor - and, with `groups`, per (tensor, group))."""
    bad, worst = [], {}
    for k, r in ref.items():
        eg, eo = row_errors(got[k], r), row_errors(orc_out[k], r)
        ratio = eg / (2.0 * eo + FLOOR[k])
        worst[k] = float(ratio[visible].max())
        for name, rows in (groups or {}).items():
            rows = rows[visible[rows]]
            if len(rows):
                worst[(k, name)] = float(ratio[rows].max())
        for i in np.nonzero(visible & ~(eg <= 2.0 * eo + FLOOR[k]))[0]:
            bad.append((k, int(i), float(eg[i]), float(eo[i])))
        g = np.asarray(got[k]).reshape(len(r), -1)
        for i in np.nonzero(~visible & ~((g == 0).all(1)))[0]:
            bad.append((k, int(i), float("inf"), 0.0))
    return bad, worst
