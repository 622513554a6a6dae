"""-m gpu: the row body of the deform / shade kernels (gm_deform.hip: gather_blend, deform_cov, shade_rotated; gm_sh.h) row by row, on
the cases of deform_cases.py: every kind, SH degrees 0..3, N = 1 .. 257 (prefixes of the same rows: the edges of the 64-row fused blocks
and of the 256-thread blocks of deform_kernel / sh_colors_kernel).

a. Every route through the row body gives the same bits: deform_kernel + sh_colors_kernel, deform_shade_kernel unpacked / packed / with
   the preprocess behind it (9-entry and 6-entry rest covariance) / with direct depth placement, the batch kernel; a row's bits do not
   depend on N (the LDS-DMA block route equals the partial-block route); the fused frame equals deform_shade_packed + the ordinary forward.
b. The packed route against the float64 definition (deform_ref.py), every element of every row: |got - ref| <= 2 r_f32 2^-24 S_abs, with
   r_f32 what a correct float32 evaluator reaches (measured on the CPU, test_deform_ref_host.py, which also shows that this gate rejects
   wrong evaluators).  (a) carries it to the other routes.
c. The scene kernel's deformed rows at the same N and degrees against its contract (deform + cov_to_scale_rot + the SH forward).
Kernel x degree x N coverage: deform_kernel, sh_colors_kernel, deform_shade_kernel<false,false>, <true,false>, <true,true>,
<true,true,true> and deform_shade_pre_batch_kernel in test_routes_give_the_same_bits; scene_shade_pre_batch_kernel in
test_scene_rows_equal_their_contract.
Measured on the MI355X: worst ratio / (2 r_f32) 0.500 for pos, 0.499 rot, 0.496 cov - the float32 emulation's own error - and 0.495 for
the colour (NOTEBOOK.md "Fused deform/shade rows, per element")."""
import numpy as np
import pytest
import torch

import deform_cases as dc
import deform_ref as ref

pytestmark = pytest.mark.gpu

FRAME_NS = (1, 63, 64, 65, 129, 257)                    # the unfused chain and the scene contract are rendered at these
C6 = [0, 1, 2, 4, 5, 8]
_COMPARED = [0, 0]                                      # tensors and elements compared bit for bit (printed per test: the checks are not vacuous)
CASES = [(kind, deg) for kind in dc.KINDS for deg in range(4)]


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(a.shape[0], -1)


def _same(got, want, what):
    for k in want:
        if k in got:
            a, b = _bits(got[k]), _bits(want[k])
            assert a.shape == b.shape, (what, k, a.shape, b.shape)
            _COMPARED[0] += 1
            _COMPARED[1] += a.size
            bad = np.argwhere(a != b)
            assert bad.size == 0, "%s: %s differs in %d elements, first at row %d element %d" % (what, k, len(bad), bad[0][0], bad[0][1])


def _inputs(kind, deg, n, table=None):
    from gpu_utils import T
    from gaussianmesh_amd.deform import pack_mesh_state
    c = dc.case(kind)
    tb = table or c
    g = dict(tri=T(c["tri"][:n], dtype=torch.int32), w=T(c["w"][:n]), cov=T(c["cov"][:n]), pos=T(c["pos"][:n]), shs=T(dc.shs(kind, deg)[:n]),
             opac=T(c["opac"][:n]), dV=T(tb["dV"]), Rv=T(tb["Rv"]), Sv=T(tb["Sv"]))
    g["packed"] = pack_mesh_state(T(tb["state"]), T(tb["verts"]))
    return g


def _camera(k):
    from gpu_utils import T
    cam = dc.frame_camera(k)
    return dict(view=T(cam["view"]), proj=T(cam["proj"]), campos=T(cam["campos"]), tanx=cam["tanx"], tany=cam["tany"])


def _packed(g, deg, campos):
    """route 3: deform_shade_kernel<PACKED>, every output"""
    from gaussianmesh_amd.deform import deform_shade_packed
    p, c6, rgb, cov, rot = deform_shade_packed(g["tri"], g["w"], g["packed"], g["cov"], g["pos"], g["shs"], campos, deg=deg, want_cov_rot=True)
    return dict(pos=p, cov6=c6, rgb=rgb, cov=cov, rot=rot)


def _tensor_routes(g, deg, campos):
    """routes 1 and 2 (the unfused pair, the unpacked fused kernel with and without cov / rot)"""
    from gaussianmesh_amd.deform import deform_shade, deform_tensors, sh_colors
    p, c, r, c6 = deform_tensors(g["tri"], g["w"], g["dV"], g["Rv"], g["Sv"], g["cov"], g["pos"])
    out = {"deform + sh_colors": dict(pos=p, cov6=c6, cov=c, rot=r, rgb=sh_colors(p, campos, g["shs"], rot=r, deg=deg))}
    args = (g["tri"], g["w"], g["dV"], g["Rv"], g["Sv"], g["cov"], g["pos"], g["shs"], campos)
    out["deform_shade, cov and rot"] = dict(zip(("pos", "cov6", "rgb", "cov", "rot"), deform_shade(*args, deg=deg, want_cov_rot=True)))
    out["deform_shade"] = dict(zip(("pos", "cov6", "rgb"), deform_shade(*args, deg=deg)))
    return out


def _begin(g, deg, cam, bg, cov=None, **kw):
    from gaussianmesh_amd import rasterizer as Rz
    return Rz.forward_deformed_begin(bg, g["tri"], g["w"], g["packed"], g["cov"] if cov is None else cov, g["pos"], g["shs"], g["opac"],
                                     cam["view"], cam["proj"], cam["tanx"], cam["tany"], dc.H, dc.W, deg, cam["campos"], **kw)


def _splat(geom, n):
    from gpu_utils import _view
    from gaussianmesh_amd import _lib
    lib = _lib.lib()
    SF = lib.gm_splat_floats()
    return _view(geom, lib.gm_geom_field(geom.data_ptr(), n, b"splat"), n * SF, torch.float32).reshape(n, SF)


def _frame_state(nr, color, radii, geom, n, deformed=None):
    """what a finished frame leaves: instance count, image, radii, the splat rows of the visible Gaussians (all-zero rows otherwise)"""
    torch.cuda.synchronize()
    r = radii.cpu().numpy()
    s = _splat(geom, n).copy()
    s[r <= 0] = 0
    st = dict(nr=nr, color=color.cpu().numpy().copy(), radii=r, splat=s)
    if deformed is not None:
        st.update(pos=deformed[0].cpu().numpy(), cov6=deformed[1].cpu().numpy(), rgb=deformed[2].cpu().numpy())
        vis = r > 0
        assert np.array_equal(_bits(s[vis][:, 6:9]), _bits(st["rgb"][vis])), "the frame's splat colours are its deformed cloud's"
    return st


def _same_frame(got, want, what, count=True):
    if count:
        assert got["nr"] == want["nr"], (what, got["nr"], want["nr"])
    assert np.array_equal(got["radii"], want["radii"]), what + ": radii"
    _same(got, {k: want[k] for k in ("splat", "pos", "cov6", "rgb") if k in want}, what)
    assert np.array_equal(_bits(got["color"].reshape(3, -1)), _bits(want["color"].reshape(3, -1))), what + ": image"


@pytest.mark.parametrize("kind,deg", CASES)
def test_routes_give_the_same_bits(kind, deg):
    from gpu_utils import T
    from gaussianmesh_amd import rasterizer as Rz
    from gaussianmesh_amd.deform import pack_cov6
    bg = T(np.array([0.1, 0.5, 0.9], np.float32))
    cams = [_camera(1), _camera(2)]
    far = T(dc.CAMPOS)
    kept = {}                                           # per N: what must not depend on N
    _COMPARED[:] = [0, 0]
    for n in dc.NS:
        what = "%s, degree %d, N = %d" % (kind, deg, n)
        g = _inputs(kind, deg, n)
        # routes 1-3 under the colour camera and under the frames' cameras
        for campos in (far, cams[0]["campos"], cams[1]["campos"]):
            p3 = _packed(g, deg, campos)
            assert all(torch.isfinite(v).all() for v in p3.values()), what
            assert torch.equal(p3["cov6"], p3["cov"].reshape(n, 9)[:, C6]), what
            routes = _tensor_routes(g, deg, campos)
            for name, out in routes.items():
                _same(out, p3, what + ": " + name + " against deform_shade_packed")
            if campos is far:
                kept[n] = {"unpacked": {k: v.cpu().numpy() for k, v in routes["deform_shade, cov and rot"].items()}}
        p3 = [_packed(g, deg, c["campos"]) for c in cams]
        dfm = lambda k: {key: p3[k][key] for key in ("pos", "cov6", "rgb")}
        # route 4: the fused frame (PRE), 9-entry rest covariance; one per camera, each teaching its workspace a capacity
        ws = [Rz.RasterWorkspace(), Rz.RasterWorkspace()]
        single = []
        for k in (0, 1):
            h = _begin(g, deg, cams[k], bg, workspace=ws[k], want_deformed=True)
            nr, color, radii, geom, *_ = h.finish()
            single.append(_frame_state(nr, color, radii, geom, n, h.deformed))
            _same(single[k], dfm(k), what + ": fused frame %d against deform_shade_packed" % k)
        vis = int((single[0]["radii"] > 0).sum())
        assert n < 63 or vis >= n // 4, (what, vis)       # the cloud is in view: the frame checks look at rows
        kept[n]["frame"] = single[0]
        # ... equals the unfused chain: deform_shade_packed, then the ordinary forward on its outputs
        if n in FRAME_NS:
            c = cams[0]
            nr0, color0, radii0, geom0, *_ = Rz.rasterize_forward(bg, p3[0]["pos"], p3[0]["rgb"], g["opac"], None, None, 1.0, p3[0]["cov6"], c["view"],
                                                                  c["proj"], c["tanx"], c["tany"], dc.H, dc.W, None, deg, c["campos"], False, False)
            _same_frame(single[0], _frame_state(nr0, color0, radii0, geom0, n), what + ": fused frame against the unfused chain")
        # route 5: the same frame from the six distinct entries - where every matrix is bit-symmetric, else pack_cov6 refuses the tensor
        c6 = pack_cov6(g["cov"])
        skewed = kind == "needle" and any(r < n for r in dc.SKEW_ROWS)
        assert (c6 is None) == skewed, what
        if c6 is not None:
            h = _begin(g, deg, cams[0], bg, cov=c6, want_deformed=True)
            nr, color, radii, geom, *_ = h.finish()
            _same_frame(_frame_state(nr, color, radii, geom, n, h.deformed), single[0], what + ": cov6 frame against the 9-entry frame")
        # route 6: direct depth placement - the second frame of a view stream
        plan, wd = Rz.new_depth_plan(bg.device), Rz.RasterWorkspace()
        _begin(g, deg, cams[0], bg, workspace=wd, depth_plan=plan).finish()
        h = _begin(g, deg, cams[0], bg, workspace=wd, depth_plan=plan, want_deformed=True, want_count=False)
        assert h.direct, what
        nr, color, radii, geom, *_ = h.finish(sync_free=True)
        ok, count = h.check()
        direct = _frame_state(count, color, radii, geom, n, h.deformed)        # (before a refused frame is begun again on the partition path)
        if not ok:
            nr, color, *_ = h.finish()
            direct["color"] = color.cpu().numpy()
        _same_frame(direct, single[0], what + ": direct-placement frame against the partition frame", count=ok)
        kept[n]["direct"] = direct
        # route 7: the batch kernel, the same table under the two cameras
        wb = [Rz.RasterWorkspace(), Rz.RasterWorkspace()]
        for w_ in wb:
            w_.capacity = max(x.capacity for x in ws)
        hs = Rz.forward_deformed_batch(bg, g["tri"], g["w"], [g["packed"], g["packed"]], g["cov"], g["pos"], g["shs"], g["opac"], cams, dc.H, dc.W,
                                       deg, wb)
        torch.cuda.synchronize()
        kept[n]["batch"] = []
        for k, h in enumerate(hs):
            ok, nr = h.check()
            assert ok, what
            st = _frame_state(nr, h.color, h.radii, h.geom, n)
            _same_frame(st, {key: single[k][key] for key in ("nr", "radii", "splat", "color")}, what + ": batch frame %d against the single frame" % k)
            kept[n]["batch"].append(st)
    # a row's bits are the same at every N that contains it
    full = kept[dc.NMAX]
    for n in dc.NS:
        what = "%s, degree %d: rows [0, %d) of N = %d against N = %d" % (kind, deg, n, dc.NMAX, n)
        _same(kept[n]["unpacked"], {k: v[:n] for k, v in full["unpacked"].items()}, what + ", deform_shade")
        for name, a, b in [("fused frame", kept[n]["frame"], full["frame"]), ("direct frame", kept[n]["direct"], full["direct"]),
                           ("batch frame 0", kept[n]["batch"][0], full["batch"][0]), ("batch frame 1", kept[n]["batch"][1], full["batch"][1])]:
            assert np.array_equal(a["radii"], b["radii"][:n]), what + ", " + name
            _same(a, {k: b[k][:n] for k in ("splat", "pos", "cov6", "rgb") if k in b}, what + ", " + name)
    print("deform rows, routes: %s degree %d: %d tensors, %d elements compared bit for bit; %d of %d rows visible in frame 0, %d in frame 1" % (
        kind, deg, _COMPARED[0], _COMPARED[1], int((full["frame"]["radii"] > 0).sum()), dc.NMAX, int((full["batch"][1]["radii"] > 0).sum())))


@pytest.mark.parametrize("kind,deg", CASES)
def test_every_element_against_float64(kind, deg):
    """deform_shade_packed, every element of every row: stage 1 from the inputs, the colour from the device's own float32 position and
    rotation, each within 2 r_f32 of the float64 definition in units of 2^-24 S_abs.  The factor 2: the emulation behind r_f32 follows
    the kernels' parenthesisation with contraction off, so the kernel's error should be the emulation's own; the factor allows for sqrtf
    and the division not being numpy's and for another row being the worst.  It is not fitted to the kernel."""
    from gpu_utils import T
    c = dc.case(kind)
    worst = dict.fromkeys(ref.TENSORS, 0.0)
    problems = []
    for n in dc.NS:
        g = _inputs(kind, deg, n)
        for cam_name, campos in dc.colour_cameras(kind):
            out = {k: v.cpu().numpy() for k, v in _packed(g, deg, T(campos)).items()}
            assert all(np.isfinite(v).all() for v in out.values()), (kind, deg, n, cam_name)        # NaN beyond the degree is never read
            assert np.array_equal(_bits(out["cov6"]), _bits(out["cov"].reshape(n, 9)[:, C6]))
            ratios = ref.row_ratios(c, deg, campos, dc.shs(kind, deg), out["pos"], out["cov"], out["rot"], out["rgb"])
            for t, (r, row, el) in ref.worst(ratios).items():
                bar = 2.0 * ref.R_F32[kind][t]
                worst[t] = max(worst[t], r / bar if bar else (np.inf if r else 0.0))
                if not r <= bar:
                    problems.append("N = %d, %s camera: %s row %d element %d at %.3g (bar %.3g); %d elements over" % (
                        n, cam_name, t, row, el, r, bar, int((ratios[t] > bar).sum())))
    print("deform rows, per element: %s degree %d: worst ratio / (2 r_f32): " % (kind, deg) + "  ".join("%s %.3f" % (t, worst[t]) for t in ref.TENSORS))
    assert not problems, "%s, degree %d:\n" % (kind, deg) + "\n".join(problems[:20])


def test_onehot_rows_are_exact_on_the_device():
    """one-hot weights: Rt is the vertex's own R transposed and npos = pos + dV[vertex], bit for bit; under the identity table (R = S = I,
    dV = 0) the covariance and the centre come through untouched.  Every N: a row in a partial block, in a full one."""
    from gpu_utils import T
    c = dc.case("onehot")
    corner = np.arange(dc.NMAX) % 3
    v = c["tri"][np.arange(dc.NMAX), corner]
    Rt = c["Rv"][v].reshape(-1, 3, 3).transpose(0, 2, 1).reshape(-1, 9)
    npos = c["pos"] + c["dV"][v]
    cov = c["cov"].reshape(-1, 9)
    values = lambda t: t.cpu().numpy().reshape(t.shape[0], -1)
    # (the sign of a zero is the float32 chain's: (1 a + 0 b) + 0 c turns -0 into +0, so bits are compared with the float32 emulation
    # and values with the facts)
    e_pos, _, e_rot = ref.stage1(*ref.stage1_inputs(c), np.float32)
    for n in dc.NS:
        g = _inputs("onehot", 3, n)
        out = _packed(g, 3, T(dc.CAMPOS))
        assert np.array_equal(values(out["rot"]), Rt[:n]) and np.array_equal(values(out["pos"]), npos[:n]), n
        _same(out, dict(rot=e_rot[:n], pos=e_pos[:n]), "one-hot rows, N = %d" % n)
        out = _tensor_routes(g, 3, T(dc.CAMPOS))["deform + sh_colors"]
        assert np.array_equal(values(out["rot"]), Rt[:n]) and np.array_equal(values(out["pos"]), npos[:n]), n
        g = _inputs("onehot", 3, n, table=dc.identity_table())
        out = _packed(g, 3, T(dc.CAMPOS))
        assert np.array_equal(values(out["cov"]), cov[:n]) and np.array_equal(values(out["pos"]), c["pos"][:n]), n
        assert np.array_equal(values(out["cov6"]), cov[:n][:, C6]), n


@pytest.mark.parametrize("kind,deg", CASES)
def test_scene_rows_equal_their_contract(kind, deg):
    """scene_shade_pre_batch_kernel on one object made of the case's rows: frame 0 deforms it, frame 1 leaves it at rest.  Each frame
    against the contract of test_gpu_scene_batch.py - deform, cov_to_scale_rot, the forward on scales / rotations / SH rows at this degree -
    bit for bit: instance count, radii, splat rows, image."""
    from gpu_utils import T
    from gaussianmesh_amd import rasterizer as Rz
    from gaussianmesh_amd.deform import cov_to_scale_rot, deform_tensors
    bg = T(np.array([0.2, 0.5, 0.7], np.float32))
    cams = [_camera(1), _camera(2)]
    for n in FRAME_NS:
        what = "%s, degree %d, N = %d" % (kind, deg, n)
        g = _inputs(kind, deg, n)
        p, c, _, _ = deform_tensors(g["tri"], g["w"], g["dV"], g["Rv"], g["Sv"], g["cov"], g["pos"])
        s0, q0 = cov_to_scale_rot(g["cov"])
        want = []
        for cam, (pos, cov) in zip(cams, ((p, c), (g["pos"], g["cov"]))):
            s, q = cov_to_scale_rot(cov)
            nr, color, radii, geom, *_ = Rz.rasterize_forward_begin(bg, pos, None, g["opac"], s, q, 1, None, cam["view"], cam["proj"], cam["tanx"],
                                                                    cam["tany"], dc.H, dc.W, g["shs"], deg, cam["campos"], False, False,
                                                                    force_M=16).finish(image_only=True)
            want.append(_frame_state(nr, color, radii, geom, n))
        ws = [Rz.RasterWorkspace(), Rz.RasterWorkspace()]
        for w_ in ws:
            w_.capacity = int(max(x["nr"] for x in want) * 1.25) + 1024
        hs = Rz.forward_scene_batch(bg, [0, n], [1, 0], g["pos"], s0, q0, g["shs"], g["opac"], g["tri"], g["w"], g["cov"].reshape(n, 9),
                                    [g["packed"], None], cams, dc.H, dc.W, deg, ws, image_only=True)
        torch.cuda.synchronize()
        for k, h in enumerate(hs):
            ok, nr = h.check()
            assert ok, what
            assert np.isfinite(want[k]["color"]).all(), what
            _same_frame(_frame_state(nr, h.color, h.radii, h.geom, n), want[k], what + ": scene frame %d against its contract" % k)
