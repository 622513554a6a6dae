"""-m gpu: every operator route on poisoned, guard-banded buffers (tests/poison.py).

The wrappers of gaussianmesh_amd/ hand their kernels torch.empty memory at 87 sites and rely on every kernel writing all that is later read
or returned.  Each case below builds its inputs once, then runs its route three times - under the fills 0x00, 0xFF (float NaN, int -1,
counter UINT_MAX) and 0x5A (float32 1.54e16, int32 1515870810), in that order - with every torch.empty / empty_like / new_empty of the
route (outputs, gradients, scratch, caller workspaces) filled with the byte and fenced by 4 KiB guard bands.  Asserted per case:
  * the harness bit: at least one guarded allocation under every fill;
  * every guard band is intact after every run (poisoned.__exit__ raises GuardViolation naming the allocation, the side and the offset);
  * deterministic routes: every tensor the route returns is bit for bit the same under the three fills;
  * the rasterizer's backward (float atomics into grad_acc, gm_render_bwd_body.inc:93,98): each fill's gradients pass test_gpu_parity's
    _grad_gate against the oracle, every gradient row of a Gaussian with radii == 0 is exactly 0.0 and every dL/dSH coefficient above
    the active degree is exactly 0.0.

WHO WRITES WHAT FIRST (read from the kernels before anything here ran on a device; a poisoned counter that a kernel trusted would be a
loop bound of four billion):
  rasterizer, geometry buffer   launch_arm_counters (gm_binning.hip:29) zero-fills slots | counters | coarse | acc | chunk_inst in one
                                memset (arm_words) as the first launch of every first half; the direct placement's arm_direct_kernel
                                (gm_bucket.hip:871) does the same plus the slab's bucket counters.  The preprocess kernels write radii,
                                tiles_touched, bin, inst16, depth_key of EVERY row (gm_preprocess.hip:148-154: radius 0, an empty record,
                                key 0xFFFFFFFF for a culled row).  splat, clamped and cov3D of a culled row stay UNWRITTEN: the kernel
                                breaks out before those stores (gm_preprocess.hip:97-117, 141-143).  Nothing reads them: the ordering
                                and the blend reach a row through order / pairs, which hold visible ids only, and preprocess_bwd
                                loads splat / cov3D / clamped only under radii > 0 (gm_preprocess.hip:291-319).
                                bk_hist_kernel writes hist, dmap, bmap and counters[VISIBLE / NBUCKETS / RENDERED / CMIN / CMAX],
                                bk_scan_kernel bucket_start, bk_scatter dpairs, bucket_sort_kernel order[:V] and chunk_inst.  Every loop
                                bound read from memory is one of those counters or bucket_start, behind their writers.
  rasterizer, binning buffer    duplicate_kernel zeroes acc (gm_binning.hip:83) and writes pairs[0][:num_rendered], refusing when
                                counters[RENDERED] > capacity; the tile pass writes hist before bk_scan reads it and pairs[1].
  rasterizer, image buffer      ranges: hipMemsetAsync (gm_api.hip:259, gm_binning.hip:306, gm_bucket.hip:1032) or every entry by bk_scan;
                                tile_order / tile_work by tile_order_by before the blend reads them; final_T / n_contrib by the blend for
                                every pixel inside the image (unless image_only); epoch only read with a work hint, which writes it first.
  rasterizer, backward          grad_acc: hipMemsetAsync (gm_api.hip:518, "the only zero-fill of a backward"); preprocess_bwd writes
                                every row of every gradient output, zeros for culled rows.
  radix sort (knn, closest)     hist by radix_hist_kernel, digit_total by radix_scan_kernel, both before radix_scatter reads them.
  Morton front end (knn,        bbox_partial[nb] by point_bbox_partial (all nb partials), bbox by point_bbox_final, keys by point_morton /
  knn_nearest, closest_faces)   cf_face_morton, all before their readers (gm_spatial.hip).
  distCUDA2 / knn_nearest       boxes / rsorted by knn_box_minmax / nn_gather_boxes before their readers; outputs once per point.
  closest_faces                 cf_gather_boxes recs and boxes, cf_super_boxes sboxes.
  ray caster                    rc_prepare writes recs and arms slots = MISS before rc_cast's atomicMin.
  geodesic distances            gd_fill writes +inf and arms counters[0 .. sweeps] (resume: the counters alone); no loop on a counter.
  surface nets                  sn_cells act, sn_edges flags and lvl[0], sn_sums / sn_scan_level the upper levels and counts, sn_vertices
                                vid; V / F rows below the counts.  TsdfVolume.extract returns V[:nv], F[:nf].
  ARAP                          arap_init x, diag, free_row; arap_local R; column step: r, p of every row, q of the free rows it reads;
                                grid step: rhs writes r, u, bb_slots, product w (free rows) and slots, update reads p / s / w of the first
                                step without using them (selects, not arithmetic) and the carry pair only from the step that wrote it.
  deform / loss / model_ops     one thread per row / pixel / element writes every output it owns; gm_ssim_fwd writes one partial per tile.
"""
import functools

import numpy as np
import pytest
import torch

from gpu_utils import T
from helpers import small_scene
from poison import FILLS, run_under_fills, same_bits

pytestmark = pytest.mark.gpu

GUARD = 4096


@pytest.fixture(autouse=True)
def _default_emission_policy():
    from gaussianmesh_amd import rasterizer
    rasterizer.set_default_emission_policy(2)
    yield
    rasterizer.set_default_emission_policy(2)


# ---- the exceptions.  The geometry / binning / image byte buffers a forward hands back are scratch ("Scratch buffers are opaque; their
# ---- layout depends only on (base address mod 256, P/R/W/H)", include/gmesh_hip.h:19): what of them is compared is THIS table, one entry
# ---- per documented view (gm_geom_field / gm_image_field / gm_binning_field, "Read-only views into the opaque scratch buffers", :173);
# ---- _fields() below reads nothing else.  `keep` names the compared elements as a function of the route's other outputs (radii,
# ---- num_rendered, V = bucket_start[2048], the image_only flag, the depth path); `quote` is the sentence that leaves the rest unspecified.
# ---- Everything of the buffers that is no entry here (padding, histograms, ping-pong halves, accumulators) is not compared.
# ---- Routes that compare no scratch at all: the autograd operator (its buffers stay inside the autograd context).
SCRATCH_VIEWS = [
    dict(buffer="geom", field="splat", dtype=torch.float32, keep="rows with radii > 0",
         quote='gmesh_hip.h:176 "the record the blend kernels gather": a culled Gaussian has no instance, nothing gathers its row, and the forward '
               'preprocess kernels leave it unwritten (gm_preprocess.hip:97-117 breaks out before splat_store; no header sentence promises its content)'),
    dict(buffer="geom", field="bucket_start", dtype=torch.int32, keep="entry [2048] = V",
         quote='gmesh_hip.h:182 "V = \"bucket_start\"[2048]"'),
    dict(buffer="geom", field="order", dtype=torch.int32, keep="entries [0, V)",
         quote='gmesh_hip.h:182 "\"order\" uint32[V] (ids of the V visible Gaussians in (depth, id) order"'),
    dict(buffer="geom", field="depth_key", dtype=torch.int32, keep="every row, partition path only",
         quote='gmesh_hip.h:177 "0xFFFFFFFF for a culled Gaussian; not written by the direct depth placement"'),
    dict(buffer="geom", field="inst16", dtype=torch.int16, keep="every row, partition path only",
         quote='gmesh_hip.h:187-188 "\\"inst16\\" uint16[P] (the record\'s instance count: 0xFFFF = 65535 or more ... 0 for a culled row)"; the direct '
               'placement carries the records in its slab instead (:188 "bin_sorted ... direct placement only")'),
    dict(buffer="image", field="ranges", dtype=torch.int32, keep="every list tile", quote='gmesh_hip.h:190 "\"ranges\" uint32[T][2]"'),
    dict(buffer="image", field="final_T", dtype=torch.float32, keep="every pixel, unless image_only",
         quote='gmesh_hip.h:487-489 "GM_FWD_IMAGE_ONLY ... the per-pixel final transmittance and contributor count in image_buffer ... are left untouched"'),
    dict(buffer="image", field="n_contrib", dtype=torch.int32, keep="every pixel, unless image_only", quote="as final_T"),
    dict(buffer="binning", field="pairs", dtype=torch.int32, keep="records [0, num_rendered)",
         quote='gmesh_hip.h:192 "\"pairs\" uint32[R][2] = (list tile id | child mask << 16, Gaussian id) per instance": R instances, the buffer '
               'of a sync-free frame is laid out for its capacity and holds nothing past the count'),
]
_ITEM = {torch.float32: 4, torch.int32: 4, torch.int16: 2}


def _fields(geom, binning, img, P, W, H, policy, nr, radii, image_only=False, direct=False, capacity=None):
    """The views of SCRATCH_VIEWS of one frame, each cut down to its `keep`, as device tensors.  direct: the frame was begun with direct depth
    placement; capacity: the instances the binning buffer was laid out for (a sync-free frame: its capacity; an exact frame: num_rendered)"""
    from gaussianmesh_amd import _lib
    lib = _lib.lib()
    s = max(policy - 1, 0)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    tiles = ((gx + (1 << s) - 1) >> s) * ((gy + (1 << s) - 1) >> s)
    SF = lib.gm_splat_floats()
    count = dict(splat=P * SF, bucket_start=2049, order=P, depth_key=P, inst16=P, ranges=2 * tiles, final_T=W * H, n_contrib=W * H, pairs=2 * nr)
    pointer = dict(geom=lambda n: lib.gm_geom_field(geom.data_ptr(), P, n), image=lambda n: lib.gm_image_field(img.data_ptr(), W, H, n),
                   binning=lambda n: lib.gm_binning_field(binning.data_ptr(), nr if capacity is None else capacity, W, H, policy, n))
    buffers = dict(geom=geom, image=img, binning=binning)
    out = {}
    for e in SCRATCH_VIEWS:
        f = e["field"]
        if (f in ("depth_key", "inst16") and direct) or (f in ("final_T", "n_contrib") and image_only) or (f == "pairs" and nr == 0):
            continue
        buf = buffers[e["buffer"]]
        off = pointer[e["buffer"]](f.encode()) - buf.data_ptr()
        out[f] = buf[off:off + count[f] * _ITEM[e["dtype"]]].view(e["dtype"]).clone()
    V = int(out["bucket_start"][2048])
    out["bucket_start"] = out["bucket_start"][2048:]
    out["order"] = out["order"][:V]
    out["splat"] = out["splat"].reshape(P, SF)[radii > 0]
    return out


def _run(name, route, compare=True, fills=FILLS):
    """route() under each fill in order; the harness-bit and guard assertions (no route here is allocation-free); with `compare` the results
    bit for bit.  Prints handed_out / unguarded per fill (NOTEBOOK.md keeps the table).  Returns the results."""
    runs = run_under_fills(route, fills, GUARD)              # (a damaged guard band raises GuardViolation out of the run that did it)
    rows = [(p.fill, p.handed_out, p.unguarded) for p, _ in runs]
    results = [out for _, out in runs]
    print("poison %-44s %s" % (name, "  ".join("0x%02X: handed_out %d unguarded %d" % r for r in rows)))
    for fill, handed_out, _ in rows:
        assert handed_out >= 1, "%s received no poisoned buffer under fill 0x%02X: the case tests nothing" % (name, fill)
    if compare:
        for fill, out in zip(fills[1:], results[1:]):
            _assert_same(name, fills[0], results[0], fill, out)
    return results


def _assert_same(name, fill_a, a, fill_b, b, path=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), (name, path)
        for k in a:
            _assert_same(name, fill_a, a[k], fill_b, b[k], "%s.%s" % (path, k))
        return
    if isinstance(a, (tuple, list)):
        assert isinstance(b, (tuple, list)) and len(a) == len(b), (name, path)
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_same(name, fill_a, x, fill_b, y, "%s[%d]" % (path, i))
        return
    if same_bits(a, b):
        return
    detail = ""
    if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype:
        x, y = a.detach().contiguous().reshape(-1), b.detach().contiguous().reshape(-1)
        item = x.element_size()
        diff = (x.view(torch.uint8).reshape(-1, item) != y.view(torch.uint8).reshape(-1, item)).any(dim=1).nonzero().reshape(-1)
        i = int(diff[0])
        detail = ": %d of %d elements differ, first at flat index %d (%r under 0x%02X, %r under 0x%02X)" % (
            diff.numel(), x.numel(), i, x[i].item(), fill_a, y[i].item(), fill_b)
    raise AssertionError("%s: output%s depends on what its buffers held before the call%s" % (name, path or "", detail))


# =====================================================================================================================================
# 1. the rasterizer, forward and backward
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _raster_scene(cam_k=1):
    """helpers.small_scene(P=500, W=70, H=50) - 5 x 4 tiles, ragged right and bottom edges - made to contain what is easy to forget:
    small_scene itself culls 2 % of the rows and leaves no tile empty, so a third of the means is moved behind the camera (one half) and
    out of the frustum to the side (the other), and the rest of the cloud is shrunk towards the centre of the image."""
    from gaussianmesh_amd import scenes
    P = 500
    sc, cam = small_scene(P=P, W=70, H=50, seed=7, D=3, cam_k=cam_k)
    n = P // 3
    c = np.asarray(cam["campos"], np.float32)
    sc["means"][n:] *= np.float32(0.6)
    sc["scales"][n:] *= np.float32(0.6)
    sc["means"][:n // 2] = c[None] * np.float32(1.5) + np.float32(0.05) * sc["means"][:n // 2]
    side = np.cross(c, [0.0, 1.0, 0.0])
    side /= np.linalg.norm(side)
    sc["means"][n // 2:n] = (sc["means"][n // 2:n] * 0.05 + side[None] * 40.0).astype(np.float32)
    sc["cov3D_precomp"] = scenes.strip_symmetric(scenes.cov3d_from_scale_rot(sc["scales"], sc["rots"])).astype(np.float32)
    return sc, cam


BG = np.array([0.3, 0.2, 0.7], np.float32)


@functools.lru_cache(maxsize=None)
def _dpix(seed=1):
    return np.random.default_rng(seed).normal(size=(3, 50, 70)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _oracle_run(D, pre_cov, pre_col, cam_k=1):
    """(forward, backward) of the CPU oracle for the scene, computed once per configuration and shared; do not modify"""
    from oracle import oracle as orc
    orc.build()
    sc, cam = _raster_scene(cam_k)
    fw = orc.forward_full(sc, cam, BG, D=D, use_precomp_cov=pre_cov, use_precomp_color=pre_col)
    bw = orc.backward_full(sc, cam, BG, fw, _dpix(), D=D, use_precomp_cov=pre_cov, use_precomp_color=pre_col)
    return fw, bw


def test_the_scene_contains_what_is_easy_to_forget():
    """from the oracle's forward alone: at least 10 % of the rows culled, at least one tile without an instance, and both kinds of culled
    row (behind the camera, outside the frustum) present"""
    for cam_k in (1, 3):
        fw, _ = _oracle_run(3, False, False, cam_k)
        radii, ranges = fw["geo"]["radii"], fw["bins"]["ranges"]
        assert (radii == 0).mean() >= 0.10 and (radii > 0).sum() >= 100, (cam_k, (radii == 0).mean())
        assert ((ranges[:, 1] - ranges[:, 0]) == 0).sum() >= 1 and ((ranges[:, 1] - ranges[:, 0]) > 64).sum() >= 1
        assert len(ranges) == 5 * 4 and fw["bins"]["R"] > 500


class _RasterInputs:
    """device tensors of the scene, made once per configuration (outside every poisoned block)"""

    def __init__(self, pre_cov, pre_col, cam_k=1):
        sc, cam = _raster_scene(cam_k)
        self.sc, self.cam = sc, cam
        self.P, self.W, self.H = sc["means"].shape[0], cam["W"], cam["H"]
        self.bg, self.means, self.opac = T(BG), T(sc["means"]), T(sc["opac"])
        self.sh = None if pre_col else T(sc["shs"])
        self.col = T(sc["colors_precomp"]) if pre_col else None
        self.scales = None if pre_cov else T(sc["scales"])
        self.rots = None if pre_cov else T(sc["rots"])
        self.cov = T(sc["cov3D_precomp"]) if pre_cov else None
        self.view, self.proj, self.campos = T(cam["view"]), T(cam["proj"]), T(cam["campos"])
        self.dpix = T(_dpix())

    def forward(self, D, policy, workspace=None, aux=False, **finish):
        from gaussianmesh_amd import rasterizer as R
        cam = self.cam
        h = R.rasterize_forward_begin(self.bg, self.means, self.col, self.opac, self.scales, self.rots, 1.0, self.cov, self.view, self.proj,
                                      cam["tanx"], cam["tany"], self.H, self.W, self.sh, D, self.campos, False, False, workspace=workspace,
                                      emission_policy=policy, aux=aux)
        return h.finish(**finish)

    def backward(self, D, policy, fw, sh=None, **kw):
        from gaussianmesh_amd import rasterizer as R
        cam = self.cam
        nr, _, radii, geom, binning, img = fw[:6]
        return R.rasterize_backward(self.bg, self.means, radii, self.col, self.scales, self.rots, 1.0, self.cov, self.view, self.proj, cam["tanx"],
                                    cam["tany"], self.dpix, self.sh if sh is None else sh, D, self.campos, geom, nr, binning, img, False,
                                    emission_policy=policy, **kw)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _gate_backward(name, fill, grads, fw_out, D, pre_cov, pre_col, bw, fw, skip):
    """the non-deterministic route's assertions for ONE fill: grads = rasterize_backward's tuple (with dconic behind it if asked for)"""
    from test_gpu_parity import _grad_gate
    what = "%s under fill 0x%02X: " % (name, fill)
    radii = _np(fw_out[2])
    assert np.array_equal(radii, fw["geo"]["radii"]), what + "radii differ from the oracle"
    dm2, dcol, dop, dm3, dcov, dsh, dsc, drot = (_np(g) for g in grads[:8])
    dconic = _np(grads[8]) if len(grads) > 8 else None
    culled = radii == 0
    named = dict(dmeans2D=dm2, dcolors=dcol, dopac=dop, dmeans3D=dm3, dcov3D=dcov, dsh=dsh, dscales=dsc, drots=drot, dconic=dconic)
    for k, g in named.items():
        if g is None:
            continue
        assert np.isfinite(g).all(), what + "%s holds a non-finite value" % k
        rows = g.reshape(g.shape[0], -1)[culled]
        assert (rows == 0.0).all(), what + "%s: %d rows of culled Gaussians are not exactly 0.0 (largest |value| %g)" % (
            k, int((rows != 0).any(axis=1).sum()), float(np.abs(rows).max()))
    nc = (D + 1) ** 2
    if dsh is not None:
        assert (dsh[:, nc:] == 0.0).all(), what + "dL/dSH above the active degree %d is not exactly 0.0" % D
        assert np.abs(dsh[:, :nc]).max() > 0
        _grad_gate(dsh[:, :nc], bw["dsh"][:, :nc], what + "dsh")
    else:
        assert pre_col
    _grad_gate(dm3, bw["dmean3D"], what + "dmeans3D")
    _grad_gate(dm2[:, :2], bw["dmean2D"][:, :2], what + "dmeans2D")
    _grad_gate(dop.reshape(-1), bw["dopacity"], what + "dopac")
    if dcol is not None:
        _grad_gate(dcol, bw["dcolor"], what + "dcolors")
    if dcov is not None:
        _grad_gate(dcov, bw["dcov3D"], what + "dcov3D")
    if dsc is not None:
        _grad_gate(dsc, bw["dscale"], what + "dscales")
        _grad_gate(drot, bw["drot"], what + "drots")
    if dconic is not None:
        _grad_gate(dconic.reshape(-1, 4)[:, [0, 1, 3]], bw["dconic"][:, [0, 1, 3]], what + "dconic")
    assert (skip and not pre_col) == (dcol is None) and (skip and not pre_cov) == (dcov is None), what + "declined intermediates"


def _unused_slots(grads):
    """what the gate does not look at - dL/dmeans2D's z slot and dL/dconic's slot [1,0] - accumulates nothing: it has to be the same bits
    under every fill"""
    out = {"dmeans2D.z": grads[0][:, 2].clone()}
    if len(grads) > 8:
        out["dconic[1,0]"] = grads[8][:, 1, 0].clone()
    return out


RASTER_CASES = [
    # name,                 D, pre_cov, pre_col, policy, skip_intermediates, want_conic
    ("sh+scale-rot D3",     3, False, False, 2, False, True),
    ("sh+cov D3",           3, True,  False, 2, False, True),
    ("colour+scale-rot D3", 3, False, True,  2, False, True),
    ("colour+cov D3",       3, True,  True,  2, False, True),
    ("sh+scale-rot D3 skip", 3, False, False, 2, True, False),
    ("sh+cov D3 skip",      3, True,  False, 2, True,  False),
    ("sh+scale-rot D1",     1, False, False, 2, False, True),
    ("sh+scale-rot D1 skip", 1, False, False, 2, True, False),
    ("colour+cov D1 skip",  1, True,  True,  2, True,  False),
    ("policy 0",            3, False, False, 0, True,  False),      # the three emission policies test_backward_under_every_emission_policy uses
    ("policy 1",            3, False, False, 1, True,  False),
    ("policy 3",            3, False, False, 3, False, True),
]


@pytest.mark.parametrize("name,D,pre_cov,pre_col,policy,skip,want_conic", RASTER_CASES, ids=[c[0].replace(" ", "_") for c in RASTER_CASES])
def test_rasterizer_forward_and_backward(name, D, pre_cov, pre_col, policy, skip, want_conic):
    """no workspace: geometry, image and binning buffers of exactly gm_geom_bytes / gm_image_bytes / gm_binning_bytes, every gradient tensor"""
    inp = _RasterInputs(pre_cov, pre_col)
    fw, bw = _oracle_run(D, pre_cov, pre_col)

    def route():
        out = inp.forward(D, policy, exact_exponent=True)
        grads = inp.backward(D, policy, out, skip_intermediates=skip, want_conic=want_conic)
        torch.cuda.synchronize()
        nr, color, radii, geom, binning, img = out
        det = dict(nr=nr, color=color, radii=radii, unused=_unused_slots(grads),
                   scratch=_fields(geom, binning, img, inp.P, inp.W, inp.H, policy, nr, radii))
        return det, out, grads
    name = "raster " + name
    results = _run(name, route, compare=False)
    assert results[0][0]["nr"] > 0 and np.abs(_np(results[0][0]["color"]) - fw["color"]).max() <= 1e-4
    for fill, (det, out, grads) in zip(FILLS, results):
        _assert_same(name, FILLS[0], results[0][0], fill, det)
        _gate_backward(name, fill, grads, out, D, pre_cov, pre_col, bw, fw, skip)


def test_rasterizer_workspace_two_frames():
    """a fresh RasterWorkspace (requests padded by growth and 256 bytes) used for two consecutive frames - the second frame finds the first
    one's state in every buffer - then the backward of the second frame"""
    from gaussianmesh_amd import rasterizer as R
    D, policy = 3, 2
    a, b = _RasterInputs(False, False, 1), _RasterInputs(False, False, 3)
    fwb, bwb = _oracle_run(D, False, False, 3)
    fwa, _ = _oracle_run(D, False, False, 1)

    def route():
        ws = R.RasterWorkspace()
        o1 = a.forward(D, policy, workspace=ws, image_only=True)
        first = dict(nr=o1[0], color=o1[1].clone(), radii=o1[2].clone())
        o2 = b.forward(D, policy, workspace=ws, exact_exponent=True)
        grads = b.backward(D, policy, o2, skip_intermediates=True)
        torch.cuda.synchronize()
        det = dict(first=first, nr=o2[0], color=o2[1], radii=o2[2], unused=_unused_slots(grads),
                   scratch=_fields(o2[3], o2[4], o2[5], b.P, b.W, b.H, policy, o2[0], o2[2]))
        return det, o2, grads
    name = "raster workspace, two frames"
    results = _run(name, route, compare=False)
    assert np.array_equal(_np(results[0][0]["first"]["radii"]), fwa["geo"]["radii"])
    assert np.abs(_np(results[0][0]["first"]["color"]) - fwa["color"]).max() <= 1e-4
    for fill, (det, out, grads) in zip(FILLS, results):
        _assert_same(name, FILLS[0], results[0][0], fill, det)
        _gate_backward(name, fill, grads, out, D, False, False, bwb, fwb, True)


def test_rasterizer_sync_free_frame_on_a_workspace():
    """finish(sync_free=True): the kernels read the count on the device and the blend writes the status words; first frame exact (it sizes
    the binning buffer), second and third sync-free on the same workspace"""
    from gaussianmesh_amd import rasterizer as R
    inp = [_RasterInputs(False, False, k) for k in (1, 3)]

    def route():
        ws = R.RasterWorkspace()
        out = []
        first = inp[0].forward(3, 2, workspace=ws, image_only=True)
        out.append((first[0], first[1].clone(), first[2].clone()))
        for k in (1, 0):
            cam = inp[k].cam
            h = R.rasterize_forward_begin(inp[k].bg, inp[k].means, None, inp[k].opac, inp[k].scales, inp[k].rots, 1.0, None, inp[k].view, inp[k].proj,
                                          cam["tanx"], cam["tany"], 50, 70, inp[k].sh, 3, inp[k].campos, workspace=ws, emission_policy=2)
            r = h.finish(sync_free=True, image_only=True)
            ok, nr = h.check()
            assert ok and r[0] == -1
            out.append((nr, r[1].clone(), r[2].clone(), _fields(r[3], r[4], r[5], inp[k].P, 70, 50, 2, nr, r[2], image_only=True, capacity=ws.capacity)))
        torch.cuda.synchronize()
        return out
    res = _run("raster sync-free on a workspace", route)[0]
    assert res[0][0] == res[2][0] > 0 and torch.equal(res[0][1], res[2][1]) and torch.equal(res[0][2], res[2][2])      # the same frame, exact and sync-free
    assert np.array_equal(res[1][2].cpu().numpy(), _oracle_run(3, False, False, 3)[0]["geo"]["radii"])


def test_rasterizer_aux_maps_and_their_gradients():
    """aux=True: depth and alpha maps next to the image (gm_forward_1_aux), their gradients through gm_backward_aux.  The oracle's backward
    has no map terms, so this route's reference is test_gpu_aux_maps' dense float64 autograd (its own test's reference), under the same gate."""
    from test_gpu_aux_maps import _dense_reference
    from test_gpu_parity import _grad_gate
    D, policy = 3, 2
    inp = _RasterInputs(False, False)
    sc, cam = inp.sc, inp.cam
    rng = np.random.default_rng(4)
    gD = (rng.normal(size=(50, 70)) * 0.2).astype(np.float32)
    gA = rng.normal(size=(50, 70)).astype(np.float32)
    ref, _, ref_aux = _dense_reference(sc, cam, BG, D, False, _dpix(), gD, gA)
    dD, dA = T(gD), T(gA)

    def route():
        out = inp.forward(D, policy, aux=True, exact_exponent=True)
        grads = inp.backward(D, policy, out, dL_ddepth=dD, dL_dalpha=dA)
        torch.cuda.synchronize()
        det = dict(nr=out[0], color=out[1], radii=out[2], depth=out[6], alpha=out[7], unused=_unused_slots(grads),
                   scratch=_fields(out[3], out[4], out[5], inp.P, inp.W, inp.H, policy, out[0], out[2]))
        return det, grads
    name = "raster aux maps + gm_backward_aux"
    results = _run(name, route, compare=False)
    radii = _np(results[0][0]["radii"])
    assert np.array_equal(radii, ref_aux["radii"].numpy())
    for fill, (det, grads) in zip(FILLS, results):
        _assert_same(name, FILLS[0], results[0][0], fill, det)
        what = "%s under fill 0x%02X: " % (name, fill)
        dm2, dcol, dop, dm3, dcov, dsh, dsc, drot = (_np(g) for g in grads)
        for k, g in dict(dmeans2D=dm2, dcolors=dcol, dopac=dop, dmeans3D=dm3, dcov3D=dcov, dsh=dsh, dscales=dsc, drots=drot).items():
            assert np.isfinite(g).all() and (g.reshape(g.shape[0], -1)[radii == 0] == 0.0).all(), what + k
        for k, g, r in (("dmeans3D", dm3, ref["means"]), ("dopac", dop.reshape(-1), ref["opac"]), ("dmeans2D", dm2[:, :2], ref["m2d"]),
                        ("dscales", dsc, ref["scales"]), ("drots", drot, ref["rots"]), ("dsh", dsh, ref["shs"])):
            _grad_gate(g, r.numpy(), what + k)


def test_rasterizer_backward_with_the_sh_step():
    """gm_backward_sh_step: dL/dSH is not returned; the Adam step of the SH rows lands in the parameter and the moments.  Gradients under the
    oracle's gate; the moments against numpy's Adam of the ORACLE's dL/dSH at test_gpu_sh_step's bars (2e-3 / 4e-3 of the tensor's maximum);
    what the rule leaves alone - coefficients above the degree, rows behind `rows` - keeps its bits."""
    from gaussianmesh_amd import rasterizer as R
    from test_gpu_parity import _grad_gate
    D, policy, rows = 1, 2, 401
    inp = _RasterInputs(False, False)
    fw, bw = _oracle_run(D, False, False)
    sc = inp.sc
    rng = np.random.default_rng(6)
    nq = (D + 1) ** 2
    m0 = (1e-3 * rng.normal(size=(rows, 16, 3))).astype(np.float32)
    v0 = (1e-6 * rng.uniform(0.1, 1.0, size=(rows, 16, 3))).astype(np.float32)
    m0[:, nq:] = 0.0
    v0[:, nq:] = 0.0
    lr_dc, lr_rest, betas, eps, step = 2.5e-3, 1.25e-4, (0.9, 0.999), 1e-15, 7
    master = (T(sc["shs"]), T(m0), T(v0))

    def route():
        p, m, v = (t.clone() for t in master)                 # (clone: not an allocation the package makes; the step is in place)
        out = inp.forward(D, policy, exact_exponent=True)
        ss = R.ShStep(p[:rows], m, v, lr_dc, lr_rest, betas, eps, step)
        cam = inp.cam
        grads = R.rasterize_backward(inp.bg, inp.means, out[2], None, inp.scales, inp.rots, 1.0, None, inp.view, inp.proj, cam["tanx"], cam["tany"],
                                     inp.dpix, p, D, inp.campos, out[3], out[0], out[4], out[5], False, emission_policy=policy, sh_step=ss)
        torch.cuda.synchronize()
        assert ss.applied and grads[1] is None and grads[5] is None and grads[4] is None
        det = dict(nr=out[0], color=out[1], radii=out[2], unused=_unused_slots(grads),
                   scratch=_fields(out[3], out[4], out[5], inp.P, inp.W, inp.H, policy, out[0], out[2]))
        return det, grads, (p, m, v)
    name = "raster backward + SH Adam step"
    results = _run(name, route, compare=False)
    radii = _np(results[0][0]["radii"])
    g = np.asarray(bw["dsh"], np.float64)[:rows]
    b1, b2 = betas
    m1 = b1 * m0.astype(np.float64) + (1 - b1) * g
    v1 = b2 * v0.astype(np.float64) + (1 - b2) * g * g
    for fill, (det, grads, (p, m, v)) in zip(FILLS, results):
        _assert_same(name, FILLS[0], results[0][0], fill, det)
        what = "%s under fill 0x%02X: " % (name, fill)
        for k, i, r in (("dmeans2D", 0, bw["dmean2D"]), ("dopac", 2, bw["dopacity"]), ("dmeans3D", 3, bw["dmean3D"]), ("dscales", 6, bw["dscale"]),
                        ("drots", 7, bw["drot"])):
            got = _np(grads[i])
            assert np.isfinite(got).all() and (got.reshape(got.shape[0], -1)[radii == 0] == 0.0).all(), what + k
            _grad_gate(got[:, :2] if i == 0 else got.reshape(r.shape), r[:, :2] if i == 0 else r, what + k)
        pg, mg, vg = _np(p), _np(m), _np(v)
        assert np.isfinite(pg).all() and np.isfinite(mg).all() and np.isfinite(vg).all(), what + "parameter / moments"
        assert np.abs(mg[:, :nq] - m1[:, :nq]).max() <= 2e-3 * np.abs(m1[:, :nq]).max(), what + "exp_avg"
        assert np.abs(vg[:, :nq] - v1[:, :nq]).max() <= 4e-3 * np.abs(v1[:, :nq]).max(), what + "exp_avg_sq"
        assert np.array_equal(pg[:rows, nq:], sc["shs"][:rows, nq:]) and np.array_equal(mg[:, nq:], m0[:, nq:]) and np.array_equal(vg[:, nq:], v0[:, nq:])
        assert np.array_equal(pg[rows:], sc["shs"][rows:]) and np.abs(pg[:rows, :nq] - sc["shs"][:rows, :nq]).max() > 0.0


def test_rasterizer_autograd_operator():
    """GaussianRasterizer as the training loop calls it (fresh buffers, exact exponents, skip_intermediates): .grad of every leaf"""
    from gpu_utils import settings
    from gaussianmesh_amd import GaussianRasterizer
    D = 3
    sc, cam = _raster_scene()
    fw, bw = _oracle_run(D, False, False)
    rast = GaussianRasterizer(settings(cam, BG, D))
    dp = T(_dpix())

    def route():
        leaves = dict(means=T(sc["means"], True), opac=T(sc["opac"], True), shs=T(sc["shs"], True), scales=T(sc["scales"], True), rots=T(sc["rots"], True))
        m2d = torch.zeros_like(leaves["means"], requires_grad=True)
        color, radii = rast(leaves["means"], m2d, leaves["opac"], shs=leaves["shs"], scales=leaves["scales"], rotations=leaves["rots"])
        (color * dp).sum().backward()
        torch.cuda.synchronize()
        return dict(color=color.detach(), radii=radii, unused={"dmeans2D.z": m2d.grad[:, 2].clone()}), {k: v.grad for k, v in leaves.items()}, m2d.grad
    name = "raster autograd operator"
    results = _run(name, route, compare=False)
    from test_gpu_parity import _grad_gate
    for fill, (det, g, m2d) in zip(FILLS, results):
        _assert_same(name, FILLS[0], results[0][0], fill, det)
        what = "%s under fill 0x%02X: " % (name, fill)
        culled = _np(det["radii"]) == 0
        for k, r in (("means", bw["dmean3D"]), ("opac", bw["dopacity"]), ("shs", bw["dsh"]), ("scales", bw["dscale"]), ("rots", bw["drot"])):
            got = _np(g[k])
            assert (got.reshape(got.shape[0], -1)[culled] == 0.0).all(), what + k
            _grad_gate(got.reshape(r.shape), r, what + k)
        assert (_np(m2d)[culled] == 0.0).all(), what + "means2D"
        _grad_gate(_np(m2d)[:, :2], bw["dmean2D"][:, :2], what + "means2D")


# =====================================================================================================================================
# 2. the fused deformed forwards
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _fused_inputs(N=70):
    """The scene of test_fused_frame_edge_cases - torus_mesh(12, 8), N bound Gaussians, 96 x 64 - on a twisted mesh frame per batch item.
    That test's non-empty sizes are N = 1 and N = 70, the 70 moved BEHIND the camera; here the cloud stays in front of it (a frame that sees
    nothing has nothing to order, emit or blend).  forward_deformed runs at both sizes; the depth plan, the batches and the scene batch at
    N = 70 alone: one Gaussian gives the slab, the K frames and the background / object split of the scene batch nothing to hold."""
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.deform import mesh_rs_packed, vertex_face_adjacency
    verts, faces = scenes.torus_mesh(12, 8)
    cl = scenes.bind_cloud_to_mesh(N, verts, faces, seed=1)
    cov = scenes.cov3d_from_scale_rot(cl["scales"], cl["rots"]).astype(np.float32)
    W, H = 96, 64
    cams = []
    for k in (0, 1, 2):
        cam = scenes.orbit_camera(k, 4, W, H, radius=6.0)
        cams.append(dict(view=T(cam["view"]), proj=T(cam["proj"]), campos=T(cam["campos"]), tanx=cam["tanx"], tany=cam["tany"]))
    g = dict(tri=T(cl["tri"], dtype=torch.int32), w=T(cl["weights"]), cov=T(cov), pos=T(cl["means"]), shs=T(cl["shs"]), opac=T(cl["opac"]),
             verts=T(verts.astype(np.float32)), faces=T(faces, dtype=torch.int32), W=W, H=H, N=N, bg=T(np.array([0.2, 0.4, 0.6], np.float32)))
    off, adj = vertex_face_adjacency(faces, verts.shape[0])
    g["adjacency"] = (torch.tensor(off, device="cuda"), torch.tensor(adj, device="cuda"))
    g["v1"] = [T(scenes.twist_bend_frame(verts, t=t)[0].astype(np.float32)) for t in (3, 5, 8)]
    g["packed"] = [mesh_rs_packed(g["verts"], v1, g["faces"], g["adjacency"]) for v1 in g["v1"]]
    torch.cuda.synchronize()
    return g, cams


def _begin_deformed(g, cm, packed, **kw):
    from gaussianmesh_amd import rasterizer as R
    return R.forward_deformed_begin(g["bg"], g["tri"], g["w"], packed, g["cov"], g["pos"], g["shs"], g["opac"], cm["view"], cm["proj"], cm["tanx"],
                                    cm["tany"], g["H"], g["W"], 3, cm["campos"], **kw)


@pytest.mark.parametrize("image_only", [False, True])
@pytest.mark.parametrize("want_deformed", [False, True])
@pytest.mark.parametrize("N", [1, 70])
def test_forward_deformed(N, want_deformed, image_only):
    g, cams = _fused_inputs(N)

    def route():
        h = _begin_deformed(g, cams[0], g["packed"][0], want_deformed=want_deformed)
        nr, color, radii, geom, binning, img = h.finish(image_only=image_only)
        torch.cuda.synchronize()
        return dict(nr=nr, color=color, radii=radii, deformed=h.deformed,
                    scratch=_fields(geom, binning, img, g["N"], g["W"], g["H"], h.policy, nr, radii, image_only=image_only))
    res = _run("forward_deformed N=%d want_deformed=%d image_only=%d" % (N, want_deformed, image_only), route)[0]
    assert res["radii"].shape == (N,) and torch.isfinite(res["color"]).all()
    assert N == 1 or (res["nr"] > 0 and int((res["radii"] > 0).sum()) > 10)


@pytest.mark.parametrize("image_only", [False, True])
@pytest.mark.parametrize("want_deformed", [False, True])
def test_forward_deformed_with_a_depth_plan(want_deformed, image_only):
    """direct depth placement: the first frame of a stream leaves its table in the plan, the next ones place every visible Gaussian in its
    bucket's slab (the slab: torch.empty of gm_depth_slab_bytes).  Three frames, the slab from a workspace and without one; the scratch of
    every frame through SCRATCH_VIEWS (a directly placed frame has no depth_key / inst16: `direct`)."""
    from gaussianmesh_amd import rasterizer as R
    g, cams = _fused_inputs()

    def route():
        out = []
        for use_ws in (False, True):
            plan = R.new_depth_plan(g["pos"].device)               # (torch.zeros: the plan is armed by the caller)
            ws = R.RasterWorkspace() if use_ws else None
            for k in range(3):
                refused = plan.refused
                h = _begin_deformed(g, cams[k], g["packed"][k], want_deformed=want_deformed, depth_plan=plan, workspace=ws)
                began_direct = h.direct
                nr, color, radii, geom, binning, img = h.finish(image_only=image_only)
                torch.cuda.synchronize()
                direct = began_direct and plan.refused == refused          # (a refused frame was begun again on the partition path)
                out.append(dict(nr=nr, color=color.clone(), radii=radii.clone(), deformed=None if h.deformed is None else tuple(t.clone() for t in h.deformed),
                                direct=direct, scratch=_fields(geom, binning, img, g["N"], g["W"], g["H"], h.policy, nr, radii, image_only=image_only, direct=direct)))
        return out
    res = _run("forward_deformed + depth_plan (slab) want_deformed=%d image_only=%d" % (want_deformed, image_only), route)[0]
    plain = _begin_deformed(g, cams[1], g["packed"][1]).finish(image_only=True)
    assert torch.equal(res[1]["color"], plain[1]) and torch.equal(res[4]["color"], plain[1]) and res[1]["nr"] == plain[0]
    assert [r["direct"] for r in res] == [False, True, True] * 2               # the slab route was taken


@pytest.mark.parametrize("aux", [False, True])
@pytest.mark.parametrize("image_only", [True, False])
def test_forward_deformed_batch(image_only, aux):
    """K = 2 frames of one launch chain, plain and with the depth / alpha maps; the workspaces learn their capacity from one single frame"""
    from gaussianmesh_amd import rasterizer as R
    g, cams = _fused_inputs()

    def route():
        ws = [R.RasterWorkspace() for _ in range(2)]
        nr0 = _begin_deformed(g, cams[0], g["packed"][0], workspace=ws[0], aux=aux).finish(image_only=image_only)[0]
        ws[1].capacity = ws[0].capacity
        hs = R.forward_deformed_batch(g["bg"], g["tri"], g["w"], g["packed"][1:3], g["cov"], g["pos"], g["shs"], g["opac"], cams[1:3], g["H"], g["W"], 3,
                                      ws, image_only=image_only, aux=aux)
        out = [nr0]
        for h in hs:
            ok, nr = h.check()
            assert ok
            r = h.result
            out.append(dict(nr=nr, color=r[1], radii=r[2], maps=r[6:],
                            scratch=_fields(r[3], r[4], r[5], g["N"], g["W"], g["H"], h.policy, nr, r[2], image_only=image_only, capacity=h.workspace.capacity)))
        torch.cuda.synchronize()
        return out
    res = _run("forward_deformed_batch K=2 image_only=%d aux=%d" % (image_only, aux), route)[0]
    single = _begin_deformed(g, cams[2], g["packed"][2], aux=aux).finish(image_only=True)
    assert torch.equal(res[2]["color"], single[1]) and res[2]["nr"] == single[0] > 0
    if aux:
        assert torch.equal(res[2]["maps"][0], single[6]) and torch.equal(res[2]["maps"][1], single[7])


@pytest.mark.parametrize("image_only", [True, False])
def test_forward_scene_batch(image_only):
    """gm_forward_scene_batch_async, K = 2: 30 static background rows in front of 40 object rows; frame 0 deforms the object, frame 1 nothing;
    with image_only off the blend also owes final_T / n_contrib of every pixel"""
    from gaussianmesh_amd import rasterizer as R
    from gaussianmesh_amd.deform import cov_to_scale_rot
    g, cams = _fused_inputs()
    nbg, P = 30, g["N"]
    s, q = cov_to_scale_rot(g["cov"])
    tri, w, ocov = g["tri"][nbg:].contiguous(), g["w"][nbg:].contiguous(), g["cov"][nbg:].reshape(-1, 9).contiguous()
    torch.cuda.synchronize()

    def route():
        ws = [R.RasterWorkspace() for _ in range(2)]
        for w_ in ws:
            w_.capacity = 20000
        hs = R.forward_scene_batch(g["bg"], [nbg, P], [1, 0], g["pos"], s, q, g["shs"], g["opac"], tri, w, ocov, [g["packed"][1], None], cams[:2],
                                   g["H"], g["W"], 3, ws, image_only=image_only)
        out = []
        for h in hs:
            ok, nr = h.check()
            assert ok
            r = h.result
            out.append(dict(nr=nr, color=r[1], radii=r[2], scratch=_fields(r[3], r[4], r[5], P, g["W"], g["H"], h.policy, nr, r[2], image_only=image_only, capacity=h.workspace.capacity)))
        torch.cuda.synchronize()
        return out
    res = _run("forward_scene_batch K=2 image_only=%d" % image_only, route)[0]
    ref = R.rasterize_forward_begin(g["bg"], g["pos"], None, g["opac"], s, q, 1, None, cams[1]["view"], cams[1]["proj"], cams[1]["tanx"], cams[1]["tany"],
                                    g["H"], g["W"], g["shs"], 3, cams[1]["campos"], False, False, force_M=16).finish(image_only=True)
    assert res[1]["nr"] == ref[0] > 0 and torch.equal(res[1]["color"], ref[1]) and torch.equal(res[1]["radii"], ref[2])      # the frame at rest: the contract
    assert res[0]["nr"] > 0 and not torch.equal(res[0]["color"], res[1]["color"])


# =====================================================================================================================================
# 3. deform.py
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _deform_inputs(N):
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.deform import pack_mesh_state, vertex_face_adjacency
    verts, faces = scenes.torus_mesh(12, 8)
    cl = scenes.bind_cloud_to_mesh(N, verts, faces, seed=4)
    V1, Rv, Sv = scenes.twist_bend_frame(verts, t=9)
    cov = scenes.cov3d_from_scale_rot(cl["scales"], cl["rots"]).astype(np.float32)
    state = np.concatenate([V1.astype(np.float32), Rv.reshape(-1, 9), Sv.reshape(-1, 9)], axis=1).astype(np.float32)
    d = dict(tri=T(cl["tri"], dtype=torch.int32), w=T(cl["weights"]), dV=T((V1 - verts).astype(np.float32)), Rv=T(Rv), Sv=T(Sv), cov=T(cov),
             pos=T(cl["means"]), shs=T(cl["shs"]), campos=T(np.array([4.0, 1.0, -3.0], np.float32)), verts=T(verts.astype(np.float32)),
             state=T(state))
    d["packed"] = pack_mesh_state(d["state"], d["verts"])
    rng = np.random.default_rng(N)
    q = rng.normal(size=(N, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q.T
    d["rot"] = T(np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                           2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(N, 3, 3))
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("N", [1, 65, 257])
def test_deform_operators(N):
    """deform_tensors, sh_colors (with and without the rotation), deform_shade (packed and not, with and without cov / rot), pack_mesh_state,
    cov_to_scale_rot, rotate_sh out of place and in place"""
    from gaussianmesh_amd import deform as df
    d = _deform_inputs(N)

    def route():
        out = {}
        out["deform_tensors"] = df.deform_tensors(d["tri"], d["w"], d["dV"], d["Rv"], d["Sv"], d["cov"], d["pos"])
        pos, cov, rot, _ = out["deform_tensors"]
        out["sh_colors"] = (df.sh_colors(pos, d["campos"], d["shs"], rot=rot, deg=3), df.sh_colors(d["pos"], d["campos"], d["shs"], deg=1))
        args = (d["tri"], d["w"], d["dV"], d["Rv"], d["Sv"], d["cov"], d["pos"], d["shs"], d["campos"])
        out["deform_shade"] = (df.deform_shade(*args, deg=3, want_cov_rot=True), df.deform_shade(*args, deg=2))
        pargs = (d["tri"], d["w"], d["packed"], d["cov"], d["pos"], d["shs"], d["campos"])
        out["deform_shade_packed"] = (df.deform_shade_packed(*pargs, deg=3, want_cov_rot=True), df.deform_shade_packed(*pargs, deg=0))
        out["pack_mesh_state"] = df.pack_mesh_state(d["state"], d["verts"])
        out["cov_to_scale_rot"] = df.cov_to_scale_rot(cov)
        out["rotate_sh"] = (df.rotate_sh(d["shs"], d["rot"], deg=3), df.rotate_sh(d["shs"], d["rot"], deg=1))
        mine = torch.empty_like(d["shs"])                      # in place: the operand is its own output (here a poisoned tensor, copied into first)
        mine.copy_(d["shs"])
        out["rotate_sh in place"] = df.rotate_sh(mine, d["rot"], deg=3, out=mine)
        torch.cuda.synchronize()
        return out
    res = _run("deform.py N=%d" % N, route)[0]
    assert torch.equal(res["rotate_sh in place"], res["rotate_sh"][0]) and torch.equal(res["pack_mesh_state"], d["packed"])
    assert torch.equal(res["deform_shade"][0][0], res["deform_tensors"][0]) and torch.equal(res["deform_shade"][0][1], res["deform_tensors"][3])


@pytest.mark.parametrize("Vm", [1, 65, 257])
def test_mesh_rs_operators(Vm):
    """mesh_rs (with and without the state record), mesh_rs_packed, the packed batch (K = 3) on mesh_rs_cases' zigzag strip of Vm vertices
    (Vm = 1: one vertex and no face; 65 and 257: one row past a wave / a workgroup), one frame of it squashed flat"""
    import mesh_rs_cases as mc
    from gaussianmesh_amd import deform as df
    V0, faces = mc.strip(Vm)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    frames = [T(mc.affine(V0, s)[0]) for s in ((1.3, 0.9, 0.7), (1.0, 1.0, 1e-7), (2.0, 0.5, 1.0))]
    v0, f = T(V0.astype(np.float32)), T(faces, dtype=torch.int32)
    off, adj = df.vertex_face_adjacency(faces, Vm)
    adjacency = (torch.tensor(off, device="cuda"), torch.tensor(adj, device="cuda"))
    torch.cuda.synchronize()

    def route():
        out = dict(rs=df.mesh_rs(v0, frames[0], f, adjacency=adjacency), rs_state=df.mesh_rs(v0, frames[1], f, adjacency=adjacency, want_state=True),
                   packed=df.mesh_rs_packed(v0, frames[0], f, adjacency), batch=df.mesh_rs_packed_batch(v0, frames, f, adjacency))
        torch.cuda.synchronize()
        return out
    res = _run("mesh_rs strip Vm=%d" % Vm, route)[0]
    assert torch.equal(res["batch"][0], res["packed"]) and res["packed"].shape == (Vm, 24)
    assert torch.equal(res["packed"], df.pack_mesh_state(df.mesh_rs(v0, frames[0], f, adjacency=adjacency, want_state=True)[2], v0))


# =====================================================================================================================================
# 4. loss.py
# =====================================================================================================================================
@pytest.mark.parametrize("shape", [(3, 17, 33), (3, 50, 70)])
def test_loss_operators(shape):
    """SSIM / L1 forward with and without the derivative maps, the backward, gm_loss_combine, and the u8 target with no mask, a one-plane mask
    and a three-plane mask.  Both sizes leave partial tiles on the right and at the bottom."""
    from gaussianmesh_amd import loss as L
    from gaussianmesh_amd.dataset import GroundTruth
    rng = np.random.default_rng(shape[1])
    a0, b0 = T(rng.uniform(0, 1, shape)), T(rng.uniform(0, 1, shape))
    rgb = torch.tensor(rng.integers(0, 256, shape), dtype=torch.uint8, device="cuda")
    m1 = torch.tensor(rng.integers(0, 256, (1,) + shape[1:]), dtype=torch.uint8, device="cuda")
    m3 = torch.tensor(rng.integers(0, 256, shape), dtype=torch.uint8, device="cuda")
    bgc = T(np.array([0.9, 0.1, 0.4], np.float32))
    up = T(rng.normal(size=()))
    torch.cuda.synchronize()

    def route():
        out = {}
        out["_fwd no grad"] = L._fwd(a0, b0, False)[3]
        a, b, maps, partial = L._fwd(a0, b0, True)
        out["_fwd grad"] = (maps, partial)
        gp = torch.full((3,), 1.0 / a.numel(), device="cuda")
        out["_bwd"] = (L._bwd(a, b, maps, gp, None), L._bwd(a, b, maps, gp, torch.full((1,), 0.25, device="cuda")))
        with torch.no_grad():
            out["no grad"] = (L.ssim(a0, b0), L.photometric_loss(a0, b0, 0.2), L.photometric_loss_u8(a0, GroundTruth(rgb, m1), bgc, 0.2))
        for name, f in (("ssim", lambda x: L.ssim(x, b0)), ("ssim per image", lambda x: L.ssim(x[None], b0[None], size_average=False).sum()),
                        ("photometric", lambda x: L.photometric_loss(x, b0, 0.2)),
                        ("u8", lambda x: L.photometric_loss_u8(x, GroundTruth(rgb), None, 0.2)),
                        ("u8 mask1", lambda x: L.photometric_loss_u8(x, GroundTruth(rgb, m1), bgc, 0.2)),
                        ("u8 mask3", lambda x: L.photometric_loss_u8(x, GroundTruth(rgb, m3), bgc, 0.35))):
            x = a0.clone().requires_grad_(True)
            y = f(x)
            (y * up).backward()
            out[name] = (y.detach(), x.grad)
        torch.cuda.synchronize()
        return out
    res = _run("loss.py %dx%dx%d" % shape, route)[0]
    assert torch.isfinite(res["photometric"][1]).all() and res["photometric"][1].abs().max() > 0
    assert torch.equal(res["no grad"][2], res["u8 mask1"][0]) and torch.equal(res["no grad"][1], res["photometric"][0])


# =====================================================================================================================================
# 5. model_ops.py
# =====================================================================================================================================
@pytest.mark.parametrize("N", [1, 257])
def test_model_ops(N):
    """mesh_activate (with the fused restrict term) and plain_activate forward and backward, FusedAdam.step (gm_adam_step_active with and without
    `active`), FusedAdam.resize (its torch.empty rows), densify_stats (in place: no allocation of its own - its accumulators are poisoned
    tensors written first, as the trainer's torch.zeros are)"""
    import ctypes as C
    from gaussianmesh_amd import _lib, model_ops as mo
    from test_gpu_model_ops import _inputs
    ins = _inputs(N, seed=N)
    order = ("bc", "dist", "scaling", "rot", "opac", "v1", "v2", "v3", "n", "r")
    dev = {k: ins[k].detach() for k in order}
    rng = np.random.default_rng(N + 1)
    ups = [T(rng.normal(size=s)) for s in ((N, 3), (N, 3), (N, 4), (N, 1))]
    plain = [T(rng.normal(size=s)) for s in ((N, 3), (N, 3), (N, 4), (N, 1))]
    sh0, g_sh = T(rng.normal(size=(N, 16, 3))), T(rng.normal(size=(N, 16, 3)))
    xyz0, g_xyz = T(rng.normal(size=(N, 3))), T(rng.normal(size=(N, 3)))
    radii = torch.tensor(rng.integers(0, 5, N), dtype=torch.int32, device="cuda")
    vgrad = T(rng.normal(size=(N, 3)))
    new = min(3, N)                                              # rows appended by resize()
    torch.cuda.synchronize()

    def route():
        out = {}
        leaves = [dev[k].clone().requires_grad_(True) for k in order[:5]]
        outs = mo.mesh_activate(*leaves, *[dev[k] for k in order[5:]], alpha=4.0, mr_weight=10.0)
        (sum((o * u).sum() for o, u in zip(outs[:4], ups)) + 0.5 * outs[4]).backward()
        out["mesh_activate"] = ([o.detach() for o in outs], [l.grad for l in leaves])
        leaves = [p.clone().requires_grad_(True) for p in plain]
        outs = mo.plain_activate(*leaves)
        sum((o * u).sum() for o, u in zip(outs, ups)).backward()
        out["plain_activate"] = ([o.detach() for o in outs], [l.grad for l in leaves])
        p_sh, p_xyz = torch.nn.Parameter(sh0.clone()), torch.nn.Parameter(xyz0.clone())
        opt = mo.FusedAdam([dict(params=[p_xyz], lr=1e-3, name="xyz"),
                            dict(params=[p_sh], lr=2.5e-3, lr_rest=1.25e-4, period=48, split=3, active=12, name="f_dc+f_rest")], eps=1e-15)
        for _ in range(2):
            p_sh.grad, p_xyz.grad = g_sh.clone(), g_xyz.clone()
            opt.step()
        out["adam"] = [(g["params"][0].detach().clone(), g["m"][0].clone(), g["values"][0].clone()) for g in opt.param_groups]
        keep = torch.arange(N, device="cuda") % 2 == 0
        grown = opt.resize(keep=keep, new_rows={"xyz": xyz0[:new], "f_dc+f_rest": sh0[:new]})
        out["resize"] = [(grown[g["name"]].detach(), g["m"][0], g["values"][0]) for g in opt.param_groups]
        acc = [torch.empty((N,), dtype=torch.float32, device="cuda") for _ in range(3)]
        for t in acc:
            t.fill_(0.5)
        mo.densify_stats(radii, vgrad, *acc)
        out["densify_stats"] = acc
        # gm_adam_step itself (FusedAdam goes through gm_adam_step_active): no wrapper allocates for it, so parameter, gradient and moments
        # are poisoned tensors written first - what the guard bands watch is the kernel's own stores at the ends of the tensor
        n = 48 * N
        p_, g_, m_, v_ = (torch.empty((n,), dtype=torch.float32, device="cuda") for _ in range(4))
        for dst, src in ((p_, sh0), (g_, g_sh), (m_, 0.1 * g_sh), (v_, 1e-3 * sh0.abs())):
            dst.copy_(src.reshape(-1))
        one = lambda ty, v: (ty * 1)(v)
        _lib.check(_lib.lib().gm_adam_step(1, one(C.c_void_p, p_.data_ptr()), one(C.c_void_p, g_.data_ptr()), one(C.c_void_p, m_.data_ptr()),
                                           one(C.c_void_p, v_.data_ptr()), one(C.c_uint64, n), one(C.c_float, 2.5e-3), one(C.c_float, 1.25e-4),
                                           one(C.c_uint32, 48), one(C.c_uint32, 3), 0.9, 0.999, 1e-15, 3, torch.cuda.current_stream().cuda_stream))
        out["gm_adam_step"] = (p_, m_, v_)
        torch.cuda.synchronize()
        return out
    res = _run("model_ops.py N=%d" % N, route)[0]
    assert res["resize"][0][0].shape[0] == (N + 1) // 2 + new and torch.isfinite(res["adam"][1][0]).all()
    assert torch.isfinite(res["gm_adam_step"][0]).all() and not torch.equal(res["gm_adam_step"][0], sh0.reshape(-1))
    assert torch.equal(res["adam"][1][0][:, 4:], sh0[:, 4:])                     # `active` = 12 elements of every 48: coefficients 4 .. 15 untouched


# =====================================================================================================================================
# 6. search and geometry operators
# =====================================================================================================================================
@pytest.mark.parametrize("P", [5, 1025, 4097])
def test_dist_cuda2(P):
    """more than one 1024-point box, a partial last box; P = 5: fewer points than a box, more than the three neighbours"""
    from gaussianmesh_amd import distCUDA2
    from oracle import oracle as orc
    rng = np.random.default_rng(P)
    pts = rng.normal(size=(P, 3)).astype(np.float32) * np.array([3, 1, 0.2], np.float32)
    dev = T(pts)
    res = _run("distCUDA2 P=%d" % P, lambda: distCUDA2(dev))[0]
    assert np.array_equal(res.cpu().numpy().view(np.uint32), orc.knn_mean_dist2(pts).view(np.uint32))


@pytest.mark.parametrize("Pq,Pr", [(777, 333), (300, 2000)])
def test_knn_nearest(Pq, Pr):
    from gaussianmesh_amd.simple_knn import knn_nearest
    rng = np.random.default_rng(Pq + Pr)
    q, r = rng.normal(size=(Pq, 3)).astype(np.float32), rng.normal(size=(Pr, 3)).astype(np.float32)
    r[7] = r[3]                                                 # a tie: the lowest index wins
    q[0] = r[7]
    dq, dr = T(q), T(r)
    d2, idx = _run("knn_nearest (%d, %d)" % (Pq, Pr), lambda: knn_nearest(dq, dr))[0]
    d = q[:, None, :] - r[None, :, :]
    brute = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(np.float32)
    assert np.array_equal(idx.cpu().numpy(), brute.argmin(axis=1)) and int(idx[0]) == 3
    assert np.array_equal(d2.cpu().numpy().view(np.uint32), brute.min(axis=1).view(np.uint32))


@pytest.mark.parametrize("N,F,kind", [(300, 2400, "grid_ties"), (777, 333, "degenerate_far")])
def test_closest_faces(N, F, kind):
    import closest_ref as cr
    from gaussianmesh_amd.mesh_bind import closest_faces
    from test_gpu_mesh_bind import _case, _same
    V, faces, P = _case(kind, N, F, seed=N + F)
    pts = T(P)
    res = _run("closest_faces (%d, %d) %s" % (N, F, kind), lambda: closest_faces(pts, V, faces, want_closest=True))[0]
    _same(tuple(x.cpu().numpy() for x in res), cr.closest_face_ref(P, V, faces), kind)


def test_ray_caster():
    """the smallest case of test_gpu_raycast's size table that has more than one face chunk and a partial wave: F = 65, R = 65; and
    mesh_pick.pick / visible_vertices on it (want_uv on and off)"""
    import ray_ref as rr
    from gaussianmesh_amd import mesh_pick, scenes
    from test_gpu_raycast import _same
    F, R = 65, 65
    rng = np.random.default_rng(1000 + F)
    V, faces = rr.torus(F)
    O, D = rr.torus_rays(V, faces, R, rng)
    o, d = T(O), T(D)
    from gaussianmesh_amd.renderer import Camera
    camera = Camera(scenes.look_at_camera((4, 3, 5), (0, 0, 0), 64, 48), "cuda")
    pix = T(np.stack(np.meshgrid(np.arange(0, 64, 7), np.arange(0, 48, 5)), -1).reshape(-1, 2))
    vd, fd = T(V), T(faces, dtype=torch.int32)
    torch.cuda.synchronize()

    def route():
        out = dict(hits=mesh_pick.ray_mesh_hits(o, d, V, faces), pick=mesh_pick.pick(camera, pix, vd, fd, check_faces=False),
                   visible=mesh_pick.visible_vertices(camera, vd, fd, check_faces=False))
        torch.cuda.synchronize()
        return out
    res = _run("ray caster F=%d R=%d" % (F, R), route)[0]
    _same(tuple(x.cpu().numpy() for x in res["hits"]), rr.ray_mesh_ref(O, D, V, faces), "torus")


def test_geodesic_distances():
    """B = 2 source sets on a path of 100 vertices in chunks of 64 sweeps: the first call fills and arms, the second is a `resume` call
    (the counters alone are armed again); the workspace is the graph's own, made by its first call"""
    import geodesic_ref as gr
    from gaussianmesh_amd.mesh_region import SurfaceGraph
    n = 100
    lens = np.random.default_rng(7).uniform(0.1, 1.0, size=n - 1).astype(np.float32)
    edges = {}
    for k in range(n - 1):
        edges[(k, k + 1)] = edges[(k + 1, k)] = lens[k]
    csr = gr.csr_of(n, edges)
    sets = [[0], [50, 99]]

    def route():
        g = SurfaceGraph.from_csr(*csr)
        a = g.distances(sets, sweeps_per_check=64)
        first = g.sweeps_enqueued
        b = g.distances(sets[:1], max_distance=3.0, sweeps_per_check=64)      # the kept workspace, with a cutoff
        torch.cuda.synchronize()
        return dict(dist=a, sweeps=first, cut=b)
    res = _run("geodesic B=2 with a resume call", route)[0]
    assert res["sweeps"] == 100                                  # 64 + 36: the budget Vm in two chunks, the second through `resume`
    ref = gr.dijkstra32(*csr, sets)
    assert np.array_equal(res["dist"].cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(res["cut"].cpu().numpy().view(np.uint32), gr.dijkstra32(*csr, sets[:1], 3.0).view(np.uint32))


def test_tsdf_integrate_and_surface_nets():
    """TsdfVolume on the smallest grid of test_gpu_tsdf whose surface is not trivial and whose scan has more than one workgroup (20 x 7 x 18 =
    2520 samples, SN_BLOCK = 256): two integrate calls from ray-cast maps of a small torus, then extract(keep="all") - V[:nv], F[:nf], the rows the counts cover"""
    import tsdf_ref as tr
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.proxy_mesh import TsdfVolume
    cams = [scenes.orbit_camera(k, 3, 40, 30, radius=3.0) for k in range(3)]
    sv, sf = scenes.torus_mesh(12, 8)
    sv = (np.asarray(sv, np.float64) * 0.3).astype(np.float32)
    depth, alpha, views, tans = tr.raycast_maps(cams, sv, np.asarray(sf, np.int32))
    d_dev, a_dev = T(depth), T(alpha)
    lo, hi = np.array([-1.0, -0.35, -0.9]), np.array([1.0, 0.35, 0.9])
    torch.cuda.synchronize()

    def route():
        vol = TsdfVolume(lo, hi, voxel_size=0.1, trunc=0.3)     # (tsdf / weight: torch.zeros, part of the definition)
        vol.integrate(cams[:2], d_dev[:2], a_dev[:2])
        vol.integrate(cams[2:], d_dev[2:], a_dev[2:], carve=False)
        V, F = vol.extract(min_weight=1, keep="all")
        small = vol._surface_nets(1, 5, 7)                        # capacities short of the need: the prefix and the counts
        torch.cuda.synchronize()
        return dict(tsdf=vol.tsdf, weight=vol.weight, V=V, F=F, stats=(vol.stats["vertices"], vol.stats["faces"]), nx=(vol.nx, vol.ny, vol.nz),
                    short=(small[0][:min(small[2], 5)], small[1][:min(small[3], 7)], small[2], small[3]))
    res = _run("TSDF integrate + surface nets", route)[0]
    assert res["nx"] == (20, 7, 18) and res["stats"][0] > 500 and res["stats"][1] > 1000 and res["short"][2:] == res["stats"]
    o32, vox, trunc = np.asarray(lo, np.float32), np.float32(0.1), np.float32(0.3)
    vol = tr.integrate_ref(np.zeros((18, 7, 20), np.float32), np.zeros((18, 7, 20), np.float32), depth[:2], alpha[:2], views[:2], tans[:2], o32, vox, trunc)
    vol = tr.integrate_ref(vol[0], vol[1], depth[2:], alpha[2:], views[2:], tans[2:], o32, vox, trunc, carve=False)
    assert np.array_equal(res["tsdf"].cpu().numpy().view(np.uint32), vol[0].view(np.uint32)) and np.array_equal(res["weight"].cpu().numpy(), vol[1])
    rv, rf = tr.surface_nets_ref(res["tsdf"].cpu().numpy(), res["weight"].cpu().numpy(), np.asarray(lo, np.float32), np.float32(0.1), 1.0)[:2]
    assert np.array_equal(res["V"].cpu().numpy().view(np.uint32), np.asarray(rv, np.float32).view(np.uint32))
    assert np.array_equal(res["F"].cpu().numpy(), np.asarray(rf, np.int32))


# =====================================================================================================================================
# 7. ARAP
# =====================================================================================================================================
@pytest.mark.parametrize("global_step", ["column", "grid"])
@pytest.mark.parametrize("mesh", ["fan", "torus_a"])
def test_arap_solver(mesh, global_step):
    """ArapSolver on the smallest mesh of arap_cases (fan: 41 vertices, one ring of valence 40, less than a wave) and on the smallest closed
    one (torus_a: 96 vertices, a partial second wave): the workspace of the column step is made by the constructor, the
    grid step's by its first solve; a second solve on the same solver finds the first one's state in the kept workspace; solve_batch
    (B = 3) makes its workspace, B = 5 makes it grow, B = 2 fits the grown one; solve_sequence allocates its [T, Vm, 3] result"""
    import arap_cases as ac
    from gaussianmesh_amd.arap import ArapSolver
    c = ac.case(mesh)
    tg = T(c["targets"])
    rng = np.random.default_rng(3)
    many = T(c["targets"][None] + 0.05 * rng.normal(size=(5,) + c["targets"].shape))
    torch.cuda.synchronize()

    def route():
        s = ArapSolver(c["V0"], c["faces"], c["handles"])
        out = {}
        out["first"] = s.solve(tg, global_step=global_step).clone()
        out["second"], out["stats"] = s.solve(many[1], init=out["first"], outer_iterations=2, cg_iterations=20, want_stats=True, global_step=global_step)
        out["batch 3"] = s.solve_batch(many[:3], global_step=global_step).clone()
        out["batch 5"], out["batch stats"] = s.solve_batch(many, init=out["first"], outer_iterations=2, want_stats=True, global_step=global_step)
        out["batch 2"] = s.solve_batch(many[3:], global_step=global_step)
        out["sequence"] = s.solve_sequence(many, batch=2, outer_iterations=2, global_step=global_step)
        out["sequence of one"] = s.solve_sequence(many[:2], batch=1, outer_iterations=1, cg_iterations=8, global_step=global_step)
        torch.cuda.synchronize()
        return out
    res = _run("ArapSolver %s %s" % (mesh, global_step), route)[0]
    assert torch.equal(res["batch 2"][0], ArapSolver(c["V0"], c["faces"], c["handles"]).solve(many[3], global_step=global_step))    # an item is a single solve, bit for bit
    assert torch.equal(res["first"][T(c["handles"], dtype=torch.int64)], tg)                             # the handles sit exactly on their targets
    assert all(torch.isfinite(res[k]).all() for k in ("first", "second", "stats", "batch 3", "batch 5", "batch stats", "sequence", "sequence of one"))
