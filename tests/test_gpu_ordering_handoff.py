"""The hand-off of the emission records inside the ordering (gm_bucket.hip / gm_binning.hip): bucket_sort_kernel<false> gathers the 2-byte
instance count GeomState::inst16[id] and writes the order alone; duplicate_kernel reads the emission record where the preprocess kernel
wrote it, bin[order[s]] (a frame of the direct depth placement still reads bin_sorted, which only that path fills).  The cases walk the
emission's and the tile sort's routes behind that gather: wave and run edges, zero and saturated counts, staged and unstaged output, one
and two tile passes, exact and short capacity, batches, the direct placement.

Every GPU case is compared with the ORACLE's preprocess, lists and image: num_rendered, point_list, tile keys and tile ranges bit for bit
under policy 0; under the culled policies 1-3 (the oracle has no lists for them) the entries each 16-px tile takes are an order-preserving
part of the oracle's list that holds every instance some pixel accepts (oracle.instance_needed), policy 1's lists are exactly that part,
and the image passes the forward gate against the oracle's image.  Comparisons between two runs of the library (a batch frame against its
single-frame call) come on top of that, never instead.

The saturated case: issue and kernel speak of a count of 65534 beside one of 65535 or more.  Under policy 0 a count is the area w x h of a
tile rectangle inside a grid of at most 65536 tiles (gm_forward_1_geom refuses more); 65534 = 2 * 7 * 31 * 151 has no factor pair that fits
a grid which also holds a rectangle of >= 65535 tiles (255 x 257, 32 x 2048, 64 x 1024, 128 x 512, 256 x 256), so the neighbour here is the
LARGEST count below saturation such a grid allows, 255 x 256 = 65280 (0xFF00: the top byte of inst16 in use), asserted on the oracle."""
import numpy as np
import pytest
import torch

import ordering_scenes as S

FWD_TOL = 1e-4
BG = np.array([0.2, 0.3, 0.4], np.float32)
SH_C0 = np.float32(0.28209479177387814)
EDGE_W, EDGE_H = 128, 96
EDGE_P = (1, 63, 64, 65, 511, 512, 513, 4097)


# ----------------------------------------------------------------------------------------------
# scenes
def edge_scene(P, W=EDGE_W, H=EDGE_H, seed=0, holes=True, big=0, sfac_mid=0.045):
    """P Gaussians over three coarse depth bins, two of three one tile wide and the others rectangles of a few tiles (sfac_mid: a standard deviation of 5 pixels at 128 x 96), some depths equal
    (ties go by id).  holes: every fifth row (1, 6, ..) has an opacity below 1/255 - visible, and under the culled policies it emits
    nothing - and every seventh (3, 10, ..) lies behind the camera, so records with a count of 0 sit between live ones.  big: that many
    rows cover the whole frame."""
    rng = np.random.default_rng(4000 + P + seed)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    keys = ((S.BIN0 << S.COARSE_SHIFT) + rng.integers(0, 3 << S.COARSE_SHIFT, P)).astype(np.uint32)
    if P >= 8:
        keys[rng.integers(0, P, P // 8)] = keys[rng.integers(0, P, P // 8)]
    sfac = np.where(rng.random(P) < 0.66, 5e-5, sfac_mid)
    if big:
        sfac[rng.choice(np.arange(P), big, replace=False)] = 3.0
    sc = S.build(W, H, rng.integers(0, gx * gy, P), keys, sfac=sfac, seed=seed)
    sc["opac"][:] = rng.uniform(0.05, 0.6, (P, 1)).astype(np.float32)
    if holes:
        sc["opac"][1::5] = 0.001
        sc["means"][3::7, 2] *= -1.0
    return sc


def saturated_pair_scene():
    """ordering_scenes.saturated_scene() (4096 x 4096, one Gaussian on all 65536 tiles) with a second large Gaussian whose rectangle misses
    the leftmost tile column alone: 255 x 256 = 65280 instances, carried by inst16 itself"""
    sc = S.saturated_scene()
    j = int(np.nonzero(sc["sfac"] < 1e-3)[0][5])
    cam, W = sc["cam"], sc["W"]
    z = float(sc["means"][j, 2])
    fx = W / (2.0 * cam["tanx"])
    px = 6096.0                                           # centre right of the frame; the radius reaches x = 24: first tile column 1
    ndcx = (2 * px + 1) / W - 1
    # the projected covariance of an isotropic Gaussian off the axis: (fx s / z)^2 (I + t t^T), t = (x / z, y / z) clamped to 1.3 tan(fov / 2)
    # (forward.cu:74-104): its larger eigenvalue is 1 + |t|^2 times the on-axis one
    tx = min(1.3 * cam["tanx"], abs(ndcx) * cam["tanx"]); ty = min(1.3 * cam["tany"], abs(float(sc["means"][j, 1])) / z)
    std_px = (px - 24.0) / 3.0 / np.sqrt(1.0 + tx * tx + ty * ty)
    s = std_px / fx * z
    sc["means"][j, 0] = np.float32(cam["view"][0, 0] * ndcx * cam["tanx"] * z)
    sc["cov3D_precomp"][j] = 0.0
    sc["cov3D_precomp"][j, [0, 3, 5]] = np.float32(s * s)
    return sc, j


# ----------------------------------------------------------------------------------------------
# the oracle's side, once per scene
_ORACLE = {}


def _oracle(orc, name, sc):
    if name not in _ORACLE:
        geo = S.oracle_geo(orc, sc)
        bins = orc.bin_instances(geo, sc["W"], sc["H"])
        color, fT, nc = orc.render_fwd(sc["W"], sc["H"], bins, geo, BG)
        vis = np.nonzero(geo["radii"] > 0)[0]
        d = geo["depths"].view(np.uint32)[vis].astype(np.int64)
        order = vis[np.lexsort((vis, d))].astype(np.uint32)
        for a in (color, order, bins["point_list"], bins["keys"], bins["ranges"]):
            a.setflags(write=False)
        _ORACLE[name] = dict(geo=geo, bins=bins, color=color, order=order, needed=None)
    return _ORACLE[name]


def _needed(orc, ref, W, H):
    if ref["needed"] is None:
        ref["needed"] = orc.instance_needed(W, H, ref["bins"], ref["geo"]).astype(bool)
    return ref["needed"]


def _ranges_of(keys, tiles):
    """{first, one past last} per tile of a sorted key column, {0, 0} for an empty list (the reference's convention)"""
    lo = np.searchsorted(keys, np.arange(tiles), "left"); hi = np.searchsorted(keys, np.arange(tiles), "right")
    r = np.stack([lo, hi], 1).astype(np.uint32)
    r[lo == hi] = 0
    return r


def assert_lists(orc, ref, W, H, P, mode, R, order, tile_keys, child_mask, point_list, ranges, what):
    """the ordering's outputs against the oracle (module docstring)"""
    bins = ref["bins"]
    assert np.array_equal(order, ref["order"]), "%s: (depth bits, id) order" % what
    tile_ref = (bins["keys"] >> np.uint64(32)).astype(np.uint32)
    if mode == 0:
        assert R == bins["R"], "%s: num_rendered %d, oracle %d" % (what, R, bins["R"])
        assert np.array_equal(point_list, bins["point_list"]), "%s: point_list" % what
        assert np.array_equal(tile_keys, tile_ref) and (child_mask == 1).all(), "%s: keys" % what
        assert np.array_equal(ranges, bins["ranges"]), "%s: ranges" % what
        return
    sh = mode - 1
    gx, gy = (W + 15) // 16, (H + 15) // 16
    pgx, pgy = (gx + (1 << sh) - 1) >> sh, (gy + (1 << sh) - 1) >> sh
    assert R <= bins["R"] and point_list.size == R
    assert (np.diff(tile_keys.astype(np.int64)) >= 0).all(), "%s: keys not sorted" % what
    assert np.array_equal(ranges, _ranges_of(tile_keys, pgx * pgy)), "%s: ranges do not delimit the lists" % what
    rank = np.full(P, -1, np.int64); rank[ref["order"]] = np.arange(ref["order"].size)
    same = tile_keys[1:] == tile_keys[:-1]
    assert (rank[point_list] >= 0).all() and (np.diff(rank[point_list])[same] > 0).all(), "%s: a list is not in (depth, id) order" % what
    par = tile_keys.astype(np.int64); gid = point_list.astype(np.int64); px, py = par % pgx, par // pgx
    got = []
    for ty_ in range(1 << sh):
        for tx_ in range(1 << sh):
            bits = (0x33 << (8 * ty_ + 2 * tx_)) if mode == 2 else (1 << ((ty_ << sh) | tx_)) if mode == 3 else 1
            sel = (child_mask & bits) != 0
            tx, ty = (px[sel] << sh) + tx_, (py[sel] << sh) + ty_
            assert ((tx < gx) & (ty < gy)).all(), "%s: a child bit outside the frame" % what
            got.append((ty * gx + tx) * P + gid[sel])
    got = np.concatenate(got)
    ref_pairs = tile_ref.astype(np.int64) * P + bins["point_list"].astype(np.int64)
    assert np.unique(got).size == got.size, "%s: a (tile, Gaussian) pair twice" % what
    kept = np.isin(ref_pairs, got)
    assert kept.sum() == got.size, "%s: an instance outside the oracle's rectangles" % what
    missing = _needed(orc, ref, W, H) & ~kept
    assert not missing.any(), "%s: %d instances some pixel accepts are missing" % (what, int(missing.sum()))
    if mode == 1:
        assert np.array_equal(point_list, bins["point_list"][kept]) and np.array_equal(tile_keys, tile_ref[kept]) and (child_mask == 1).all(), what


def assert_frame(orc, ref, sc, st, mode, what):
    """a forward_state() result against the oracle: radii, lists, image"""
    from helpers import assert_forward_gate
    W, H, P = sc["W"], sc["H"], sc["key"].size
    assert np.array_equal(st["radii"], ref["geo"]["radii"]), "%s: radii" % what
    assert_lists(orc, ref, W, H, P, mode, st["R"], st["order"], st["tile_keys"], st["child_mask"], st["point_list"], st["ranges"], what)
    assert_forward_gate(dict(geo=ref["geo"], bins=ref["bins"], color=ref["color"]), st["color"], W, H, FWD_TOL, what)


def _fwd(sc, mode):
    from gpu_utils import forward_state
    return forward_state(sc, sc["cam"], BG, use_precomp_cov=True, use_precomp_color=True, tile_cull=mode)


def _field(geom, P, name, count, dtype):
    from gpu_utils import _view
    from gaussianmesh_amd import _lib
    p = _lib.lib().gm_geom_field(geom.data_ptr(), P, name.encode())
    assert p, "gm_geom_field does not answer %s" % name
    return _view(geom, p, count, dtype)


# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("P", EDGE_P)
def test_wave_and_run_edges(oracle, P, mode):
    """P at the edges of a wave (64), of an emission workgroup's run (512) and of a bucket workgroup's round (256 x 16 = 4096), with
    zero-count records between live ones; inst16 is the record's count, row for row"""
    sc = edge_scene(P)
    ref = _oracle(oracle, "edge:%d" % P, sc)
    st = _fwd(sc, mode)
    assert_frame(oracle, ref, sc, st, mode, "P %d policy %d" % (P, mode))
    geo = ref["geo"]
    inst16 = _field(st["geom"], P, "inst16", P, torch.int16).view(np.uint16)
    rec = _field(st["geom"], P, "bin", 4 * P, torch.int32).view(np.uint32).reshape(P, 4)
    carried = ((rec[:, 0] >> 12) & 0xF) | ((rec[:, 0] >> 28) << 4) | (((rec[:, 1] >> 12) & 0xF) << 8) | ((rec[:, 1] >> 28) << 12)
    assert np.array_equal(inst16, carried.astype(np.uint16)), "inst16 is not the count the record carries"
    culled = geo["radii"] == 0
    assert (inst16[culled] == 0).all(), "a culled row with a count"
    if mode == 0:
        assert np.array_equal(inst16.astype(np.uint32), geo["tiles"].astype(np.uint32)), "inst16 against the oracle's tiles_touched"
    elif P >= 63:                                           # a visible row that emits nothing lies between rows that do
        z = np.nonzero(~culled & (inst16 == 0))[0]
        assert z.size and ((z > 0) & (z < P - 1)).any() and int(inst16.astype(np.int64).sum()) == st["R"]
    if P >= 63:
        assert culled[3::7].all() and culled.sum() < P // 4


@pytest.mark.gpu
def test_saturated_and_largest_unsaturated_count(oracle):
    """both sides of GM_BIN_COUNT_SAT through inst16: 65536 instances (inst16 = 0xFFFF, the count comes from tiles_touched) beside 65280
    (inst16 = 0xFF00, used as it is) - see the module docstring for why not 65534"""
    sc, j = saturated_pair_scene()
    W, H, P = sc["W"], sc["H"], sc["key"].size
    ref = _oracle(oracle, "saturated_pair", sc)
    t = ref["geo"]["tiles"].astype(np.int64)
    big = int(np.argmax(t))
    assert t[big] == 65536 and t[j] == 255 * 256 and (np.delete(t, [big, j]) <= 1).all(), (t[big], t[j])
    st = _fwd(sc, 0)
    inst16 = _field(st["geom"], P, "inst16", P, torch.int16).view(np.uint16)
    assert inst16[big] == 0xFFFF and inst16[j] == 0xFF00 and st["tiles"][big] == 65536
    assert_frame(oracle, ref, sc, st, 0, "saturated pair")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_two_pass_tile_route(oracle, mode):
    """1024 x 768: 3072 list tiles of 16 px, two 8-bit tile passes (the first reads what the emission wrote, the second the first one's
    output) and tile_ranges_kernel.  Three Gaussians cover the frame: their workgroup's instances exceed the LDS stage (DUP_STAGE 2048) and go out unstaged"""
    sc = edge_scene(400, W=1024, H=768, seed=1, big=3, sfac_mid=2e-2)
    ref = _oracle(oracle, "two_pass", sc)
    assert ref["bins"]["ranges"].shape[0] == 3072 > 2048 and int(ref["geo"]["tiles"].max()) == 3072 > 2048
    assert_frame(oracle, ref, sc, _fwd(sc, mode), mode, "two-pass policy %d" % mode)


def _capacity_frame(sc, cap, mode=0):
    from gpu_utils import T
    from gaussianmesh_amd import rasterizer as Rz
    cam, W, H = sc["cam"], sc["W"], sc["H"]
    ws = Rz.RasterWorkspace()
    ws.capacity = cap
    h = Rz.rasterize_forward_begin(T(BG), T(sc["means"]), T(sc["colors_precomp"]), T(sc["opac"]), None, None, 1.0, T(sc["cov3D_precomp"]), T(cam["view"]),
                                   T(cam["proj"]), cam["tanx"], cam["tany"], H, W, None, 0, T(cam["campos"]), workspace=ws, emission_policy=mode)
    out = h.finish(sync_free=True)
    assert out[0] == -1 and ws.capacity == cap
    return h, ws, out


def _handle_state(out, cap, sc, mode, nr):
    """what forward_state() returns, of a frame finished through a handle on a binning buffer laid out for `cap`"""
    from gpu_utils import _view
    from gaussianmesh_amd import _lib
    lib = _lib.lib()
    torch.cuda.synchronize()
    color, radii, geom, binning, img = out[1:6]
    W, H, P = sc["W"], sc["H"], sc["key"].size
    sh = max(mode - 1, 0)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    tiles = ((gx + (1 << sh) - 1) >> sh) * ((gy + (1 << sh) - 1) >> sh)
    V = int(_field(geom, P, "bucket_start", 2049, torch.int32)[2048])
    pairs = _view(binning, lib.gm_binning_field(binning.data_ptr(), cap, W, H, mode, b"pairs"), 2 * nr, torch.int32).view(np.uint32).reshape(nr, 2)
    return dict(R=nr, color=color.cpu().numpy(), radii=radii.cpu().numpy(), geom=geom, order=_field(geom, P, "order", P, torch.int32).view(np.uint32)[:V].copy(),
                point_list=np.ascontiguousarray(pairs[:, 1]), tile_keys=pairs[:, 0] & 0xFFFF, child_mask=pairs[:, 0] >> 16,
                ranges=_view(img, lib.gm_image_field(img.data_ptr(), W, H, b"ranges"), 2 * tiles, torch.int32).view(np.uint32).reshape(tiles, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("slack", [0, -1])
def test_capacity_exact_and_one_below(oracle, slack):
    """a capacity of exactly num_rendered fills the instance stream to its last pair; one below, the
    emission refuses the frame (background, empty lists) and finish() renders it again, exactly"""
    sc = edge_scene(513)
    ref = _oracle(oracle, "edge:513", sc)
    R = ref["bins"]["R"]
    h, ws, out = _capacity_frame(sc, R + slack)
    ok, nr = h.check()
    assert nr == R
    if slack == 0:
        assert ok and h.refusal == 0
        assert_frame(oracle, ref, sc, _handle_state(out, R, sc, 0, nr), 0, "capacity == num_rendered")
        return
    assert not ok and h.refusal == 1
    torch.cuda.synchronize()
    assert np.array_equal(out[1].cpu().numpy(), np.broadcast_to(BG[:, None, None], (3, sc["H"], sc["W"]))), "a refused frame is the background"
    out2 = h.finish()
    assert out2[0] == R and ws.capacity >= R
    assert_frame(oracle, ref, sc, _handle_state(out2, R, sc, 0, R), 0, "refused, then redone")      # (the exact path lays the buffer out for the count)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_unstaged_emission(oracle, mode):
    """every run of 256 sorted positions (and so every run of 512) has more instances than the LDS stage holds - 200 of the 513 Gaussians
    cover all 48 tiles, and the culled policy 1 drops only those below 1/255 opacity: the instances go straight to their slots"""
    sc = edge_scene(513, seed=2, big=200)
    ref = _oracle(oracle, "unstaged", sc)
    t = ref["geo"]["tiles"].astype(np.int64) * (sc["opac"][:, 0] >= 1.0 / 255.0)
    runs = [int(t[ref["order"][a:a + 256]].sum()) for a in range(0, ref["order"].size - 255, 256)]
    assert len(runs) >= 1 and min(runs) > 2048, runs
    assert_frame(oracle, ref, sc, _fwd(sc, mode), mode, "unstaged policy %d" % mode)


# ----------------------------------------------------------------------------------------------
# the deformed routes: batches and the direct depth placement
def _deformed_oracle(orc, name, sc, means):
    """the oracle's frame of a deformed route under the identity state: colours are the DC term of deformed_inputs()'s SH rows"""
    d = S.deformed_inputs(sc)
    o = dict(sc)
    o["means"] = means
    o["colors_precomp"] = np.maximum(SH_C0 * d["shs"][:, 0, :] + np.float32(0.5), np.float32(0.0)).astype(np.float32)
    return _oracle(orc, name, o)


@pytest.mark.gpu
def test_batch_of_three_different_frames(oracle):
    """K = 3, blockIdx.z of every launch: a frame of 513 Gaussians with holes and rectangles, a frame of 4097, an EMPTY frame.  Each frame
    against the oracle, and bit for bit its single-frame call at the same capacity"""
    from gaussianmesh_amd import rasterizer as Rz
    from gpu_utils import T
    from helpers import assert_forward_gate
    from test_gpu_batch import _state
    from test_gpu_ordering_paths import _begin, _device_inputs
    scs = [edge_scene(513, seed=3), edge_scene(4097, seed=4)]
    sc = dict(scs[0])
    for f in ("means", "opac", "cov3D_precomp", "colors_precomp", "key", "tile", "sfac"):
        sc[f] = np.concatenate([s_[f] for s_ in scs])
    group = np.concatenate([np.full(s_["key"].size, k) for k, s_ in enumerate(scs)])
    K, W, H, P = 3, sc["W"], sc["H"], sc["key"].size
    g = _device_inputs(sc, frames=(group, K))
    refs = [_deformed_oracle(oracle, "batch:%d" % k, sc, S.frame_means(sc, group, k)) for k in range(K)]
    assert refs[2]["bins"]["R"] == 0 and refs[0]["bins"]["R"] > 0 and refs[1]["bins"]["R"] > 0
    cap = max(r["bins"]["R"] for r in refs) + 7
    single = []
    for k in range(K):
        ws1 = Rz.RasterWorkspace()
        ws1.capacity = cap
        h = _begin(g, sc, k, workspace=ws1, want_count=False)
        h.finish(sync_free=True, image_only=True)
        ok, nr = h.check()
        assert ok and nr == refs[k]["bins"]["R"]
        torch.cuda.synchronize()
        single.append(_state(h, P, W, H, 0, nr))
    ws = [Rz.RasterWorkspace() for _ in range(K)]
    for w_ in ws:
        w_.capacity = cap
    hs = Rz.forward_deformed_batch(T(BG), g["tri"], g["weights"], g["packed"], g["cov"], g["pos"], g["shs"], g["opac"], [g["cam"]] * K, H, W, 3, ws,
                                   image_only=True, emission_policy=0)
    torch.cuda.synchronize()
    for k, h in enumerate(hs):
        ok, nr = h.check()
        ref = refs[k]
        assert ok and nr == ref["bins"]["R"], (k, ok, nr)
        st = _state(h, P, W, H, 0, nr)
        pairs = st["pairs"].view(np.uint32).reshape(-1, 2) if nr else np.zeros((0, 2), np.uint32)
        assert np.array_equal(st["radii"], ref["geo"]["radii"])
        assert_lists(oracle, ref, W, H, P, 0, nr, st["order"].view(np.uint32), pairs[:, 0] & 0xFFFF, pairs[:, 0] >> 16, pairs[:, 1],
                     st["ranges"].view(np.uint32).reshape(-1, 2), "batch frame %d" % k)
        assert_forward_gate(dict(geo=ref["geo"], bins=ref["bins"], color=ref["color"]), st["color"], W, H, FWD_TOL, "batch frame %d" % k)
        for field, a in single[k].items():
            assert np.array_equal(st[field], a), "frame %d of the batch: %s differs from the single-frame call" % (k, field)


@pytest.mark.gpu
def test_direct_placement_reads_bin_sorted(oracle):
    """A frame of the direct depth placement has no `bin` array (its records go to the bucket slabs and from there, sorted, to bin_sorted).
    The array is zeroed between the frame's halves: an emission that gathered bin[order[s]] would emit nothing.  The lists are the
    oracle's, `bin` is still zero afterwards and bin_sorted holds the records with the oracle's counts in the oracle's order"""
    from gaussianmesh_amd import rasterizer as Rz
    from test_gpu_ordering_paths import _begin, _device_inputs, _lists
    sc = edge_scene(4097, seed=5)
    W, H, P = sc["W"], sc["H"], sc["key"].size
    ref = _deformed_oracle(oracle, "direct", sc, sc["means"])
    R = ref["bins"]["R"]
    g = _device_inputs(sc)
    plan = Rz.new_depth_plan(g["pos"].device)
    ws = Rz.RasterWorkspace()
    _begin(g, sc, depth_plan=plan, workspace=ws).finish()                     # the stream's first frame: partition path, leaves its table
    h = _begin(g, sc, depth_plan=plan, workspace=ws, want_count=False)
    assert h.direct
    torch.cuda.synchronize()
    from gaussianmesh_amd import _lib
    p_bin = _lib.lib().gm_geom_field(h.geom.data_ptr(), P, b"bin")
    off = p_bin - h.geom.data_ptr()
    assert h.geom[off:off + 16 * P].any(), "the partition frame before left no records"
    h.geom[off:off + 16 * P].zero_()
    torch.cuda.synchronize()
    cap = ws.capacity
    out = h.finish(sync_free=True)
    ok, nr = h.check()
    assert ok and h.refusal == 0 and nr == R and plan.refused == 0
    order, pairs = _lists(out[3], out[4], cap, P, W, H, nr)
    assert np.array_equal(out[2].cpu().numpy(), ref["geo"]["radii"])
    ranges = _handle_state(out, cap, sc, 0, nr)["ranges"]
    assert_lists(oracle, ref, W, H, P, 0, nr, order, pairs[:, 0] & 0xFFFF, pairs[:, 0] >> 16, pairs[:, 1], ranges, "direct placement")
    from helpers import assert_forward_gate
    assert_forward_gate(dict(geo=ref["geo"], bins=ref["bins"], color=ref["color"]), out[1].cpu().numpy(), W, H, FWD_TOL, "direct placement")
    assert int(_field(out[3], P, "counters", 32, torch.int32)[S.CNT_DIRECT_FAIL]) == 0
    assert not _field(out[3], P, "bin", 4 * P, torch.int32).any(), "a direct-placement frame wrote bin"
    rec = _field(out[3], P, "bin_sorted", 4 * order.size, torch.int32).view(np.uint32).reshape(-1, 4)
    carried = ((rec[:, 0] >> 12) & 0xF) | ((rec[:, 0] >> 28) << 4) | (((rec[:, 1] >> 12) & 0xF) << 8) | ((rec[:, 1] >> 28) << 12)
    assert np.array_equal(carried, ref["geo"]["tiles"].astype(np.uint32)[order]), "bin_sorted: the records' counts in depth order"


# ----------------------------------------------------------------------------------------------
# no device
@pytest.mark.parametrize("P", [0, 1, 63, 4097])
def test_inst16_carve(P):
    """gm_geom_field answers inst16; the field starts on a 256-byte boundary like its neighbours, right behind the P records of `bin` and
    P counts before cov3D's boundary; gm_geom_bytes covers the carve (layout arithmetic on a fictitious, 256-byte aligned base address)"""
    import ctypes
    from gaussianmesh_amd import _lib
    lib = _lib.lib()
    base = 1 << 20
    n = max(P, 1)                                           # (the library lays an empty cloud out as one row)
    f = lambda name: lib.gm_geom_field(ctypes.c_void_p(base), P, name.encode())
    up = lambda a: (a + 255) & ~255
    names = ["splat", "radii", "tiles_touched", "bin", "inst16", "cov3D", "clamped", "depth_key"]
    at = {k: f(k) for k in names}
    assert all(at.values()), at
    assert all(v % 256 == 0 for v in at.values()), "a field off its 256-byte boundary: %s" % at
    assert [at[k] for k in names] == sorted(at.values()), "field order"
    assert at["inst16"] == up(at["bin"] + 16 * n) and at["cov3D"] == up(at["inst16"] + 2 * n) and at["clamped"] == up(at["cov3D"] + 24 * n)
    assert at["cov3D"] - at["bin"] == up(16 * n) + up(2 * n)
    # grad_acc is the last field: the buffer ends 256 bytes (the slack for an unaligned base) behind its 12 floats per row
    total, last = lib.gm_geom_bytes(P), f("grad_acc")
    assert last % 256 == 0 and last > max(f(k) for k in ("order", "bin_sorted", "bucket_start", "counters", "dmap", "bmap", "inst16"))
    assert total == last - base + 48 * n + 256, (total, last - base)
