"""Every data-dependent route of the ordering stage (gm_bucket.hip: depth partition, bucket_sort_kernel, the tile pass; the emission of
gm_binning.hip) on synthetic depth keys (ordering_scenes.py), each case asserting from the device's own bucket table WHICH route it took.

The contract is the reference's: one stable sort of the instances by (tile, depth bits), emitted in id order
(RAST/rasterizer_impl.cu:407-489) - `order` is the (depth bits, id) lexsort of the visible Gaussians, `point_list` and `ranges` are the
oracle's under policy 0, bit for bit, and the other emission policies render policy 0's image.  No tolerance anywhere but the forward gate
where an image is compared with the oracle.  The route witness is separate from those assertions: it reads "dmap", "bmap", "bucket_start"
and "counters" (gm_geom_field) and a case whose witness does not show the route it was built for fails."""
import numpy as np
import pytest
import torch

import ordering_scenes as S

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-4
BG = np.array([0.2, 0.3, 0.4], np.float32)


def _depth_case(orc, name):
    sc, ex = S.depth_case(name)
    geo = S.oracle_geo(orc, sc)
    S.check_preconditions(sc, geo)
    bins = orc.bin_instances(geo, sc["W"], sc["H"])
    return sc, ex, geo, bins


def _tables(geom, P):
    """the device's bucket table and sizes after a frame"""
    from gpu_utils import _view
    from gaussianmesh_amd import _lib
    lib = _lib.lib()
    torch.cuda.synchronize()
    gp = lambda n: lib.gm_geom_field(geom.data_ptr(), P, n.encode())
    assert gp("bmap") and gp("dmap"), "gm_geom_field does not answer bmap / dmap"
    u = lambda n, c: _view(geom, gp(n), c, torch.int32).view(np.uint32).copy()
    return dict(dmap=u("dmap", S.COARSE_BINS), bmap=u("bmap", 2 * 2048).reshape(2048, 2), bucket_start=u("bucket_start", 2049), counters=u("counters", 32))


def _witness(what, keys_visible, geom, P, direct_cap=None, tile=None):
    t = _tables(geom, P)
    s = S.route_summary(keys_visible, t["dmap"], t["bucket_start"], t["counters"], bmap=None if direct_cap else t["bmap"], cap=direct_cap)
    s["tables"] = t
    S.show(what, s, tile)
    return s


def _assert_route(name, sc, ex, s, order=None, tiles=None):
    """the witness shows the route the case was built for"""
    rows = {r[0]: r for r in s["rows"]}
    assert s["stable"] == sorted(ex["special"].get("stable", [])), (name, "stable passes", s["stable"])
    assert s["slow"] == sorted(ex["special"].get("slow", [])), (name, "slow path", s["slow"])
    assert s["fast"] == s["nonempty"] - len(s["stable"]) - len(s["slow"])
    assert s["visible"] == sc["key"].size
    if ex["fallback"]:
        assert s["nbuckets"] == s["coarse_bins"] == ex["bins"], (name, "one bucket per non-empty coarse bin", s["nbuckets"], s["coarse_bins"])
        assert set(s["fast_bits"]) <= {20}
    else:
        assert 1700 <= s["nbuckets"] <= S.NB_MAX and s["nbuckets"] > 4 * s["coarse_bins"], (name, s["nbuckets"])
    if "target_n" in ex:                               # the loaded bucket holds exactly what was put there
        b = set(S.bucket_of(s["tables"]["dmap"], sc["key"][(sc["key"] >= (S.BIN0 << 20) + S.T_LO) & (sc["key"] < (S.BIN0 << 20) + S.T_HI)]).tolist())
        assert len(b) == 1 and rows[b.pop()][1] == ex["target_n"], (name, "the target bucket")
    if "pile" in ex:
        b = int(S.bucket_of(s["tables"]["dmap"], sc["key"][(sc["key"] >= (S.BIN0 << 20) + S.T_LO) & (sc["key"] < (S.BIN0 << 20) + S.T_HI)])[0])
        assert rows[b][4] == ex["pile"], (name, "largest bin of the pile's bucket", rows[b])
    if "wide_n" in ex:
        b = int(S.bucket_of(s["tables"]["dmap"], np.array([(S.BIN0 + 4) << 20], np.uint32))[0])
        assert rows[b][1:4] == (ex["wide_n"], 20, 3), (name, "the one bucket of the sparse coarse bin", rows[b])
        assert ex["special"] or s["fast_bits"].get(20) == 1
    if name == "one_bin_uniform":
        assert s["nonempty"] == s["nbuckets"] == s["fast"]
    if "rectangles" in ex:
        n = S.straddles(order, s["tables"]["bucket_start"], s["rows"], tiles)
        n_slow = S.straddles(order, s["tables"]["bucket_start"], [r for r in s["rows"] if r[5] == "slow"], tiles)
        print("run_straddle: %d groups of 64 positions cross a run boundary between Gaussians of several instances (%d in the slow bucket)" % (n, n_slow))
        assert n - n_slow >= 1 and n_slow >= 1


def _want_order(sc, geo):
    vis = np.nonzero(geo["radii"] > 0)[0]
    d = geo["depths"].view(np.uint32)[vis].astype(np.int64)
    return vis[np.lexsort((vis, d))].astype(np.uint32)


@pytest.mark.parametrize("name", S.DEPTH_CASES)
def test_depth_order(oracle, name):
    """single-frame partition route (gm_forward_0 / gm_forward_1)"""
    from gpu_utils import forward_state
    from helpers import assert_forward_gate
    sc, ex, geo, bins = _depth_case(oracle, name)
    W, H, cam = sc["W"], sc["H"], sc["cam"]
    st = forward_state(sc, cam, BG, use_precomp_cov=True, use_precomp_color=True, tile_cull=0)
    # the contract first: it does not depend on the witness's fields
    assert np.array_equal(st["radii"], geo["radii"]) and np.array_equal(st["depth_key"], sc["key"])
    assert np.array_equal(st["order"], _want_order(sc, geo)), "%s: (depth bits, id) order" % name
    assert st["R"] == bins["R"] and np.array_equal(st["point_list"], bins["point_list"]), "%s: point_list" % name
    assert np.array_equal(st["ranges"], bins["ranges"]), "%s: ranges" % name
    color, fT, nc = oracle.render_fwd(W, H, bins, geo, BG)
    assert_forward_gate(dict(geo=geo, bins=bins, color=color), st["color"], W, H, FWD_TOL, "%s policy 0" % name)
    for mode in (1, 2, 3):
        cu = forward_state(sc, cam, BG, use_precomp_cov=True, use_precomp_color=True, tile_cull=mode)
        assert np.array_equal(cu["order"], st["order"]), (name, mode)
        assert np.array_equal(cu["color"], st["color"]) and np.array_equal(cu["final_T"], st["final_T"]), "%s: policy %d renders another image" % (name, mode)
    # then the route it took
    s = _witness(name, sc["key"], st["geom"], sc["key"].size, tile=S.tile_expectation(bins["R"], (W // 16) * (H // 16), bins["R"]))
    _assert_route(name, sc, ex, s, order=st["order"], tiles=geo["tiles"])


def _tile_case(orc, name):
    sc, ex = S.tile_case(name)
    geo = S.oracle_geo(orc, sc)
    assert S.check_preconditions(sc, geo) == ex["R"]
    return sc, ex, geo, orc.bin_instances(geo, sc["W"], sc["H"])


@pytest.mark.parametrize("name", S.TILE_CASES)
def test_tile_pass(oracle, name):
    """one-tile Gaussians: R == P exactly.  Lists and ranges bit for bit, the image through the forward gate, and the default policy
    renders policy 0's image.  The tile sort's route (workgroup width, passes, scan chunks) in the printed line is tile_expectation's
    MODEL of launch_tile_sort, not read from the device; the cases sit on both sides of each of its thresholds."""
    from gpu_utils import forward_state
    from helpers import assert_forward_gate
    sc, ex, geo, bins = _tile_case(oracle, name)
    W, H = sc["W"], sc["H"]
    st = forward_state(sc, sc["cam"], BG, use_precomp_cov=True, use_precomp_color=True, tile_cull=0)
    assert st["R"] == bins["R"] == ex["R"]
    assert np.array_equal(st["order"], _want_order(sc, geo)), name
    assert np.array_equal(st["tile_keys"], (bins["keys"] >> np.uint64(32)).astype(np.uint32)), "%s: tile keys" % name
    assert np.array_equal(st["point_list"], bins["point_list"]), "%s: point_list" % name
    assert np.array_equal(st["ranges"], bins["ranges"]), "%s: ranges" % name
    assert st["ranges"].shape[0] == ex["tiles"]
    color, fT, nc = oracle.render_fwd(W, H, bins, geo, BG)
    assert_forward_gate(dict(geo=geo, bins=bins, color=color), st["color"], W, H, FWD_TOL, "%s policy 0" % name)
    cu = forward_state(sc, sc["cam"], BG, use_precomp_cov=True, use_precomp_color=True, tile_cull=2)
    assert np.array_equal(cu["color"], st["color"]) and np.array_equal(cu["final_T"], st["final_T"]), "%s: policy 2 renders another image" % name
    s = _witness(name, sc["key"], st["geom"], sc["key"].size, tile=ex)
    assert int(s["R"]) == ex["R"] and not s["slow"] and not s["stable"]


@pytest.mark.parametrize("name,spare", S.SYNC_FREE_CASES)
def test_tile_pass_sync_free(oracle, name, spare):
    """finish(sync_free=True): the host only knows the capacity - it picks the kernel - and the device's count bounds the work"""
    from gpu_utils import T, _view
    from gaussianmesh_amd import _lib, rasterizer as Rz
    sc, ex, geo, bins = _tile_case(oracle, name)
    W, H, cam, P = sc["W"], sc["H"], sc["cam"], sc["key"].size
    cap = ex["R"] + spare
    route = S.tile_expectation(ex["R"], ex["tiles"], cap)
    ws = Rz.RasterWorkspace()
    ws.capacity = cap
    h = Rz.rasterize_forward_begin(T(BG), T(sc["means"]), T(sc["colors_precomp"]), T(sc["opac"]), None, None, 1.0, T(sc["cov3D_precomp"]), T(cam["view"]),
                                   T(cam["proj"]), cam["tanx"], cam["tany"], H, W, None, 0, T(cam["campos"]), workspace=ws, emission_policy=0)
    nr, color, radii, geom, binning, img = h.finish(sync_free=True)
    assert nr == -1 and ws.capacity == cap
    ok, count = h.check()
    assert ok and count == ex["R"]
    lib = _lib.lib()
    pairs = _view(binning, lib.gm_binning_field(binning.data_ptr(), cap, W, H, 0, b"pairs"), 2 * count, torch.int32).view(np.uint32).reshape(count, 2)
    assert np.array_equal(pairs[:, 1], bins["point_list"]) and np.array_equal(pairs[:, 0] & 0xFFFF, (bins["keys"] >> np.uint64(32)).astype(np.uint32))
    ranges = _view(img, lib.gm_image_field(img.data_ptr(), W, H, b"ranges"), 2 * ex["tiles"], torch.int32).view(np.uint32).reshape(-1, 2)
    assert np.array_equal(ranges, bins["ranges"])
    from gpu_utils import forward_state
    ref = forward_state(sc, cam, BG, use_precomp_cov=True, use_precomp_color=True, tile_cull=0)
    assert np.array_equal(color.cpu().numpy(), ref["color"])
    _witness("%s capacity R + %d" % (name, spare), sc["key"], geom, P, tile=route)      # (the tile sort's part of the line is the model's)


# ----------------------------------------------------------------------------------------------
# the deformed routes: the same keys through forward_deformed_begin (partition path and direct placement) and forward_deformed_batch
def _device_inputs(sc, frames=None):
    from gpu_utils import T
    from gaussianmesh_amd.deform import pack_mesh_state
    d = S.deformed_inputs(sc, frames)
    g = {k: T(d[k]) for k in ("weights", "pos", "cov", "opac", "shs", "verts")}
    g["tri"] = T(d["tri"], dtype=torch.int32)
    g["packed"] = [pack_mesh_state(T(st), g["verts"]) for st in d["states"]]
    cam = sc["cam"]
    g["cam"] = dict(view=T(cam["view"]), proj=T(cam["proj"]), campos=T(cam["campos"]), tanx=cam["tanx"], tany=cam["tany"])
    return g


def _begin(g, sc, k=0, **kw):
    from gaussianmesh_amd import rasterizer as Rz
    from gpu_utils import T
    c = g["cam"]
    return Rz.forward_deformed_begin(T(BG), g["tri"], g["weights"], g["packed"][k], g["cov"], g["pos"], g["shs"], g["opac"], c["view"], c["proj"], c["tanx"],
                                     c["tany"], sc["H"], sc["W"], 3, c["campos"], False, emission_policy=0, **kw)


def _lists(geom, binning, cap, P, W, H, nr):
    from gpu_utils import _view
    from gaussianmesh_amd import _lib
    lib = _lib.lib()
    torch.cuda.synchronize()
    gp = lambda n: lib.gm_geom_field(geom.data_ptr(), P, n.encode())
    V = int(_view(geom, gp("bucket_start"), 2049, torch.int32)[2048])
    order = _view(geom, gp("order"), P, torch.int32)[:V].view(np.uint32).copy()
    pairs = _view(binning, lib.gm_binning_field(binning.data_ptr(), cap, W, H, 0, b"pairs"), 2 * nr, torch.int32).view(np.uint32).reshape(nr, 2).copy()
    return order, pairs


def _slab_capacity(P):
    """slab_capacity() of gm_common.h (entries a bucket's slab holds: a power of two, 256 .. 4096), checked against what the library sizes
    a slab for: gm_depth_slab_bytes(P) holds 2048 slabs of `cap` 8-byte pairs and 16-byte records plus less than one more capacity step"""
    from gaussianmesh_amd import _lib
    c = 256
    while c < 4096 and c * 128 < P:
        c <<= 1
    nbytes = _lib.lib().gm_depth_slab_bytes(P)
    assert 2048 * 24 * c <= nbytes < 2048 * 24 * 2 * c, "slab_capacity(%d) is no longer %d: %d bytes" % (P, c, nbytes)
    return c


@pytest.mark.parametrize("name,refused", S.DIRECT_CASES)
def test_direct_placement(oracle, name, refused):
    """The plan is primed by the same scene on the partition path; the next frame places its Gaussians with that table.  Piles of up to 48
    equal keys and buckets up to the slab's capacity are ACCEPTED (equal keys in id order); a pile of 49 or a bucket above the slab is
    refused with status 2 and comes out right when the frame is begun again."""
    from gaussianmesh_amd import rasterizer as Rz
    sc, ex, geo, bins = _depth_case(oracle, name)
    W, H, P = sc["W"], sc["H"], sc["key"].size
    g = _device_inputs(sc)
    # partition path, with the deformed positions and covariances read back: the deformation under the identity state changes no bit
    h0 = _begin(g, sc, want_deformed=True)
    o0 = h0.finish()
    assert np.array_equal(h0.deformed[0].cpu().numpy().view(np.uint32), sc["means"].view(np.uint32)), "the identity deformation moved a position"
    assert np.array_equal(h0.deformed[1].cpu().numpy().view(np.uint32), sc["cov3D_precomp"].view(np.uint32))
    ord0, pairs0 = _lists(o0[3], o0[4], o0[0], P, W, H, o0[0])
    img0 = o0[1].clone()
    assert o0[0] == bins["R"] and np.array_equal(ord0, _want_order(sc, geo)) and np.array_equal(pairs0[:, 1], bins["point_list"])
    cap = _slab_capacity(P)
    assert cap == 4096 or name == "one_bin_uniform"
    plan = Rz.new_depth_plan(img0.device)
    ws = Rz.RasterWorkspace()
    _begin(g, sc, depth_plan=plan, workspace=ws).finish()                    # the stream's first frame: partition path, leaves its table
    h = _begin(g, sc, depth_plan=plan, workspace=ws, want_count=False)
    assert h.direct
    bcap = ws.capacity
    out = h.finish(sync_free=True)
    ok, nr = h.check()
    s = _witness("%s direct" % name, sc["key"], out[3], P, direct_cap=cap)
    assert int(s["tables"]["counters"][S.CNT_DIRECT_FAIL]) == int(refused)
    if "pile" in ex:                                   # (the bucket the pile's key maps to under the table the frame was placed with)
        b = int(S.bucket_of(s["tables"]["dmap"], sc["key"][(sc["key"] >= (S.BIN0 << 20) + S.T_LO) & (sc["key"] < (S.BIN0 << 20) + S.T_HI)])[0])
        row = {r[0]: r for r in s["rows"]}[b]
        assert row[1] == ex["target_n"] and row[4] == ex["pile"], "the pile's bin does not hold exactly the pile under the entries' own key range: %s" % (row,)
    if name == "bucket_n:4096":
        assert s["nmax"] == 4096 == cap
    if not refused:
        assert ok and h.refusal == 0 and not s["refused"], (name, h.refusal, s["refused"])
        assert nr == bins["R"]
        ord1, pairs1 = _lists(out[3], out[4], bcap, P, W, H, nr)
        assert np.array_equal(ord1, ord0), "%s: visible order of the direct placement" % name
        assert np.array_equal(pairs1, pairs0) and torch.equal(out[1], img0)
        assert plan.refused == 0
    else:
        assert not ok and h.refusal == 2 and len(s["refused"]) == 1, (name, ok, h.refusal, s["refused"])
        n, bits, mx = s["refused"][0]
        assert (n > cap) if name.startswith("bucket_n") else (n <= cap and mx == ex["pile"] > S.BS_BIN_MAX)
        o2 = h.finish()                                                       # begun again on the partition path
        ord2, pairs2 = _lists(o2[3], o2[4], o2[0], P, W, H, o2[0])          # (the exact path lays the buffer out for the count)
        assert plan.refused == 1 and o2[0] == bins["R"]
        assert np.array_equal(ord2, ord0) and np.array_equal(pairs2, pairs0) and torch.equal(o2[1], img0)


@pytest.mark.parametrize("batch", S.BATCHES)
def test_batch_frames_of_different_cases(oracle, batch):
    """blockIdx.z of every ordering launch: the frames of one batch are DIFFERENT cases (a slow-path frame beside an ordinary one; a
    fallback frame, a pile frame and a frame with a 20-bit bucket).  Each frame equals its single-frame result byte for byte
    (test_gpu_batch._state) and the oracle's order and lists."""
    from gaussianmesh_amd import rasterizer as Rz
    from gpu_utils import T
    from test_gpu_batch import _state
    sc, group, scs = S.batch_scene(batch)
    K, W, H, P = len(batch), sc["W"], sc["H"], sc["key"].size
    g = _device_inputs(sc, frames=(group, K))
    ref_ws = [Rz.RasterWorkspace() for _ in range(K)]
    for k in range(K):
        _begin(g, sc, k, workspace=ref_ws[k]).finish(image_only=True)
    cap = max(w_.capacity for w_ in ref_ws)
    ref = []
    for k in range(K):
        ref_ws[k].capacity = cap
        h = _begin(g, sc, k, workspace=ref_ws[k], want_count=False)
        h.finish(sync_free=True, image_only=True)
        ok, nr = h.check()
        assert ok and nr == scs[k]["key"].size
        torch.cuda.synchronize()
        ref.append((_state(h, P, W, H, 0, nr), nr))
    ws = [Rz.RasterWorkspace() for _ in range(K)]
    for w_ in ws:
        w_.capacity = cap
    hs = Rz.forward_deformed_batch(T(BG), g["tri"], g["weights"], g["packed"], g["cov"], g["pos"], g["shs"], g["opac"], [g["cam"]] * K, H, W, 3, ws,
                                   image_only=True, emission_policy=0)
    torch.cuda.synchronize()
    for k, h in enumerate(hs):
        ok, nr = h.check()
        assert ok and nr == ref[k][1]
        st = _state(h, P, W, H, 0, nr)
        for field, a in ref[k][0].items():
            assert np.array_equal(st[field], a), "frame %d (%s) of the batch: %s differs from the single-frame call" % (k, batch[k], field)
        shown = group == k
        geo = S.oracle_geo(oracle, sc, means=S.frame_means(sc, group, k))
        S.check_preconditions(sc, geo, shown=shown)
        bins = oracle.bin_instances(geo, W, H)
        assert np.array_equal(st["order"].view(np.uint32), _want_order(sc, geo)), "frame %d (%s): order" % (k, batch[k])
        pairs = st["pairs"].view(np.uint32).reshape(-1, 2)
        assert np.array_equal(pairs[:, 1], bins["point_list"]) and np.array_equal(st["ranges"].view(np.uint32).reshape(-1, 2), bins["ranges"])
        s = _witness("batch frame %d: %s" % (k, batch[k]), sc["key"][shown], h.geom, P)
        ex = S.depth_case(batch[k])[1]
        _assert_route(batch[k], scs[k], ex, s)


def test_saturated_instance_count(oracle):
    """GM_BIN_COUNT_SAT: one Gaussian on all 65536 list tiles of a 4096 x 4096 frame under policy 0 - its emission record says "65535 or
    more" and bucket_sort_kernel and duplicate_kernel look the count up in tiles_touched."""
    from gpu_utils import forward_state
    from helpers import assert_forward_gate
    from gaussianmesh_amd import rasterizer as Rz
    sc = S.saturated_scene()
    W, H, cam = sc["W"], sc["H"], sc["cam"]
    geo = S.oracle_geo(oracle, sc)
    R = S.check_preconditions(sc, geo)
    assert int(geo["tiles"].max()) == 65536 >= 0xFFFF
    bins = oracle.bin_instances(geo, W, H)
    st = forward_state(sc, cam, BG, use_precomp_cov=True, use_precomp_color=True, tile_cull=0)
    print("saturated count: tiles_touched max %d, R %d" % (int(st["tiles"].max()), st["R"]))
    assert np.array_equal(st["tiles"], geo["tiles"]) and st["R"] == bins["R"] == R
    assert np.array_equal(st["order"], _want_order(sc, geo))
    assert np.array_equal(st["point_list"], bins["point_list"]) and np.array_equal(st["ranges"], bins["ranges"])
    color, fT, nc = oracle.render_fwd(W, H, bins, geo, BG)
    assert_forward_gate(dict(geo=geo, bins=bins, color=color), st["color"], W, H, FWD_TOL, "saturated count policy 0")
    mode = Rz.get_default_emission_policy(W, H)
    assert mode != 0
    cu = forward_state(sc, cam, BG, use_precomp_cov=True, use_precomp_color=True, tile_cull=mode)     # lists per parent tile: nothing saturates
    assert np.array_equal(cu["color"], st["color"]), "policy %d renders another image than policy 0" % mode
    s = _witness("saturated count", sc["key"], st["geom"], sc["key"].size, tile=S.tile_expectation(R, 65536, R))
    assert int(s["R"]) == R


def test_witness_over_the_older_ordering_scenes(oracle):
    """The routes the six scenes of test_gpu_parity.test_ordering_paths really take, printed (that test's docstring quotes them), and what
    it claims about the two pile scenes asserted: one bucket above the LDS, on the slow path at two passes - a sub-range of a coarse bin
    has 10 low bits even when every key in it is equal."""
    from gpu_utils import forward_state
    from test_gpu_parity import ORDERING_CASES, ordering_scene
    for case in ORDERING_CASES:
        sc, cam, modes, W, H = ordering_scene(case)
        fw = oracle.forward_full(sc, cam, BG, D=3)
        vis = fw["geo"]["radii"] > 0
        st = forward_state(sc, cam, BG, D=3, tile_cull=0)
        gx, gy = (W + 15) // 16, (H + 15) // 16
        s = _witness("test_ordering_paths[%s]" % case, fw["geo"]["depths"].view(np.uint32)[vis], st["geom"], sc["means"].shape[0],
                     tile=S.tile_expectation(st["R"], gx * gy, st["R"]))
        if case in ("equal_depths", "depth_pileup"):
            assert len(s["slow"]) == 1 and s["slow"][0][0] > S.BS_CAP and s["slow"][0][1] == 2 and not s["stable"], (case, s["slow"], s["stable"])
        if case == "many_tiles":
            assert gx * gy > 2048
        if case != "equal_depths":                         # every bucket off the slow path takes the counting split, with 10 to 20 low bits
            assert s["fast"] == s["nonempty"] - len(s["slow"]) and set(s["fast_bits"]) <= set(range(10, 21)) and max(s["fast_bits"]) > 10
        if case == "depth_pileup":
            assert max(s["fast_bits"]) == 20
        if case == "twenty_octaves":                       # the proportional table, not its fallback
            assert s["coarse_bins"] >= 150 and s["nbuckets"] > 4 * s["coarse_bins"]
