"""gm_forward_deformed_batch_aux_async (rasterizer.forward_deformed_batch(aux=True)): the batch's frames with their depth and opacity maps.
The contract is equivalence, frame by frame and bit for bit, with the single-frame calls gm_forward_0_deformed_stream_async +
gm_forward_1_aux in sync-free mode (forward_deformed_begin(aux=True).finish(sync_free=True)) at equal capacity: colour, radii, lists,
ranges, status words, both maps, and the per-pixel state when it is kept; plus the images of the non-aux batch, refused and empty
frames, and a geometry buffer whose latch a direct-placement frame left set."""
import numpy as np
import pytest
import torch

from test_gpu_batch import _scene, _state

pytestmark = pytest.mark.gpu


def _image_state(h, W, H):
    from gpu_utils import _view
    from gaussianmesh_amd import _lib
    lib = _lib.lib()
    return {f: _view(h.img, lib.gm_image_field(h.img.data_ptr(), W, H, f.encode()), W * H, dt)
            for f, dt in (("final_T", torch.float32), ("n_contrib", torch.int32))}


def _single(Rz, g, bg, packed, cov, cm, W, H, ws, image_only, hint, aux=True):
    h = Rz.forward_deformed_begin(bg, g["tri"], g["weights"], packed, cov, g["pos"], g["shs"], g["opac"], cm["view"], cm["proj"],
                                  cm["tanx"], cm["tany"], H, W, 3, cm["campos"], False, workspace=ws, want_count=False, aux=aux)
    out = h.finish(sync_free=True, image_only=image_only, work_hint=hint)
    return h, out


@pytest.mark.parametrize("K,cov6,image_only", [(1, True, True), (1, False, False), (4, True, True), (4, False, False), (4, True, False),
                                               (4, False, True), (8, True, True), (8, False, False)])
def test_aux_batch_frames_equal_the_single_frame_aux_calls(K, cov6, image_only):
    from gaussianmesh_amd import rasterizer as Rz
    from gaussianmesh_amd.deform import mesh_rs_packed, mesh_rs_packed_batch, pack_cov6
    P, W, H, F = (30000 if K < 8 else 29989), 480, 270, 8
    g, cams = _scene(P, W, H, F)
    policy = Rz.get_default_emission_policy(W, H)
    bg = torch.tensor([0.2, 0.5, 0.7], device="cuda")
    cov = pack_cov6(g["cov"]) if cov6 else g["cov"]
    assert cov is not None
    pairs = [(1, 5), (4, 2), (6, 7), (3, 0), (0, 1), (2, 3), (5, 4), (7, 6)][:K]
    # the capacity: exact passes of the single-frame path
    ref_ws = [Rz.RasterWorkspace() for _ in range(K)]
    for (t, c), ws in zip(pairs, ref_ws):
        packed = mesh_rs_packed(g["verts"], g["v1"][t], g["faces"], g["adjacency"])
        cm = cams[c]
        Rz.forward_deformed_begin(bg, g["tri"], g["weights"], packed, cov, g["pos"], g["shs"], g["opac"], cm["view"], cm["proj"], cm["tanx"],
                                  cm["tany"], H, W, 3, cm["campos"], False, workspace=ws).finish(image_only=image_only)
    cap = max(ws.capacity for ws in ref_ws)
    ref, hint = [], Rz.new_work_hint(W, H, bg.device)
    for (t, c), ws in zip(pairs, ref_ws):
        ws.capacity = cap
        packed = mesh_rs_packed(g["verts"], g["v1"][t], g["faces"], g["adjacency"])
        h, out = _single(Rz, g, bg, packed, cov, cams[c], W, H, ws, image_only, hint)
        ok, nr = h.check()
        assert ok and nr > 0
        ref.append((_state(h, P, W, H, policy, nr), nr, out[6].clone(), out[7].clone(), None if image_only else _image_state(h, W, H)))
    tables = mesh_rs_packed_batch(g["verts"], [g["v1"][t] for t, _ in pairs], g["faces"], g["adjacency"])
    # the plain batch (its images) and the aux batch
    plain_ws = [Rz.RasterWorkspace() for _ in range(K)]
    aux_ws = [Rz.RasterWorkspace() for _ in range(K)]
    for w_ in plain_ws + aux_ws:
        w_.capacity = cap
    camk = [cams[c] for _, c in pairs]
    plain = Rz.forward_deformed_batch(bg, g["tri"], g["weights"], tables, cov, g["pos"], g["shs"], g["opac"], camk, H, W, 3, plain_ws,
                                      image_only=image_only, work_hint=Rz.new_work_hint(W, H, bg.device))
    hs = Rz.forward_deformed_batch(bg, g["tri"], g["weights"], tables, cov, g["pos"], g["shs"], g["opac"], camk, H, W, 3, aux_ws,
                                   image_only=image_only, work_hint=hint, aux=True)
    torch.cuda.synchronize()
    for k, h in enumerate(hs):
        assert plain[k].check()[0]
        ok, nr = h.check()
        assert ok and nr == ref[k][1], (k, ok, nr, ref[k][1])
        assert len(h.result) == 8 and h.result[6] is h.maps[0] and h.result[7] is h.maps[1]
        st = _state(h, P, W, H, policy, nr)
        for name, a in ref[k][0].items():
            assert np.array_equal(st[name], a), "frame %d of an aux batch of %d: %s differs from the single-frame call" % (k, K, name)
        depth, alpha = h.result[6], h.result[7]
        assert depth.shape == (1, H, W) and alpha.shape == (1, H, W)
        assert np.array_equal(depth.cpu().numpy(), ref[k][2].cpu().numpy()), "frame %d: depth" % k
        assert np.array_equal(alpha.cpu().numpy(), ref[k][3].cpu().numpy()), "frame %d: alpha" % k
        assert np.array_equal(h.color.cpu().numpy(), plain[k].color.cpu().numpy()), "frame %d: image of the aux batch != plain batch" % k
        assert float(alpha.max()) > 0.5 and float(depth.max()) > 0.0
        if not image_only:
            ist = _image_state(h, W, H)
            for f in ("final_T", "n_contrib"):
                assert np.array_equal(ist[f], ref[k][4][f]), (k, f)
                assert np.array_equal(ist[f], _image_state(plain[k], W, H)[f]), (k, f, "plain batch")
            assert np.array_equal(alpha.cpu().numpy().reshape(-1), (np.float32(1.0) - ist["final_T"]).reshape(-1)), "alpha != 1 - final_T"


def test_a_refused_frame_of_an_aux_batch_is_redone_with_exact_maps():
    from gaussianmesh_amd import rasterizer as Rz, scenes
    from gaussianmesh_amd.deform import mesh_rs_packed_batch
    from gpu_utils import T
    P, W, H, F = 30000, 480, 270, 8
    g, cams = _scene(P, W, H, F)
    bg = torch.tensor([0.9, 0.1, 0.3], device="cuda")
    near = cams[2]
    cf = scenes.orbit_camera(2, F, W, H, radius=18.0)
    far = dict(view=T(cf["view"]), proj=T(cf["proj"]), campos=T(cf["campos"]), tanx=cf["tanx"], tany=cf["tany"])
    tables = mesh_rs_packed_batch(g["verts"], [g["v1"][1], g["v1"][1]], g["faces"], g["adjacency"])
    alone = []
    for cm, tab in ((near, tables[0]), (far, tables[1])):
        out = Rz.forward_deformed_begin(bg, g["tri"], g["weights"], tab, g["cov"], g["pos"], g["shs"], g["opac"], cm["view"], cm["proj"], cm["tanx"],
                                        cm["tany"], H, W, 3, cm["campos"], False, aux=True).finish(image_only=True)
        alone.append((out[0], out[1].clone(), out[6].clone(), out[7].clone()))
    assert alone[0][0] > 1.1 * alone[1][0] > 0
    ws = [Rz.RasterWorkspace() for _ in range(2)]
    for w_ in ws:
        w_.capacity = (alone[0][0] + alone[1][0]) // 2
    hs = Rz.forward_deformed_batch(bg, g["tri"], g["weights"], tables, g["cov"], g["pos"], g["shs"], g["opac"], [near, far], H, W, 3, ws,
                                   image_only=True, aux=True)
    (ok0, nr0), (ok1, nr1) = hs[0].check(), hs[1].check()
    assert (ok0, nr0) == (False, alone[0][0]) and (ok1, nr1) == (True, alone[1][0])
    assert torch.equal(hs[1].color, alone[1][1]) and torch.equal(hs[1].maps[0], alone[1][2]) and torch.equal(hs[1].maps[1], alone[1][3])
    assert torch.equal(hs[0].color, bg.reshape(3, 1, 1).expand(3, H, W))                   # refused: background, both maps 0
    assert float(hs[0].maps[0].abs().max()) == 0.0 and float(hs[0].maps[1].abs().max()) == 0.0
    out = hs[0].finish(image_only=True)                                                   # again, through gm_forward_1_aux
    torch.cuda.synchronize()
    assert out[0] == alone[0][0] and len(out) == 8
    assert torch.equal(out[1], alone[0][1]) and torch.equal(out[6], alone[0][2]) and torch.equal(out[7], alone[0][3])


def test_a_frame_that_sees_nothing_inside_an_aux_batch_has_zero_maps():
    from gaussianmesh_amd import rasterizer as Rz, scenes
    from gaussianmesh_amd.deform import mesh_rs_packed_batch
    from gpu_utils import T
    P, W, H, F = 20000, 320, 200, 4
    g, cams = _scene(P, W, H, F)
    bg = torch.tensor([0.3, 0.6, 0.1], device="cuda")
    away = scenes.look_at_camera((8.0, 1.5, 0.0), (16.0, 1.5, 0.0), W, H, 60.0)
    blind = dict(view=T(away["view"]), proj=T(away["proj"]), campos=T(away["campos"]), tanx=away["tanx"], tany=away["tany"])
    frames = [(1, cams[1]), (2, blind), (3, cams[3])]
    tables = mesh_rs_packed_batch(g["verts"], [g["v1"][t] for t, _ in frames], g["faces"], g["adjacency"])
    alone = []
    for (t, cm), tab in zip(frames, tables):
        out = Rz.forward_deformed_begin(bg, g["tri"], g["weights"], tab, g["cov"], g["pos"], g["shs"], g["opac"], cm["view"], cm["proj"],
                                        cm["tanx"], cm["tany"], H, W, 3, cm["campos"], False, aux=True).finish(image_only=True)
        alone.append((out[0], out[1].clone(), out[6].clone(), out[7].clone()))
    assert alone[1][0] == 0 and alone[0][0] > 0 and alone[2][0] > 0
    ws = [Rz.RasterWorkspace() for _ in frames]
    for w_ in ws:
        w_.capacity = max(a[0] for a in alone) + 1024
    hs = Rz.forward_deformed_batch(bg, g["tri"], g["weights"], tables, g["cov"], g["pos"], g["shs"], g["opac"], [cm for _, cm in frames], H, W, 3,
                                   ws, image_only=True, aux=True)
    for k, h in enumerate(hs):
        ok, nr = h.check()
        assert ok and nr == alone[k][0]
        assert torch.equal(h.color, alone[k][1]) and torch.equal(h.maps[0], alone[k][2]) and torch.equal(h.maps[1], alone[k][3]), k
    assert float(hs[1].maps[0].abs().max()) == 0.0 and float(hs[1].maps[1].abs().max()) == 0.0
    assert torch.equal(hs[1].color, bg.reshape(3, 1, 1).expand(3, H, W))


def test_an_aux_batch_rearms_the_latch_a_direct_placement_frame_left():
    """A workspace whose geometry buffer last held a direct-placement frame (its depth-stale latch set: gm_forward_1_aux would refuse it)
    is used in an aux batch: the batch arms its counters itself, so the maps are rendered, not refused."""
    from gaussianmesh_amd import _lib, rasterizer as Rz
    from gaussianmesh_amd.deform import mesh_rs_packed_batch
    from gpu_utils import _view
    P, W, H, F = 30000, 480, 270, 8
    g, cams = _scene(P, W, H, F)
    bg = torch.tensor([1.0, 1.0, 1.0], device="cuda")
    tables = mesh_rs_packed_batch(g["verts"], [g["v1"][2], g["v1"][3]], g["faces"], g["adjacency"])
    plan = Rz.new_depth_plan(bg.device)
    ws = [Rz.RasterWorkspace() for _ in range(2)]
    begin = lambda cm, tab, w_, **kw: Rz.forward_deformed_begin(bg, g["tri"], g["weights"], tab, g["cov"], g["pos"], g["shs"], g["opac"], cm["view"],
                                                                 cm["proj"], cm["tanx"], cm["tany"], H, W, 3, cm["campos"], False, workspace=w_, **kw)
    alone = []
    for cm, tab, w_ in ((cams[2], tables[0], ws[0]), (cams[3], tables[1], ws[1])):
        out = begin(cm, tab, w_, aux=True).finish(image_only=True)
        alone.append((out[0], out[1].clone(), out[6].clone(), out[7].clone()))
    for c, direct in ((1, False), (2, True)):                          # the first frame primes the plan, the second places directly
        h = begin(cams[c], tables[0], ws[0], depth_plan=plan)
        assert h.direct == direct
        h.finish(sync_free=True, image_only=True)
        if not h.check()[0]:
            ws[0].release(h)              # (refused or not: the direct first half set the latch; the batch must not see it)
    torch.cuda.synchronize()
    geom = ws[0]._bufs["geom"]
    stale = _view(geom, _lib.lib().gm_geom_field(geom.data_ptr(), P, b"counters"), 16, torch.int32)[9]
    assert stale == 1, "the direct-placement frame did not leave the latch set"
    cap = max(w_.capacity for w_ in ws)
    for w_ in ws:
        w_.capacity = cap
    hs = Rz.forward_deformed_batch(bg, g["tri"], g["weights"], tables, g["cov"], g["pos"], g["shs"], g["opac"], [cams[2], cams[3]], H, W, 3, ws,
                                   image_only=True, aux=True)
    for k, h in enumerate(hs):
        ok, nr = h.check()
        assert ok and h.refusal == 0 and nr == alone[k][0], (k, ok, h.refusal)
        assert torch.equal(h.color, alone[k][1]) and torch.equal(h.maps[0], alone[k][2]) and torch.equal(h.maps[1], alone[k][3]), k
    assert float(hs[0].maps[1].max()) > 0.5
