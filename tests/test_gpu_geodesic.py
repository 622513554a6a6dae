"""-m gpu: gm_mesh_geodesic (mesh_region.SurfaceGraph.distances) against its definition - the float32 Dijkstra of tests/geodesic_ref.py,
bit for bit, the +inf rows included - at every size where a partial workgroup or a second one can go wrong, on graphs made to hurt, with
and without a cutoff, in chunks and in one call; then the glue above it: SingleObjectDeform.set_region_handles / drag_region and the CLI's
--pick_sequence with radii against --handle_sequence built from the reference distances."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import geodesic_ref as gr
from test_gpu_arap import _scene64, _tool
from test_gpu_raycast import _all_pixels, _run_cli

pytestmark = pytest.mark.gpu
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


def _graph(csr):
    from gaussianmesh_amd.mesh_region import SurfaceGraph
    return SurfaceGraph.from_csr(*csr)


def _same(got, ref, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == ref.shape and got.dtype == f32, what
    bad = np.nonzero(_bits(got) != _bits(ref))
    assert len(bad[0]) == 0, "%s: %d of %d distances differ, first at set %d vertex %d: device %r Dijkstra %r" % (
        what, len(bad[0]), ref.size, bad[0][0], bad[1][0], got[bad[0][0], bad[1][0]], ref[bad[0][0], bad[1][0]])


def _raw(csr, sets, cutoff=math.inf, sweeps=64, resume=0, dist=None):
    """gm_mesh_geodesic through ctypes on device buffers, one call: (dist [B,Vm] on the device, unsettled)"""
    from gaussianmesh_amd import _lib
    lib = _lib.lib()
    off, cols, lens = _dev(csr[0], torch.int32), _dev(np.r_[csr[1], 0], torch.int32), _dev(np.r_[csr[2], 0])
    Vm, B = len(csr[0]) - 1, len(sets)
    soff = _dev(np.cumsum([0] + [len(s) for s in sets]), torch.int32)
    src = _dev(np.concatenate([np.asarray(s, np.int64) for s in sets] + [np.zeros(1, np.int64)]), torch.int32)
    if dist is None:
        dist = torch.full((B, Vm), -7.0, dtype=torch.float32, device="cuda")
    uns = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    nbytes = lib.gm_mesh_geodesic_workspace_bytes(Vm, B, sweeps)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    _lib.check(lib.gm_mesh_geodesic(Vm, off.data_ptr(), cols.data_ptr(), lens.data_ptr(), B, soff.data_ptr(), src.data_ptr(), cutoff, sweeps, resume,
                                    dist.data_ptr(), uns.data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream))
    return dist, int(uns.item())


# ---- 1. sizes ----
@functools.lru_cache(maxsize=None)
def _random_case(Vm):
    """(csr, three source sets, the Dijkstra of all three), computed once; B = 1 takes the first"""
    rng = np.random.default_rng(100 + Vm)
    csr = gr.random_graph(Vm, rng)
    sets = [[int(rng.integers(Vm))], sorted(set(rng.integers(0, Vm, size=min(Vm, 5)).tolist())), [Vm - 1, 0]]
    return csr, sets, gr.dijkstra32(*csr, sets)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Vm", [1, 2, 63, 64, 65, 255, 256, 257, 513, 5000])
def test_random_graphs_at_every_block_edge(Vm, B):
    csr, sets, ref = _random_case(Vm)
    deg = np.diff(csr[0])
    if Vm >= 63:
        assert deg.min() == 0 and deg.max() == 12                                        # degrees 0 to 12, isolated vertices among them
    got = _graph(csr).distances(sets[:B])
    _same(got, ref[:B], "Vm %d B %d" % (Vm, B))
    if Vm == 5000:
        assert np.isinf(ref[0]).sum() > 100 and np.isfinite(ref[0]).sum() > 3000          # both kinds of row are there to be compared


# ---- 2. many sweeps: chunks, resume, the early out ----
@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_path_graph_in_chunks_and_in_one_call(order):
    """700 vertices in a line: the 64 rows of a wave read before any of them stores, so a distance travels about one hop a sweep
    whichever way the line is numbered, and chunks of 64 sweeps need the resume path many times; the lengths make the running sum round"""
    n = 700
    rng = np.random.default_rng(7)
    lens = rng.uniform(0.1, 1.0, size=n - 1).astype(f32)
    ident = np.arange(n) if order == "ascending" else np.arange(n)[::-1]                  # position along the line -> vertex id
    edges = {}
    for k in range(n - 1):
        edges[(int(ident[k]), int(ident[k + 1]))] = edges[(int(ident[k + 1]), int(ident[k]))] = lens[k]
    csr = gr.csr_of(n, edges)
    sets = [[int(ident[0])], [int(ident[350])]]
    ref = gr.dijkstra32(*csr, sets)
    assert np.array_equal(_bits(ref[0][ident]), _bits(np.r_[f32(0), np.cumsum(lens, dtype=f32)]))       # the left-to-right float32 sum itself
    g = _graph(csr)
    _same(g.distances(sets, sweeps_per_check=64), ref, "chunks of 64")
    print("%s: %d sweeps enqueued in chunks of 64" % (order, g.sweeps_enqueued))
    assert 128 <= g.sweeps_enqueued <= 700                                               # more than one chunk (resume was taken), within the budget Vm
    one, unsettled = _raw(csr, sets, sweeps=1024)
    assert unsettled == 0
    _same(one, ref, "one call of 1024 sweeps")
    # resume by hand: a chunk too short leaves rows unsettled and says so; going on from there ends at the same bits
    part, unsettled = _raw(csr, sets, sweeps=3)
    assert unsettled > 0 and np.isinf(part.cpu().numpy()).any()
    for _ in range(11):                                                                   # 3 + 11 * 64 > 700 = Vm sweeps always suffice
        part, unsettled = _raw(csr, sets, sweeps=64, resume=1, dist=part)
        if unsettled == 0:
            break
    assert unsettled == 0
    _same(part, ref, "resumed by hand")
    again, unsettled = _raw(csr, sets, sweeps=2, resume=1, dist=part.clone())              # a settled state stays as it is
    assert unsettled == 0 and torch.equal(again, part)


def test_max_sweeps_too_small_raises():
    from gaussianmesh_amd._lib import GmeshError
    n = 300
    edges = {}
    for k in range(n - 1):
        edges[(n - 1 - k, n - 2 - k)] = edges[(n - 2 - k, n - 1 - k)] = f32(1)
    csr = gr.csr_of(n, edges)
    g = _graph(csr)
    with pytest.raises(GmeshError, match="did not settle"):
        g.distances([[n - 1]], sweeps_per_check=4, max_sweeps=10)                         # descending numbering: one hop a sweep
    _same(g.distances([[n - 1]]), gr.dijkstra32(*csr, [[n - 1]]), "default budget")     # Vm sweeps always suffice
    for kw in (dict(sweeps_per_check=0), dict(max_sweeps=0), dict(max_distance=-1.0), dict(max_distance=math.nan)):
        with pytest.raises(ValueError):
            g.distances([[0]], **kw)
    for bad in ([[n]], [[-1]], [[0.5]], [[0], [1, n + 5]]):
        with pytest.raises(ValueError, match="source set"):
            g.distances(bad)
    assert g.distances([]).shape == (0, n)


# ---- 3. graphs made to hurt ----
def test_star_with_a_hub_of_5000_neighbours():
    n = 5001
    rng = np.random.default_rng(3)
    spokes = rng.uniform(0.5, 2.0, size=n - 1).astype(f32)
    edges = {}
    for k in range(1, n):
        edges[(0, k)] = edges[(k, 0)] = spokes[k - 1]
    csr = gr.csr_of(n, edges)
    sets = [[0], [4000], [17, 4999]]
    _same(_graph(csr).distances(sets), gr.dijkstra32(*csr, sets), "star")


def test_zero_lengths_duplicates_empty_sets_and_components():
    rng = np.random.default_rng(11)
    csr = gr.random_graph(600, rng, zero_fraction=0.2)
    assert (csr[2] == 0).sum() > 100
    sets = [[5, 5, 5, 300, 5], [], [599]]                                                 # duplicate sources; an empty set among three
    ref = gr.dijkstra32(*csr, sets)
    assert np.isinf(ref[1]).all() and (ref[0] == 0).sum() > 2                             # zero-length edges spread the zero
    _same(_graph(csr).distances(sets), ref, "zero lengths")
    # two components: the one without a source stays +inf
    a, b = gr.random_graph(200, rng, max_degree=8), gr.random_graph(130, rng, max_degree=8)
    off = np.r_[a[0], a[0][-1] + b[0][1:]].astype(np.int32)
    csr = (off, np.r_[a[1], b[1] + 200].astype(np.int32), np.r_[a[2], b[2]])
    sets = [[3], [250], [3, 250]]
    ref = gr.dijkstra32(*csr, sets)
    assert np.isinf(ref[0][200:]).all() and np.isinf(ref[1][:200]).all() and np.isfinite(ref[2]).sum() > 150
    _same(_graph(csr).distances(sets), ref, "two components")


def test_equal_hop_paths_whose_float_sums_differ():
    """0 -> 5 by two paths of three hops with the same lengths in another order: 2^-24, 2^-24, 1 sums to 1 + 2^-23, but 1, 2^-24, 2^-24 to
    1 (each small term is absorbed after the large one): the minimum over paths takes the smaller float32 sum, in either direction"""
    t = f32(2.0 ** -24)
    edges = {}
    for p, q, l in ((0, 1, t), (1, 2, t), (2, 5, f32(1)), (0, 3, f32(1)), (3, 4, t), (4, 5, t), (5, 6, f32(0.1))):
        edges[(p, q)] = edges[(q, p)] = l
    csr = gr.csr_of(7, edges)
    ref = gr.dijkstra32(*csr, [[0], [5]])
    up, down = f32(f32(f32(0) + t + t) + f32(1)), f32(f32(f32(1) + t) + t)
    assert up != down and ref[0][5] == min(up, down) and ref[1][0] == min(f32(f32(f32(1) + t) + t), f32(f32(t + t) + f32(1)))
    _same(_graph(csr).distances([[0], [5]]), ref, "rounding")


# ---- 4. the cutoff ----
def test_cutoff_is_inclusive_and_changes_no_kept_value():
    csr, sets, ref = _random_case(5000)
    g = _graph(csr)
    finite = np.sort(np.unique(ref[0][np.isfinite(ref[0]) & (ref[0] > 0)]))
    at = finite[len(finite) // 3]                                                         # one vertex's exact distance
    below = np.nextafter(at, f32(0), dtype=f32)
    for cut, kept in ((at, True), (below, False)):
        exp = np.where(ref <= cut, ref, f32(np.inf))
        assert np.array_equal(_bits(exp), _bits(gr.dijkstra32(*csr, sets, max_distance=cut)))       # the reference agrees with itself
        got = g.distances(sets, max_distance=float(cut))
        _same(got, exp, "cutoff %r" % cut)
        assert bool((got[0].cpu().numpy() == at).any()) == kept
    n_kept = int(np.isfinite(np.where(ref[0] <= at, ref[0], np.inf)).sum())
    assert 100 < n_kept < np.isfinite(ref[0]).sum() - 100
    zero = g.distances(sets, max_distance=0.0).cpu().numpy()                              # only what zero-length paths reach: the sources
    assert np.array_equal(_bits(zero), _bits(np.where(ref <= 0, ref, f32(np.inf))))


# ---- 5. a mesh ----
def test_torus_unfolded_eight_sets_twice():
    from gaussianmesh_amd import scenes
    from gaussianmesh_amd.mesh_region import SurfaceGraph
    V, F = scenes.torus_mesh(100, 75)
    g = SurfaceGraph(V, F)
    assert g.Vm == 7500 and len(g.csr[1]) == 12 * 7500
    rng = np.random.default_rng(1)
    sets = [[int(v)] for v in rng.integers(0, 7500, size=5)] + [rng.integers(0, 7500, size=40).tolist(), [0, 7499], list(range(0, 7500, 75))]
    ref = gr.dijkstra32(*g.csr, sets)
    first = g.distances(sets)
    print("torus 100 x 75, 8 sets: %d sweeps enqueued" % g.sweeps_enqueued)
    _same(first, ref, "torus")
    assert torch.equal(g.distances(sets), first)
    r = 1.0
    _same(g.distances(sets, max_distance=r), np.where(ref <= f32(r), ref, f32(np.inf)), "torus within 1.0")


# ---- 6. the C ABI on the device ----
def test_abi_on_the_device():
    from gaussianmesh_amd import _lib
    lib = _lib.lib()
    csr, sets, ref = _random_case(257)
    got, unsettled = _raw(csr, sets, sweeps=300)
    assert unsettled == 0
    _same(got, ref, "one raw call")
    # source ids outside [0, Vm) are skipped, not clamped onto another vertex
    got, unsettled = _raw(csr, [sets[0] + [-1, 257, 2 ** 31 - 1, -2 ** 31], [-5], sets[2]], sweeps=300)
    assert unsettled == 0
    _same(got, np.stack([ref[0], np.full(257, np.inf, f32), ref[2]]), "sources out of range")
    # column ids outside [0, Vm) are forced into range: no fault (and no meaning)
    wild = (csr[0], np.where(np.arange(len(csr[1])) % 7 == 0, csr[1] + 100000 * (np.arange(len(csr[1])) % 2 * 2 - 1), csr[1]).astype(np.int32), csr[2])
    forced = (csr[0], np.clip(wild[1], 0, 256).astype(np.int32), csr[2])
    got, _ = _raw(wild, sets, sweeps=300)
    torch.cuda.synchronize()
    want, _ = _raw(forced, sets, sweeps=300)
    assert torch.equal(got, want)
    # Vm == 0: success, nothing launched, nothing written
    uns = torch.full((1,), 123, dtype=torch.int32, device="cuda")
    assert lib.gm_mesh_geodesic(0, None, None, None, 0, None, None, math.inf, 1, 0, None, uns.data_ptr(), None, 0, None) == 0
    torch.cuda.synchronize()
    assert int(uns.item()) == 123
    # a refusal leaves dist alone
    dist = torch.full((1, 257), -7.0, device="cuda")
    assert lib.gm_mesh_geodesic(257, 4096, 4096, 4096, 1, 4096, 4096, math.nan, 1, 0, dist.data_ptr(), uns.data_ptr(), 4096, 1 << 20, None) == 1
    torch.cuda.synchronize()
    assert bool((dist == -7.0).all())


# ---- 7. the editing surface ----
def _reference_regions(o, picks, anchors, grab, free):
    """(ids, owner) from the REFERENCE distances on the object's rest mesh"""
    from gaussianmesh_amd.mesh_region import region_handles
    csr = gr.surface_graph_ref(o.vertex.cpu().numpy(), o.faces.cpu().numpy())
    d = gr.dijkstra32(*csr, [[int(v)] for v in list(picks) + list(anchors)], max_distance=grab if free is None else free)
    return region_handles(d[:len(picks)], d[len(picks):] if len(anchors) else None, grab, free), d


def _far_apart(o):
    """two handle vertices and an anchor vertex of the object's rest mesh, far from each other along the surface"""
    csr = gr.surface_graph_ref(o.vertex.cpu().numpy(), o.faces.cpu().numpy())
    a = 0
    b = int(np.argmax(gr.dijkstra32(*csr, [[a]])[0]))
    c = int(np.argmax(gr.dijkstra32(*csr, [[a, b]])[0]))
    return [a, b], [c]


def test_region_drag_moves_patches_rigidly_and_holds_the_rest(tmp_path):
    d = str(tmp_path)
    _scene64(d)
    tool = _tool(d)
    o = tool.gaussians_list[0]
    picks, anchors = _far_apart(o)
    grab, free = 0.6, 2.0
    (ids, owner), dref = _reference_regions(o, picks, anchors, grab, free)
    got = o.surface_distances([[v] for v in picks + anchors], max_distance=free)
    _same(got, dref, "surface_distances")
    solver = o.set_region_handles(picks, grab, free, anchor_vertices=anchors)
    assert np.array_equal(solver.handles, ids) and np.array_equal(o.region[1].cpu().numpy(), owner)
    n_moved, n_held = [(owner == i).sum() for i in range(2)], (owner < 0).sum()
    print("regions: moved %s, held %d of %d vertices" % (n_moved, n_held, o.vertex.shape[0]))
    assert min(n_moved) >= 4 and 20 <= n_held < o.vertex.shape[0] - 60                    # patches, a held far field, and a band that bends
    disp = np.array([[0.3, 0.2, -0.1], [-0.25, 0.15, 0.2]], f32)
    o.drag_region(disp, outer_iterations=2)
    V1, rest = o.mesh_vertex_current.cpu().numpy(), o.vertex.cpu().numpy()
    assert np.array_equal(_bits(V1[ids[owner < 0]]), _bits(rest[ids[owner < 0]]))         # held: the rest rows bit for bit
    for i in range(2):
        assert np.array_equal(_bits(V1[ids[owner == i]]), _bits(rest[ids[owner == i]] + disp[i]))       # each patch: rest + its displacement
    free_rows = np.setdiff1d(np.arange(len(rest)), ids)
    assert np.abs(V1[free_rows] - rest[free_rows]).max() > 0.05                           # the band follows
    # the tool's entry, the screen's entry and the refusals
    other = _tool(d)
    other.drag_region_one_gaussian("Object", picks, disp, grab, free, anchor_vertices=anchors, outer_iterations=2)
    assert torch.equal(other.gaussians_list[0].mesh_vertex_current, o.mesh_vertex_current)
    from gaussianmesh_amd.mesh_pick import screen_offset
    cam = tool.get_camera(d)[1]
    p, q = _tool(d).gaussians_list[0], _tool(d).gaussians_list[0]
    p.set_region_handles(picks, grab, free, anchor_vertices=anchors); q.set_region_handles(picks, grab, free, anchor_vertices=anchors)
    off = _dev([[3.0, -2.0], [-1.5, 2.5]])
    at = q.vertex[torch.as_tensor(picks, device="cuda")]
    p.drag_region_pixels(cam, off, outer_iterations=2); q.drag_region(screen_offset(cam, at, off) - at, outer_iterations=2)
    assert torch.equal(p.mesh_vertex_current, q.mesh_vertex_current) and not torch.equal(p.mesh_vertex_current, p.vertex)
    with pytest.raises(ValueError, match="handle 0 and handle 1 overlap"):
        o.set_region_handles(picks, 50.0)
    with pytest.raises(ValueError, match="meets the region of anchor 0"):
        o.set_region_handles(picks[:1], 50.0, anchor_vertices=anchors)
    with pytest.raises(ValueError, match="free_radius"):
        o.set_region_handles(picks, 0.5, 0.25)
    fresh = _tool(d).gaussians_list[0]
    with pytest.raises(ValueError, match="set_region_handles"):
        fresh.drag_region(disp)
    fresh.set_handles(picks)
    with pytest.raises(ValueError, match="set_region_handles"):                          # plain handles are no regions
        fresh.drag_region(disp)


def test_cli_pick_sequence_with_radii_equals_the_handle_sequence(tmp_path):
    from gaussianmesh_amd.mesh_pick import screen_offset
    d = str(tmp_path)
    _scene64(d)
    tool = _tool(d)
    o, cam = tool.gaussians_list[0], tool.get_camera(d)[1]
    pix = _all_pixels()
    vertex = o.pick(cam, pix)["vertex"].cpu().numpy()
    hits = np.nonzero(vertex >= 0)[0]
    csr = gr.surface_graph_ref(o.vertex.cpu().numpy(), o.faces.cpu().numpy())
    first = hits[0]                                                                       # handle 0; handle 1 and the anchor: the picked vertices farthest away
    d0 = gr.dijkstra32(*csr, [[int(vertex[first])]])[0]
    second = hits[int(np.argmax(d0[vertex[hits]]))]
    d01 = gr.dijkstra32(*csr, [[int(vertex[first]), int(vertex[second])]])[0]
    third = hits[int(np.argmax(d01[vertex[hits]]))]
    grab, free = 0.5, 1.75
    assert d0[vertex[second]] > 2 * grab and d01[vertex[third]] > 2 * grab
    chosen = [first, second, third]
    picked = vertex[chosen]
    offsets = np.array([[[2.0 * (k + 1), -1.5 * (k + 1)], [-1.0 * (k + 1), 2.5 * (k + 1)]] for k in range(3)], f32)
    doc = dict(camera_id=1, handles=pix[chosen[:2]].tolist(), anchors=pix[chosen[2:]].tolist(), offsets=offsets.tolist(), grab_radius=grab, free_radius=free)
    picks = os.path.join(d, "picks.json")
    with open(picks, "w") as fh:
        json.dump(doc, fh)
    assert _run_cli(d, os.path.join(d, "by_pick"), ["--pick_sequence", picks]) == 3
    (ids, owner), _ = _reference_regions(o, picked[:2], picked[2:], grab, free)
    assert (owner == 0).sum() >= 3 and (owner == 1).sum() >= 3 and (owner < 0).sum() >= 20 and len(ids) < o.vertex.shape[0] - 40
    rest = o.vertex.cpu().numpy()
    at = o.vertex[torch.as_tensor(picked[:2], device="cuda")]
    positions = []
    for k in range(3):
        disp = (screen_offset(cam, at, _dev(offsets[k])) - at).cpu().numpy()
        positions.append(np.where((owner >= 0)[:, None], rest[ids] + disp[np.maximum(owner, 0)], rest[ids]))
    np.savez(os.path.join(d, "handles.npz"), handles=ids, positions=np.stack(positions).astype(f32))
    assert _run_cli(d, os.path.join(d, "by_handle"), ["--handle_sequence", os.path.join(d, "handles.npz")]) == 3
    names = sorted(os.listdir(os.path.join(d, "by_pick")))
    assert names == ["%05d.%s" % (k, e) for k in range(3) for e in ("obj", "png")] == sorted(os.listdir(os.path.join(d, "by_handle")))
    for n in names:
        assert open(os.path.join(d, "by_pick", n), "rb").read() == open(os.path.join(d, "by_handle", n), "rb").read(), n
    # without the radii the same file is the single-vertex drag: other frames
    with open(picks, "w") as fh:
        json.dump({k: v for k, v in doc.items() if not k.endswith("_radius")}, fh)
    assert _run_cli(d, os.path.join(d, "by_vertex"), ["--pick_sequence", picks]) == 3
    assert open(os.path.join(d, "by_vertex", "00002.png"), "rb").read() != open(os.path.join(d, "by_pick", "00002.png"), "rb").read()
    # regions that overlap end the run and name the picks
    for change, word in ((dict(grab_radius=50.0, free_radius=60.0), "handle 0 and handle 1 overlap"),
                         (dict(handles=doc["handles"][:1], offsets=offsets[:, :1].tolist(), grab_radius=50.0, free_radius=60.0), "handle 0 meets the region of anchor 0")):
        with open(picks, "w") as fh:
            json.dump(dict(doc, **change), fh)
        with pytest.raises(SystemExit, match=word):
            _run_cli(d, os.path.join(d, "refused"), ["--pick_sequence", picks])
