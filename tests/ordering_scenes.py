"""Synthetic-key scenes for the ordering stage (gm_bucket.hip + the emission of gm_binning.hip) and the host-side witness of the
route a frame took through it.

A scene is built from a per-Gaussian list of (tile, depth key bits): the camera sits at the origin and looks along +z, a Gaussian's
z is the float whose bits are its key, x and y put its centre on the middle pixel of its tile, and an isotropic covariance of
(sfac z)^2 gives it a radius of a few pixels, so it touches that one tile.  Nothing of this is assumed: check_preconditions() asserts on
the oracle's preprocess that every Gaussian is visible, carries exactly the requested depth bits and touches the requested tiles.

The witness (route_summary) classifies every depth bucket the way bucket_sort_kernel does - entries, bits of the key range, radix
passes, the largest of the 1024 bins of the counting split - from the DEVICE's own table (gm_geom_field "dmap", "bmap", "bucket_start",
"counters") and the oracle's keys.  The tile sort leaves no such record on the device: its part of a summary line comes from
tile_expectation(), a model of launch_tile_sort's thresholds.  The constants below mirror gm_bucket.hip / gm_common.h."""
import numpy as np

from gaussianmesh_amd import scenes

BS_CAP, BS_BIN_MAX, BS_BINS = 4096, 48, 1024
COARSE_SHIFT, COARSE_BINS, BUCKET_BUDGET, NB_MAX = 20, 2048, 1792, 2048
SCAN_ITEMS = 256
CNT_RENDERED, CNT_VISIBLE, CNT_NBUCKETS, CNT_DIRECT_FAIL = 0, 4, 5, 8
W0, H0 = 1024, 512                    # 64 x 32 = 2048 list tiles of 16 px: the most the one-pass tile sort (and a batch) takes
BIN0 = 0x410                          # coarse bin of the view depths [8, 9): key bits 0x41000000 .. 0x410FFFFF
FAR = -1.0e30                         # z offset that puts a Gaussian behind the camera (batch frames: the other frames' Gaussians)


def camera(W, H):
    cam = scenes.look_at_camera((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), W, H)
    cam["W"], cam["H"] = W, H
    return cam


def build(W, H, tile, kbits, sfac=5e-5, seed=0):
    """tile [P] list tile (16 px, row-major), kbits [P] uint32 depth key bits, sfac: scalar or [P] - standard deviation of the splat as a
    fraction of its depth (5e-5: radius of a few pixels, one tile; 6e-3: a rectangle of about 3 x 3 tiles; 3: the whole frame)."""
    tile = np.asarray(tile, np.int64); kbits = np.ascontiguousarray(kbits, np.uint32)
    P = kbits.size
    cam = camera(W, H)
    gx = (W + 15) // 16
    z = kbits.view(np.float32).astype(np.float64)
    px = (tile % gx) * 16 + 8.0; py = (tile // gx) * 16 + 8.0
    ndcx = (2 * px + 1) / W - 1; ndcy = (2 * py + 1) / H - 1
    means = np.stack([cam["view"][0, 0] * ndcx * cam["tanx"] * z, cam["view"][1, 1] * ndcy * cam["tany"] * z, z], 1).astype(np.float32)
    s = np.broadcast_to(np.asarray(sfac, np.float64), (P,)) * z
    cov = np.zeros((P, 6), np.float32); cov[:, 0] = cov[:, 3] = cov[:, 5] = s * s
    rng = np.random.default_rng(1000 + seed)
    return dict(means=means, opac=np.full((P, 1), 0.08, np.float32), cov3D_precomp=cov, colors_precomp=rng.random((P, 3)).astype(np.float32),
                key=kbits, tile=tile, sfac=np.broadcast_to(np.asarray(sfac, np.float64), (P,)).copy(), W=W, H=H, cam=cam)


def deformed_inputs(sc, frames=None):
    """The same Gaussians as inputs of the deformed routes (forward_deformed_begin / forward_deformed_batch): rest positions = the means,
    rest covariances = the precomputed ones as 3 x 3, and an identity mesh state, under which the deformation returns both bit for bit
    (position + 0, R = S = 1).  frames (batches): [group id per Gaussian, number of groups]: Gaussians of group j hang on triangle j, and
    the mesh state of batch frame k moves every triangle but k behind the camera, so frame k shows group k alone.
    Returns host arrays: tri, weights, verts, cov [P,3,3], pos, shs [P,16,3], opac, states (one [Vm,21] per frame)."""
    P = sc["means"].shape[0]
    group, ngroups = (np.zeros(P, np.int64), 1) if frames is None else frames
    verts = np.zeros((3 * ngroups, 3), np.float32)
    verts[0::3, 0] = 1.0; verts[1::3, 1] = 1.0; verts[2::3, 2] = 1.0
    tri = (3 * group[:, None] + np.arange(3)[None, :]).astype(np.int32)
    weights = np.tile(np.array([0.5, 0.25, 0.25], np.float32), (P, 1))
    c6 = sc["cov3D_precomp"]
    cov = np.stack([c6[:, 0], c6[:, 1], c6[:, 2], c6[:, 1], c6[:, 3], c6[:, 4], c6[:, 2], c6[:, 4], c6[:, 5]], 1).reshape(P, 3, 3)
    rng = np.random.default_rng(7)
    shs = np.zeros((P, 16, 3), np.float32)
    shs[:, 0, :] = rng.uniform(-1.0, 1.5, (P, 3))
    states = []
    for k in range(ngroups):
        st = np.zeros((3 * ngroups, 21), np.float32)
        st[:, 0:3] = verts
        for j in (3, 7, 11, 12, 16, 20):
            st[:, j] = 1.0
        if frames is not None:
            away = np.repeat(np.arange(ngroups) != k, 3)
            st[away, 2] += FAR
        states.append(st)
    return dict(tri=tri, weights=weights, verts=verts, cov=np.ascontiguousarray(cov, np.float32), pos=sc["means"].copy(), shs=shs, opac=sc["opac"],
                states=states)


def frame_means(sc, group, k):
    """means of batch frame k of deformed_inputs(sc, (group, n)): what the deformation leaves (float32 position + offset)"""
    m = sc["means"].copy()
    m[group != k, 2] = (m[group != k, 2].astype(np.float64) + (0.5 * FAR + 0.25 * FAR + 0.25 * FAR)).astype(np.float32)
    return m


def oracle_geo(orc, sc, means=None):
    cam = sc["cam"]
    return orc.preprocess(sc["means"] if means is None else means, sc["opac"], cam["view"], cam["proj"], cam["campos"], sc["W"], sc["H"],
                          cam["tanx"], cam["tany"], colors_precomp=sc["colors_precomp"], cov3D_precomp=sc["cov3D_precomp"])


def check_preconditions(sc, geo, shown=None):
    """On the oracle's preprocess: everything visible (shown: the subset a batch frame shows; the rest culled), the depth bits are the
    requested bits, one-tile Gaussians touch one tile, rectangles touch 2..40 (sfac 6e-3) or every tile (sfac >= 1)."""
    P = sc["key"].size
    shown = np.ones(P, bool) if shown is None else shown
    assert ((geo["radii"] > 0) == shown).all(), "%d of %d Gaussians visible, %d wanted" % ((geo["radii"] > 0).sum(), P, shown.sum())
    assert np.array_equal(geo["depths"].view(np.uint32)[shown], sc["key"][shown]), "depth bits differ from the requested keys"
    gx, gy = (sc["W"] + 15) // 16, (sc["H"] + 15) // 16
    small, full = sc["sfac"] < 1e-3, sc["sfac"] >= 1.0
    t = geo["tiles"].astype(np.int64)
    assert (t[shown & small] == 1).all(), "a small splat touches more than one tile"
    assert (t[shown & full] == gx * gy).all(), "a full-frame splat does not touch every tile"
    mid = shown & ~small & ~full
    assert ((t[mid] >= 2) & (t[mid] <= 40)).all(), "a rectangle outside 2..40 tiles: %s" % np.unique(t[mid])
    return int(t[shown].sum())


def check_bins(sc, geo, bins):
    """the oracle's lists are the (tile, key, id) lexsort of the one-tile Gaussians, and the tile histogram is the requested one"""
    gx, gy = (sc["W"] + 15) // 16, (sc["H"] + 15) // 16
    one = (geo["radii"] > 0) & (geo["tiles"] == 1)
    if one.all():
        ids = np.arange(sc["key"].size)
        want = np.lexsort((ids, sc["key"].astype(np.int64), sc["tile"]))
        assert np.array_equal(bins["point_list"], want.astype(np.uint32))
    tl = (bins["keys"] >> np.uint64(32)).astype(np.int64)
    small = np.bincount(sc["tile"][one], minlength=gx * gy)
    assert (np.bincount(tl, minlength=gx * gy) >= small).all()
    if one.all():
        assert np.array_equal(np.bincount(tl, minlength=gx * gy), small)


# ----------------------------------------------------------------------------------------------
# the host model of the bucket table, for DESIGNING cases only (the device's table is what the witness reads)
def model_bucket_range(j, nb):
    return -(-(j << COARSE_SHIFT) // nb), -(-((j + 1) << COARSE_SHIFT) // nb)


TARGET = 100                                   # the bucket of BIN0 the single-bucket cases load
# key offsets inside BIN0 that fall into bucket TARGET whether the bin gets 1792 buckets or one less or more (float rounding of the
# table): the middle half of the bucket's range under 1792; the base population stays out of buckets TARGET - 2 .. TARGET + 2
_T0, _T1 = model_bucket_range(TARGET, BUCKET_BUDGET)
T_LO, T_HI = _T0 + (_T1 - _T0) // 4, _T1 - (_T1 - _T0) // 4
HOLE_LO, HOLE_HI = model_bucket_range(TARGET - 2, BUCKET_BUDGET)[0], model_bucket_range(TARGET + 2, BUCKET_BUDGET)[1]


def _base(rng, n, hole=True):
    off = rng.integers(0, 1 << COARSE_SHIFT, n)
    if hole:
        off = off[(off < HOLE_LO) | (off >= HOLE_HI)]
    return ((BIN0 << COARSE_SHIFT) + off).astype(np.uint32)


def _shuffled(rng, W, H, keys, sfac=None):
    """ids in random order (ties between equal keys must come out in id order, whatever the ids are), tiles at random"""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    p = rng.permutation(keys.size)
    sf = 5e-5 if sfac is None else sfac[p]
    return build(W, H, rng.integers(0, gx * gy, keys.size), keys[p], sfac=sf)


def _in_target(n):
    """n keys spread evenly over the safe part of bucket TARGET (at most ceil(n / span) on one value)"""
    return ((BIN0 << COARSE_SHIFT) + T_LO + (np.arange(n, dtype=np.int64) * (T_HI - T_LO)) // max(n, 1)).astype(np.uint32)


NBASE = 300000                         # (above 262144 the direct placement's slabs hold 4096 entries: slab_capacity)


def depth_case(name):
    """-> (scene, expectation) of a depth-order case.  expectation: what the witness must show, as
    dict(special={route: [(n, passes), ..]} for the buckets that are not on the fast path, fallback=bool, target_n=entries of the loaded bucket)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    kind, _, arg = name.partition(":")
    arg = int(arg) if arg else 0
    W, H = W0, H0
    if kind == "one_bin_uniform":
        return _shuffled(rng, W, H, _base(rng, 200000, hole=False)), dict(special={}, fallback=False)
    if kind == "bucket_n":
        keys = np.concatenate([_base(rng, NBASE), _in_target(arg)])
        special = {"slow": [(arg, 2)]} if arg > BS_CAP else {}
        return _shuffled(rng, W, H, keys), dict(special=special, fallback=False, target_n=arg)
    if kind == "pile":
        # (4096 equal keys fill the LDS alone: every pass then sees one digit, and an even number of passes that each reverse ties
        # restores the order - the piles with other keys around them, 3000 among them, are the ones such a mistake cannot pass)
        extras = min(200, BS_CAP - arg)
        spread = _in_target(T_HI - T_LO)                          # every value of the safe range once
        pile_key = spread[7]
        ex = spread[spread != pile_key][:: max(1, (spread.size - 1) // max(extras, 1))][:extras]
        keys = np.concatenate([_base(rng, NBASE), np.full(arg, pile_key, np.uint32), ex])
        special = {"stable": [(arg + extras, 2)]} if arg > BS_BIN_MAX else {}
        return _shuffled(rng, W, H, keys), dict(special=special, fallback=False, target_n=arg + extras, pile=arg)
    if kind == "wide_bucket":
        wide = ((BIN0 + 4) << COARSE_SHIFT)
        few = (wide + rng.integers(0, 1 << COARSE_SHIFT, 60)).astype(np.uint32)
        parts = [_base(rng, 600000, hole=False), few]              # (dense enough that the sparse bin's share stays below two buckets)
        special = {}
        if arg:                                                    # arg keys inside one of the 1024 bins of the 20-bit bucket
            parts.append((wide + 5 * 1024 + rng.integers(0, 1024, arg)).astype(np.uint32))
            special = {"stable": [(60 + arg, 3)]}
        return _shuffled(rng, W, H, np.concatenate(parts)), dict(special=special, fallback=False, wide_n=60 + arg)
    if kind == "table_fallback":
        sparse = ((np.arange(0x3E8, 0x3E8 + 320, dtype=np.uint32) << COARSE_SHIFT) | 0x12345)
        sparse = sparse[(sparse >> COARSE_SHIFT) != BIN0]
        keys = np.concatenate([sparse, _base(rng, arg, hole=False)])
        special = {"slow": [(arg, 3)]} if arg > BS_CAP else {}
        return _shuffled(rng, W, H, keys), dict(special=special, fallback=True, bins=sparse.size + 1)
    if kind == "run_straddle":
        # bucket starts at every residue modulo 256 (a uniform bin), one bucket on the slow path, and 3300 rectangles of ~9 instances
        # among the one-tile Gaussians of every kind of bucket, so the per-run instance totals differ from the position counts
        keys = np.concatenate([_base(rng, 60000), _in_target(5000 - 37)])
        sfac = np.full(keys.size, 5e-5)
        sfac[rng.choice(60000 - 2000, 3000, replace=False)] = 6e-3
        sfac[keys.size - 1 - rng.choice(4000, 300, replace=False)] = 6e-3
        return _shuffled(rng, W, H, keys, sfac=sfac), dict(special={"slow": [(5000 - 37, 2)]}, fallback=False, target_n=5000 - 37, rectangles=3300)
    raise KeyError(name)


DEPTH_CASES = (["one_bin_uniform"] + ["bucket_n:%d" % n for n in (1, 255, 256, 257, 4095, 4096, 4097, 12000)] +
               ["pile:%d" % n for n in (2, 48, 49, 300, 3000, 4096)] + ["wide_bucket", "wide_bucket:200", "table_fallback:3000", "table_fallback:100000",
                                                                 "run_straddle"])
# the subset that also runs through the direct placement: (case, refused)
DIRECT_CASES = [("bucket_n:4096", False), ("bucket_n:4097", True), ("pile:2", False), ("pile:48", False), ("pile:49", True), ("pile:300", True),
                ("one_bin_uniform", False)]
# frames of one batch, a different case per frame: a slow-path frame beside an ordinary one; a fallback frame, a pile frame and a 20-bit bucket
BATCHES = [("bucket_n:12000", "one_bin_uniform"), ("table_fallback:100000", "pile:300", "wide_bucket:200")]


def batch_scene(batch):
    """the cases of `batch` as ONE cloud (deformed_inputs(.., frames=(group, K)) shows case k in frame k) -> (scene, group, the cases' scenes)"""
    scs = [depth_case(n)[0] for n in batch]
    sc = dict(scs[0])
    for f in ("means", "opac", "cov3D_precomp", "colors_precomp", "key", "tile", "sfac"):
        sc[f] = np.concatenate([s_[f] for s_ in scs])
    group = np.concatenate([np.full(s_["key"].size, k) for k, s_ in enumerate(scs)])
    return sc, group, scs


def tile_case(name):
    """-> (W, H, scene, expectation): one-tile Gaussians, so R == P.  expectation: dict(R, tiles, waves, passes, chunks)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    kind, _, arg = name.partition(":")
    arg = int(arg) if arg else 0
    W, H = W0, H0
    gx, gy = W // 16, H // 16
    if kind == "R":
        R, tile = arg, rng.integers(0, gx * gy, arg)
    elif kind == "all_in_one_tile":
        R, tile = arg, np.full(arg, 777)
    elif kind == "first_and_last_tile_only":
        R = 20001
        tile = np.where(rng.random(R) < 0.4, 0, gx * gy - 1)
    elif kind == "tiles":
        W, H = {2047: (23 * 16, 89 * 16), 2048: (W0, H0), 2049: (683 * 16, 3 * 16), 2080: (40 * 16, 52 * 16)}[arg]
        gx, gy = W // 16, H // 16
        assert gx * gy == arg
        R = 30011
        tile = 3 * rng.integers(0, arg // 3, R)                    # two of three tiles stay empty ...
        tile[:5] = arg - 1                                         # ... the last one does not
    else:
        raise KeyError(name)
    keys = ((BIN0 << COARSE_SHIFT) + rng.integers(0, 1 << COARSE_SHIFT, R)).astype(np.uint32)
    sc = build(W, H, tile, keys)
    return sc, tile_expectation(R, gx * gy, R)


def tile_expectation(R, tiles, n_host):
    """A MODEL of launch_tile_sort (gm_bucket.hip), not a witness: nothing on the device records the tile sort's route, so this repeats
    its thresholds - one 11-bit pass up to 2048 list tiles, else two 8-bit passes; 4-wave workgroups up to 2^19 instances KNOWN TO THE HOST
    (n_host: the count, or the capacity of a sync-free finish), else 8-wave ones; 32 histogram rows of waves x 1024 keys per scan chunk.
    chunks: scan workgroups per digit group the launch has (sized by n_host); chunks_used: those the device's count R gives work to.
    Should those thresholds move, this model and the cases around them (TILE_CASES) move with them."""
    one_pass = tiles <= 2048
    waves = (4 if n_host <= (1 << 19) else 8) if one_pass else 4
    tile_keys = waves * 16 * 64
    chunks = lambda n: -(-(-(-n // tile_keys)) // 32)
    return dict(R=R, tiles=tiles, waves=waves, passes=1 if one_pass else 2, chunks=chunks(n_host), chunks_used=chunks(R))


TILE_CASES = (["R:%d" % r for r in (1, 4095, 4096, 4097, 131072, 131073, 1 << 19, (1 << 19) + 1, 786432, 786433)] +
              ["all_in_one_tile:12289", "all_in_one_tile:600000", "first_and_last_tile_only"] + ["tiles:%d" % t for t in (2047, 2048, 2049, 2080)])
# sync-free finish: (case, capacity - R)
SYNC_FREE_CASES = [("R:4096", 1), ("R:131073", 1), ("R:%d" % (1 << 19), 1), ("R:131073", (1 << 19) + 5000 - 131073), ("tiles:2049", 1)]


def saturated_scene():
    """4096 x 4096 under policy 0: 65536 list tiles; one Gaussian over the whole frame (its instance count saturates the emission record)
    between a few hundred small ones"""
    rng = np.random.default_rng(11)
    W = H = 4096
    n = 300
    keys = np.concatenate([(0x40800000 + rng.integers(0, 1 << 22, n)).astype(np.uint32), np.array([0x41000000], np.uint32),
                           (0x41100000 + rng.integers(0, 1 << 22, n)).astype(np.uint32)])
    tile = rng.integers(0, 65536, keys.size); tile[n] = 128 * 256 + 128
    sfac = np.full(keys.size, 5e-5); sfac[n] = 3.0
    p = rng.permutation(keys.size)
    sc = build(W, H, tile[p], keys[p], sfac=sfac[p])
    sc["opac"][:] = 0.3
    return sc


# ----------------------------------------------------------------------------------------------
# the witness
def bucket_of(dmap, keys):
    """depth_bucket() of gm_bucket.hip with the device's table (dmap[c] = first bucket << 16 | buckets)"""
    k = keys.astype(np.int64)
    c = k >> COARSE_SHIFT
    e = dmap.astype(np.int64)[c]
    return (e >> 16) + (((k & ((1 << COARSE_SHIFT) - 1)) * (e & 0xFFFF)) >> COARSE_SHIFT)


def classify_buckets(keys, dmap, bucket_start, nbuckets, bmap=None, cap=None):
    """keys: depth bits of the visible Gaussians (the oracle's).  Every non-empty bucket -> (n, bits, passes, largest bin, route); the sizes
    must be the device's (bucket_start).  bmap None: the direct placement, which takes a bucket's key range from its own entries and
    refuses (route 'refused') what the one-word sort cannot do; cap: its slab capacity."""
    b = bucket_of(dmap, keys)
    nb_all = bucket_start.size - 1
    sizes = np.bincount(b, minlength=nb_all)
    dev = np.diff(bucket_start.astype(np.int64))
    assert np.array_equal(sizes[:nbuckets], dev[:nbuckets]) and sizes[nbuckets:].sum() == 0, "bucket sizes differ from the table applied to the oracle's keys"
    k = keys.astype(np.int64)
    if bmap is not None:
        first, bits = bmap.reshape(-1, 2)[:, 0].astype(np.int64), bmap.reshape(-1, 2)[:, 1].astype(np.int64)
    else:
        first = np.full(nb_all, 1 << 40, np.int64); np.minimum.at(first, b, k)
        last = np.zeros(nb_all, np.int64); np.maximum.at(last, b, k)
        width = np.where(sizes > 0, last - first, 0)
        bits = np.array([int(w).bit_length() for w in width], np.int64)
    rel = k - first[b]
    assert (rel >= 0).all() and (rel < (np.int64(1) << bits[b])).all(), "a key outside its bucket's range"
    hb = np.minimum(bits, 10)
    binw = np.minimum(rel >> (bits - hb)[b], BS_BINS - 1)
    occ = np.bincount(b * BS_BINS + binw, minlength=nb_all * BS_BINS).reshape(nb_all, BS_BINS).max(axis=1)
    out = []
    for j in np.nonzero(sizes)[0]:
        n, bt, mx = int(sizes[j]), int(bits[j]), int(occ[j])
        if bmap is None:
            route = "refused" if (n > cap or bt > 20 or (n <= BS_CAP and mx > BS_BIN_MAX)) else "fast"
        else:
            route = "slow" if n > BS_CAP else ("stable" if mx > BS_BIN_MAX else "fast")
        out.append((int(j), n, bt, (bt + 7) // 8, mx, route))
    return out


def route_summary(keys, dmap, bucket_start, counters, bmap=None, cap=None):
    nbuckets = int(counters[CNT_NBUCKETS])
    rows = classify_buckets(keys, dmap, bucket_start, nbuckets, bmap, cap)
    s = dict(nbuckets=nbuckets, nonempty=len(rows), visible=int(counters[CNT_VISIBLE]), R=int(counters[CNT_RENDERED]), fast=0, fast_bits={}, stable=[],
             slow=[], refused=[], nmax=max([r[1] for r in rows] or [0]), coarse_bins=int(np.unique(keys >> COARSE_SHIFT).size))
    for (j, n, bits, passes, mx, route) in rows:
        if route == "fast":
            s["fast"] += 1
            s["fast_bits"][bits] = s["fast_bits"].get(bits, 0) + 1
        else:
            s[route].append((n, passes) if route != "refused" else (n, bits, mx))
    for r in ("stable", "slow", "refused"):
        s[r].sort()
    s["rows"] = rows
    return s


def show(what, s, tile=None):
    line = "route %-28s buckets: %d (%d non-empty; %d coarse bins), fast %d (key bits %s), stable (n, passes) %s, slow (n, passes) %s%s; largest %d; visible %d, R %d" % (
        what, s["nbuckets"], s["nonempty"], s["coarse_bins"], s["fast"], dict(sorted(s["fast_bits"].items())), s["stable"], s["slow"],
        (", refused (n, bits, bin) %s" % s["refused"]) if s["refused"] else "", s["nmax"], s["visible"], s["R"])
    if tile is not None:
        line += "; list tiles %d, tile sort (model): %d pass(es), %d-wave workgroups, %d scan chunk(s) launched, %d with work" % (
            tile["tiles"], tile["passes"], tile["waves"], tile["chunks"], tile["chunks_used"])
    print(line)
    return line


def straddles(order, bucket_start, rows, tiles):
    """64-position groups of bucket_sort_kernel's last loop that cross a multiple of SCAN_ITEMS with a Gaussian of more than one instance
    on BOTH sides (chunk_add's two-run case where neither total is a position count).  tiles: per Gaussian instance counts."""
    n = 0
    t = tiles[order]
    for (j, cnt, bits, passes, mx, route) in rows:
        s0 = int(bucket_start[j])
        rounds = -(-cnt // 256)
        starts = [s0 + 64 * g for g in range(-(-cnt // 64))] if route == "slow" else [s0 + (w * rounds + r) * 64 for w in range(4) for r in range(rounds)]
        for p0 in starts:
            cut = (p0 // SCAN_ITEMS + 1) * SCAN_ITEMS
            end = min(p0 + 64, s0 + cnt)
            if p0 < cut < end and (t[p0:cut] > 1).any() and (t[cut:end] > 1).any():
                n += 1
    return n
