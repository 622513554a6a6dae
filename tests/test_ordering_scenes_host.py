"""The case list of tests/test_gpu_ordering_paths.py is well formed: for every synthetic-key scene the ORACLE's preprocess reports every
Gaussian visible, exactly the requested depth bits and the requested tiles, and its lists are the (tile, key, id) order the scene was
built for.  Runs without a GPU; the witness's arithmetic is checked against a brute-force count on a small table."""
import numpy as np
import pytest

import ordering_scenes as S


@pytest.mark.parametrize("name", S.DEPTH_CASES)
def test_depth_case_preconditions(oracle, name):
    sc, ex = S.depth_case(name)
    geo = S.oracle_geo(oracle, sc)
    R = S.check_preconditions(sc, geo)
    bins = oracle.bin_instances(geo, sc["W"], sc["H"])
    assert bins["R"] == R
    S.check_bins(sc, geo, bins)
    if "rectangles" in ex:
        assert int((geo["tiles"] > 1).sum()) == ex["rectangles"] and R > sc["key"].size
    else:
        assert R == sc["key"].size
    if "target_n" in ex:                                  # the loaded bucket's keys lie where the construction says, the base keeps out
        off = sc["key"].astype(np.int64) - (S.BIN0 << S.COARSE_SHIFT)
        assert int(((off >= S.T_LO) & (off < S.T_HI)).sum()) == ex["target_n"]
        assert int(((off >= S.HOLE_LO) & (off < S.HOLE_HI)).sum()) == ex["target_n"]
    if "pile" in ex:
        assert int(np.bincount(sc["key"] - sc["key"].min()).max()) >= ex["pile"]
        vals, cnt = np.unique(sc["key"], return_counts=True)
        assert int(cnt.max()) == ex["pile"] or ex["pile"] < 4     # (random base keys may coincide in pairs or triples)


@pytest.mark.parametrize("name", S.TILE_CASES)
def test_tile_case_preconditions(oracle, name):
    sc, ex = S.tile_case(name)
    geo = S.oracle_geo(oracle, sc)
    assert S.check_preconditions(sc, geo) == ex["R"]
    bins = oracle.bin_instances(geo, sc["W"], sc["H"])
    assert bins["R"] == ex["R"] and bins["ranges"].shape[0] == ex["tiles"]
    S.check_bins(sc, geo, bins)
    if name.startswith("tiles:"):
        assert bins["ranges"][-1, 1] == ex["R"] and bins["ranges"][-1, 0] < ex["R"]           # the last tile is populated
        empty = np.bincount(sc["tile"], minlength=ex["tiles"]) == 0
        assert empty.sum() > ex["tiles"] // 2 and (bins["ranges"][empty] == 0).all()             # empty lists: {0, 0}


def test_tile_route_expectations():
    e = S.tile_expectation
    assert (e(1 << 19, 2048, 1 << 19)["waves"], e((1 << 19) + 1, 2048, (1 << 19) + 1)["waves"]) == (4, 8)
    assert (e(131072, 2048, 131072)["chunks"], e(131073, 2048, 131073)["chunks"]) == (1, 2)
    assert (e(786432, 2048, 786432)["chunks"], e(786433, 2048, 786433)["chunks"]) == (3, 4)
    assert (e(30011, 2048, 30011)["passes"], e(30011, 2049, 30011)["passes"]) == (1, 2)
    assert e(131073, 2048, (1 << 19) + 5000) == dict(R=131073, tiles=2048, waves=8, passes=1, chunks=3, chunks_used=1)


@pytest.mark.parametrize("batch", S.BATCHES)
def test_batch_frames_show_one_case_each(oracle, batch):
    sc, group, scs = S.batch_scene(batch)
    for k in range(len(batch)):
        geo = S.oracle_geo(oracle, sc, means=S.frame_means(sc, group, k))
        assert S.check_preconditions(sc, geo, shown=group == k) == scs[k]["key"].size


def test_saturated_scene_preconditions(oracle):
    sc = S.saturated_scene()
    geo = S.oracle_geo(oracle, sc)
    R = S.check_preconditions(sc, geo)
    assert int(geo["tiles"].max()) == 65536 and R == 65536 + sc["key"].size - 1
    big = int(np.argmax(geo["tiles"]))
    assert (sc["key"] < sc["key"][big]).sum() >= 100 and (sc["key"] > sc["key"][big]).sum() >= 100


def test_witness_on_a_hand_made_table():
    """two coarse bins: bin 0x410 split into 4 buckets, bin 0x414 in one; bucket 1 holds a pile of 49, bucket 4 is the 20-bit one"""
    dmap = np.zeros(S.COARSE_BINS, np.uint32)
    dmap[0x410] = (0 << 16) | 4; dmap[0x414] = (4 << 16) | 1
    q = 1 << 18
    keys = np.concatenate([0x41000000 + np.arange(10), np.full(49, 0x41000000 + q + 5), 0x41000000 + q + 1024 * np.arange(3),
                           0x41000000 + 2 * q + np.arange(5000) * 50, 0x41400000 + 1024 * np.arange(60) + 3]).astype(np.uint32)
    rng = np.random.default_rng(0)
    keys = keys[rng.permutation(keys.size)]
    sizes = np.array([10, 52, 5000, 0, 60])
    bs = np.zeros(2049, np.uint32); bs[1:6] = np.cumsum(sizes); bs[6:] = bs[5]
    bmap = np.zeros((2048, 2), np.uint32)
    for j in range(4):
        bmap[j] = (0x41000000 + j * q, 18)
    bmap[4] = (0x41400000, 20)
    cnt = np.zeros(32, np.uint32); cnt[S.CNT_NBUCKETS] = 5; cnt[S.CNT_VISIBLE] = keys.size; cnt[S.CNT_RENDERED] = keys.size
    s = S.route_summary(keys, dmap, bs, cnt, bmap=bmap)
    assert (s["fast"], s["stable"], s["slow"], s["nmax"], s["nonempty"]) == (2, [(52, 3)], [(5000, 3)], 5000, 4)
    assert s["fast_bits"] == {18: 1, 20: 1}
    # the direct placement's view of the same buckets: ranges from the entries; the pile and the overfull bucket are refused
    s = S.route_summary(keys, dmap, bs, cnt, bmap=None, cap=4096)
    assert s["fast"] == 2 and [r[0] for r in s["refused"]] == [52, 5000]
    with pytest.raises(AssertionError):                                # sizes that are not the table's
        bs[2] += 1
        S.route_summary(keys, dmap, bs, cnt, bmap=bmap)
