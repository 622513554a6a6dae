"""Host side of the per-Gaussian blend weights (gm_blend_weights, gaussianmesh_amd/contribution.py): the float64 reference's own
identities on the shared scenes, the C entry point's refusals on the arguments alone, and select / importance_rows / split_plain on CPU
tensors.  No GPU."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import blend_weights_ref as ref


@pytest.mark.parametrize("name", ref.SCENES)
def test_reference_identities_and_census(oracle, name):
    """sum_i w_i = 1 - T_final per pixel to 1e-12 (asserted inside the walk, pixel by pixel); 1 - T_final is the oracle's own opacity -
    the difference of two renders on backgrounds 0 and 1 - to the forward gate's 1e-4; no pixel has a decision at a threshold."""
    sc, cam, fw, mask, r = ref.reference(oracle, name)
    W, H = cam["W"], cam["H"]
    f1 = oracle.forward_full(sc, cam, np.ones(3, np.float32), use_precomp_color=True)
    alpha = 1.0 - (f1["color"][0].astype(np.float64) - fw["color"][0])
    err = np.abs(r["one_minus_T"] - alpha)
    print("%s: %d Gaussians contribute, %d pixels stop, up to %d accepted entries per pixel; |1 - T - oracle| max %.3g; census %d" % (
        name, int((r["n_acc"] > 0).sum()), int(r["stopped"].sum()), int(r["accepted"].max()), err.max(), r["census"]))
    assert err.max() <= 1e-4
    assert r["census"] == 0
    assert np.all(r["inside"] <= r["total"] * (1 + 1e-12)) and np.all(r["peak"] <= 0.99 + 1e-12)
    assert np.array_equal(r["n_acc"] == 0, r["total"] == 0)
    # an all-255 mask: inside == total
    if name == "s0":
        full = ref.walk(fw, W, H, None)
        assert np.allclose(full["inside"], full["total"], rtol=1e-14, atol=0) and np.array_equal(full["total"], r["total"])


def test_saturating_scene_reaches_the_stop_rule(oracle):
    """1887 of 1920 pixels stop, after up to 111 accepted entries (more than one batch of 64 survivors); the largest weight is a front-most
    entry's alpha, just below the scene's opacity 0.95 (the min(0.99, .) clamp is the single-Gaussian GPU case's, opacity 1)."""
    r = ref.reference(oracle, "sat")[4]
    assert r["stopped"].sum() == 1887 and r["accepted"].max() == 111 and r["n_acc"].sum() > 60000
    assert 0.9 < r["peak"].max() <= 0.95


def test_symbol_and_signature():
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    name = "gm_blend_weights"
    assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(l, name)
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
    assert m and len(m.group(1).split(",")) == 13 == len(_lib.SIGNATURES[name][1])
    assert m.group(1).strip().endswith("void* stream")
    assert l.gm_abi_version() == 3


def test_argument_validation_happens_before_any_gpu_work():
    """Every refusal is decided on the arguments alone: bogus non-null pointers are never dereferenced, no device is touched."""
    from gaussianmesh_amd import _lib
    l = _lib.lib()
    P, W, H, cap = 10, 64, 48, 100
    gb, ib, bb = l.gm_geom_bytes(P), l.gm_image_bytes(W, H), l.gm_binning_bytes(cap)
    geom, binning, img, mask, sums, peak = 1 << 30, 2 << 30, 3 << 30, 4 << 30, 5 << 30, 6 << 30

    def call(pol=2, geom=geom, binning=binning, img=img, P=P, cap=cap, W=W, H=H, mask=mask, sums=sums, peak=peak):
        return l.gm_blend_weights(pol, geom, binning, img, P, cap, W, H, mask, sums, peak, 0, None)

    for pol in (-1, 4, 9):
        assert call(pol=pol) == 1 and b"emission policy" in l.gm_last_error()
    assert call(P=-1) == 1 and b"invalid sizes" in l.gm_last_error()
    for w, h in ((0, 48), (64, 0), (-3, 48)):
        assert call(W=w, H=h) == 1 and b"invalid sizes" in l.gm_last_error()
    for w, h in ((65521, 16), (16, 65521)):
        assert call(W=w, H=h) == 1 and b"4095 x 4095 tiles" in l.gm_last_error()
    assert call(pol=0, W=8192, H=8192) == 1 and b"list tiles" in l.gm_last_error()           # 262144 lists of 16 px; fine under policy 3
    assert call(cap=-1) == 1 and b"capacity" in l.gm_last_error()
    for kw in (dict(geom=None), dict(binning=None), dict(img=None), dict(sums=None)):
        assert call(**kw) == 1 and b"null" in l.gm_last_error(), kw
    # overlaps: sums / peak against each other, the mask and the three state buffers (range overlap, first and last byte)
    for kw, what in ((dict(peak=sums), b"sums overlaps peak"), (dict(peak=sums + 16 * P - 1), b"sums overlaps peak"),
                     (dict(sums=peak + 4 * P - 1), b"sums overlaps peak"),
                     (dict(mask=sums + 8), b"mask overlaps sums"), (dict(sums=mask + W * H - 1), b"mask overlaps sums"),
                     (dict(peak=mask), b"mask overlaps peak"),
                     (dict(sums=geom), b"geom_buffer overlaps sums"), (dict(sums=geom + gb - 1), b"geom_buffer overlaps sums"),
                     (dict(peak=geom + 64), b"geom_buffer overlaps peak"),
                     (dict(sums=binning + bb - 1), b"binning_buffer overlaps sums"), (dict(peak=binning), b"binning_buffer overlaps peak"),
                     (dict(sums=img + ib - 1), b"image_buffer overlaps sums"), (dict(peak=img + 8), b"image_buffer overlaps peak")):
        assert call(**kw) == 1 and what in l.gm_last_error(), (kw, l.gm_last_error())
    # P == 0 returns GM_OK and touches nothing (every pointer bogus or NULL)
    assert call(P=0) == 0 and call(P=0, geom=None, binning=None, img=None, sums=None, peak=None, mask=None) == 0
    # peak and mask are optional; a frame without instances needs no launch
    assert call(cap=0, peak=None, mask=None) == 0


def test_python_wrapper_names_the_offending_argument():
    from gaussianmesh_amd import contribution as cb
    from gaussianmesh_amd._lib import GmeshError
    u8 = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(GmeshError, match="no CPU path"):
        cb.blend_weights(2, u8, u8, u8, 4, 8, 8, num_rendered=0)
    with pytest.raises(GmeshError, match="geom"):
        cb.blend_weights(2, u8.float(), u8, u8, 4, 8, 8, num_rendered=0)
    with pytest.raises(GmeshError, match="mask"):
        cb._check("mask", torch.zeros(8, 8), torch.uint8, (8, 8), u8.device)
    with pytest.raises(GmeshError, match="sums"):
        cb._check("sums", torch.zeros(4, 3, dtype=torch.int64), torch.int64, (4, 2), u8.device)
    with pytest.raises(GmeshError, match="peak.*contiguous"):
        cb._check("peak", torch.zeros(8, dtype=torch.int32)[::2], torch.int32, (4,), u8.device)


def _contribution(total_units, inside_units255, peak):
    from gaussianmesh_amd import contribution as cb
    sums = torch.tensor(np.stack([total_units, inside_units255], 1), dtype=torch.int64)
    bits = torch.tensor(np.asarray(peak, np.float32)).view(torch.int32)
    return cb.contribution_from_raw(sums, bits, 3)


def test_select_and_importance_rows():
    from gaussianmesh_amd import contribution as cb
    U = 1 << 24
    #                 row:  0        1          2      3 (never seen)  4            5 (tie with 1)  6
    total = np.array([4 * U, 2 * U, U, 0, 8 * U, 2 * U, 3], np.int64)
    inside = np.array([255 * 4 * U, 255 * U, 0, 0, 255 * 4 * U + 1, 255 * U + 1, 3 * 255], np.int64)
    peak = np.array([0.5, 0.25, 1.0 / 255.0, 0.0, 0.99, 0.003, 1e-6], np.float32)
    c = _contribution(total, inside, peak)
    assert c.views == 3 and c.total.dtype == torch.float64 and c.peak.dtype == torch.float32
    assert c.total.tolist() == [4.0, 2.0, 1.0, 0.0, 8.0, 2.0, 3 * 2.0 ** -24]
    assert c.inside[0].item() == 4.0 and c.inside[1].item() == 1.0
    # inside / total > threshold, strictly: row 1 sits exactly at 0.5, rows 4 and 5 one unit above; the never-seen row is False
    assert cb.select(c).tolist() == [True, False, False, False, True, True, True]
    assert cb.select(c, threshold=0.0).tolist() == [True, True, False, False, True, True, True]
    assert cb.select(c, threshold=1.0).tolist() == [False] * 7
    assert cb.select(c, min_total=2.0).tolist() == [True, False, False, False, True, False, False]
    # the largest totals, ties by row id: order 4, 0, 1, 5, 2, 6, 3
    rows = lambda f: [i for i, k in enumerate(cb.importance_rows(c, keep_fraction=f).tolist()) if k]
    assert rows(1.0) == [0, 1, 2, 3, 4, 5, 6] and rows(0.0) == []
    assert rows(3 / 7) == [0, 1, 4]                        # of the tied rows 1 and 5 the lower id
    assert rows(0.5) == [0, 1, 4, 5]                       # round(3.5) = 4 (half to even)
    assert rows(0.36) == [0, 1, 4] and rows(0.35) == [0, 4]    # round(2.52) = 3, round(2.45) = 2
    # min_peak: 1/255 (as float32) keeps a row whose largest weight is exactly that, and drops the never-seen row
    assert cb.importance_rows(c, min_peak=1.0 / 255.0).tolist() == [True, True, True, False, True, False, False]
    assert cb.importance_rows(c, min_peak=0.0).tolist() == [True] * 7
    assert cb.importance_rows(c, keep_fraction=0.5, min_peak=0.1).tolist() == [True, True, False, False, True, False, False]
    assert cb.importance_rows(c).tolist() == [True] * 7
    from gaussianmesh_amd._lib import GmeshError
    with pytest.raises(GmeshError):
        cb.importance_rows(c, keep_fraction=1.5)


def test_split_plain_round_trips_through_ply(tmp_path):
    from gaussianmesh_amd import contribution as cb, io as gio
    from gaussianmesh_amd.bg_model import PlainGaussians
    g = torch.Generator().manual_seed(3)
    P = 37
    pc = PlainGaussians(3, device="cpu")
    pc._set_params(torch.randn(P, 3, generator=g), torch.randn(P, 16, 3, generator=g), torch.randn(P, 3, generator=g),
                   torch.randn(P, 4, generator=g), torch.randn(P, 1, generator=g))
    pc.active_sh_degree = 2
    rows = torch.rand(P, generator=g) < 0.4
    sel, rest = cb.split_plain(pc, rows)
    assert sel.get_number == int(rows.sum()) and rest.get_number == P - int(rows.sum())
    assert sel.active_sh_degree == rest.active_sh_degree == 2 and sel.max_sh_degree == 3 and sel.optimizer is None
    for part, m in ((sel, rows), (rest, ~rows)):
        for name in ("_xyz", "_features", "_scaling", "_rotation", "_opacity"):
            assert torch.equal(getattr(part, name), getattr(pc, name)[m]), name
        path = str(tmp_path / "part.ply")
        gio.save_plain_gaussians(path, cb.plain_columns(part))
        back = cb.load_plain(path, 3, "cpu")
        for name in ("_xyz", "_features", "_scaling", "_rotation", "_opacity"):
            assert torch.equal(getattr(back, name), getattr(part, name)), name
    # all rows / no rows
    a, b = cb.split_plain(pc, torch.ones(P, dtype=torch.bool))
    assert a.get_number == P and b.get_number == 0
    from gaussianmesh_amd._lib import GmeshError
    with pytest.raises(GmeshError):
        cb.split_plain(pc, torch.ones(P + 1, dtype=torch.bool))


def test_cli_refuses_to_overwrite_its_input(tmp_path):
    from gaussianmesh_amd import contribution as cb
    scene = str(tmp_path / "scene.ply")
    open(scene, "wb").close()
    for argv in (["--gaussian", scene, "-s", "x", "--out_object", scene],
                 ["--gaussian", scene, "-s", "x", "--out_pruned", str(tmp_path / "." / "scene.ply"), "--min_peak", "0.1"],
                 ["--gaussian", scene, "-s", "x"],
                 ["--gaussian", scene, "-s", "x", "--out_pruned", str(tmp_path / "p.ply")],
                 ["--gaussian", scene, "-s", "x", "--out_object", str(tmp_path / "a.ply"), "--out_background", str(tmp_path / "a.ply")]):
        with pytest.raises(SystemExit):
            cb.parse_args(argv)
    a = cb.parse_args(["--gaussian", scene, "-s", "x", "--out_object", str(tmp_path / "o.ply"), "--out_background", str(tmp_path / "b.ply")])
    assert a.threshold == 0.5 and a.resolution == -1
