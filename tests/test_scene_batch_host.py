"""Host side of the scene batch (gm_forward_scene_batch_async, rasterizer.forward_scene_batch): declared, typed, and every refusal decided
on the arguments alone - no device is touched, so all of it holds on a machine without one.  Plus the CLI's background options."""
import ctypes as C
import os
import re
import subprocess
import sys


from gaussianmesh_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gm_forward_scene_batch_async"
MB = 1 << 20
W, H, P = 64, 48, 10
HW = W * H


def _header():
    return open(os.path.join(ROOT, "include", "gmesh_hip.h")).read()


def _declared_args(name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, _header())
    assert m, name
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_header_declares_the_scene_batch_and_python_signature_matches():
    assert NAME in _lib.header_symbols() and NAME in _lib.SIGNATURES
    args = _declared_args(NAME)
    assert len(_lib.SIGNATURES[NAME][1]) == len(args)
    base = _declared_args("gm_forward_deformed_batch_async")
    assert args[:8] == base[:8]                                   # policy, K, frames, P, deg, M, width, height as the object batch
    assert args[8:11] == ["int n_objects", "const int* object_rows", "const unsigned int* deformed"]
    assert args[-5:] == base[-5:]                                 # capacity, flags, work hint, debug, stream
    m = re.search(r"#define GM_SCENE_OBJECTS_MAX (\d+)", _header())
    assert m and int(m.group(1)) == _lib.GM_SCENE_OBJECTS_MAX == 32
    assert re.search(r"#define GM_ABI_VERSION 3\b", _header()) and _lib.lib().gm_abi_version() == 3


def _frames(K):
    """K frames whose pointers pass every check of the object batch: distinct, 256-byte aligned, non-null, 1 MiB apart"""
    frames = (_lib.BatchFrame * _lib.GM_BATCH_MAX)()
    for k in range(K):
        f = frames[k]
        f.packed, f.viewmatrix, f.projmatrix, f.cam_pos = 4096, 4096, 4096, 4096
        f.geom_buffer, f.binning_buffer, f.image_buffer = (16 + k) * MB, (32 + k) * MB, (48 + k) * MB
        f.out_color, f.radii, f.status_host = (64 + k) * MB, (80 + k) * MB, (96 + k) * MB
    return frames


def _call(K=2, frames=None, rows=(4, 7, 10), masks=None, P_=P, M=16, W_=W, H_=H, pol=2, cap=1000, flags=1, tri=4096, pos=4096, scales=4096,
          rots=4096, bg=4096, n=None):
    l = _lib.lib()
    rows_a = None if rows is None else (C.c_int * len(rows))(*rows)
    masks = [0] * K if masks is None else masks
    masks_a = None if masks == "null" else (C.c_uint * max(len(masks), 1))(*masks)
    n = (len(rows) - 1 if rows is not None else 0) if n is None else n
    one = 4096
    return l.gm_forward_scene_batch_async(pol, K, _frames(K) if frames is None else frames, P_, 3, M, W_, H_, n, rows_a, masks_a, pos, scales,
                                          rots, one, one, tri, one, one, bg, cap, flags, None, 0, None)


def _refused(rc, msg):
    err = _lib.lib().gm_last_error()
    assert rc == 1 and msg in err, err
    assert err.startswith(b"gm_forward_scene_batch") or b"emission policy" in err, err


def test_the_object_batch_refusals_hold_for_the_scene_batch():
    fr = (_lib.BatchFrame * (_lib.GM_BATCH_MAX + 1))()
    _refused(_call(K=_lib.GM_BATCH_MAX + 1, frames=fr), b"frames")
    _refused(_call(K=0), b"frames")
    _refused(_call(flags=8), b"unknown flags")
    _refused(_call(flags=2), b"unknown flags")                       # GM_BATCH_COV6: the scene's covariances are [*,9]
    _refused(_call(P_=0), b"single-frame calls")
    _refused(_call(M=9), b"M == 16")
    _refused(_call(cap=0), b"binning_capacity")
    _refused(_call(W_=3840, H_=2160, pol=2), b"list tiles")
    _refused(_call(pol=9), b"emission policy")
    for kw in (dict(pos=None), dict(scales=None), dict(rots=None), dict(bg=None), dict(rows=None), dict(masks="null")):
        _refused(_call(**kw), b"null required input")
    fr = _frames(2)
    fr[1].viewmatrix = None
    _refused(_call(frames=fr), b"null pointer")
    fr = _frames(2)
    fr[1].image_buffer += 16
    _refused(_call(frames=fr), b"256-byte aligned")
    fr = _frames(2)
    fr[1].binning_buffer = fr[0].binning_buffer
    _refused(_call(frames=fr), b"share a buffer")


def test_the_row_layout_and_the_masks_are_checked():
    _refused(_call(rows=tuple(range(34)), P_=40, masks=[0, 0]), b"n_objects")       # 33 objects: more than the mask's 32 bits
    _refused(_call(rows=(0,), n=-1), b"n_objects")
    _refused(_call(rows=(4, 3, 10)), b"ascend")
    _refused(_call(rows=(4, 7, 11)), b"ascend")                     # beyond P
    _refused(_call(rows=(-1, 7, 10)), b"ascend")
    _refused(_call(masks=[0, 4]), b"at or above n_objects")          # object 2 of 2
    _refused(_call(rows=(10,), masks=[1, 0]), b"at or above n_objects")   # background only: no bit at all
    fr = _frames(2)
    fr[1].packed = None
    _refused(_call(frames=fr, masks=[0, 2]), b"packed is NULL")
    _refused(_call(masks=[1, 0], tri=None), b"tri / w / cov")


def test_frames_whose_buffers_overlap_as_ranges_are_refused():
    l = _lib.lib()
    gb, ib = l.gm_geom_bytes(P), l.gm_image_bytes(W, H)
    assert gb < MB and ib < MB and l.gm_binning_bytes(1000) < MB
    cases = [
        ("geom_buffer", 1, lambda fr: fr[0].geom_buffer + ((gb - 1) & ~255)),            # starts inside frame 0's geometry buffer
        ("binning_buffer", 2, lambda fr: fr[1].binning_buffer + 256),
        ("image_buffer", 0, lambda fr: fr[2].image_buffer + ((ib - 1) & ~255)),
        ("out_color", 2, lambda fr: fr[1].out_color + 4 * (3 * HW - 1)),                 # on frame 1's last colour float
        ("radii", 1, lambda fr: fr[0].radii + 4 * (P - 1)),
        ("radii", 2, lambda fr: fr[0].radii),
        ("status_host", 1, lambda fr: fr[2].status_host + 12),
        ("binning_buffer", 1, lambda fr: fr[0].image_buffer),                             # a buffer of another kind
        ("out_color", 0, lambda fr: fr[0].geom_buffer + 512),                            # within one frame
    ]
    for field, k, at in cases:
        fr = _frames(3)
        setattr(fr[k], field, at(fr))
        _refused(_call(K=3, frames=fr, masks=[0, 0, 0]), b"overlaps")
    # NULL radii / status_host are fine (not ranges), and a NULL gather table in a frame that deforms nothing passes the frame checks:
    # these calls get as far as the range test, which then refuses their (deliberately) overlapping colour images
    fr = _frames(3)
    fr[0].radii = fr[1].radii = fr[0].status_host = fr[1].status_host = None
    fr[0].packed = fr[1].packed = fr[2].packed = None
    fr[2].out_color = fr[1].out_color + 4
    _refused(_call(K=3, frames=fr, masks=[0, 0, 0]), b"frame 1's out_color buffer overlaps frame 2's out_color buffer")


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "gaussianmesh_amd.edit_sequence", "--object_gaussian", "o.ply", "--object_origin_mesh", "m.obj",
                           "--camera_path", ".", "--render_path", "out", "--mesh_sequence", "seq"] + list(args), cwd=ROOT, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)


def test_cli_refuses_maps_of_a_scene_and_a_background_flag_without_a_background():
    r = _cli("--background_gaussian", "bg.ply", "--save_maps")
    assert r.returncode == 2 and "--save_maps" in r.stdout and "background" in r.stdout, r.stdout[-2000:]
    r = _cli("--is_exist_bg")
    assert r.returncode == 2 and "--background_gaussian" in r.stdout, r.stdout[-2000:]
