"""Host side of the batched depth / alpha maps (gm_forward_deformed_batch_aux_async) and of the edit-sequence route
(deform.plan_sequence): declared, typed, validated on the arguments alone, and the grouping of a sequence into launches."""
import ctypes as C
import os
import re

import pytest

from gaussianmesh_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_args(name):
    text = open(os.path.join(ROOT, "include", "gmesh_hip.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, name
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_header_declares_the_batch_arguments_plus_two_map_arrays():
    name = "gm_forward_deformed_batch_aux_async"
    args, base = _declared_args(name), _declared_args("gm_forward_deformed_batch_async")
    assert name in _lib.header_symbols()
    assert args[:len(base)] == base
    assert args[len(base):] == ["float* const* out_depth", "float* const* out_alpha"]
    assert _lib.SIGNATURES[name][1][:len(base)] == _lib.SIGNATURES["gm_forward_deformed_batch_async"][1]
    assert len(_lib.SIGNATURES[name][1]) == len(args)


def test_abi_version_is_still_3():
    text = open(os.path.join(ROOT, "include", "gmesh_hip.h")).read()
    assert re.search(r"#define GM_ABI_VERSION 3\b", text)
    assert _lib.lib().gm_abi_version() == 3


W, H = 64, 48
HW = W * H
MB = 1 << 20


def _frames(K):
    """K frames whose pointers pass every check of the non-map batch: distinct, 256-byte aligned, non-null"""
    frames = (_lib.BatchFrame * _lib.GM_BATCH_MAX)()
    for k in range(K):
        f = frames[k]
        f.packed, f.viewmatrix, f.projmatrix, f.cam_pos = 4096, 4096, 4096, 4096
        f.geom_buffer, f.binning_buffer, f.image_buffer = (16 + k) * MB, (32 + k) * MB, (48 + k) * MB
        f.out_color = (64 + k) * MB
    return frames


def _call(K, depth, alpha, frames=None, flags=1, W_=W, H_=H, pol=2, cap=1000):
    l = _lib.lib()
    arr = lambda ptrs: None if ptrs is None else (C.c_void_p * len(ptrs))(*ptrs)
    one = 4096
    return l.gm_forward_deformed_batch_aux_async(pol, K, _frames(K) if frames is None else frames, 10, 3, 16, W_, H_, one, one, one, one, one, one,
                                                 one, cap, flags, None, 0, None, arr(depth), arr(alpha))


def _maps(K, base):
    return [base + k * MB for k in range(K)]


def test_the_aux_batch_refuses_before_any_gpu_work():
    """Every refusal below is decided on the arguments alone: no device is touched, so it holds on a box without one."""
    l = _lib.lib()
    K = 4
    depth, alpha = _maps(K, 128 * MB), _maps(K, 160 * MB)
    # the batch's own refusals
    assert _call(_lib.GM_BATCH_MAX + 1, None, None, frames=(_lib.BatchFrame * 9)()) == 1 and b"frames" in l.gm_last_error()
    assert _call(0, None, None) == 1 and b"frames" in l.gm_last_error()
    assert _call(K, depth, alpha, flags=8) == 1 and b"unknown flags" in l.gm_last_error()
    assert _call(K, depth, alpha, W_=3840, H_=2160, pol=2) == 1 and b"list tiles" in l.gm_last_error()
    assert _call(K, depth, alpha, cap=0) == 1 and b"binning_capacity" in l.gm_last_error()
    assert _call(K, depth, alpha, frames=(_lib.BatchFrame * _lib.GM_BATCH_MAX)()) == 1 and b"null pointer" in l.gm_last_error()
    # a NULL inside a non-null array
    assert _call(K, depth[:2] + [0] + depth[3:], alpha) == 1 and b"null map pointer" in l.gm_last_error()
    assert _call(K, None, [0] + alpha[1:]) == 1 and b"null map pointer" in l.gm_last_error()
    # maps on a colour image: on its first float, inside its third plane, on its last float - of this frame or of another
    for k, at in ((0, 0), (1, 2 * HW + 5), (3, 3 * HW - 1)):
        for j in (k, (k + 1) % K):
            d = list(depth)
            d[j] = (64 + k) * MB + 4 * at
            assert _call(K, d, alpha) == 1 and b"overlaps" in l.gm_last_error(), (k, at, j)
    a = list(alpha)
    a[2] = 64 * MB + 4 * (3 * HW - 1)
    assert _call(K, None, a) == 1 and b"overlaps" in l.gm_last_error()
    # maps overlapping each other: the same pointer, and a partial overlap between frames (by range, not by pointer)
    assert _call(K, depth, depth) == 1 and b"overlaps" in l.gm_last_error()
    d = list(depth)
    d[1] = d[0]
    assert _call(K, d, None) == 1 and b"overlaps" in l.gm_last_error()
    d = list(depth)
    d[3] = d[1] + 4 * (HW - 1)
    assert _call(K, d, alpha) == 1 and b"overlaps" in l.gm_last_error()
    a = list(alpha)
    a[0] = depth[2] - 4 * (HW - 1)
    assert _call(K, depth, a) == 1 and b"overlaps" in l.gm_last_error()
    a = list(alpha)
    a[1] = depth[1] + 4 * 7
    assert _call(K, depth, a) == 1 and b"overlaps" in l.gm_last_error()


def test_the_batch_entry_point_is_unchanged():
    """gm_forward_deformed_batch_async keeps its refusals and messages (it now shares one validation with the aux entry point)."""
    l = _lib.lib()
    one = 4096
    call = lambda flags: l.gm_forward_deformed_batch_async(2, 2, _frames(2), 10, 3, 16, W, H, one, one, one, one, one, one, one, 1000, flags, None, 0, None)
    assert call(8) == 1 and l.gm_last_error().startswith(b"gm_forward_deformed_batch: unknown flags")


# ---- plan_sequence: the route of an edit sequence ----
def _plan(sizes, K, **kw):
    from gaussianmesh_amd.deform import plan_sequence
    return plan_sequence(sizes, K, **kw)


def test_plan_batches_at_frames_per_launch_and_the_remainder():
    s = [(480, 270)] * 10
    assert _plan(s, 4) == [("learn", [0]), ("batch", [1, 2, 3, 4]), ("batch", [5, 6, 7, 8]), ("batch", [9])]
    assert _plan(s, 1) == [("learn", [0])] + [("batch", [i]) for i in range(1, 10)]
    assert _plan(s, 8) == [("learn", [0]), ("batch", list(range(1, 9))), ("batch", [9])]
    assert _plan(s[:1], 4) == [("learn", [0])]
    assert _plan([], 4) == []


def test_plan_ends_a_batch_at_a_resolution_change_and_learns_each_resolution_once():
    a, b = (480, 270), (320, 240)
    s = [a, a, a, b, b, a, a, a, a, a, a, b]
    assert _plan(s, 4) == [("learn", [0]), ("batch", [1, 2]), ("learn", [3]), ("batch", [4]), ("batch", [5, 6, 7, 8]), ("batch", [9, 10]),
                           ("batch", [11])]


def test_plan_takes_the_single_frame_path_above_2048_list_tiles():
    a, big = (480, 270), (3840, 2160)
    # 4K: 8160 tiles of 32 px under policy 2 - the batch's one-pass tile sort cannot take it; policy 3 (64 px: 2040 tiles) can
    assert _plan([a, big, big, a], 4, emission_policy=2) == [("learn", [0]), ("single", [1]), ("single", [2]), ("batch", [3])]
    assert _plan([big, big, big], 4, emission_policy=3) == [("learn", [0]), ("batch", [1, 2])]
    assert _plan([(768, 768)] * 3, 4, emission_policy=1) == [("single", [0]), ("single", [1]), ("single", [2])]     # 48 x 48 tiles of 16 px
    assert _plan([(704, 736)] * 3, 4, emission_policy=1) == [("learn", [0]), ("batch", [1, 2])]                     # 44 x 46 = 2024
    assert _plan([a] * 3, 4, batchable=False) == [("single", [0]), ("single", [1]), ("single", [2])]


@pytest.mark.parametrize("K", [0, _lib.GM_BATCH_MAX + 1, -1])
def test_plan_refuses_frames_per_launch_out_of_range(K):
    with pytest.raises(ValueError):
        _plan([(64, 64)], K)
