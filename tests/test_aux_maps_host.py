"""Host side of the depth / alpha maps (gm_forward_1_aux, gm_backward_aux): declared, typed, and validated before any GPU work."""
import os
import re

import pytest

from gaussianmesh_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_args(name):
    text = open(os.path.join(ROOT, "include", "gmesh_hip.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name, extra", [("gm_forward_1_aux", ("float* out_depth", "float* out_alpha")),
                                         ("gm_backward_aux", ("const float* dL_ddepth", "const float* dL_dalpha", "float* dL_dz"))])
def test_header_declares_and_lib_types_the_aux_entry_points(name, extra):
    base = {"gm_forward_1_aux": "gm_forward_1_geom", "gm_backward_aux": "gm_backward_p"}[name]
    args, base_args = _declared_args(name), _declared_args(base)
    assert name in _lib.header_symbols()
    assert len(args) == len(base_args) + len(extra)
    assert len(_lib.SIGNATURES[name][1]) == len(args)
    # the base's arguments, then the new ones (gm_backward_aux: before debug / stream)
    if name == "gm_forward_1_aux":
        assert args[:len(base_args)] == base_args and tuple(args[len(base_args):]) == extra
    else:
        assert args[:-2 - len(extra)] == base_args[:-2] and tuple(args[-2 - len(extra):-2]) == extra and args[-2:] == base_args[-2:]


def test_abi_version_unchanged():
    text = open(os.path.join(ROOT, "include", "gmesh_hip.h")).read()
    assert re.search(r"#define GM_ABI_VERSION 3\b", text)


def test_aux_entry_points_validate_before_any_gpu_work():
    """aliasing and bad sizes are refused on the arguments alone: no device is touched, so this holds without one"""
    l = _lib.lib()
    W, H = 64, 48
    HW = W * H
    base = 1 << 24
    color = base
    fwd = lambda depth, alpha, P=10, w=W, h=H, pol=2, flags=0: l.gm_forward_1_aux(
        pol, 4096, 4096, 4096, P, 100, 0, 4096, w, h, color, 0, None, None, flags, None, depth, alpha)
    assert fwd(color, None) == 1 and b"overlap" in l.gm_last_error()                        # depth on the red plane
    assert fwd(None, color + 4 * (2 * HW)) == 1 and b"overlap" in l.gm_last_error()        # alpha on the blue plane
    assert fwd(None, color + 4 * (3 * HW - 1)) == 1                                          # last float of the image
    assert fwd(base + (8 << 20), base + (8 << 20) + 4 * (HW - 1)) == 1                       # the two maps overlap
    assert fwd(None, None, P=-1) == 1 and b"invalid sizes" in l.gm_last_error()
    assert fwd(None, None, w=0) == 1
    assert fwd(None, None, pol=7) == 1 and b"emission policy" in l.gm_last_error()
    assert fwd(None, None, flags=3) == 1
    one = 4096
    P = 100
    d3 = base
    bwd = lambda dz, P=P, pol=2, dD=None, dA=None: l.gm_backward_aux(
        pol, P, 3, 16, 10, one, W, H, one, one, None, one, 1.0, one, None, one, one, one, 1.0, 1.0, None, one, one, one, one,
        one, None, one + 8192, None, d3, None, one, one, one, dD, dA, dz, 0, None)
    assert bwd(d3 + 4 * (3 * P - 1)) == 1 and b"dL_dz" in l.gm_last_error()                  # dL_dz inside dL_dmean3D
    assert bwd(None, pol=9) == 1 and b"emission policy" in l.gm_last_error()
    assert bwd(None, P=-3, dD=one) == 1


_REFUSED_LATER = 9          # an emission policy out of range: what a call that got past the overlap check is refused for


def _backward_aux(l, P, mean3d, mean2d, opacity, dz, pol):
    one = 4096
    return l.gm_backward_aux(pol, P, 3, 16, 10, one, 64, 48, one, one, None, one, 1.0, one, None, one, one, one, 1.0, 1.0, None, one, one, one,
                             one, mean2d, None, opacity, None, mean3d, None, one, one, one, None, None, dz, 0, None)


@pytest.mark.parametrize("target", ["dL_dmean3D", "dL_dmean2D", "dL_dopacity"])
def test_backward_aux_refuses_dz_on_every_gradient_output_it_is_checked_against(target):
    """dL_dz ([P] floats) against dL_dmean3D ([P,3]), dL_dmean2D ([P,3]) and dL_dopacity ([P]): refused when it reaches the first or the
    last byte of one of them, not when it lies back to back with it.  The overlap check is the first thing the call does, so made-up
    addresses do, and a call that passes it is recognised by the next refusal (the policy)."""
    l = _lib.lib()
    P = 7
    at = {"dL_dmean3D": 1 << 24, "dL_dmean2D": 2 << 24, "dL_dopacity": 3 << 24}
    nbytes = {"dL_dmean3D": 12 * P, "dL_dmean2D": 12 * P, "dL_dopacity": 4 * P}[target]
    t, dz_bytes = at[target], 4 * P
    call = lambda dz, pol=2: _backward_aux(l, P, at["dL_dmean3D"], at["dL_dmean2D"], at["dL_dopacity"], dz, pol)
    for dz in (t - dz_bytes + 1,           # dL_dz's last byte is the target's first
               t - dz_bytes + 4,           # ... its last float the target's first
               t,                          # the same start
               t + nbytes - 4,             # dL_dz's first float is the target's last
               t + nbytes - 1):            # ... its first byte the target's last
        for pol in (2, _REFUSED_LATER):   # ahead of every other check of the call
            assert call(dz, pol) == 1, (target, dz - t, pol)
            assert b"overlaps" in l.gm_last_error() and b"dL_dz" in l.gm_last_error(), (target, dz - t, l.gm_last_error())
    for dz in (t - dz_bytes, t + nbytes):  # back to back, before and behind: not an overlap
        assert call(dz, _REFUSED_LATER) == 1, (target, dz - t)
        assert b"overlaps" not in l.gm_last_error() and b"emission policy" in l.gm_last_error(), (target, dz - t, l.gm_last_error())


def test_forward_1_aux_names_the_overlap_and_lets_back_to_back_maps_through():
    l = _lib.lib()
    W, H = 64, 48
    HW = W * H
    color, maps = 1 << 24, (1 << 24) + (8 << 20)
    fwd = lambda depth, alpha, pol=2: l.gm_forward_1_aux(pol, 4096, 4096, 4096, 10, 100, 0, 4096, W, H, color, 0, None, None, 0, None, depth, alpha)
    for pol in (2, _REFUSED_LATER):
        assert fwd(maps, maps + 4 * (HW - 1), pol) == 1 and b"overlap" in l.gm_last_error()       # alpha starts on depth's last float
        assert fwd(maps + 4 * (HW - 1), maps, pol) == 1 and b"overlap" in l.gm_last_error()       # depth starts on alpha's last float
        assert fwd(None, color + 4 * (3 * HW - 1), pol) == 1 and b"overlap" in l.gm_last_error()  # alpha starts on the image's last float
    # back to back: depth right behind the image, alpha right behind depth; and the maps right in front of the image
    assert fwd(color + 4 * 3 * HW, color + 4 * 4 * HW, _REFUSED_LATER) == 1
    assert b"overlap" not in l.gm_last_error() and b"emission policy" in l.gm_last_error()
    assert fwd(color - 4 * HW, color - 4 * 2 * HW, _REFUSED_LATER) == 1
    assert b"overlap" not in l.gm_last_error() and b"emission policy" in l.gm_last_error()
