"""Shared cases of the skinning tests (test_skin_host.py, test_gpu_skin.py): the meshes at the sizes where the kernels can go wrong,
the skeletons, the (mesh, skeleton) pairs, poses, and the float64 reference (skin_ref.System and its dense solve) run once per case and
shared.  check_general_position(), called by the host test for every case, asserts on the CPU and from the reference alone that the
inputs sit away from the two decisions rounding could flip: no (vertex, bone) pair has d_ij / d_min within 1e-9 of the near set's
threshold 1 + 1e-4, and for every cut of compaction (1 .. 4 kept) the two reference weights on either side of it differ by more than
1e-9 - except where the larger of the two is exactly 0 after clamping: such slots are unused whichever bone takes them (the far torus of
two_tori, whose rows see most bones with a right-hand side of exact zeros)."""
import functools
import math

import numpy as np

import pose_interp_cases
import skin_ref


def _grid(nx, ny):
    g = np.stack(np.meshgrid(np.linspace(-1, 1, nx), np.linspace(-1, 1, ny), indexing="ij"), -1).reshape(-1, 2)
    flat = np.concatenate([g, np.zeros((g.shape[0], 1))], 1)
    idx = np.arange(nx * ny).reshape(nx, ny)
    ff = np.concatenate([np.stack([idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:]], -1).reshape(-1, 3),
                         np.stack([idx[:-1, :-1], idx[1:, 1:], idx[:-1, 1:]], -1).reshape(-1, 3)], 0)
    return flat, ff


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(V0 float32 [Vm,3], faces int32 [F,3]); do not modify"""
    if name in ("torus_96", "torus_1073", "flat_patch", "two_tori"):
        return pose_interp_cases.mesh(name)
    if name in ("flat_255", "flat_256", "flat_257"):                   # flat_patch's grid at 16 x 16, cut or padded: the row kernels' block edge
        verts, faces = _grid(16, 16)
        if name == "flat_255":                                         # the last vertex and its faces cut away
            faces = faces[(faces != 255).all(axis=1)]
            verts = verts[:255]
        elif name == "flat_257":                                       # one vertex past the corner, on a triangle of its own
            verts = np.concatenate([verts, [[1.15, 1.1, 0.05]]], 0)
            faces = np.concatenate([faces, [[255, 254, 256]]], 0)
    elif name == "unreferenced":                                       # torus_96 and a vertex no face names
        verts, faces = pose_interp_cases.mesh("torus_96")
        verts = np.concatenate([verts, [[0.3, 0.2, -0.1]]], 0)
    else:
        raise KeyError(name)
    return np.asarray(verts, np.float32), np.asarray(faces, np.int32)


def _circle(n, radius, centre, first, seed):
    """n joints on a circle in the xz plane, jittered so that no vertex sits symmetrically between two bones"""
    rng = np.random.default_rng(seed)
    ang = first + np.arange(n) * (2 * math.pi / n) + rng.uniform(-0.05, 0.05, n)
    return np.stack([radius * np.cos(ang), rng.uniform(-0.04, 0.04, n), radius * np.sin(ang)], 1) + np.asarray(centre)


@functools.lru_cache(maxsize=None)
def skeleton(name):
    """(joints float32 [Nj,3], parents int64 [Nj]); do not modify"""
    if name == "ring5":                                                # a chain of 6 joints round the torus's centre circle: 5 bones
        joints, parents = _circle(6, 2.0, (0, 0, 0), 0.1, 5), [-1, 0, 1, 2, 3, 4]
    elif name == "one_bone":
        joints, parents = [[-1.9, 0.03, 0.2], [1.8, -0.02, 0.4]], [-1, 0]
    elif name == "chain3":                                             # across the flat patch, a little above it
        joints, parents = [[-0.93, 0.031, 0.21], [0.047, -0.023, 0.26], [0.91, 0.043, 0.17]], [-1, 0, 1]
    elif name == "star17":                                             # 17 spokes from the middle of the torus to its centre circle
        joints, parents = np.concatenate([[[0.02, 0.11, -0.03]], _circle(17, 2.0, (0, 0, 0), 0.05, 17)], 0), [-1] + [0] * 17
    elif name == "inside":                                             # wholly inside the first torus of two_tori (centre circle of radius 1)
        joints, parents = _circle(4, 1.0, (-1.6, 0, 0), 0.3, 4), [-1, 0, 1, 1]
    else:
        raise KeyError(name)
    return np.asarray(joints, np.float32), np.asarray(parents, np.int64)


CASES = (("torus_96", "ring5"), ("torus_1073", "ring5"), ("torus_96", "one_bone"), ("flat_patch", "chain3"), ("flat_255", "chain3"),
         ("flat_256", "chain3"), ("flat_257", "chain3"), ("torus_96", "star17"), ("two_tori", "inside"), ("unreferenced", "ring5"))
IDS = ["%s-%s" % c for c in CASES]


@functools.lru_cache(maxsize=None)
def system(mesh_name, skeleton_name):
    V0, faces = mesh(mesh_name)
    joints, parents = skeleton(skeleton_name)
    return skin_ref.System(V0, faces, joints, parents)


@functools.lru_cache(maxsize=None)
def dense(mesh_name, skeleton_name):
    """full [J,Vm] float64 of the dense solve; do not modify"""
    return system(mesh_name, skeleton_name).dense()


def pose(skeleton_name, T, seed=0):
    """(rotations float64 [T,Nj,3] axis-angle up to about 1 rad, root_translation float64 [T,3])"""
    rng = np.random.default_rng(1000 + seed)
    Nj = len(skeleton(skeleton_name)[0])
    return rng.uniform(-0.6, 0.6, (T, Nj, 3)), rng.uniform(-0.3, 0.3, (T, 3))


def check_general_position(mesh_name, skeleton_name):
    """the two conditions of the module's docstring; returns (the closest d_ij / d_min comes to the threshold, the smallest gap across a cut)"""
    s, full = system(mesh_name, skeleton_name), dense(mesh_name, skeleton_name)
    ratio = np.sqrt(s.d2 / s.d2min)
    margin = float(np.abs(ratio - (1.0 + 1e-4)).min())
    assert margin > 1e-9, "%s-%s: d_ij / d_min within %.3g of 1 + 1e-4" % (mesh_name, skeleton_name, margin)
    v = -np.sort(-np.maximum(full, 0.0), axis=0)                       # falling along the bones
    gap = float("inf")
    for keep in range(1, min(4, s.J - 1) + 1):
        hi, lo = v[keep - 1], v[keep]
        live = s.unknown & (hi > 0.0)
        if live.any():
            gap = min(gap, float((hi - lo)[live].min()))
    assert gap > 1e-9, "%s-%s: two weights across a cut of compaction within %.3g" % (mesh_name, skeleton_name, gap)
    return margin, gap
