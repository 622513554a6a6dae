"""Shared cases of the pose-interpolation tests (test_pose_interp_ref_host.py, test_gpu_pose_interp.py): the meshes at the sizes where the
kernels can go wrong, key poses, the pairs that are interpolated, and the float64 reference (pose_interp_ref.Reference) run once per
case and shared.  All coordinates stay below 4 in magnitude, and every face's rotation between two paired keys stays below 3.1 rad
(test_pose_interp_ref_host.py checks both), so the band near a half turn, where the definition leaves the side open, is never entered."""
import functools
import math

import numpy as np

from gaussianmesh_amd import scenes

import arap_cases
import pose_interp_ref

MESHES = ("torus_96", "torus_256", "torus_1073", "flat_patch", "two_tori", "pinned")
TS = (0.0, 1e-9, 0.25, 0.5, 1.0)
AXIS = (0.0, 1.0, 0.0)
SHIFT = np.array([0.4, 0.3, -0.2])
# mesh -> its name in arap_cases, for the solved ARAP pose
ARAP = {"torus_96": "torus_a", "torus_1073": "torus_c", "flat_patch": "flat_patch", "pinned": "torus_a"}


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(V0 float32 [Vm,3], faces int32 [F,3])"""
    if name.startswith("torus_"):
        verts, faces = scenes.torus_mesh(*{"torus_96": (12, 8), "torus_256": (16, 16), "torus_1073": (37, 29)}[name])
    elif name == "flat_patch":
        verts, faces, _ = arap_cases.flat_patch_mesh()
    elif name == "two_tori":                                           # two components: 96 + 63 vertices
        (va, fa), (vb, fb) = scenes.torus_mesh(12, 8), scenes.torus_mesh(9, 7)
        verts = np.concatenate([0.5 * va + [-1.6, 0.0, 0.0], 0.5 * vb[:, [1, 0, 2]] + [1.6, 0.2, 0.0]], 0)
        faces = np.concatenate([fa, fb[:, [0, 2, 1]] + len(va)], 0)    # (the swapped axes mirror the second torus: its faces are turned back)
    elif name == "pinned":
        return arap_cases.pinned_mesh()
    else:
        raise KeyError(name)
    return verts.astype(np.float32), np.asarray(faces, np.int32)


def turned(V, angle, axis=AXIS, shift=SHIFT, centre=None):
    """V turned rigidly by `angle` about `axis` through its centroid (or `centre`), then shifted; float64"""
    V = np.asarray(V, np.float64)
    c = V.mean(0) if centre is None else np.asarray(centre, np.float64)
    return (V - c) @ arap_cases.rotation(axis, angle).T + c + shift


def twisted(V):
    """a twist about the y axis through the centroid, 0.2 rad at the bottom to 0.8 rad at the top, with a 1.3x stretch along y"""
    V = np.asarray(V, np.float64)
    c = V.mean(0)
    d = V - c
    phi = 0.5 + 0.3 * d[:, 1] / np.abs(d[:, 1]).max()
    out = np.stack([np.cos(phi) * d[:, 0] + np.sin(phi) * d[:, 2], 1.3 * d[:, 1], -np.sin(phi) * d[:, 0] + np.cos(phi) * d[:, 2]], 1)
    return out + c


@functools.lru_cache(maxsize=None)
def key(mesh_name, key_name):
    """a key pose of the mesh, float32 [Vm,3]; do not modify"""
    V0 = mesh(mesh_name)[0].astype(np.float64)
    if key_name == "rest":
        K = V0
    elif key_name == "turn179":
        K = turned(V0, math.radians(179.0))
    elif key_name == "turn177":
        K = turned(V0, math.radians(177.0))
    elif key_name == "twist":
        K = twisted(V0)
    elif key_name == "arap":                                           # the solved pose of the shared ARAP reference run
        pose = arap_cases.reference_run(ARAP[mesh_name])[0][-1]
        K = V0.copy()
        K[:len(pose)] = pose
    elif key_name == "own_way":                                        # two_tori: each component about its own centroid, its own way
        K = V0.copy()
        K[:96] = turned(V0[:96], 2.5, (0, 1, 0), (0.0, 0.3, 0.0))
        K[96:] = turned(V0[96:], -2.0, (1, 0, 0), (0.1, -0.2, 0.3))
    elif key_name == "collapsed":                                      # the twist with face 0 collapsed onto its first vertex
        K = twisted(V0)
        f = mesh(mesh_name)[1][0]
        K[f[1]] = K[f[0]]
        K[f[2]] = K[f[0]]
    else:
        raise KeyError(key_name)
    return K.astype(np.float32)


def pairs(mesh_name):
    """the (A, B) key names interpolated on this mesh"""
    p = [("rest", "twist"), ("twist", "turn179"), ("rest", "turn177"), ("turn179", "turn179")]
    if mesh_name in ARAP:
        p += [("rest", "arap"), ("arap", "twist")]
    if mesh_name == "two_tori":
        p += [("rest", "own_way")]
    return p


def anchors(mesh_name):
    """the anchor ids of the anchored mode: at least one per component that has a free vertex"""
    Vm = mesh(mesh_name)[0].shape[0]
    if mesh_name == "two_tori":
        return np.array([0, 40, 96, 130])
    if mesh_name == "pinned":
        return np.array([5, 50, 80])
    return np.array([0, Vm // 3, (2 * Vm) // 3])


ALL = [(m, a, b, mode) for m in MESHES for (a, b) in pairs(m) for mode in ("centroid", "anchors")]


@functools.lru_cache(maxsize=None)
def reference(mesh_name, mode):
    V0, faces = mesh(mesh_name)
    return pose_interp_ref.Reference(V0, faces, None if mode == "centroid" else anchors(mesh_name))


@functools.lru_cache(maxsize=None)
def reference_run(mesh_name, a, b, mode):
    """[len(TS),Vm,3] float64 of the float32 keys; do not modify"""
    return reference(mesh_name, mode).between(key(mesh_name, a), key(mesh_name, b), TS)
