"""Shared cases of the ARAP tests (test_arap_host.py, test_gpu_arap.py): small meshes with their handles and handle targets, and the
float64 reference (arap_ref.Reference) run once per case and shared.  All coordinates stay below 4 in magnitude."""
import functools
import math

import numpy as np

from gaussianmesh_amd import scenes

import arap_ref

NAMES = ("torus_a", "torus_b", "torus_c", "flat_patch", "fan", "one_handle")
OUTER = 10                      # outer iterations of the shared reference run


def rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def flat_patch_mesh():
    """the 12 x 9 flat grid of test_gpu_mesh_rs.py: open boundary, planar one-rings"""
    g = np.stack(np.meshgrid(np.linspace(-1, 1, 12), np.linspace(-1, 1, 9), indexing="ij"), -1).reshape(-1, 2)
    flat = np.concatenate([g, np.zeros((g.shape[0], 1))], 1)
    idx = np.arange(12 * 9).reshape(12, 9)
    ff = np.concatenate([np.stack([idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:]], -1).reshape(-1, 3),
                         np.stack([idx[:-1, :-1], idx[1:, 1:], idx[:-1, 1:]], -1).reshape(-1, 3)], 0).astype(np.int32)
    return flat, ff, idx


def fan_mesh(n=40):
    """an apex over n rim vertices on the unit circle: one one-ring of valence n"""
    t = np.arange(n) * (2 * math.pi / n)
    verts = np.concatenate([[[0.0, 0.0, 0.5]], np.stack([np.cos(t), np.sin(t), np.zeros(n)], -1)], 0)
    faces = np.array([[0, 1 + k, 1 + (k + 1) % n] for k in range(n)], np.int32)
    return verts, faces


def _torus(nu, nv):
    verts, faces = scenes.torus_mesh(nu, nv)
    V0 = verts.astype(np.float32)
    ang = np.arctan2(V0[:, 2].astype(np.float64), V0[:, 0].astype(np.float64))
    still = np.nonzero(np.abs(ang) < 0.25)[0]
    moved = np.nonzero(np.abs(np.abs(ang) - math.pi) < 0.25)[0]
    target = V0[moved].astype(np.float64) @ rotation((0, 0, 1), 0.6).T + np.array([0.0, 0.8, 0.0])
    return V0, faces, np.concatenate([still, moved]), np.concatenate([V0[still].astype(np.float64), target], 0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(V0 float32 [Vm,3], faces int32 [F,3], handles int64 [H], targets float32 [H,3])"""
    if name in ("torus_a", "torus_b", "torus_c"):
        V0, faces, handles, targets = _torus(*{"torus_a": (12, 8), "torus_b": (30, 20), "torus_c": (37, 29)}[name])
    elif name == "flat_patch":
        flat, faces, idx = flat_patch_mesh()
        V0 = flat.astype(np.float32)
        left, right = idx[0, :], idx[-1, :]
        c = np.array([1.0, 0.0, 0.0])
        moved = (V0[right].astype(np.float64) - c) @ rotation((0, 1, 0), -0.9).T + c + np.array([0.6, 0.0, 0.7])
        handles, targets = np.concatenate([left, right]), np.concatenate([V0[left].astype(np.float64), moved], 0).astype(np.float32)
    elif name == "fan":
        verts, faces = fan_mesh()
        V0 = verts.astype(np.float32)
        handles = np.array([0, 1, 14, 27])
        targets = np.concatenate([[[0.2, 0.1, 1.1]], V0[[1, 14, 27]].astype(np.float64)], 0).astype(np.float32)
    elif name == "one_handle":
        V0, faces = case("torus_c")["V0"], case("torus_c")["faces"]
        handles = np.array([5])
        targets = (V0[[5]].astype(np.float64) + np.array([0.3, -0.2, 0.5])).astype(np.float32)
    else:
        raise KeyError(name)
    return dict(name=name, V0=V0, faces=np.asarray(faces, np.int32), handles=np.asarray(handles, np.int64), targets=targets)


def start(c, init=None):
    """the starting positions of a solve: init (the rest pose when None) with the handle rows at their targets, float32"""
    X = np.array(c["V0"] if init is None else init, np.float32)
    X[c["handles"]] = c["targets"]
    return X


@functools.lru_cache(maxsize=None)
def reference(name):
    return arap_ref.Reference(case(name)["V0"], case(name)["faces"], case(name)["handles"])


@functools.lru_cache(maxsize=None)
def reference_run(name):
    """(positions after each of OUTER outer iterations with exact global steps [OUTER,Vm,3], stats [OUTER,8]); do not modify"""
    return reference(name).solve(start(case(name)), OUTER)


def pinned_mesh():
    """torus_mesh(12, 8) plus vertex 96, which no face names, and vertex 97, which sits exactly on vertex 3 and belongs only to the
    zero-area face (97, 3, 4): both are pinned.  Returns (V0 float32, faces)."""
    verts, faces = scenes.torus_mesh(12, 8)
    V0 = np.concatenate([verts, [[0.5, 3.0, -0.25]], verts[3:4]], 0).astype(np.float32)
    return V0, np.concatenate([faces, [[97, 3, 4]]], 0).astype(np.int32)
