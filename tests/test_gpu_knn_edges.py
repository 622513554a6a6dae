"""-m gpu: the Morton front end of the two k-NN operators (bounding box, 30-bit codes, the sort that hands back its own result) at its
edges - a flat axis, a cloud away from the origin, a cloud that is one point, a box and one point - through distCUDA2 and knn_nearest,
each bit for bit against the float32 brute force that defines it (oracle.knn_mean_dist2, _brute_np).  closest_faces, the third user of
that front end, has these cases in test_gpu_mesh_bind.py."""
import numpy as np
import pytest
import torch

from test_gpu_bg_train import _brute_np

pytestmark = pytest.mark.gpu
f32 = np.float32


def _cloud(kind):
    rng = np.random.default_rng(len(kind))
    if kind == "flat z":                                   # a flat axis: extent 0 in z, two boxes
        pts = rng.normal(size=(1500, 3)).astype(f32)
        pts[:, 2] = 0.0
    elif kind == "off origin":                             # the origin lies outside the true bounding box
        pts = rng.normal(size=(1500, 3)).astype(f32) + np.array([100, 50, 25], f32)
    elif kind == "one point":                              # every extent is 0 and every distance is 0
        pts = np.tile(np.array([[0.5, -1.25, 3.0]], f32), (1100, 1))
    else:
        assert kind == "two boxes and one"
        pts = rng.normal(size=(2049, 3)).astype(f32)
    return pts


@pytest.mark.parametrize("kind", ["flat z", "off origin", "one point", "two boxes and one"])
def test_distCUDA2_edges(oracle, kind):
    from gaussianmesh_amd import distCUDA2
    pts = _cloud(kind)
    ref = oracle.knn_mean_dist2(pts)
    assert np.isfinite(ref).all()
    if kind == "one point":
        assert (ref == 0).all()
    out = distCUDA2(torch.as_tensor(pts).cuda()).cpu().numpy()
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))


def _nearest_case(kind):
    rng = np.random.default_rng(len(kind))
    if kind == "coplanar":                                 # x constant; queries on the plane, off it, outside the box
        r = rng.normal(size=(600, 3)).astype(f32)
        r[:, 0] = 0.75
        q = rng.normal(size=(300, 3)).astype(f32)
        q[:100, 0] = 0.75
        q[200:] += np.array([0, 9, -9], f32)
    elif kind == "one point":                              # every reference point the same: the lowest index wins every tie
        r = np.tile(np.array([[0.5, -1.25, 3.0]], f32), (300, 1))
        q = rng.normal(size=(100, 3)).astype(f32) * 3
        q[0] = r[0]
    else:
        assert kind == "wave and one, box and one"
        r = rng.normal(size=(257, 3)).astype(f32)
        q = rng.normal(size=(65, 3)).astype(f32) * 1.5
    return q, r


@pytest.mark.parametrize("kind", ["coplanar", "one point", "wave and one, box and one"])
def test_knn_nearest_edges(kind):
    from gaussianmesh_amd.simple_knn import knn_nearest
    q, r = _nearest_case(kind)
    wd, wi = _brute_np(q, r)
    assert np.isfinite(wd).all()
    if kind == "coplanar":
        outside = ((q < r.min(0)) | (q > r.max(0))).any(1)
        assert (q[:100, 0] == 0.75).all() and (q[100:200, 0] != 0.75).all() and outside[200:].all()
    if kind == "one point":
        assert (wi == 0).all()
    d2, idx = knn_nearest(torch.as_tensor(q).cuda(), torch.as_tensor(r).cuda())
    assert np.array_equal(idx.cpu().numpy(), wi)
    assert np.array_equal(d2.cpu().numpy().view(np.uint32), wd.astype(f32).view(np.uint32))

