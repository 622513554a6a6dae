#!/usr/bin/env python
"""Time of the closest-face search that binds a plain Gaussian cloud to a proxy mesh (gm_closest_face, the whole launch chain: bounding box,
Morton codes, two sorts, boxes, query), HIP events, median of 20 after 3 warm-ups:
    1 M queries x 15 000 faces (the C3 mesh), 200 k x 300 000, 1 M x 300 000, and gm_knn_nearest at 1 M x 15 000 points beside them.
On the host: edittool.point_mesh_squared_distance (numpy, float64) at 20 000 x 2 400, one run, and the device path at that size.
    python tools/mesh_bind_time.py [--no-host]"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
from gaussianmesh_amd import _lib, edittool, scenes
from gaussianmesh_amd.simple_knn import knn_nearest

dev = torch.device("cuda:0")
lib = _lib.lib()


def near_surface(verts, faces, n, rng, sigma=0.05):
    f = faces[rng.integers(len(faces), size=n)]
    a, b, c = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
    w = rng.dirichlet((1.0, 1.0, 1.0), size=n)
    nrm = np.cross(b - a, c - a); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return (w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c + rng.normal(0.0, sigma, size=(n, 1)) * nrm).astype(np.float32)


def median_ms(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), float(min(out)), float(max(out))


def closest_chain(P, V, F):
    """the C call alone on preallocated buffers (no allocation, no copy inside the timed window)"""
    N, Vm, nF = P.shape[0], V.shape[0], F.shape[0]
    d2 = torch.empty(N, device=dev); face = torch.empty(N, dtype=torch.int32, device=dev); close = torch.empty((N, 3), device=dev)
    nbytes = lib.gm_closest_face_workspace_bytes(N, nF)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    return lambda: _lib.check(lib.gm_closest_face(N, P.data_ptr(), Vm, V.data_ptr(), nF, F.data_ptr(), d2.data_ptr(), face.data_ptr(), close.data_ptr(),
                                                  ws.data_ptr(), nbytes, st)), nbytes


rng = np.random.default_rng(0)
meshes = {"15k": scenes.torus_mesh(), "300k": scenes.torus_mesh(400, 375)}
t = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
rows = {}
for label, mesh, N in (("1M x 15k", "15k", 1000000), ("200k x 300k", "300k", 200000), ("1M x 300k", "300k", 1000000)):
    V, F = meshes[mesh]
    fn, nbytes = closest_chain(t(near_surface(V, F, N, rng)), t(V), t(F, torch.int32))
    rows[label] = median_ms(fn)
    print("gm_closest_face %-12s median %.3f ms (min %.3f, max %.3f), workspace %.1f MB" % ((label,) + rows[label] + (nbytes / 1e6,)), flush=True)
print("1M x 300k over 1M x 15k: %.2f x" % (rows["1M x 300k"][0] / rows["1M x 15k"][0]))
V, F = meshes["15k"]
q, r = t(near_surface(V, F, 1000000, rng)), t(near_surface(V, F, 15000, rng, sigma=0.0))
print("gm_knn_nearest  1M x 15k points  median %.3f ms (min %.3f, max %.3f) [python wrapper: allocates its workspace per call]" % median_ms(lambda: knn_nearest(q, r)))
if "--no-host" not in sys.argv:
    V, F = scenes.torus_mesh(40, 30)
    P = near_surface(V, F, 20000, rng)
    fn, _ = closest_chain(t(P), t(V), t(F, torch.int32))
    print("gm_closest_face 20k x 2.4k      median %.3f ms (min %.3f, max %.3f)" % median_ms(fn))
    t0 = time.perf_counter()
    edittool.point_mesh_squared_distance(P, V, F)
    print("host edittool.point_mesh_squared_distance 20k x 2.4k (numpy float64, one run): %.1f s" % (time.perf_counter() - t0))
