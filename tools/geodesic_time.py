#!/usr/bin/env python
"""Time of the surface distances behind mesh_region (SurfaceGraph.distances: gm_mesh_geodesic in chunks of sweeps_per_check launches, one
4-byte read-back a chunk), wall clock around whole calls with the device idle before and after, median after a warm-up, on tori of about
7.5 k, 60 k and 480 k vertices (unfolded graphs, 12 neighbours a vertex), for B = 1 and 8 source sets of one vertex each, unlimited and
limited to the radius that covers about 5 % of the surface around the first source.  Next to each: scipy.sparse.csgraph.dijkstra on the
same graph on the host (limit= where a radius applies) - for TIME only, the host path is float64 - and how far the two are apart.
Then the chunk length: sweeps_per_check 16 / 64 / 256 on the middle mesh.
    python tools/geodesic_time.py [--quick]        (--quick: without the 480 k mesh)"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import dijkstra
from gaussianmesh_amd import scenes
from gaussianmesh_amd.mesh_region import SurfaceGraph

dev = torch.device("cuda:0")


def median_s(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return float(np.median(out)), float(min(out)), float(max(out))


def host_s(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn()
        out.append(time.perf_counter() - t0)
    return float(np.median(out))


quick = "--quick" in sys.argv
meshes = [(100, 75), (300, 200)] + ([] if quick else [(800, 600)])
graphs = {}
for nu, nv in meshes:
    V, F = scenes.torus_mesh(nu, nv)
    t0 = time.perf_counter()
    g = SurfaceGraph(V, F, device=dev)
    built = time.perf_counter() - t0
    graphs[(nu, nv)] = g
    off, cols, lens = g.csr
    host = csr_matrix((lens.astype(np.float64), cols, off), shape=(g.Vm, g.Vm))
    rng = np.random.default_rng(nu)
    sources = [0] + rng.integers(0, g.Vm, size=7).tolist()
    first = g.distances([[0]])
    radius = float(first[0].kthvalue(g.Vm // 20).values)
    print("torus_mesh(%d, %d): %d vertices, %d graph entries, surface_graph + upload %.2f s, 5 %% radius %.4f" % (nu, nv, g.Vm, len(cols), built, radius), flush=True)
    for B in (1, 8):
        sets = [[s] for s in sources[:B]]
        for limit in (None, radius):
            reps = 3 if g.Vm > 100000 else 7
            dev_t = median_s(lambda: g.distances(sets, max_distance=limit), reps)
            d = g.distances(sets, max_distance=limit).cpu().numpy()
            sweeps = g.sweeps_enqueued
            kw = {} if limit is None else dict(limit=limit)
            ref = [None]

            def on_host():
                ref[0] = dijkstra(host, directed=True, indices=sources[:B], **kw)
            host_t = host_s(on_host, 1 if g.Vm > 100000 else 3)
            both = np.isfinite(d) & np.isfinite(ref[0])
            apart = float(np.abs(d[both] - ref[0][both]).max()) if both.any() else 0.0
            print("  B %d %-15s device median %8.3f ms (min %.3f, max %.3f), %4d sweeps enqueued | scipy dijkstra %9.3f ms | %6.1f x | "
                  "reached %d / %d, max |float32 - float64| %.2g, reached sets differ at %d vertices" % (
                      B, "unlimited" if limit is None else "r = %.4f" % limit, dev_t[0] * 1e3, dev_t[1] * 1e3, dev_t[2] * 1e3, sweeps, host_t * 1e3,
                      host_t / dev_t[0], int(np.isfinite(d).sum()), d.size, apart, int((np.isfinite(d) != np.isfinite(ref[0])).sum())), flush=True)
g = graphs[(300, 200)]
sets = [[s] for s in [0] + np.random.default_rng(300).integers(0, g.Vm, size=7).tolist()]
for chunk in (16, 64, 256):
    t = median_s(lambda: g.distances(sets, sweeps_per_check=chunk), 7)
    print("sweeps_per_check %3d on %d vertices, B 8, unlimited: median %.3f ms (min %.3f, max %.3f), %d sweeps enqueued" % (
        chunk, g.Vm, t[0] * 1e3, t[1] * 1e3, t[2] * 1e3, g.sweeps_enqueued), flush=True)
