"""The definitions gm_mesh_geodesic and mesh_region.surface_graph are held to, written for reading: a float32 Dijkstra over a CSR (heapq,
cutoff, several source sets), the same fixed point by Jacobi sweeps in numpy, and surface_graph restated edge by edge in plain loops."""
import heapq
import math

import numpy as np

f32 = np.float32


def dijkstra32(row_offsets, cols, lengths, source_sets, max_distance=math.inf):
    """float32 [B, Vm]: per source set the smallest left-to-right float32 path sum, +inf beyond max_distance (inclusive) or unreachable"""
    Vm = len(row_offsets) - 1
    cut = f32(max_distance)
    out = np.full((len(source_sets), Vm), np.inf, f32)
    for b, srcs in enumerate(source_sets):
        d = out[b]
        heap = []
        for s in srcs:
            if d[s] != 0:
                d[s] = 0
                heap.append((0.0, int(s)))
        heapq.heapify(heap)
        while heap:
            du, u = heapq.heappop(heap)
            if du > d[u]:
                continue
            for e in range(row_offsets[u], row_offsets[u + 1]):
                cand = f32(f32(du) + lengths[e])
                w = cols[e]
                if cand <= cut and cand < d[w]:
                    d[w] = cand
                    heapq.heappush(heap, (float(cand), int(w)))
    return out


def jacobi32(row_offsets, cols, lengths, sources, max_distance=math.inf):
    """(float32 [Vm], sweeps): d <- min(d, min_u fl(d[u] + l_uv)) over all rows at once from the previous d, until nothing lowers"""
    Vm = len(row_offsets) - 1
    rows = np.repeat(np.arange(Vm), np.diff(np.asarray(row_offsets, np.int64)))
    d = np.full(Vm, np.inf, f32)
    d[list(sources)] = 0
    sweeps = 0
    while True:
        sweeps += 1
        cand = (d[cols] + lengths).astype(f32)
        cand[~(cand <= f32(max_distance))] = np.inf
        new = d.copy()
        np.minimum.at(new, rows, cand)
        if np.array_equal(new, d):
            return d, sweeps
        d = new


def _norm(x):
    return math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])


def _dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def unfolded(a, b, c, e):
    """the virtual edge across (a, b) between the opposite points c and e (float64 triples): its float32 length, or None"""
    ab = [b[k] - a[k] for k in range(3)]
    L = _norm(ab)
    if not L > 0:
        return None
    u = [x / L for x in ab]
    ca, ea = [c[k] - a[k] for k in range(3)], [e[k] - a[k] for k in range(3)]
    cx, ex = _dot(ca, u), _dot(ea, u)
    cy = math.sqrt(max(_dot(ca, ca) - cx * cx, 0.0))
    ey = math.sqrt(max(_dot(ea, ea) - ex * ex, 0.0))
    if not (cy > 0 and ey > 0):
        return None
    xs = cx + (ex - cx) * cy / (cy + ey)
    if not 0 < xs < L:
        return None
    return f32(np.hypot(cx - ex, cy + ey))


def surface_graph_ref(vertices, faces, unfold=True):
    """mesh_region.surface_graph, edge by edge: (row_offsets int32, cols int32, lengths float32)"""
    V = np.asarray(vertices, f32).astype(np.float64).tolist()
    F = np.asarray(faces, np.int64).tolist()
    best = {}

    def add(p, q, length):
        for key in ((p, q), (q, p)):
            if key not in best or length < best[key]:
                best[key] = length
    wings = {}
    for face in F:
        for k in range(3):
            p, q, o = face[(k + 1) % 3], face[(k + 2) % 3], face[k]
            if p == q:
                continue
            add(p, q, f32(_norm([V[p][i] - V[q][i] for i in range(3)])))
            wings.setdefault((min(p, q), max(p, q)), []).append(o)
    if unfold:
        for (a, b), opp in wings.items():
            if len(opp) == 2 and opp[0] != opp[1]:
                length = unfolded(V[a], V[b], V[opp[0]], V[opp[1]])
                if length is not None:
                    add(opp[0], opp[1], length)
    Vm = len(V)
    keys = sorted(best)
    off = np.zeros(Vm + 1, np.int64)
    for p, _ in keys:
        off[p + 1] += 1
    return np.cumsum(off).astype(np.int32), np.array([q for _, q in keys], np.int32), np.array([best[k] for k in keys], f32)


def random_graph(Vm, rng, max_degree=12, zero_fraction=0.0):
    """a symmetric CSR with 0 .. max_degree neighbours a vertex (about a tenth of the vertices isolated), lengths in (0, 1], many of
    them multiples of 1/16 so that distinct paths tie exactly"""
    edges = {}
    alone = rng.random(Vm) < 0.1
    want = np.where(alone, 0, rng.integers(0, max_degree + 1, size=Vm))
    degree = np.zeros(Vm, np.int64)
    for p in range(Vm):
        for q in rng.integers(0, Vm, size=want[p]):
            if p != q and (p, int(q)) not in edges and not alone[q] and degree[p] < max_degree and degree[q] < max_degree:
                degree[p] += 1; degree[q] += 1
                l = f32(rng.integers(1, 17)) / f32(16) if rng.random() < 0.3 else f32(rng.uniform(0.01, 1.0))
                if rng.random() < zero_fraction:
                    l = f32(0)
                edges[(p, int(q))] = edges[(int(q), p)] = l
    return csr_of(Vm, edges)


def csr_of(Vm, edges):
    """{(p, q): length} (both directions given) -> CSR"""
    keys = sorted(edges)
    off = np.zeros(Vm + 1, np.int64)
    for p, _ in keys:
        off[p + 1] += 1
    return np.cumsum(off).astype(np.int32), np.array([q for _, q in keys], np.int32).reshape(-1), np.array([edges[k] for k in keys], f32).reshape(-1)


def grid_mesh(n):
    """n x n vertices in the plane z = 0 with unit spacing, one diagonal per cell: (vertices float32 [n*n,3], faces int32)"""
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="xy")
    V = np.stack([i.reshape(-1), j.reshape(-1), np.zeros(n * n)], 1).astype(f32)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    F = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)], 0).astype(np.int32)
    return V, F
