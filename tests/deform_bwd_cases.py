"""Inputs of the tests of gm_deform_shade_bwd (test_deform_bwd_ref_host.py, test_gpu_deform_bwd.py): the cases of deform_cases.py (257 rows on
the 96-vertex torus; a smaller N is the prefix [:N]) with seeded upstream gradients, and rewired bindings of the `twist` case for the edges
of the vertex accumulation (one wave per vertex, 64 lanes striding the list):

  edges        vertex 0 has no incident entry, vertices 1..5 have 1, 63, 64, 65 and 129, the last vertex none; the rest is spread evenly
  hub          vertex 7 holds all three corners of rows 0..199: a list of 600 entries, longer than four waves' lanes
  last_unused  the case's own binding with the last vertex id rewired to its neighbour: the tables' last row gets no entry

Upstream gradients: N(0, 1), g_cov6 scaled by 1 / max|O| of its row so that the three routes contribute comparably.  Everything is cached
and read-only."""
import functools

import numpy as np

import deform_cases as dc
import deform_ref as ref

REWIRED = ("edges", "hub", "last_unused")
KINDS = dc.KINDS + REWIRED
NS = (1, 63, 64, 65, 257)
EDGE_COUNTS = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 5: 129}
HUB, HUB_ROWS = 7, 200


def base_kind(kind):
    return "twist" if kind in REWIRED else kind


def _rewire(kind, tri):
    Vm = dc.mesh()[0].shape[0]
    tri = tri.copy()
    if kind == "edges":
        flat = np.empty(3 * dc.NMAX, np.int32)
        order = np.random.default_rng(7).permutation(flat.size)
        at = 0
        for v, n in EDGE_COUNTS.items():
            flat[order[at:at + n]] = v
            at += n
        rest = order[at:]
        flat[rest] = 6 + np.arange(rest.size) % (Vm - 7)                        # vertices 6 .. Vm - 2
        tri = flat.reshape(-1, 3)
    elif kind == "hub":
        tri[:HUB_ROWS] = HUB
    elif kind == "last_unused":
        tri[tri == Vm - 1] = Vm - 2
    return tri


@functools.lru_cache(maxsize=None)
def case(kind):
    """deform_cases.case of the kind (a rewired binding: the twist case with another tri), plus Vm"""
    c = dict(dc.case(base_kind(kind)))
    c["kind"] = kind
    c["Vm"] = c["dV"].shape[0]
    if kind in REWIRED:
        c["tri"] = dc._ro(_rewire(kind, c["tri"]))
    return c


def shs(kind, deg):
    return dc.shs(base_kind(kind), deg)


@functools.lru_cache(maxsize=None)
def cameras(kind):
    """the two colour cameras: far, and 1e-3 from row NEAR_ROW's deformed centre under this kind's binding"""
    c = case(kind)
    npos = ref.stage1(*ref.stage1_inputs(c), np.float64)[0]
    return (("far", dc.CAMPOS), ("near", dc._ro((npos[dc.NEAR_ROW] + 1e-3 * np.array([0.6, 0.0, 0.8])).astype(np.float32))))


@functools.lru_cache(maxsize=None)
def upstream(kind):
    """dict g_pos [257,3], g_cov6 [257,6], g_rgb [257,3], float32"""
    c = case(kind)
    rng = np.random.default_rng(500 + KINDS.index(kind))
    O = ref.stage1(*ref.stage1_inputs(c), np.float64)[1]
    g6 = rng.normal(size=(dc.NMAX, 6)) / np.abs(O).max(1, keepdims=True)
    return dict(g_pos=dc._ro(rng.normal(size=(dc.NMAX, 3)).astype(np.float32)), g_cov6=dc._ro(g6.astype(np.float32)),
                g_rgb=dc._ro(rng.normal(size=(dc.NMAX, 3)).astype(np.float32)))


def list_lengths(kind, n=dc.NMAX):
    return np.bincount(case(kind)["tri"][:n].reshape(-1), minlength=case(kind)["Vm"])


def forward64(kind, deg, campos, n=dc.NMAX):
    """float64 forward of the first n rows: (npos, rgb)"""
    c = case(kind)
    npos, _, Rt = ref.stage1(*ref.stage1_inputs(c, n), np.float64)
    return npos, ref.stage2(deg, npos, Rt, campos, shs(kind, deg)[:n], np.float64)


def args(kind, deg, campos, n=dc.NMAX):
    """the positional arguments of deform_bwd_ref.backward up to g_rgb, for the first n rows"""
    c, u = case(kind), upstream(kind)
    return (deg, c["tri"][:n], c["w"][:n], c["dV"], c["Rv"], c["Sv"], c["cov"][:n], c["pos"][:n], shs(kind, deg)[:n], campos, u["g_pos"][:n],
            u["g_cov6"][:n], u["g_rgb"][:n])
