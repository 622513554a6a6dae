"""One mesh whose rows put arap_rotation (gaussianmesh_amd/csrc/gm_arap_shared.h) on every route of its eigen-route polar decomposition and
its callers' row loops on every ring size around ARAP_POSE_BATCH = 8.  Host only, numpy only.  Used by test_polar_routes_host.py (CPU)
and test_gpu_polar_routes.py (GPU).

THE MESH is a disjoint union of small components: closed tetrahedra and open fans (an apex over n rim vertices, n - 1 faces; the apex
row has n edges).  Every rest coordinate is a multiple of 1/4; component k sits at the rest offset (3 k, 0, 0).  The pose of a
component is its own 3 x 3 map A applied to its LOCAL coordinates (no offset: components overlap in the pose, which ARAP does not see),
so row i of the component has S_i = A M_i with M_i = sum_j w_ij (p_i - p_j)(p_i - p_j)^T, and A chooses the route.  Every map but the
three generic ones has one entry per row, plus or minus a power of two: those poses are exact in float32 and the pose edges in float64.

THE CLASS OF A ROW comes from the SVD of its float64 S_i = U diag(s0, s1, s2) V^T, d = sign det(U V^T): r = s1 / s0 and
gap = (s1 + d s2) / s0 (the proper polar factor is determined to eps / gap; the eigen-route, which squares the condition number, to
eps / gap^2):
    identity   r <= 2.5e-13, or S = 0     the device and the reference both return I (their cut is r <= 1e-12)
    well       gap >= 1e-2                R_i is the SVD's rotation element by element
    gap0       r >= 1e-2, gap < 1e-2      reflected rows with s1 ~ s2: the last direction is free; held to the window bar
    window     4e-12 <= r, gap < 1e-2     needles: R_i maximises tr(R^T S_i) only to within the window bar
No row may have r in (2.5e-13, 4e-12): the device measures s as |S e_k|, the reference by SVD, and next to the cut they could disagree.
THE BARS on the deficit tr(R_svd^T S) - tr(Q^T S) >= 0 of a rotation Q (test_polar_routes_host.py holds eigen_route to them):
    well    64 eps s0        a backward-stable rotation loses O(eps s0)
    window  8 sqrt(eps) s0   the eigenvector of S^T S is off by an angle of about eps s0^2 / s1^2 (capped at 1) and the loss is about
                             s1 angle^2: largest near s1 = sqrt(eps) s0, about sqrt(eps) s0 = 1.5e-8 s0; 8 covers the order of the sums
    identity  0
"""
import functools

import numpy as np

import arap_ref

EPS = float(np.finfo(np.float64).eps)
RING_SIZES = (3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 24, 25)
NEEDLE_K = (0, 4, 10, 20, 24, 27, 30, 34, 36, 42, 50)
IDENTITY_BELOW, WINDOW_FROM, WELL_GAP = 2.5e-13, 4e-12, 1e-2
IDENTITY, WELL, WINDOW, GAP0 = "identity", "well", "window", "gap0"
P = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])     # a quarter turn about z: exact
TRANSLATION = np.array([0.25, 0.5, -0.25])
MOVED_BY = np.array([0.25, 0.0, 0.25])                                  # "one_moved": rim vertex 1 of the fan by this much
SPACING = 3.0


def rot(axis, ang):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def needle(k):
    return "needle%d" % k


def needle_reflected(k):
    return "needle%d_reflected" % k


@functools.lru_cache(maxsize=None)
def maps():
    """name -> 3 x 3 float64 map, in a fixed order.  "translation" and "one_moved" are the identity map; their pose adds TRANSLATION to
    every vertex / MOVED_BY to one vertex."""
    m = {}
    for k in NEEDLE_K:
        m[needle(k)] = P @ np.diag([1.0, 2.0 ** -k, 2.0 ** -(k + 1)])
        m[needle_reflected(k)] = np.diag([1.0, 2.0 ** -k, -(2.0 ** -(k + 1))])
    m["line"] = P @ np.diag([1.0, 0.0, 0.0])
    m["point"] = np.zeros((3, 3))
    m["plane"] = P @ np.diag([1.0, 0.5, 0.0])
    m["mirror"] = np.diag([1.0, 1.0, -1.0])
    m["point_reflection"] = -np.eye(3)
    m["half_turn"] = np.diag([-1.0, -1.0, 1.0])
    m["two_p"] = 2.0 * P
    m["rest"] = np.eye(3)
    m["translation"] = np.eye(3)
    m["one_moved"] = np.eye(3)
    m["generic_a"] = rot([1, 2, -0.5], 0.9) @ np.diag([1.3, 0.8, 1.1])
    m["generic_b"] = rot([0.2, 1, 0.4], 2.1) @ np.diag([0.7, 1.6, 0.9])
    m["generic_c"] = rot([-1, 0.3, 0.8], 1.4) @ np.diag([2.0, 0.5, 1.2])
    return m


GENERIC = ("generic_a", "generic_b", "generic_c")
RING_MAPS = ("generic_a", needle_reflected(0), needle(20))                # every ring size: a generic, a reflected and a window map


def exact(name):
    return name not in GENERIC


# ---------------------------------------------------------------------------------------------- components
def _perimeter():
    """the 32 points of the square |x|, |y| <= 1 on the 1/4 lattice, counter-clockwise from (1, 0)"""
    q = np.arange(-4, 5) / 4.0
    pts = [(1.0, y) for y in q[4:]] + [(x, 1.0) for x in q[-2::-1]] + [(-1.0, y) for y in q[-2::-1]] + [(x, -1.0) for x in q[1:]] + \
          [(1.0, y) for y in q[1:4]]
    assert len(pts) == 32 and len(set(pts)) == 32
    return np.array(pts)


def tet():
    v = np.array([[0, 0, 0], [1, 0.25, 0], [0.25, 1, 0.25], [0.5, 0.25, 1]], np.float64)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int64)
    return v, f


def regular_tet():
    """all four rows alike up to the signs of the axes: under a diagonal map every row has the same singular values"""
    v = np.array([[0, 0, 0], [1, 1, 0], [1, 0, 1], [0, 1, 1]], np.float64)
    return v, tet()[1]


def fan(n, planar=False):
    """apex (vertex 0) at (1/4, 0, 1/2) over n rim vertices spread over the square (planar: the apex in the rim's plane); faces
    (apex, rim k, rim k + 1), k = 0 .. n - 2: open, so the apex has n edges, the first and last rim vertex 2, the others 3"""
    rim = _perimeter()[(np.arange(n) * 32) // max(n, 5)]              # (n < 5: over part of the square, so that no apex angle is obtuse)
    v = np.concatenate([[[0.25, 0.0, 0.0 if planar else 0.5]], np.concatenate([rim, np.zeros((n, 1))], 1)], 0)
    k = np.arange(n - 1)
    f = np.stack([np.zeros(n - 1, np.int64), 1 + k, 2 + k], 1)
    return v, f


def component(kind, map_name):
    """kind: "tet", "rtet" (the regular one), "fan<n>" or "planar<n>" """
    if kind == "tet":
        v, f = tet()
    elif kind == "rtet":
        v, f = regular_tet()
    elif kind.startswith("planar"):
        v, f = fan(int(kind[6:]), planar=True)
    else:
        v, f = fan(int(kind[3:]))
    assert np.array_equal(v * 4, np.round(v * 4))
    x = v @ maps()[map_name].T
    if map_name == "translation":
        x = x + TRANSLATION
    if map_name == "one_moved":
        x[1] += MOVED_BY
    return dict(kind=kind, map=map_name, v=v, f=f, x=x)


OTHER_KINDS = ("tet", "fan4", "planar5")
# Next to the cut a component's rows must all stay on one side of the forbidden band, which is 16 wide where k = 36 and k = 42 are 64
# apart: the rows of one component may differ by 4 in r.  The tetrahedron above spreads by 8 (k = 42 puts two of its rows at 4.2e-13
# and 5.1e-13, inside the band), so these maps go on the components that stay clear of it: the regular tetrahedron (one r for all four
# rows: 8.3e-12 at k = 36, 1.3e-13 at k = 42) and, at k = 36, the fans listed (at k = 42 no fan of this module stays clear: every one
# has a row above 2.5e-13).  The regular tetrahedron also gives the maps that keep lengths
# their rows with EQUAL singular values (mirror: s1 = s2 to the last bit, so gap = 0).
KINDS_OF = {36: ("tet", "rtet", "fan6", "planar6"), 42: ("rtet",)}
WITH_REGULAR_TET = ("mirror", "point_reflection", "half_turn", "two_p", "rest", "generic_a", needle(0), needle_reflected(0))


def kinds_of(name):
    for k, kinds in KINDS_OF.items():
        if name in (needle(k), needle_reflected(k)):
            return kinds
    return OTHER_KINDS + (("rtet",) if name in WITH_REGULAR_TET else ())


@functools.lru_cache(maxsize=None)
def full_spec():
    """the whole table: every map on a tetrahedron and two fans (one planar: rank-2 rows at every pose), every ring size with a generic,
    a reflected and a window map; "one_moved" on a fan of 6 (rim vertices 3 .. 6 are unmoved rows next to the moved apex row)"""
    spec = []
    for name in maps():
        if name == "one_moved":
            spec.append(("fan6", name))
            continue
        spec += [(kind, name) for kind in kinds_of(name)]
    spec += [("fan%d" % n, name) for n in RING_SIZES for name in RING_MAPS]
    return tuple(spec)


class Mesh:
    """V0 / V1 float32 [Vm,3], faces int32, comp [Vm] (component index, -1: a padding vertex no face names), comps (the component
    dicts with their first row `base`), and lazily the reference, the rows' S and SVD, class and bar"""

    def __init__(self, spec, pad_front=0):
        V0, V1, F, comp, comps = [], [], [], [], []
        base = pad_front
        for p in range(pad_front):                                      # unreferenced vertices: pinned rows
            V0.append([[-SPACING * (p + 1), 0.5, 0.25]]); V1.append([[0.25 * p, -0.5, 0.75]]); comp.append([-1])
        for k, (kind, name) in enumerate(spec):
            c = dict(component(kind, name), base=base, index=k)
            V0.append(c["v"] + [SPACING * k, 0.0, 0.0]); V1.append(c["x"]); F.append(c["f"] + base); comp.append([k] * len(c["v"]))
            comps.append(c)
            base += len(c["v"])
        self.spec, self.comps = tuple(spec), comps
        V0_64, V1_64 = np.concatenate(V0, 0), np.concatenate(V1, 0)
        self.V0, self.V1 = V0_64.astype(np.float32), V1_64.astype(np.float32)
        assert np.array_equal(self.V0.astype(np.float64), V0_64)        # the rest pose is exact whatever the maps
        self.V1_unrounded = V1_64
        self.faces = np.concatenate(F, 0).astype(np.int32)
        self.comp = np.concatenate(comp, 0)
        self.Vm = len(self.V0)

    def rows_of(self, c):
        return np.arange(c["base"], c["base"] + len(c["v"]))

    @functools.cached_property
    def ref(self):
        return arap_ref.Reference(self.V0, self.faces, [])

    @functools.cached_property
    def table(self):
        """per row: S [Vm,3,3], s [Vm,3], d [Vm], R_svd [Vm,3,3], r, gap, cls (object array), bar, valence, ok (the row and all its
        neighbours are well or identity: the gradient row is compared element by element)"""
        ref, X = self.ref, self.V1.astype(np.float64)
        S = np.zeros((self.Vm, 3, 3))
        np.add.at(S, ref.I, ref.w[:, None, None] * (X[ref.I] - X[ref.J])[:, :, None] * ref.E0[:, None, :])
        U, s, Vt = np.linalg.svd(S)
        d = np.where(np.linalg.det(U @ Vt) < 0, -1.0, 1.0)
        D = np.tile(np.eye(3), (self.Vm, 1, 1))
        D[:, 2, 2] = d
        R = U @ D @ Vt
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(s[:, 0] > 0, s[:, 1] / s[:, 0], 0.0)
            gap = np.where(s[:, 0] > 0, (s[:, 1] + d * s[:, 2]) / s[:, 0], 0.0)
        cls = np.full(self.Vm, "forbidden", object)
        cls[(r >= WINDOW_FROM) & (gap < WELL_GAP)] = WINDOW
        cls[(r >= 1e-2) & (gap < WELL_GAP)] = GAP0
        cls[gap >= WELL_GAP] = WELL
        cls[(r <= IDENTITY_BELOW) | (s[:, 0] == 0)] = IDENTITY
        R[cls == IDENTITY] = np.eye(3)
        bar = np.where(cls == WELL, 64 * EPS, np.where(cls == IDENTITY, 0.0, 8 * np.sqrt(EPS))) * s[:, 0]
        good = np.isin(cls, (WELL, IDENTITY))
        ok = good.copy()
        np.logical_and.at(ok, ref.I, good[ref.J])
        return dict(S=S, s=s, d=d, R=R, r=r, gap=gap, cls=cls, bar=bar, valence=np.bincount(ref.I, minlength=self.Vm), ok=ok)

    def component_classes(self, c):
        return set(self.table["cls"][self.rows_of(c)])

    def handles(self):
        """two vertices of every component (a fan: its first and last rim vertex), for the solves with free rows"""
        return np.array([c["base"] + k for c in self.comps for k in ((0, 1) if c["kind"].endswith("tet") else (1, len(c["v"]) - 1))], np.int64)


@functools.lru_cache(maxsize=None)
def mesh(which):
    """"all": the whole table.  "well": its components all of whose rows are well or identity; "window": the others.  "p256" / "p257":
    a part of the table behind 42 / 43 vertices no face names, 256 / 257 rows: the last component, a window fan of 17, ends with row 255
    / lies across rows 255 | 256, the edge between two workgroups of the row kernels.  ("fan<n>", map): that fan alone."""
    if isinstance(which, tuple):
        return Mesh([which])
    if which == "all":
        return Mesh(full_spec())
    if which in ("well", "window"):
        m = mesh("all")
        calm = [c["index"] for c in m.comps if m.component_classes(c) <= {WELL, IDENTITY}]
        return Mesh([s for k, s in enumerate(full_spec()) if (k in calm) == (which == "well")])
    if which in ("p256", "p257"):
        spec = [(kinds_of(name)[0], name) for name in maps() if name != "one_moved"] + [("fan%d" % n, needle(20)) for n in (7, 8, 9, 15, 16, 17)]
        m = Mesh(spec, pad_front=int(which[1:]) - sum(len(component(*s)["v"]) for s in spec))
        assert m.Vm == int(which[1:]) and m.comps[-1]["base"] + 18 == m.Vm
        return m
    raise KeyError(which)


GROUPS = ("all", "well", "window", "p256", "p257")


# ---------------------------------------------------------------------------------------------- the device's arithmetic, in float64 numpy
def jacobi3(A):
    """gm_mat3.h jacobi3, statement by statement: A (symmetric 3 x 3, a copy is diagonalised) -> (diagonalised A, V)"""
    A = np.array(A, np.float64)
    V = np.eye(3)
    scale = abs(A[0, 0]) + abs(A[1, 1]) + abs(A[2, 2]) + 1e-300
    for sweep in range(10):
        off = abs(A[0, 1]) + abs(A[0, 2]) + abs(A[1, 2])
        if off <= 1e-16 * scale:
            break
        for pq in range(3):
            p, q = (1 if pq == 2 else 0), (1 if pq == 0 else 2)
            apq = A[p, q]
            if abs(apq) <= 1e-300:
                continue
            theta = (A[q, q] - A[p, p]) / (2.0 * apq)
            t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
            cs = 1.0 / np.sqrt(t * t + 1.0)
            sn = t * cs
            r = 3 - p - q
            arp, arq = A[r, p], A[r, q]
            A[p, p] -= t * apq; A[q, q] += t * apq; A[p, q] = A[q, p] = 0.0
            A[r, p] = A[p, r] = cs * arp - sn * arq
            A[r, q] = A[q, r] = sn * arp + cs * arq
            for k in range(3):
                vp, vq = V[k, p], V[k, q]
                V[k, p] = cs * vp - sn * vq; V[k, q] = sn * vp + cs * vq
    return A, V


def eigen_route(F):
    """gm_arap_shared.h arap_rotation, statement by statement, in float64: the proper rotation closest to F; identity for rank <= 1"""
    F = np.asarray(F, np.float64)
    Q = np.eye(3)
    C = np.array([[F[0, i] * F[0, j] + F[1, i] * F[1, j] + F[2, i] * F[2, j] for j in range(3)] for i in range(3)])
    with np.errstate(all="ignore"):
        _, E = jacobi3(C)
        FE = np.array([[F[i, 0] * E[0, k] + F[i, 1] * E[1, k] + F[i, 2] * E[2, k] for k in range(3)] for i in range(3)])
        sig = [float(np.sqrt(FE[0, k] * FE[0, k] + FE[1, k] * FE[1, k] + FE[2, k] * FE[2, k])) for k in range(3)]
        for step in range(3):
            a = 1 if step == 1 else 0
            b = a + 1
            if sig[a] < sig[b]:
                sig[a], sig[b] = sig[b], sig[a]
                FE[:, [a, b]] = FE[:, [b, a]]
                E[:, [a, b]] = E[:, [b, a]]
        if not sig[1] > 1e-12 * sig[0]:
            return Q
        ep, eq = E[:, 0].copy(), E[:, 1].copy()
        cross = lambda a, b: np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
        em = cross(ep, eq)
        up = FE[:, 0] / sig[0]
        dpq = 0.0
        for i in range(3):
            dpq += up[i] * FE[i, 1]
        uq = FE[:, 1] - dpq * up
        lq = 0.0
        for i in range(3):
            lq += uq[i] * uq[i]
        uq = uq / np.sqrt(lq)
        um = cross(up, uq)
        return np.array([[up[i] * ep[j] + uq[i] * eq[j] + um[i] * em[j] for j in range(3)] for i in range(3)])


def deficit(S, R_opt, Q):
    """tr(R_opt^T S) - tr(Q^T S): what the rotation Q loses against the optimum, per row"""
    return np.einsum("nab,nab->n", R_opt, S) - np.einsum("nab,nab->n", Q, S)


# ---------------------------------------------------------------------------------------------- key poses for the pose interpolator
INTERP_KINDS = ("tet", "rtet", "fan4", "planar5")
INTERP_KEYS = ("rest", needle(10), needle(30), "line", "point", "generic_a")
INTERP_TS = (0.0, 0.25, 0.5, 1.0)
INTERP_PAIRS = tuple((a, b) for a in INTERP_KEYS for b in INTERP_KEYS if a != b)


@functools.lru_cache(maxsize=None)
def interp_key(name):
    """the two tetrahedra and two fans, every component posed by the map `name`: (V0, faces) do not depend on the name, V1 is the key"""
    return Mesh([(kind, name) for kind in INTERP_KINDS])


def interp_anchors():
    """the first vertex of every component"""
    return np.array([c["base"] for c in interp_key("rest").comps], np.int64)
