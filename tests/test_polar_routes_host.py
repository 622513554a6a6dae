"""Host checks of tests/polar_route_cases.py: the table populates what it claims, and the float64 restatement of the device's
arap_rotation (polar_route_cases.eigen_route) stays within every bar the GPU test holds the device to, against the SVD.  This is what
shows that the bars are those of the method and not of one machine: orthogonality and det within 1e-13 on every row, the deficit
tr(R_svd^T S) - tr(Q^T S) within 64 eps s0 on `well` rows and 8 sqrt(eps) s0 on `window` and `gap0` rows, exactly I on `identity` rows,
and |Q - R_svd| <= 1e-10 on `well` rows.  The worst value of each is printed."""
import functools

import numpy as np

import polar_route_cases as pc


@functools.lru_cache(maxsize=None)
def routed():
    """(mesh, table, Q [Vm,3,3] of eigen_route on every row's S); shared, do not modify"""
    m = pc.mesh("all")
    return m, m.table, np.array([pc.eigen_route(S) for S in m.table["S"]])


def test_poses_are_exact_in_float32_apart_from_the_generic_ones():
    m = pc.mesh("all")
    for name, A in pc.maps().items():
        if pc.exact(name):                                              # one entry per row at most, plus or minus a power of two: every
            nz = A[A != 0]                                              # pose coordinate is one exact product
            assert ((A != 0).sum(axis=1) <= 1).all() and np.array_equal(np.abs(nz), 2.0 ** np.round(np.log2(np.abs(nz)))), name
    inexact = set()
    for c in m.comps:
        rows = m.rows_of(c)
        same = np.array_equal(m.V1[rows].astype(np.float64), m.V1_unrounded[rows])
        assert same or not pc.exact(c["map"]), (c["kind"], c["map"])
        if not same:
            inexact.add(c["map"])
    assert inexact == set(pc.GENERIC)
    assert np.array_equal(m.V0 * 4, np.round(m.V0 * 4)) and np.isfinite(m.V1).all()
    assert float(np.abs(m.V1).max()) < 4.0                              # the solver tests' 1e-6 bar counts on it
    t = m.table
    for c in m.comps:                                                   # the `unmoved` shortcut: whole components, and rows next to moved ones
        rows = m.rows_of(c)
        X, Y = m.V1[rows].astype(np.float64), c["v"]
        if c["map"] in ("rest", "translation"):
            assert np.array_equal(X - X[0], Y - Y[0])
        if c["map"] == "one_moved":
            assert np.array_equal(np.nonzero((X != Y).any(axis=1))[0], [1]) and t["valence"][rows[0]] == 6
            unmoved = [k for k in range(len(rows)) if k != 1 and m.ref.W[rows[k], rows[1]] == 0]
            assert unmoved == [3, 4, 5, 6] and all(m.ref.W[rows[k], rows[0]] > 0 for k in unmoved)     # next to the apex, a moved row


def test_every_class_and_every_ring_size_is_populated_and_the_band_is_empty():
    m, t, _ = routed()
    cls, r = t["cls"], t["r"]
    counts = {c: int((cls == c).sum()) for c in (pc.IDENTITY, pc.WELL, pc.WINDOW, pc.GAP0)}
    print("Vm %d, rows per class %s" % (m.Vm, counts))
    assert sum(counts.values()) == m.Vm and min(counts.values()) > 0
    assert not ((r > pc.IDENTITY_BELOW) & (r < pc.WINDOW_FROM)).any()
    moved_off_zero = (cls == pc.IDENTITY) & (t["s"][:, 0] > 0)
    print("identity rows with S != 0: r up to %.3g; window rows: r from %.3g" % (r[moved_off_zero].max(), r[cls == pc.WINDOW].min()))
    assert r[moved_off_zero].max() > 1e-13 and r[cls == pc.WINDOW].min() < 1e-11     # both sides of the 1e-12 cut are approached
    assert (t["d"][cls != pc.IDENTITY] < 0).any() and ((t["s"][:, 1] - t["s"][:, 2] <= 4 * pc.EPS * t["s"][:, 0]) & (t["r"] > 0.1)).sum() >= 4   # s1 = s2
    assert ((t["s"][:, 0] > 0) & (t["s"][:, 1] == 0)).any() and (m.comp == -1).sum() == 0
    apex = {}
    for c in m.comps:
        if c["kind"].startswith("fan"):
            i, n = c["base"], int(c["kind"][3:])
            assert t["valence"][i] == n
            apex.setdefault(n, []).append((cls[i], t["d"][i], bool(t["ok"][i])))
    for n in pc.RING_SIZES:
        seen = apex[n]
        assert any(k == pc.WELL and ok for k, d, ok in seen) and any(k == pc.WINDOW for k, d, ok in seen), n
        assert any(d < 0 and k == pc.WELL and ok for k, d, ok in seen), n      # the reflected apex row is compared element by element too
    for which, Vm in (("p256", 256), ("p257", 257)):
        p = pc.mesh(which)
        last = p.rows_of(p.comps[-1])
        assert p.Vm == Vm and last[-1] == Vm - 1 and set(p.table["cls"][last]) == {pc.WINDOW} and (p.comp == -1).sum() == Vm - 214
        assert not ((p.table["r"] > pc.IDENTITY_BELOW) & (p.table["r"] < pc.WINDOW_FROM)).any()
    w, win = pc.mesh("well"), pc.mesh("window")
    assert w.Vm + win.Vm == m.Vm and set(w.table["cls"]) == {pc.WELL, pc.IDENTITY} and w.table["ok"].all()
    assert all(win.component_classes(c) & {pc.WINDOW, pc.GAP0} for c in win.comps)


def test_the_eigen_route_in_float64_stays_within_every_bar():
    m, t, Q = routed()
    cls, S, s0 = t["cls"], t["S"], t["s"][:, 0]
    orth = np.abs(np.einsum("nba,nbc->nac", Q, Q) - np.eye(3)).reshape(m.Vm, -1).max(axis=1)
    det = np.abs(np.linalg.det(Q) - 1.0)
    print("worst |Q^T Q - I| = %.3g, worst |det Q - 1| = %.3g" % (orth.max(), det.max()))
    assert orth.max() <= 1e-13 and det.max() <= 1e-13
    lost = pc.deficit(S, t["R"], Q)
    for k in (pc.WELL, pc.WINDOW, pc.GAP0):
        rows = cls == k
        ratio = lost[rows] / t["bar"][rows]
        i = np.nonzero(rows)[0][np.argmax(ratio)]
        print("%-8s %3d rows: worst deficit / s0 = %.3g (bar %.3g; at r = %.3g, gap = %.3g); least = %.3g" % (
            k, rows.sum(), (lost[rows] / s0[rows]).max(), t["bar"][i] / s0[i], t["r"][i], t["gap"][i], (lost[rows] / s0[rows]).min()))
        assert (lost[rows] <= t["bar"][rows]).all(), k
        assert (lost[rows] >= -64 * pc.EPS * s0[rows]).all(), k        # nothing beats the optimum by more than rounding
    ident = cls == pc.IDENTITY
    assert np.array_equal(Q[ident], np.tile(np.eye(3), (ident.sum(), 1, 1)))
    well = cls == pc.WELL
    dQ = np.abs(Q - t["R"]).reshape(m.Vm, -1).max(axis=1)
    print("worst |Q - R_svd| on well rows = %.3g (gap there %.3g); on window and gap0 rows = %.3g" % (
        dQ[well].max(), t["gap"][np.nonzero(well)[0][np.argmax(dQ[well])]], dQ[~well & ~ident].max()))
    assert dQ[well].max() <= 1e-10
    assert dQ[~well & ~ident].max() > 1e-3                               # the table does enter the regime where only the energy is guaranteed


def test_the_restatement_knows_a_rotation_a_reflection_and_a_wrong_answer():
    """eigen_route on matrices with a known answer, and the bars against the faults they are there for: a transposed rotation, a lost
    flip and a mis-sorted pair of columns each miss the well bar by orders of magnitude"""
    Rz = pc.rot([0.3, -1, 0.5], 1.1)
    st = np.diag([2.0, 0.7, 0.3])
    W = pc.rot([1, 1, 0.2], 0.4)
    F = Rz @ W @ st @ W.T
    assert np.abs(pc.eigen_route(F) - Rz).max() <= 1e-14
    Fm = Rz @ W @ np.diag([2.0, 0.7, -0.3]) @ W.T                       # det < 0: the weakest direction flips
    Q = pc.eigen_route(Fm)
    assert abs(np.linalg.det(Q) - 1.0) <= 1e-14 and np.abs(Q - Rz).max() <= 1e-14
    assert np.array_equal(pc.eigen_route(np.outer([1.0, 2, 3], [0.5, -1, 2])), np.eye(3)) and np.array_equal(pc.eigen_route(np.zeros((3, 3))), np.eye(3))
    m, t, Qs = routed()
    well = np.nonzero((t["cls"] == pc.WELL) & (np.abs(t["R"] - np.swapaxes(t["R"], 1, 2)).reshape(m.Vm, -1).max(axis=1) > 0.1))[0]
    S, R = t["S"][well], t["R"][well]
    flip = R @ np.diag([1.0, -1.0, -1.0])                               # proper, orthogonal, and not the optimum
    assert len(well) > 100
    for wrong in (np.swapaxes(R, 1, 2), flip):
        assert (pc.deficit(S, R, wrong) > 1e6 * t["bar"][well]).all()
