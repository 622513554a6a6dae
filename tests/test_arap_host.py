"""Host side of the ARAP solver: the float64 reference of tests/arap_ref.py against itself (exact global steps against PCG, the
energy's monotony, fixed points), arap.edge_csr against the reference's weights, the ArapSolver constructor's refusals, gm_arap_solve's
declaration, typing and refusals (before any GPU work), and the command line's argument handling."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from gaussianmesh_amd import _lib, scenes
from gaussianmesh_amd.arap import ArapSolver, edge_csr

import arap_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference against itself ----
@pytest.mark.parametrize("name", ac.NAMES)
def test_reference_direct_and_pcg_agree(name):
    """exact global steps against PCG at tolerance 1e-10 (at most 400 steps): within 1e-8 after 10 outer iterations (a float64 prototype
    measured at most 4.3e-10), and every PCG solve converged"""
    direct, _ = ac.reference_run(name)
    pcg, stats = ac.reference(name).solve(ac.start(ac.case(name)), ac.OUTER, pcg=(400, 1e-10))
    worst = float(np.abs(direct - pcg).max())
    print("%s: direct vs PCG %.3g, PCG steps at most %d" % (name, worst, int(stats[:, 2:5].max())))
    assert worst <= 1e-8
    assert stats[:, 2:5].max() <= 400 and stats[:, 5:8].max() <= 1e-10
    assert np.abs(direct).max() < 4.0


@pytest.mark.parametrize("name", ac.NAMES)
def test_reference_energy_never_rises(name):
    """the chain E(local 0), E(global 0), E(local 1), ... with exact global steps, and with only 3 CG steps per solve"""
    _, stats = ac.reference_run(name)
    _, stats3 = ac.reference(name).solve(ac.start(ac.case(name)), ac.OUTER, pcg=(3, 0.0))
    for st in (stats, stats3):
        chain = st[:, :2].reshape(-1)
        assert (np.diff(chain) <= 1e-9 * chain[0]).all(), chain
    assert stats3[-1, 1] < stats3[0, 0]


def test_reference_fixed_points():
    c, ref = ac.case("torus_a"), ac.reference("torus_a")
    V0 = c["V0"].astype(np.float64)
    X, stats = ref.solve(c["V0"], 3)                                   # handles at rest
    assert np.abs(X[-1] - V0).max() <= 1e-12 and stats[:, :2].max() <= 1e-20
    Q, t = ac.rotation((1, 2, -0.5), 0.9), np.array([0.3, -2.0, 5.0])
    rigid = (V0 @ Q.T + t).astype(np.float32)                          # handles at their rigid images, init the rigid image
    X, _ = ref.solve(rigid, 3)
    assert np.abs(X[-1] - rigid).max() <= 1e-6                         # (rigid is rounded to float32: 5 * 2^-24 = 3e-7 off a true rigid image)
    one = ac.reference("one_handle")
    moved = (ac.case("one_handle")["V0"].astype(np.float64) + t).astype(np.float32)
    X, _ = one.solve(moved, 2)
    assert np.abs(X[-1] - moved).max() <= 1e-6


# ---- edge_csr ----
@pytest.mark.parametrize("name", ("torus_a", "flat_patch", "fan", "pinned"))
def test_edge_csr_against_the_reference_weights(name):
    V0, faces = ac.pinned_mesh() if name == "pinned" else (ac.case(name)["V0"], ac.case(name)["faces"])
    off, cols, w = edge_csr(V0, faces)
    Vm = len(V0)
    assert off.dtype == np.int32 and cols.dtype == np.int32 and w.dtype == np.float64
    assert off.shape == (Vm + 1,) and off[0] == 0 and off[-1] == len(cols) == len(w) and (np.diff(off) >= 0).all()
    rows = np.repeat(np.arange(Vm), np.diff(off))
    assert (rows != cols).all() and (w > 0).all()                       # no diagonal, positive
    for i in range(Vm):
        assert (np.diff(cols[off[i]:off[i + 1]]) > 0).all(), i          # ascending, no duplicates
    dense = np.zeros((Vm, Vm))
    dense[rows, cols] = w
    assert np.array_equal(dense, dense.T)                               # symmetric, bit for bit
    import arap_ref
    W = arap_ref.weight_matrix(V0, faces)
    assert np.array_equal(dense != 0, W != 0)
    assert np.abs(dense - W).max() <= 1e-12 * np.abs(W).max() and (np.abs(dense - W) <= 1e-12 * np.abs(W)).all()


# ---- ArapSolver's constructor (host work: no device needed) ----
def test_solver_refusals():
    verts, faces = scenes.torus_mesh(8, 6)
    with pytest.raises(ValueError, match="twice"):
        ArapSolver(verts, faces, [3, 7, 3], device="cpu")
    with pytest.raises(ValueError, match="outside"):
        ArapSolver(verts, faces, [3, len(verts)], device="cpu")
    with pytest.raises(ValueError, match="outside"):
        ArapSolver(verts, faces, [-1], device="cpu")
    with pytest.raises(ValueError, match="empty"):
        ArapSolver(verts, faces, [], device="cpu")
    with pytest.raises(ValueError, match="integer"):
        ArapSolver(verts, faces, [1.5], device="cpu")
    two = np.concatenate([verts, verts + np.array([0.0, 5.0, 0.0])], 0)        # a second torus, not connected to the first
    faces2 = np.concatenate([faces, faces + len(verts)], 0)
    with pytest.raises(ValueError, match="without a handle"):
        ArapSolver(two, faces2, [3], device="cpu")
    assert ArapSolver(two, faces2, [3, len(verts) + 3], device="cpu").Vm == 2 * len(verts)
    with pytest.raises(_lib.GmeshError, match="no CPU path"):
        ArapSolver(verts, faces, [3], device="cpu").solve(np.zeros((1, 3), np.float32))


def test_degenerate_face_and_unreferenced_vertex_are_pinned_not_refused():
    V0, faces = ac.pinned_mesh()
    s = ArapSolver(V0, faces, [0, 50], device="cpu")
    assert list(s.pinned) == [96, 97]
    off, cols, w = s.csr
    assert off[97] == off[96] == off[98] and 97 not in cols and 96 not in cols


# ---- the C entry points ----
@pytest.mark.parametrize("name, ret, n", [("gm_arap_solve", "int", 15), ("gm_arap_workspace_bytes", "size_t", 1)])
def test_header_declares_and_lib_types_the_entry_points(name, ret, n):
    text = open(os.path.join(ROOT, "include", "gmesh_hip.h")).read()
    m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, name), text)
    assert m and len(m.group(1).split(",")) == n
    assert name in _lib.header_symbols()
    assert len(_lib.SIGNATURES[name][1]) == n
    assert hasattr(_lib.lib(), name)
    assert "#define GM_ABI_VERSION 3" in text and _lib.lib().gm_abi_version() == 3


def test_arap_solve_refuses_before_any_gpu_work():
    l = _lib.lib()
    Vm = 100
    need = l.gm_arap_workspace_bytes(Vm)
    assert need > 0
    a = 1 << 30                                                        # non-null "pointers", 1 MiB apart: never dereferenced
    P = {k: a + (i << 20) for i, k in enumerate(("off", "cols", "w", "V0", "fixed", "init", "out", "stats", "ws"))}

    def call(Vm=Vm, outer=2, cg=8, tol=1e-6, nbytes=need, **kw):
        p = dict(P, **kw)
        return l.gm_arap_solve(Vm, p["off"], p["cols"], p["w"], p["V0"], p["fixed"], p["init"], outer, cg, tol, p["out"], p["stats"], p["ws"],
                               nbytes, None)
    for kw in (dict(Vm=0), dict(Vm=-3)):
        assert call(**kw) == 1 and b"Vm" in l.gm_last_error(), kw
    assert call(outer=-1) == 1 and b"outer_iterations" in l.gm_last_error()
    for cg in (0, -5):
        assert call(cg=cg) == 1 and b"cg_iterations" in l.gm_last_error()
    for tol in (-1e-3, float("nan"), float("inf"), -float("inf")):
        assert call(tol=tol) == 1 and b"cg_tolerance" in l.gm_last_error(), tol
    for k in ("off", "cols", "w", "V0", "fixed", "init", "out", "ws"):
        assert call(**{k: None}) == 1 and b"null" in l.gm_last_error(), k
    # partial overlaps (4 bytes in): every pair of V0 / V_init / V_out / stats / workspace; V_out == V_init alone is allowed (and then
    # reaches the workspace check)
    names = ("V0", "init", "out", "stats", "ws")
    for i, x in enumerate(names):
        for y in names[i + 1:]:
            assert call(**{y: P[x] + 4}) == 1 and b"overlaps" in l.gm_last_error(), (x, y)
    assert call(out=P["V0"]) == 1 and call(init=P["V0"]) == 1 and call(stats=P["ws"]) == 1
    assert call(out=P["init"], nbytes=need - 1) == 3 and b"workspace" in l.gm_last_error()
    assert call(nbytes=need - 1) == 3 and b"workspace" in l.gm_last_error()
    assert call(nbytes=0) == 3


def test_workspace_bytes_are_monotonic():
    l = _lib.lib()
    sizes = [1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 7500, 60000, 100000, 1000000, 10000000]
    got = [l.gm_arap_workspace_bytes(n) for n in sizes]
    assert got == sorted(got) and len(set(got)) > 10
    assert l.gm_arap_workspace_bytes(0) == l.gm_arap_workspace_bytes(1) > 0
    assert got[sizes.index(7500)] >= 7500 * (22 * 8 + 4)


def test_the_kernel_file_waits_for_nothing_and_allocates_nothing():
    """gm_arap_solve's "no host synchronisation, no device allocation", no atomics, no workgroup waiting on another: the translation
    unit names no such call"""
    text = open(os.path.join(ROOT, "gaussianmesh_amd", "csrc", "gm_arap.hip")).read()
    assert "gm_arap.hip" in open(os.path.join(ROOT, "gaussianmesh_amd", "csrc", "Makefile")).read()
    code = re.sub(r"//[^\n]*", "", text)
    hits = re.findall(r"hipMemcpy\w*|hipMemset\w*|hip\w*Synchronize|hipMalloc\w*|hipFree\w*|GM_LAUNCH_CHECK|atomic\w*|hipLaunchCooperative\w*|"
                      r"cooperative_groups|__threadfence\w*|while\s*\(", code)
    assert not hits, hits


def test_edit_surface_is_declared():
    from gaussianmesh_amd import deform, edittool
    for cls in (deform.SingleObjectDeform, edittool.SingleObjectDeform):
        assert all(hasattr(cls, k) for k in ("set_handles", "drag", "deform_vertices", "mesh_vertex_current"))
    assert hasattr(edittool.ObjectVisualTool, "drag_one_gaussian") and hasattr(edittool.SceneVisualTool, "drag_one_gaussian")


# ---- the command line ----
def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "gaussianmesh_amd.edit_sequence", "--object_gaussian", "o.ply", "--object_origin_mesh", "m.obj",
                           "--camera_path", ".", "--render_path", "out"] + list(args), cwd=ROOT, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=300)


def test_cli_wants_exactly_one_kind_of_sequence():
    r = _cli()
    assert r.returncode == 2 and "--mesh_sequence" in r.stdout and "--handle_sequence" in r.stdout, r.stdout[-2000:]
    r = _cli("--mesh_sequence", "seq", "--handle_sequence", "h.npz")
    assert r.returncode == 2 and "not allowed with" in r.stdout, r.stdout[-2000:]
