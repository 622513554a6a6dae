"""Host side of the whole-chip ARAP global step (gm_arap_solve_grid, ArapSolver.solve(global_step="grid")): the declaration, typing
and export of its two entry points, its refusals before any GPU work (gm_arap_solve's table), its workspace size, the refusal of an
unknown global_step, and the command line's --arap_global_step."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from gaussianmesh_amd import _lib, scenes
from gaussianmesh_amd.arap import ArapSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name, ret, n", [("gm_arap_solve_grid", "int", 15), ("gm_arap_grid_workspace_bytes", "size_t", 1)])
def test_header_declares_and_lib_types_the_entry_points(name, ret, n):
    text = open(os.path.join(ROOT, "include", "gmesh_hip.h")).read()
    m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, name), text)
    assert m and len(m.group(1).split(",")) == n
    assert name in _lib.header_symbols()
    assert len(_lib.SIGNATURES[name][1]) == n
    assert hasattr(_lib.lib(), name)
    assert "#define GM_ABI_VERSION 3" in text and _lib.lib().gm_abi_version() == 3


def test_both_entry_points_are_typed_alike():
    assert _lib.SIGNATURES["gm_arap_solve_grid"] == _lib.SIGNATURES["gm_arap_solve"]
    assert _lib.SIGNATURES["gm_arap_grid_workspace_bytes"] == _lib.SIGNATURES["gm_arap_workspace_bytes"]


def test_arap_solve_grid_refuses_before_any_gpu_work():
    """the table of test_arap_host.test_arap_solve_refuses_before_any_gpu_work, for gm_arap_solve_grid: the pointers are never
    dereferenced (there is no device in this test)"""
    l = _lib.lib()
    Vm = 100
    need = l.gm_arap_grid_workspace_bytes(Vm)
    assert need > 0
    a = 1 << 30                                                        # non-null "pointers", 1 MiB apart
    P = {k: a + (i << 20) for i, k in enumerate(("off", "cols", "w", "V0", "fixed", "init", "out", "stats", "ws"))}

    def call(Vm=Vm, outer=2, cg=8, tol=1e-6, nbytes=need, **kw):
        p = dict(P, **kw)
        return l.gm_arap_solve_grid(Vm, p["off"], p["cols"], p["w"], p["V0"], p["fixed"], p["init"], outer, cg, tol, p["out"], p["stats"], p["ws"],
                                    nbytes, None)
    for kw in (dict(Vm=0), dict(Vm=-3)):
        assert call(**kw) == 1 and b"Vm" in l.gm_last_error(), kw
    assert b"gm_arap_solve_grid" in l.gm_last_error()
    assert call(outer=-1) == 1 and b"outer_iterations" in l.gm_last_error()
    for cg in (0, -5):
        assert call(cg=cg) == 1 and b"cg_iterations" in l.gm_last_error()
    for tol in (-1e-3, float("nan"), float("inf"), -float("inf")):
        assert call(tol=tol) == 1 and b"cg_tolerance" in l.gm_last_error(), tol
    for k in ("off", "cols", "w", "V0", "fixed", "init", "out", "ws"):
        assert call(**{k: None}) == 1 and b"null" in l.gm_last_error(), k
    names = ("V0", "init", "out", "stats", "ws")
    for i, x in enumerate(names):
        for y in names[i + 1:]:
            assert call(**{y: P[x] + 4}) == 1 and b"overlaps" in l.gm_last_error(), (x, y)
    assert call(out=P["V0"]) == 1 and call(init=P["V0"]) == 1 and call(stats=P["ws"]) == 1
    assert call(out=P["init"], nbytes=need - 1) == 3 and b"workspace" in l.gm_last_error()       # V_out == V_init reaches the workspace check
    assert call(nbytes=need - 1) == 3 and b"workspace" in l.gm_last_error()
    assert call(nbytes=0) == 3
    assert call(nbytes=l.gm_arap_workspace_bytes(Vm)) == 3             # the column step's workspace is not enough for this one


def test_grid_workspace_bytes_are_monotonic():
    l = _lib.lib()
    sizes = [1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 7500, 60000, 100000, 1000000, 10000000]
    got = [l.gm_arap_grid_workspace_bytes(n) for n in sizes]
    assert got == sorted(got) and len(set(got)) > 10
    assert l.gm_arap_grid_workspace_bytes(0) == l.gm_arap_grid_workspace_bytes(1) > 0
    # x r u w p s (18 doubles), the rotations (9), the row sums (1), the free-row mask (an int), and 12 sums per workgroup of 256 rows
    assert got[sizes.index(7500)] >= 7500 * (28 * 8 + 4) + 12 * 8 * 30
    assert got[-1] <= 10000000 * 240                                   # O(Vm)


def test_an_unknown_global_step_is_a_value_error_before_anything_else():
    verts, faces = scenes.torus_mesh(8, 6)
    s = ArapSolver(verts, faces, [3], device="cpu")
    for bad in ("bogus", "", None, "Grid"):
        with pytest.raises(ValueError, match="global_step"):
            s.solve(np.zeros((7, 2), np.float32), global_step=bad)      # (the misshapen handle_positions is never looked at)
    with pytest.raises(_lib.GmeshError, match="no CPU path"):          # a known one goes on to the device check
        s.solve(np.zeros((1, 3), np.float32), global_step="grid")


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "gaussianmesh_amd.edit_sequence", "--object_gaussian", "o.ply", "--object_origin_mesh", "m.obj",
                           "--camera_path", ".", "--render_path", "out", "--handle_sequence", "h.npz"] + list(args), cwd=ROOT, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)


def test_cli_rejects_an_unknown_global_step():
    r = _cli("--arap_global_step", "bogus")
    assert r.returncode == 2 and "--arap_global_step" in r.stdout and "column" in r.stdout and "grid" in r.stdout, r.stdout[-2000:]
