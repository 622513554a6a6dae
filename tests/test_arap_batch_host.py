"""Host side of the batched ARAP solves (gm_arap_solve_batch, ArapSolver.solve_batch / solve_sequence, edit_sequence --arap_batch): the
run boundaries, the order of the Python refusals, the declaration and typing of the two entry points, the C refusals that need no
device (made on pointers that are never dereferenced), and the command line's refusal before any device work."""
import os
import re

import numpy as np
import pytest

import arap_cases as ac
from gaussianmesh_amd import _lib, arap, edit_sequence
from gaussianmesh_amd.arap import ArapSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("T, batch, want", [(0, 4, []), (1, 4, [(0, 1)]), (4, 4, [(0, 4)]), (5, 4, [(0, 4), (4, 5)]),
                                            (9, 4, [(0, 4), (4, 8), (8, 9)]), (3, 1, [(0, 1), (1, 2), (2, 3)])])
def test_sequence_runs(T, batch, want):
    assert arap.sequence_runs(T, batch) == want


def test_sequence_runs_refuses_nonsense():
    for T, batch in ((-1, 4), (3, 0), (3, -2)):
        with pytest.raises(ValueError, match="sequence_runs"):
            arap.sequence_runs(T, batch)


def test_a_solver_without_a_device_refuses_in_order():
    """a bad global_step is a ValueError before anything else (even before the missing device, and before the shapes are looked at);
    otherwise GmeshError"""
    c = ac.case("torus_a")
    s = ArapSolver(c["V0"], c["faces"], c["handles"], device="cpu")
    H = len(c["handles"])
    good, bad = np.zeros((2, H, 3), np.float32), np.zeros((2, H + 1, 2), np.float32)
    for fn in (s.solve_batch, s.solve_sequence):
        for hp in (good, bad):
            with pytest.raises(ValueError, match="global_step"):
                fn(hp, global_step="rows")
        for step in ("column", "grid"):
            with pytest.raises(_lib.GmeshError, match="no CPU path"):
                fn(good, global_step=step)
        with pytest.raises(_lib.GmeshError, match="no CPU path"):
            fn(good)


@pytest.mark.parametrize("name, ret, n", [("gm_arap_solve_batch", "int", 17), ("gm_arap_batch_workspace_bytes", "size_t", 3)])
def test_header_declares_and_lib_types_the_entry_points(name, ret, n):
    text = open(os.path.join(ROOT, "include", "gmesh_hip.h")).read()
    m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, name), text)
    assert m and len(m.group(1).split(",")) == n
    assert name in _lib.header_symbols()
    assert len(_lib.SIGNATURES[name][1]) == n
    assert hasattr(_lib.lib(), name)
    assert "#define GM_ABI_VERSION 3" in text and _lib.lib().gm_abi_version() == 3
    assert "#define GM_ARAP_BATCH_MAX 64" in text and _lib.GM_ARAP_BATCH_MAX == 64 == edit_sequence.ARAP_BATCH_MAX


def test_batch_workspace_bytes():
    """0 for arguments that would be refused; otherwise the shared row words once and a slab per item: at least 21 (column) or 27
    (grid) doubles per vertex and item, and not B times the single solve's (diag and free_row are not repeated)"""
    l = _lib.lib()
    for Vm, B, step in ((0, 1, 0), (-1, 1, 0), (100, 0, 0), (100, -1, 1), (100, 65, 0), (100, 4, 2), (100, 4, -1)):
        assert l.gm_arap_batch_workspace_bytes(Vm, B, step) == 0, (Vm, B, step)
    for step, doubles, single in ((0, 21, l.gm_arap_workspace_bytes), (1, 27, l.gm_arap_grid_workspace_bytes)):
        for Vm in (1, 96, 257, 7500):
            got = [l.gm_arap_batch_workspace_bytes(Vm, B, step) for B in (1, 2, 3, 8, 64)]
            assert got == sorted(got) and len(set(got)) == 5
            assert got[1] - got[0] == got[2] - got[1] >= 8 * doubles * Vm          # one slab per item
            assert got[4] == got[0] + 63 * (got[1] - got[0])
            if Vm == 7500:
                assert got[3] < 8 * single(Vm)


def test_arap_solve_batch_refuses_before_any_gpu_work():
    l = _lib.lib()
    Vm, B, outer = 100, 4, 2
    a = 1 << 30                                                        # non-null "pointers", 1 MiB apart: never dereferenced
    P = {k: a + (i << 20) for i, k in enumerate(("off", "cols", "w", "V0", "fixed", "init", "out", "stats", "ws"))}

    def call(B=B, step=0, Vm=Vm, outer=outer, cg=8, tol=1e-6, nbytes=None, **kw):
        p = dict(P, **kw)
        if nbytes is None:
            nbytes = l.gm_arap_batch_workspace_bytes(Vm, B, step)
        return l.gm_arap_solve_batch(B, step, Vm, p["off"], p["cols"], p["w"], p["V0"], p["fixed"], p["init"], outer, cg, tol, p["out"], p["stats"],
                                     p["ws"], nbytes, None)

    def refused(what, rc=1, **kw):
        assert call(**kw) == rc and b"gm_arap_solve_batch" in l.gm_last_error() and what in l.gm_last_error(), (kw, l.gm_last_error())
    for b in (0, -1, 65):
        refused(b"B =", B=b, nbytes=1 << 20)
    for step in (2, -1):
        refused(b"global_step", step=step, nbytes=1 << 20)
    for step in (0, 1):
        need = l.gm_arap_batch_workspace_bytes(Vm, B, step)
        refused(b"Vm", Vm=0, step=step, nbytes=need)
        refused(b"outer_iterations", outer=-1, step=step)
        refused(b"cg_iterations", cg=0, step=step)
        for tol in (-1e-3, float("nan"), float("inf")):
            refused(b"cg_tolerance", tol=tol, step=step)
        for k in ("off", "cols", "w", "V0", "fixed", "init", "out", "ws"):
            refused(b"null", step=step, **{k: None})
        names = ("V0", "init", "out", "stats", "ws")
        for i, x in enumerate(names):
            for y in names[i + 1:]:
                refused(b"overlaps", step=step, **{y: P[x] + 4})
        # the [B] extents: an array that begins inside item B - 1 of V_init / V_out, or in the last item's stats rows, overlaps; one
        # that begins where they end does not (it reaches the workspace check)
        last_item = 12 * Vm * (B - 1) + 4
        refused(b"overlaps", step=step, V0=P["init"] + last_item)
        refused(b"overlaps", step=step, stats=P["out"] + last_item)
        refused(b"overlaps", step=step, ws=P["stats"] + 64 * outer * (B - 1) + 8)
        refused(b"workspace", rc=3, step=step, stats=P["out"] + 12 * Vm * B, nbytes=need - 1)
        refused(b"workspace", rc=3, step=step, out=P["init"], nbytes=need - 1)        # V_out == V_init alone is allowed
        refused(b"workspace", rc=3, step=step, nbytes=0)


@pytest.mark.parametrize("k", ["0", "65", "-3"])
def test_cli_refuses_an_arap_batch_out_of_range_before_any_device_work(k, monkeypatch):
    """SystemExit with a message, raised ahead of every import that would touch the device or read a file (none of the named files
    exists)"""
    import builtins
    real = builtins.__import__

    def no_torch(name, *a, **kw):
        assert name != "torch" and not name.endswith("edittool"), name
        return real(name, *a, **kw)
    monkeypatch.setattr(builtins, "__import__", no_torch)
    with pytest.raises(SystemExit) as e:
        edit_sequence.main(["--object_gaussian", "o.ply", "--object_origin_mesh", "m.obj", "--camera_path", ".", "--render_path", "out",
                            "--handle_sequence", "h.npz", "--arap_batch", k])
    assert "--arap_batch" in str(e.value) and "1 .. 64" in str(e.value)
