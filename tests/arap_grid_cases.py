"""Cases at the workgroup edges of the whole-chip ARAP global step (test_gpu_arap_grid.py), beside those of arap_cases.py: a mesh of
exactly one 256-row workgroup, and the same with a 257th row that is pinned, so that the second workgroup adds only zeros to every sum.
The float64 reference (arap_ref.Reference) runs once per case and is shared."""
import functools

import numpy as np

import arap_cases as ac
import arap_ref

NAMES = ("one_block", "one_block_plus_pinned")
EXTRA_REST, EXTRA_START = [0.5, 3.0, -0.25], [1.25, -3.5, 0.75]


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(V0 float32 [Vm,3], faces, handles, targets, init float32 [Vm,3]: the start of the solve before the handles are placed)"""
    V0, faces, handles, targets = ac._torus(16, 16)                    # 256 vertices; one ring held, the opposite ring rotated and lifted
    init = V0.copy()
    if name == "one_block_plus_pinned":                                # a vertex that no face names: no equation, it keeps its start
        V0 = np.concatenate([V0, [EXTRA_REST]], 0).astype(np.float32)
        init = np.concatenate([init, [EXTRA_START]], 0).astype(np.float32)
    elif name != "one_block":
        raise KeyError(name)
    return dict(name=name, V0=V0, faces=np.asarray(faces, np.int32), handles=np.asarray(handles, np.int64), targets=targets, init=init)


@functools.lru_cache(maxsize=None)
def reference_run(name):
    """(positions after each of arap_cases.OUTER outer iterations with exact global steps, stats); do not modify"""
    c = case(name)
    return arap_ref.Reference(c["V0"], c["faces"], c["handles"]).solve(ac.start(c, c["init"]), ac.OUTER)
