"""-m gpu: mesh_graph.MeshGraph on the device - one upload of the edge CSR shared by every operator that SingleObjectDeform builds, with
the results of operators built from the plain arrays, and ArapSolver on a mesh without an edge."""
import numpy as np
import pytest
import torch

import pose_interp_cases as pc
from test_gpu_arap import _dev, _drags, _scene64, _tool

pytestmark = pytest.mark.gpu


def test_the_editors_operators_share_one_graph(tmp_path):
    """set_handles, interpolate_to, simulate and fit_pose(regularizer="arap") on the 12 x 8 torus object: all four operators hold the
    tensors of o.mesh_graph, and the meshes are those of operators built from the arrays, each with a graph of its own"""
    from gaussianmesh_amd.arap import ArapEnergy, ArapSolver
    from gaussianmesh_amd.dynamics import MeshDynamics
    from gaussianmesh_amd.pose_interp import PoseInterpolator
    d = str(tmp_path)
    _scene64(d)
    tool = _tool(d)
    o = tool.gaussians_list[0]
    ids, pos = _drags(o.vertex.cpu().numpy(), T=4)
    pos = _dev(pos)
    target = _dev(pc.turned(o.vertex.cpu().numpy().astype(np.float64), 0.5))          # a rigid image of the rest pose: the fit starts from a proper one
    held = target[_dev(ids, torch.int64)].expand(2, len(ids), 3)                          # the simulation holds the handles where the target has them
    cam = tool.get_camera(d)[1]
    view = (cam, tool.render_gaussian(cam).clone())

    solver = o.set_handles(ids)
    dragged = o.drag_sequence(pos, batch=2)
    between = o.interpolate_to(target, 2)
    simulated = o.simulate(2, held)
    fitter = o.fit_pose([view], 1, regularizer="arap")
    assert bool(torch.isfinite(fitter.losses[0]))

    g = o.mesh_graph
    ops = (solver, o._operators["pose_interp"], o._operators["dynamics"], fitter.arap)
    assert o.arap is solver and isinstance(fitter.arap, ArapEnergy)
    for op in ops:
        assert op.mesh is g and op.csr is g.csr
        for mine, shared in ((op.rest, g.rest), (op._off, g.off), (op._cols, g.cols), (op._w, g.w)):
            assert mine is shared and mine.data_ptr() == shared.data_ptr()
    assert ops[1]._faces is g.faces and ops[1]._vf_off is g.vf_off and ops[1]._vf_faces is g.vf_faces

    plain = ArapSolver(o.vertex, o.faces, ids)
    assert plain.mesh is not g and plain._off.data_ptr() != g.off.data_ptr()
    assert torch.equal(dragged, plain.solve_sequence(pos, batch=2))
    assert torch.equal(between, PoseInterpolator(o.vertex, o.faces).sequence([dragged[-1], target], 2))
    m = MeshDynamics(o.vertex, o.faces, handles=ids)
    m.reset(positions=target)
    assert torch.equal(simulated, m.run(2, held))
    # nothing wrote the shared tensors
    assert torch.equal(g.rest, o.vertex) and np.array_equal(g.off.cpu().numpy(), g.csr[0]) and np.array_equal(g.cols.cpu().numpy(), g.csr[1])
    assert np.array_equal(g.w.cpu().numpy(), g.csr[2])


@pytest.mark.parametrize("global_step", ["column", "grid"])
def test_arap_solver_on_a_mesh_without_an_edge(global_step):
    """Vm = 4, F = 0: every vertex is pinned, so a solve is `init` with the handle rows replaced, bit for bit"""
    from gaussianmesh_amd.arap import ArapSolver
    V0 = np.array([[0.0, 0.0, 0.0], [1.0, 0.5, -0.25], [-2.0, 3.0, 1.5], [0.75, -1.0, 2.0]], np.float32)
    s = ArapSolver(V0, np.zeros((0, 3), np.int32), [1])
    assert s.pinned.tolist() == [0, 1, 2, 3] and len(s.csr[1]) == 0
    init = _dev(np.arange(12, dtype=np.float32).reshape(4, 3) * 0.37 - 1.0)
    hp = _dev([[[3.5, -0.125, 0.3]], [[-1.0, 2.0, 0.6]]])
    for start in (None, init):
        for b in range(2):
            want = (_dev(V0) if start is None else start).clone()
            want[1] = hp[b, 0]
            got, stats = s.solve(hp[b], init=start, global_step=global_step, want_stats=True)
            assert torch.equal(got, want) and stats.shape == (4, 8) and bool(torch.isfinite(stats).all())
        want = (_dev(V0) if start is None else start).expand(2, 4, 3).clone()
        want[:, 1] = hp[:, 0]
        got, stats = s.solve_batch(hp, init=start, global_step=global_step, want_stats=True)
        assert torch.equal(got, want) and stats.shape == (2, 4, 8) and bool(torch.isfinite(stats).all())
    assert torch.equal(init, _dev(np.arange(12, dtype=np.float32).reshape(4, 3) * 0.37 - 1.0))
