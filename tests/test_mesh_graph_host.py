"""Host side of mesh_graph.MeshGraph: its arrays against edge_csr / components, the shared vertex-id check with every refusal, one CSR
per mesh however many operators are built over it, and SingleObjectDeform sharing one graph across handle selections.  No device."""
import numpy as np
import pytest
import torch

import arap_cases as ac
from gaussianmesh_amd import mesh_graph, scenes
from gaussianmesh_amd.arap import ArapEnergy, ArapSolver, components, edge_csr
from gaussianmesh_amd.dynamics import MeshDynamics
from gaussianmesh_amd.mesh_graph import MeshGraph
from gaussianmesh_amd.pose_interp import PoseInterpolator


def _torus86():
    verts, faces = scenes.torus_mesh(8, 6)
    return verts.astype(np.float32), np.asarray(faces, np.int32)


@pytest.fixture
def csr_calls(monkeypatch):
    """the number of edge_csr calls MeshGraph makes, as a one-element list"""
    calls, real = [0], mesh_graph.edge_csr

    def counting(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(mesh_graph, "edge_csr", counting)
    return calls


@pytest.mark.parametrize("mesh, edgeless", [(ac.pinned_mesh, [96, 97]), (_torus86, [])])
def test_the_graphs_arrays(mesh, edgeless):
    V0, faces = mesh()
    g = MeshGraph(V0, faces, device="cpu")
    off, cols, weights = edge_csr(V0, faces)
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(g.csr, (off, cols, weights)))
    rows = np.repeat(np.arange(len(V0)), np.diff(off.astype(np.int64)))
    assert g.Vm == len(V0) and g.F == len(faces) and np.array_equal(g.rows, rows) and g.rows.dtype == np.int64
    assert np.array_equal(g.rest_host, V0) and g.rest_host.dtype == np.float32
    assert np.array_equal(g.faces_host, faces) and g.faces_host.dtype == np.int64
    assert g.edgeless.dtype == bool and np.nonzero(g.edgeless)[0].tolist() == edgeless
    assert np.array_equal(g.label, components(len(V0), rows, cols.astype(np.int64))) and g.label is g.label
    for bad in (V0[:, :2], V0[:0], V0.reshape(-1)):
        with pytest.raises(ValueError, match="^Caller: rest_vertices"):
            MeshGraph(bad, faces, device="cpu", who="Caller")
    with pytest.raises(ValueError, match="face index outside"):
        MeshGraph(V0, faces + len(V0), device="cpu")
    empty = MeshGraph(V0[:4], np.zeros((0, 3), np.int32), device="cpu")   # a mesh without an edge: every vertex edgeless, its own component
    assert empty.F == 0 and empty.edgeless.all() and empty.label.tolist() == [0, 1, 2, 3] and len(empty.csr[1]) == 0


def test_vertex_ids():
    g = MeshGraph(*_torus86(), device="cpu")
    assert g.Vm == 48
    for ids in ([3, 47, 0], np.array([3, 47, 0], np.int32), np.array([3, 47, 0], np.int64), torch.tensor([3, 47, 0]), torch.tensor([3, 47, 0], dtype=torch.int32),
                np.array([3, 47, 0], np.uint8)):
        got = g.vertex_ids(ids, "Caller", "handle")
        assert got.dtype == np.int64 and got.tolist() == [3, 47, 0]                    # the order given
    for bad, word in (([0.5], "integer"), (np.array([1.0]), "integer"), ([True], "integer"), ([48], "outside"), ([-1], "outside"), ([0, 5, 0], "twice"),
                      ([], "empty"), (np.zeros(0, np.int64), "empty")):
        with pytest.raises(ValueError, match="^Caller: .*%s" % word) as e:
            g.vertex_ids(bad, "Caller", "handle")
        assert "handle" in str(e.value)
    for none in ([], (), np.zeros(0, np.int64), torch.zeros(0)):
        got = g.vertex_ids(none, "Caller", "pinned", allow_empty=True)
        assert got.dtype == np.int64 and got.shape == (0,)
    assert g.vertex_ids([0, 5, 0], "Caller", "pinned", distinct=False).tolist() == [0, 5, 0]
    assert mesh_graph.vertex_ids([2], 3, "Caller", "handle").tolist() == [2]
    with pytest.raises(ValueError, match="^Caller: source set 1 id outside"):
        mesh_graph.vertex_ids([3], 3, "Caller", "source set 1", allow_empty=True, distinct=False)
    held = np.zeros(48, bool)
    g.require_anchored(held, np.array([7]), "Caller", "handle")                           # one component, one handle in it
    two = MeshGraph(np.concatenate([g.rest_host, g.rest_host + 10.0]), np.concatenate([g.faces_host, g.faces_host + 48]), device="cpu")
    for what, words in (("handle", "without a handle"), ("anchor", "without an anchor")):
        with pytest.raises(ValueError, match="^Caller: vertex 48 .*%s .*48 such vertices.*singular" % words):
            two.require_anchored(np.zeros(96, bool), np.array([7]), "Caller", what)


def test_one_csr_per_mesh(csr_calls):
    V0, faces = ac.pinned_mesh()
    handles = ac.case("torus_a")["handles"]
    g = MeshGraph(V0, faces, device="cpu")
    assert MeshGraph.of(g, None, "cpu") is g and MeshGraph.of(g, None, "cuda") is g
    with pytest.raises(ValueError, match="^Caller: .*faces"):
        MeshGraph.of(g, faces, "cpu", "Caller")
    shared = [ArapSolver(g, None, handles), ArapEnergy(g, None), PoseInterpolator(g, None), PoseInterpolator(g, None, anchors=[5]),
              MeshDynamics(g, None, pinned=[3], handles=[7, 9])]
    assert csr_calls[0] == 1
    assert all(op.csr is g.csr and op.mesh is g and op.device.type == "cpu" and op.Vm == 98 for op in shared)
    own = [ArapSolver(V0, faces, handles, device="cpu"), ArapEnergy(V0, faces, device="cpu"), PoseInterpolator(V0, faces, device="cpu"),
           PoseInterpolator(V0, faces, anchors=[5], device="cpu"), MeshDynamics(V0, faces, pinned=[3], handles=[7, 9], device="cpu")]
    assert csr_calls[0] == 6
    for a, b in zip(shared, own):
        assert all(np.array_equal(x, y) for x, y in zip(a.csr, b.csr))
        for name in ("held", "pinned", "handles", "label", "anchors", "mass"):
            if hasattr(b, name):
                assert np.array_equal(getattr(a, name), getattr(b, name)), (type(a).__name__, name)
    assert shared[0].pinned.tolist() == [96, 97] and shared[0].handles.tolist() == handles.tolist()
    assert sorted(np.nonzero(shared[2].held)[0].tolist()) == [0, 96, 97] and sorted(np.nonzero(shared[3].held)[0].tolist()) == [5, 96, 97]
    assert sorted(np.nonzero(shared[4].held)[0].tolist()) == [3, 7, 9, 96, 97] and shared[4].pinned.tolist() == [3]
    assert shared[1].scale == own[1].scale and shared[3].F == len(faces)


def test_single_object_deform_builds_the_graph_once_per_face_tensor(csr_calls):
    from gaussianmesh_amd.deform import SingleObjectDeform
    V0, faces = _torus86()
    o = SingleObjectDeform(torch.zeros(1, 3), torch.eye(3)[None], torch.ones(1, 1), torch.zeros(1, 16, 3), torch.tensor([[0, 1, 2]]),
                           torch.full((1, 3), 1.0 / 3.0), torch.as_tensor(V0))
    with pytest.raises(ValueError, match="^set_handles: .*no faces"):
        o.set_handles([0, 1])
    with pytest.raises(ValueError, match="no faces"):
        o.mesh_graph
    assert csr_calls[0] == 0
    first = o.set_handles([0, 1], faces=faces)
    g = o.mesh_graph
    second = o.set_handles([5, 9, 30])
    assert csr_calls[0] == 1 and o.mesh_graph is g and first.mesh is g and second.mesh is g and second is not first
    assert first.handles.tolist() == [0, 1] and second.handles.tolist() == [5, 9, 30] and second.csr is g.csr
    o._set_faces(faces)                                                # a new face tensor, whatever it holds
    third = o.set_handles([5, 9, 30])
    assert csr_calls[0] == 2 and o.mesh_graph is not g and third.mesh is o.mesh_graph
    assert all(np.array_equal(a, b) for a, b in zip(third.csr, g.csr))
