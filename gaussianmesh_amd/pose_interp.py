"""The meshes between key poses of a proxy mesh: rotation-aware interpolation on the device (gm_pose_interp, csrc/gm_pose_interp.hip).
A linear blend of two poses collapses whatever rotates between them; here every face's deformation gradient is interpolated in polar
form (the rotation along its geodesic, the stretch linearly; Alexa, Cohen-Or & Levin 2000) and the vertices are recovered from one
Poisson solve per coordinate over the cotangent Laplacian of arap.edge_csr (Xu et al. 2005): the matrix of the ARAP global step, and
its solver.  Every in-between is independent of the others, so T of them are one launch chain - one solve per frame where a handle
drag (ArapSolver) takes a dozen.  The result is a [T,Vm,3] stack of meshes: what render_sequence, SingleObjectDeform.deform_vertices
and edit_sequence --save_meshes take.  Definition, ABI and rules: INTEGRATION.md section Z.
NEAR A HALF TURN.  A face whose rotation between the two keys lies within 1e-3 rad of pi may turn either way (the two geodesics are
equally long, and neighbouring faces may disagree): add a key in between."""
import numpy as np
import torch

from . import _lib
from ._op import enqueue, host, on_device
from .mesh_graph import MeshGraph

EASES = ("linear", "smoothstep")


def segment_ts(inbetweens, ease="linear"):
    """The parameters of the `inbetweens` frames strictly between two keys: k / (inbetweens + 1), k = 1 .. inbetweens, float64; through
    3 t^2 - 2 t^3 with ease="smoothstep".  Host arithmetic only."""
    if isinstance(inbetweens, bool) or int(inbetweens) != inbetweens or inbetweens < 0:
        raise ValueError("segment_ts: inbetweens = %r; an integer >= 0" % (inbetweens,))
    if ease not in EASES:
        raise ValueError('segment_ts: ease must be "linear" or "smoothstep"; got %r' % (ease,))
    t = np.arange(1, int(inbetweens) + 1, dtype=np.float64) / (int(inbetweens) + 1)
    return t * t * (3.0 - 2.0 * t) if ease == "smoothstep" else t


def component_rows(label):
    """A component labelling (arap.components: the least vertex id of each) as (index int32 [Vm] 0 .. C - 1 in the order of the least
    ids, offsets int32 [C+1], rows int32 [Vm] ascending within a component)"""
    uniq, index = np.unique(label, return_inverse=True)
    index = index.reshape(-1)
    rows = np.argsort(index, kind="stable")
    offsets = np.zeros(len(uniq) + 1, np.int64)
    np.cumsum(np.bincount(index, minlength=len(uniq)), out=offsets[1:])
    return index.astype(np.int32), offsets.astype(np.int32), rows.astype(np.int32)


class PoseInterpolator:
    """In-betweens of key poses of one mesh.  Built once: the mesh's MeshGraph (rest_vertices may be one, with faces=None: it is shared, not
    rebuilt) - the edge CSR, the faces at every vertex, the connected components of the weighted edge graph -, the mask of held rows, and
    on a device the workspace, grown to the largest batch seen.
    rest_vertices [Vm,3], faces [F,3] vertex ids.  anchors=None: the vertex of least id of every component is held on its linear path
    and every component is then translated so that its mean is (1 - t) mean_A + t mean_B - a spin about the centroid comes out as a
    spin.  anchors=[ids]: those rows are held at (1 - t) A_i + t B_i and nothing is translated (feet on the ground).  PINNED vertices
    (weights sum to 0: unreferenced, or every face at them degenerate) are components of their own and move linearly either way.
    ValueError for an anchor id out of range or given twice, an empty anchor list, and a component that has a free vertex but no anchor
    (the system would be singular)."""

    def __init__(self, rest_vertices, faces, anchors=None, device="cuda"):
        who = "PoseInterpolator"
        g = self.mesh = MeshGraph.of(rest_vertices, faces, device, who)
        held = g.edgeless.copy()
        if anchors is None:
            held[np.unique(g.label)] = True
            h = None
        else:
            h = g.vertex_ids(anchors, who, "anchor")
            held[h] = True
            g.require_anchored(held, h, who, "anchor")
        self.device, self.Vm, self.F, self.csr, self.label = g.device, g.Vm, g.F, g.csr, g.label
        self.anchors, self.pinned, self.held = h, np.nonzero(g.edgeless)[0], held
        if self.device.type != "cuda":                                 # the set-up above is host work; between() needs the device
            return
        t = lambda a: on_device(a, torch.int32, self.device)
        self.rest, self._off, self._cols, self._w = g.device_csr
        self._faces, self._vf_off, self._vf_faces = g.device_faces
        self._held = on_device(held.astype(np.uint8), torch.uint8, self.device)
        if anchors is None:
            index, c_off, c_rows = component_rows(g.label)
            self.C, self._label, self._comp_off, self._comp_rows = len(c_off) - 1, t(index), t(c_off), t(c_rows)
        else:
            self.C, self._label, self._comp_off, self._comp_rows = 0, None, None, None
        self._ws = None                                                # made by the first between(), grown to the largest T seen

    def between(self, A, B, ts, cg_iterations=512, cg_tolerance=1e-6, out=None, want_stats=False):
        """The meshes [T,Vm,3] float32 on the device at parameters ts (T numbers, each in [0, 1]) between the key poses A and B ([Vm,3],
        read as float32): ts = 0 gives A and ts = 1 gives B up to the solve's tolerance and the float32 rounding.  Cut into launch
        chains of at most GM_POSE_INTERP_BATCH_MAX (64) frames; a frame's bits depend on its t alone, not on the batch, the order or
        the call.  out: a contiguous float32 [T,Vm,3] tensor on the device that shares no memory with A or B.  With want_stats returns
        (meshes, stats float64 [T,6]): CG steps used for x / y / z, final |r| / |b| for x / y / z.  Stream-ordered; nothing here waits
        for the device (reading stats does).  ValueError for a ts that is empty, not finite or outside [0, 1], and for shapes;
        GmeshError without a device.
        The defaults (at most 512 CG steps per coordinate, relative residual 1e-6) began as unmeasured values, 256 and 1e-6, and the cap
        was raised after tools/pose_interp_time.py: from the linear blend, with one held vertex per
        component, the tolerance asks for at most 127 steps at 1073 vertices and at most 339 at 7.5 k on an MI355X, where 256 stopped
        short at |r| / |b| = 8e-4; 512 lies above the largest count seen.  A step costs about 31 us at 7.5 k vertices, whatever T up
        to 8: 64 in-betweens take 0.2 ms each."""
        who = "PoseInterpolator.between"
        self.mesh.need_device(who)
        tv = np.asarray(host(ts), np.float64).reshape(-1)
        if tv.size == 0 or not np.all(np.isfinite(tv)) or float(tv.min()) < 0.0 or float(tv.max()) > 1.0:
            raise ValueError("%s: ts must be at least one finite number in [0, 1]; got %s" % (who, tv.tolist() if tv.size <= 8 else "%d values" % tv.size))
        a, b = self.mesh.rows_f32(A, who, "A"), self.mesh.rows_f32(B, who, "B")
        T, Vm, dev = tv.size, self.Vm, self.rest.device
        given, out = out is not None, self.mesh.out_f32(out, (T, Vm, 3), who)
        lo, hi = out.data_ptr(), out.data_ptr() + 12 * T * Vm
        for k in (a, b) if given else ():
            if k.data_ptr() < hi and lo < k.data_ptr() + 12 * Vm:
                raise ValueError("%s: out shares memory with a key pose" % who)
        stats = torch.zeros((T, 6), dtype=torch.float64, device=dev) if want_stats else None
        t_dev = torch.as_tensor(tv, dtype=torch.float64, device=dev)
        top = _lib.GM_POSE_INTERP_BATCH_MAX
        need = _lib.lib().gm_pose_interp_workspace_bytes(Vm, self.F, min(T, top))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        for s in range(0, T, top):
            e = min(s + top, T)
            enqueue(dev, "gm_pose_interp", e - s, Vm, self.F, self._off, self._cols, self._w, self.rest, self._faces, self._vf_off, self._vf_faces,
                    self._held, self.C, self._comp_off, self._comp_rows, self._label, a, b, t_dev[s:e], int(cg_iterations), float(cg_tolerance),
                    out[s:e], None if stats is None else stats[s:e], workspace=self._ws)
        return (out, stats) if want_stats else out

    def sequence(self, keys, inbetweens, ease="linear", **between_options):
        """The animation through K >= 2 key poses (keys [K,Vm,3], or a list of [Vm,3] tensors) with `inbetweens` >= 0 frames between
        consecutive keys: [(K - 1)(inbetweens + 1) + 1, Vm, 3] float32.  The key frames are the keys' own bits (read as float32),
        copied; only the frames strictly between are solved, at segment_ts(inbetweens, ease).  inbetweens = 0 returns the keys.
        between_options: cg_iterations, cg_tolerance."""
        who = "PoseInterpolator.sequence"
        self.mesh.need_device(who)
        if "out" in between_options or "want_stats" in between_options:
            raise ValueError("%s: out and want_stats are between()'s; the result is allocated here" % who)
        ts = segment_ts(inbetweens, ease)
        if torch.is_tensor(keys) or isinstance(keys, np.ndarray):
            if keys.ndim != 3:
                raise ValueError("%s: keys must be [K,%d,3]; got %s" % (who, self.Vm, tuple(keys.shape)))
            keys = list(keys)
        keys = [self.mesh.rows_f32(k, who, "every key") for k in keys]
        if len(keys) < 2:
            raise ValueError("%s: at least two keys; got %d" % (who, len(keys)))
        n = len(ts)
        out = torch.empty(((len(keys) - 1) * (n + 1) + 1, self.Vm, 3), dtype=torch.float32, device=self.rest.device)
        for k, key in enumerate(keys):
            out[k * (n + 1)].copy_(key)
            if n and k + 1 < len(keys):
                self.between(key, keys[k + 1], ts, out=out[k * (n + 1) + 1:(k + 1) * (n + 1)], **between_options)
        return out
