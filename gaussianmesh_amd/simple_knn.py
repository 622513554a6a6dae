"""distCUDA2: mean squared distance to the 3 nearest neighbours (scene/simple_knn/__init__.py:15-28).
knn_nearest: the nearest point of a second cloud (k = 1), for the neighbour pruning of train_bg_gaussian.py:129-137."""
import torch

from . import _lib
from ._op import enqueue, f32, need_cuda, workspace


def distCUDA2(points: torch.Tensor) -> torch.Tensor:
    need_cuda(points, "distCUDA2", "a tensor")
    pts = f32(points)
    P = pts.shape[0]
    means = torch.zeros((P,), dtype=torch.float32, device=pts.device)
    if P == 0:
        return means
    ws = workspace(pts.device, "gm_knn_workspace_bytes", P)
    enqueue(pts.device, "gm_knn", P, pts, means, workspace=ws)
    return means


def knn_nearest(query: torch.Tensor, ref: torch.Tensor):
    """For every row of query [Pq,3] the nearest row of ref [Pr,3]: (d2 float32 [Pq], idx int64 [Pq]).  d2 is the SQUARED distance
    (dx*dx + dy*dy) + dz*dz, d = query - ref, in float32 without contraction; ties go to the lowest index (gm_knn_nearest): a float32
    brute force gives the same bits.  An empty ref is an error."""
    if query.dim() != 2 or query.shape[1] != 3 or ref.dim() != 2 or ref.shape[1] != 3:
        raise ValueError("knn_nearest: query and ref must be [P,3]; got %s and %s" % (tuple(query.shape), tuple(ref.shape)))
    if ref.shape[0] == 0:
        raise ValueError("knn_nearest: the reference set is empty")
    if query.device.type != "cuda" or ref.device != query.device:
        raise _lib.GmeshError("knn_nearest needs both tensors on the same HIP (cuda) device; there is no CPU path")
    q, r = f32(query), f32(ref)
    Pq, Pr = q.shape[0], r.shape[0]
    d2 = torch.empty((Pq,), dtype=torch.float32, device=q.device)
    idx = torch.empty((Pq,), dtype=torch.int32, device=q.device)
    if Pq == 0:
        return d2, idx.long()
    ws = workspace(q.device, "gm_knn_nearest_workspace_bytes", Pq, Pr)
    enqueue(q.device, "gm_knn_nearest", Pq, q, Pr, r, d2, idx, workspace=ws)
    return d2, idx.long()
