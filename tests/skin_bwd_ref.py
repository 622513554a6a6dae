"""float64 torch restatement of both skinning blends and of forward kinematics, CPU only, written from DEFINITION, POSE at the top of
csrc/gm_skin.hip and not from the kernels: autograd through it DEFINES what gm_skin_pose_bwd returns (test_gpu_skin_bwd.py), the
gradient off the rotation manifold included.  The forward's decisions are constants here as there: the Shepperd branch (an argmax), the
sign that makes q_w >= 0, the slots' signs s_k, the |b_r| < 1e-12 fallback and the sum == 0 row are all taken from detached values.
check_gradient_position() asserts, from this reference alone, that a case sits away from every decision a rounding could flip."""
import numpy as np
import torch

import skin_cases as sc

F64 = torch.float64


def rodrigues(r):
    """[...,3] axis-angle -> [...,3,3], written in th2 = r . r with the series below 1e-8: finite gradient at r = 0"""
    th2 = (r * r).sum(-1)[..., None, None]
    small = th2 < 1e-8
    th = torch.sqrt(torch.where(small, torch.ones_like(th2), th2))
    a = torch.where(small, 1 - th2 / 6 + th2 * th2 / 120, torch.sin(th) / th)
    b = torch.where(small, 0.5 - th2 / 24 + th2 * th2 / 720, (1 - torch.cos(th)) / th ** 2)
    z = torch.zeros_like(r[..., 0])
    K = torch.stack([torch.stack([z, -r[..., 2], r[..., 1]], -1), torch.stack([r[..., 2], z, -r[..., 0]], -1),
                     torch.stack([-r[..., 1], r[..., 0], z], -1)], -2)
    return torch.eye(3, dtype=r.dtype) + a * K + b * (K @ K)


def fk(joints, parents, r, tr):
    """bone transforms [T,J,3,4] float64 of rotations r [T,Nj,3] and root translation tr [T,3] (skinning's CONVENTION)"""
    Nj = r.shape[1]
    R = rodrigues(r)
    c = torch.as_tensor(np.asarray(joints, np.float32).astype(np.float64))
    A, t = [None] * Nj, [None] * Nj
    for k in range(Nj):
        own = c[k] - R[:, k] @ c[k]
        if k == 0:
            A[0], t[0] = R[:, 0], own + tr
        else:
            p = int(parents[k])
            A[k] = A[p] @ R[:, k]
            t[k] = torch.einsum("tab,tb->ta", A[p], own) + t[p]
    A, t = torch.stack(A, 1), torch.stack(t, 1)
    p = torch.as_tensor(np.asarray(parents[1:], np.int64))
    return torch.cat([A[:, p], t[:, p, :, None]], 3)


def quaternion(A, info=None):
    """[...,3,3] -> unit quaternions [...,4] with w >= 0 by Shepperd's branch; info gets which [...], the branch margin and min |q_w|"""
    tr = A[..., 0, 0] + A[..., 1, 1] + A[..., 2, 2]
    c = torch.stack([tr, A[..., 0, 0], A[..., 1, 1], A[..., 2, 2]], -1).detach()
    which = c.argmax(-1)
    q0 = torch.stack([1 + tr, A[..., 2, 1] - A[..., 1, 2], A[..., 0, 2] - A[..., 2, 0], A[..., 1, 0] - A[..., 0, 1]], -1)
    q1 = torch.stack([A[..., 2, 1] - A[..., 1, 2], 1 + A[..., 0, 0] - A[..., 1, 1] - A[..., 2, 2], A[..., 0, 1] + A[..., 1, 0], A[..., 0, 2] + A[..., 2, 0]], -1)
    q2 = torch.stack([A[..., 0, 2] - A[..., 2, 0], A[..., 0, 1] + A[..., 1, 0], 1 + A[..., 1, 1] - A[..., 0, 0] - A[..., 2, 2], A[..., 1, 2] + A[..., 2, 1]], -1)
    q3 = torch.stack([A[..., 1, 0] - A[..., 0, 1], A[..., 0, 2] + A[..., 2, 0], A[..., 1, 2] + A[..., 2, 1], 1 + A[..., 2, 2] - A[..., 0, 0] - A[..., 1, 1]], -1)
    q = torch.stack([q0, q1, q2, q3], -2).gather(-2, which[..., None, None].expand(*which.shape, 1, 4)).squeeze(-2)
    q = q / q.norm(dim=-1, keepdim=True)
    if info is not None:
        top = c.sort(-1).values
        info.update(which=which, branch=float((top[..., -1] - top[..., -2]).min()), qw=float(q[..., 0].detach().abs().min()))
    return torch.where(q[..., :1].detach() < 0, -q, q)


def linear(x, ids, w, M):
    """x [Vm,3], ids int64 [Vm,4], w [Vm,4], M [T,J,3,4] (all float64) -> [T,Vm,3]"""
    Mk = M[:, ids]
    y = torch.einsum("tvkab,vb->tvka", Mk[..., :3], x) + Mk[..., 3]
    acc, tot = (w[None, :, :, None] * y).sum(2), w.sum(1)
    ok = tot != 0
    return torch.where(ok[None, :, None], acc / torch.where(ok, tot, torch.ones_like(tot))[None, :, None], x[None].expand_as(acc))


def dqs(x, ids, w, M, info=None):
    qr = quaternion(M[..., :3], info)
    t = M[..., 3]
    qd = 0.5 * torch.cat([-(t * qr[..., 1:]).sum(-1, keepdim=True), qr[..., :1] * t + torch.linalg.cross(t, qr[..., 1:])], -1)
    dq = torch.cat([qr, qd], -1)[:, ids]                                # [T,Vm,4,8]
    dot = (dq[..., :4] * dq[:, :, :1, :4]).sum(-1).detach()
    s = torch.where(dot < 0, -1.0, 1.0).to(F64)
    b = ((w[None] * s)[..., None] * dq).sum(2)
    n = b[..., :4].norm(dim=-1, keepdim=True)
    ok = ~(n.detach() < 1e-12)
    if info is not None:
        used = (w[None] > 0).expand_as(dot)
        info.update(sign=float(dot.abs()[used].min()) if bool(used.any()) else float("inf"),
                    n=float(n.detach()[ok].min()) if bool(ok.any()) else float("inf"), fallback=int((~ok).sum()))
    b = b / torch.where(ok, n, torch.ones_like(n))
    bw, bv, dw, dv = b[..., :1], b[..., 1:4], b[..., 4:5], b[..., 5:]
    xx = x[None].expand_as(bv)
    moved = xx + 2 * torch.linalg.cross(bv, torch.linalg.cross(bv, xx) + bw * xx) + 2 * (bw * dv - dw * bv + torch.linalg.cross(bv, dv))
    return torch.where(ok, moved, linear(x, ids, w, M))


def blend(x, ids, w, M, kind, info=None):
    return dqs(x, ids, w, M, info) if kind == "dqs" else linear(x, ids, w, M)


def tensors(rest, ids, w):
    """the float32 / int inputs of the kernels as the float64 / int64 CPU tensors of this reference"""
    return (torch.as_tensor(np.asarray(rest, np.float32).astype(np.float64)), torch.as_tensor(np.asarray(ids).astype(np.int64)),
            torch.as_tensor(np.asarray(w, np.float32).astype(np.float64)))


def gradient(rest, ids, w, M32, g_out, kind, info=None):
    """d sum(out * g_out) / d transforms [T,J,3,4] float64 (numpy) at the float32 transforms M32, g_out float32 [T,Vm,3]"""
    x, idt, wt = tensors(rest, ids, w)
    M = torch.as_tensor(np.asarray(M32, np.float32).astype(np.float64)).requires_grad_(True)
    y = blend(x, idt, wt, M, kind, info)
    g, = torch.autograd.grad((y * torch.as_tensor(np.asarray(g_out, np.float32).astype(np.float64))).sum(), M)
    return g.numpy()


def reference_weights(mesh, skeleton):
    s = sc.system(mesh, skeleton)
    import skin_ref
    return skin_ref.compact(sc.dense(mesh, skeleton), s.unknown, s.near, 4)


def check_gradient_position(rest, ids, w, M32, floor=1e-6):
    """From the reference alone: the Shepperd margin (largest minus second of trace, A00, A11, A22), |q_k . q_0| on every slot with
    w > 0 and |b_r| all exceed `floor`, so no rounding of the device's float64 flips a decision.  Returns the three figures."""
    x, idt, wt = tensors(rest, ids, w)
    info = {}
    with torch.no_grad():
        dqs(x, idt, wt, torch.as_tensor(np.asarray(M32, np.float32).astype(np.float64)), info)
    assert info["branch"] > floor, "Shepperd margin %.3g" % info["branch"]
    assert info["sign"] > floor, "|q_k . q_0| = %.3g on a used slot" % info["sign"]
    assert info["n"] > floor, "|b_r| = %.3g" % info["n"]
    return info["branch"], info["sign"], info["n"]
