"""float64 numpy reference of the skinning stage (gaussianmesh_amd/skinning.py, csrc/gm_skin.hip), written from the definition in
INTEGRATION.md section AE and not from the kernels: forward kinematics with 4 x 4 matrices, segment distances / near sets / h / p, a
dense np.linalg.solve per bone over the unknown rows of diag(h) + L (L from mesh_graph.edge_csr, area from dynamics.vertex_masses: both
are INPUTS of the kernels), the compaction rule, both blends - and pcg(), a plain restatement of the Jacobi-PCG with the same start and
the same stopping rule, used only to measure what such a solve leaves against the dense one (the tolerance of test_gpu_skin.py)."""
import numpy as np

from gaussianmesh_amd.dynamics import vertex_masses
from gaussianmesh_amd.mesh_graph import edge_csr


# ---- forward kinematics ------------------------------------------------------------------------------------------------------------------
def rotation_matrix(rotvec):
    """cos(a) I + sin(a) [k]x + (1 - cos(a)) k k^T for rotvec = a k"""
    r = np.asarray(rotvec, np.float64)
    a = float(np.linalg.norm(r))
    if a == 0.0:
        return np.eye(3)
    k = r / a
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.cos(a) * np.eye(3) + np.sin(a) * Kx + (1.0 - np.cos(a)) * np.outer(k, k)


def about(R, c):
    """4 x 4: rotate by R about the point c"""
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = c - R @ c
    return M


def bone_transforms(joints, parents, rotations, root_translation=None):
    """float64 [T,J,3,4]: bone b moves with G_parents[b+1]; rotations [T,Nj,3,3] or [T,Nj,3] (axis-angle)"""
    joints = np.asarray(joints, np.float32).astype(np.float64)
    rot = np.asarray(rotations, np.float64)
    T, Nj = rot.shape[0], len(joints)
    out = np.zeros((T, Nj - 1, 3, 4))
    for t in range(T):
        G = []
        for k in range(Nj):
            R = rot[t, k] if rot.ndim == 4 else rotation_matrix(rot[t, k])
            M = about(R, joints[k])
            if k == 0:
                shift = np.eye(4)
                if root_translation is not None:
                    shift[:3, 3] = np.asarray(root_translation, np.float64)[t]
                G.append(shift @ M)
            else:
                G.append(G[int(parents[k])] @ M)
        for b in range(Nj - 1):
            out[t, b] = G[int(parents[b + 1])][:3]
    return out


# ---- the weights -------------------------------------------------------------------------------------------------------------------------
def segment_d2(V, a, b):
    """[J,Vm] squared distances of the points V [Vm,3] to the segments a[j] -> b[j]"""
    out = np.zeros((len(a), len(V)))
    for j in range(len(a)):
        ab = b[j] - a[j]
        ll = float(ab @ ab)
        s = np.clip(((V - a[j]) @ ab) / ll, 0.0, 1.0) if ll > 0.0 else np.zeros(len(V))
        foot = a[j] + s[:, None] * ab
        out[j] = ((V - foot) ** 2).sum(axis=1)
    return out


class System:
    """Everything of one (mesh, skeleton) before the solve.  d2 [J,Vm], d2min, near bool [J,Vm], h, p [J,Vm], the CSR, diag = h + d,
    unknown bool [Vm]."""

    def __init__(self, V0, faces, joints, parents, heat=1.0):
        V = np.asarray(V0, np.float32).astype(np.float64)
        joints = np.asarray(joints, np.float32).astype(np.float64)
        parents = np.asarray(parents)
        self.Vm, self.J = len(V), len(joints) - 1
        self.a, self.b = joints[parents[1:]], joints[1:]
        self.d2 = segment_d2(V, self.a, self.b)
        box = V.max(axis=0) - V.min(axis=0)
        floor = 1e-3 * np.sqrt((box * box).sum())
        self.d2min = np.maximum(self.d2.min(axis=0), floor * floor)
        self.near = self.d2 <= (1.0 + 1e-4) ** 2 * self.d2min
        area = vertex_masses(V0, faces, 1.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.h = np.where(area > 0.0, heat * area / self.d2min, 0.0)
        self.p = self.near / self.near.sum(axis=0)
        off, cols, w = edge_csr(V0, faces)
        self.rows = np.repeat(np.arange(self.Vm), np.diff(off.astype(np.int64)))
        self.cols, self.w = cols.astype(np.int64), w
        self.d = np.bincount(self.rows, weights=w, minlength=self.Vm)
        self.diag = self.h + self.d
        self.unknown = self.diag > 0.0

    def apply(self, x):
        """(diag(h) + L) x for x [Vm] or [Vm,k]"""
        x = np.asarray(x, np.float64)
        if x.ndim == 1:
            return self.diag * x - np.bincount(self.rows, weights=self.w * x[self.cols], minlength=self.Vm)
        nb = (self.w[:, None] * x[self.cols].reshape(len(self.cols), -1))
        s = np.zeros((self.Vm, nb.shape[1]))
        np.add.at(s, self.rows, nb)
        return (self.diag.reshape(-1, 1) * x.reshape(self.Vm, -1) - s).reshape(x.shape)

    def dense(self):
        """full [J,Vm]: np.linalg.solve over the unknown rows; the other rows keep p"""
        A = np.zeros((self.Vm, self.Vm))
        np.add.at(A, (self.rows, self.cols), -self.w)
        A[np.arange(self.Vm), np.arange(self.Vm)] += self.diag
        u = np.nonzero(self.unknown)[0]
        full = self.p.copy()
        if len(u):
            full[:, u] = np.linalg.solve(A[np.ix_(u, u)], (self.h * self.p)[:, u].T).T
        return full

    def pcg(self, cg_iterations, cg_tolerance):
        """The Jacobi-preconditioned CG as the definition states it, per bone: x0 = p_j, the test |r|^2 <= tol^2 |b|^2 before every step,
        out at p . A p <= 0.  Returns (full [J,Vm], steps [J], residual [J])."""
        full, steps, res = self.p.copy(), np.zeros(self.J), np.zeros(self.J)
        u = self.unknown
        tol2 = cg_tolerance * cg_tolerance
        for j in range(self.J):
            x = self.p[j].copy()
            b = np.where(u, self.h * x, 0.0)
            r = np.where(u, b - self.apply(x), 0.0)
            z = np.where(u, r / np.where(u, self.diag, 1.0), 0.0)
            p = z.copy()
            bb, rr, rz = float(b @ b), float(r @ r), float(r @ z)
            used = 0
            for it in range(cg_iterations):
                if not rr > tol2 * bb:
                    break
                q = np.where(u, self.apply(p), 0.0)
                pq = float(p @ q)
                if not pq > 0.0:
                    break
                alpha = rz / pq
                x = x + alpha * p
                r = r - alpha * q
                z = np.where(u, r / np.where(u, self.diag, 1.0), 0.0)
                rr, rz_new = float(r @ r), float(r @ z)
                p = z + (rz_new / rz) * p
                rz = rz_new
                used = it + 1
            full[j], steps[j] = x, used
            res[j] = np.sqrt(rr / bb) if bb > 0.0 else (np.inf if rr > 0.0 else 0.0)
        return full, steps, res


def compact(full, unknown, near, max_influences):
    """(bone_ids int32 [Vm,4], bone_w float32 [Vm,4]) of the columns full [J,Vm] by the compaction rule"""
    J, Vm = full.shape
    ids, w = np.zeros((Vm, 4), np.int32), np.zeros((Vm, 4), np.float32)
    for i in range(Vm):
        v = np.maximum(full[:, i], 0.0)
        order = sorted(range(J), key=lambda j: (-v[j], j))[:max_influences]          # falling weight, ties to the lower bone
        kept = [float(v[j]) for j in order] + [0.0] * (4 - len(order))
        total = ((kept[0] + kept[1]) + kept[2]) + kept[3]
        if not unknown[i] or not total > 0.0:
            ids[i] = int(np.nonzero(near[:, i])[0][0])
            w[i, 0] = 1.0
            continue
        for s in range(4):
            used = s < len(order) and kept[s] > 0.0
            ids[i, s] = order[s] if used else order[0]
            w[i, s] = np.float32(kept[s] / total) if used else 0.0
    return ids, w


# ---- the blends --------------------------------------------------------------------------------------------------------------------------
def blend_linear(rest, ids, w, transforms):
    """[T,Vm,3] float64: (sum_k w_k (M_k x)) / (sum_k w_k), the slots in order; a row whose weights sum to 0 stays"""
    x = np.asarray(rest, np.float32).astype(np.float64)
    M = np.asarray(transforms, np.float32).astype(np.float64)
    wk = np.asarray(w, np.float32).astype(np.float64)
    out = np.zeros((M.shape[0],) + x.shape)
    for t in range(M.shape[0]):
        acc, total = np.zeros_like(x), np.zeros(len(x))
        for k in range(4):
            Mk = M[t, ids[:, k]]
            acc += wk[:, k, None] * (np.einsum("vab,vb->va", Mk[:, :, :3], x) + Mk[:, :, 3])
            total += wk[:, k]
        ok = total != 0.0
        out[t] = np.where(ok[:, None], acc / np.where(ok, total, 1.0)[:, None], x)
    return out


def quaternion(A):
    """the unit quaternion (w, x, y, z), w >= 0, of the rotation matrix A: Shepperd's method, the branch of the largest of (trace, A00,
    A11, A22)"""
    tr = A[0, 0] + A[1, 1] + A[2, 2]
    which = int(np.argmax([tr, A[0, 0], A[1, 1], A[2, 2]]))
    if which == 0:
        q = np.array([1.0 + tr, A[2, 1] - A[1, 2], A[0, 2] - A[2, 0], A[1, 0] - A[0, 1]])
    elif which == 1:
        q = np.array([A[2, 1] - A[1, 2], 1.0 + A[0, 0] - A[1, 1] - A[2, 2], A[0, 1] + A[1, 0], A[0, 2] + A[2, 0]])
    elif which == 2:
        q = np.array([A[0, 2] - A[2, 0], A[0, 1] + A[1, 0], 1.0 + A[1, 1] - A[0, 0] - A[2, 2], A[1, 2] + A[2, 1]])
    else:
        q = np.array([A[1, 0] - A[0, 1], A[0, 2] + A[2, 0], A[1, 2] + A[2, 1], 1.0 + A[2, 2] - A[0, 0] - A[1, 1]])
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0.0 else q


def qmul(a, b):
    return np.concatenate([[a[0] * b[0] - a[1:] @ b[1:]], a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:])])


def dual_quaternion(M):
    """[8]: (q_r, q_d) of the rigid motion M = [A | t], q_d = (0, t) q_r / 2"""
    qr = quaternion(M[:, :3])
    return np.concatenate([qr, 0.5 * qmul(np.concatenate([[0.0], M[:, 3]]), qr)])


def blend_dqs(rest, ids, w, transforms):
    """[T,Vm,3] float64 by dual-quaternion blending; |b_r| < 1e-12: the linear blend"""
    x = np.asarray(rest, np.float32).astype(np.float64)
    M = np.asarray(transforms, np.float32).astype(np.float64)
    wk = np.asarray(w, np.float32).astype(np.float64)
    lin = blend_linear(rest, ids, w, transforms)
    out = np.zeros_like(lin)
    for t in range(M.shape[0]):
        dq = np.stack([dual_quaternion(M[t, j]) for j in range(M.shape[1])], 0)
        q = dq[ids]                                                                   # [Vm,4,8]
        sign = np.where((q[:, :, :4] * q[:, :1, :4]).sum(axis=2) < 0.0, -1.0, 1.0)
        b = np.zeros((len(x), 8))
        for k in range(4):
            b += (wk[:, k] * sign[:, k])[:, None] * q[:, k]
        n = np.linalg.norm(b[:, :4], axis=1)
        ok = ~(n < 1e-12)
        b = b / np.where(ok, n, 1.0)[:, None]
        bw, bv, dw, dv = b[:, 0:1], b[:, 1:4], b[:, 4:5], b[:, 5:8]
        moved = x + 2.0 * np.cross(bv, np.cross(bv, x) + bw * x) + 2.0 * (bw * dv - dw * bv + np.cross(bv, dv))
        out[t] = np.where(ok[:, None], moved, lin[t])
    return out


def blend(rest, ids, w, transforms, kind):
    return (blend_dqs if kind == "dqs" else blend_linear)(rest, ids, w, transforms)
