"""As-rigid-as-possible deformation (Sorkine & Alexa 2007) restated in float64 numpy: the definition gm_arap_solve is held to
(INTEGRATION.md section Q).  Dense Laplacian, np.linalg.svd for the local step, np.linalg.solve for an exact global step; `pcg` is the
Jacobi-preconditioned conjugate-gradient variant with the device's stopping rule.  Written independently of gaussianmesh_amd.arap
(its own weights); numpy only."""
import numpy as np


def weight_matrix(vertices, faces):
    """Dense symmetric [Vm,Vm] edge weights: every face corner c opposite edge (a, b) adds max(0.5 cot(angle at c), 1e-3) to w_ab,
    cot = (u . w) / |u x w|; a face with |u x w| <= 1e-30 adds nothing.  float64 from the float32 vertices."""
    V = np.asarray(vertices, np.float32).astype(np.float64)
    W = np.zeros((len(V), len(V)))
    for tri in np.asarray(faces, np.int64):
        for k in range(3):
            c, a, b = tri[k], tri[(k + 1) % 3], tri[(k + 2) % 3]
            u, w = V[a] - V[c], V[b] - V[c]
            n = np.cross(u, w)
            area2 = np.sqrt(n @ n)
            if not area2 > 1e-30 or a == b:
                continue
            wt = max(0.5 * (u @ w) / area2, 1e-3)
            W[a, b] += wt
            W[b, a] += wt
    return W


class Reference:
    def __init__(self, rest_vertices, faces, fixed_ids):
        self.V0 = np.asarray(rest_vertices, np.float32).astype(np.float64)
        self.W = weight_matrix(rest_vertices, faces)
        self.I, self.J = np.nonzero(self.W)
        self.w = self.W[self.I, self.J]
        self.E0 = self.V0[self.I] - self.V0[self.J]                     # rest edges p_i - p_j
        deg = self.W.sum(axis=1)
        self.L = np.diag(deg) - self.W
        self.pinned = deg <= 0.0
        held = self.pinned.copy()
        held[np.asarray(fixed_ids, np.int64)] = True
        self.held, self.free = held, ~held
        self.deg = deg
        self.scale = float((self.w * (self.E0 ** 2).sum(axis=1)).sum())  # sum_ij w_ij |p_i - p_j|^2: the size of E's terms

    def rotations(self, X):
        S = np.zeros((len(self.V0), 3, 3))
        np.add.at(S, self.I, self.w[:, None, None] * (X[self.I] - X[self.J])[:, :, None] * self.E0[:, None, :])
        U, s, Vt = np.linalg.svd(S)
        D = np.tile(np.eye(3), (len(S), 1, 1))
        D[:, 2, 2] = np.linalg.det(U @ Vt)
        R = U @ D @ Vt
        R[~(s[:, 1] > 1e-12 * s[:, 0])] = np.eye(3)                     # rank <= 1: the identity
        return R

    def energy(self, X, R):
        d = (X[self.I] - X[self.J]) - np.einsum("nab,nb->na", R[self.I], self.E0)
        return float((self.w * (d ** 2).sum(axis=1)).sum())

    def rhs(self, R):
        B = np.zeros_like(self.V0)
        np.add.at(B, self.I, 0.5 * self.w[:, None] * np.einsum("nab,nb->na", R[self.I] + R[self.J], self.E0))
        return B

    def global_direct(self, X, B):
        f, h = self.free, self.held
        out = X.copy()
        if f.any():
            out[f] = np.linalg.solve(self.L[np.ix_(f, f)], B[f] - self.L[np.ix_(f, h)] @ X[h])
        return out

    def global_pcg(self, X, B, cg_iterations, cg_tolerance):
        """per column: x warm-started, stop at |r| <= tol |b| or after cg_iterations steps; returns (X, steps [3], |r| / |b| [3])"""
        f, h = self.free, self.held
        out, used, res = X.copy(), np.zeros(3, int), np.zeros(3)
        if not f.any():
            return out, used, res
        A, d = self.L[np.ix_(f, f)], self.deg[f]
        for c in range(3):
            b = B[f, c] - self.L[np.ix_(f, h)] @ X[h, c]
            x = X[f, c].copy()
            r = b - A @ x
            z = r / d
            p, rz, bb, rr = z.copy(), r @ z, b @ b, r @ r
            for it in range(cg_iterations):
                if not rr > cg_tolerance ** 2 * bb:
                    break
                q = A @ p
                pq = p @ q
                if not pq > 0:
                    break
                alpha = rz / pq
                x += alpha * p
                r -= alpha * q
                z = r / d
                rz_new, rr = r @ z, r @ r
                p = z + (rz_new / rz) * p
                rz = rz_new
                used[c] = it + 1
            out[f, c] = x
            res[c] = np.sqrt(rr / bb) if bb > 0 else (np.inf if rr > 0 else 0.0)
        return out, used, res

    def solve(self, init, outer_iterations, pcg=None):
        """init float32 [Vm,3] with the held rows at their targets.  pcg None: exact global steps; (cg_iterations, cg_tolerance): PCG.
        Returns (positions after every outer iteration [outer,Vm,3] float64, stats [outer,8] as gm_arap_solve lays them out)."""
        X = np.asarray(init, np.float32).astype(np.float64)
        hist, stats = [], np.zeros((outer_iterations, 8))
        for k in range(outer_iterations):
            R = self.rotations(X)
            stats[k, 0] = self.energy(X, R)
            B = self.rhs(R)
            if pcg is None:
                X = self.global_direct(X, B)
            else:
                X, stats[k, 2:5], stats[k, 5:8] = self.global_pcg(X, B, *pcg)
            stats[k, 1] = self.energy(X, R)
            hist.append(X.copy())
        return np.array(hist).reshape(outer_iterations, len(self.V0), 3), stats
