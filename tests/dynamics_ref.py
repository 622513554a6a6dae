"""Projective-dynamics steps of an elastic mesh with the ARAP energy as its potential, restated in float64 numpy: the definition
gm_mesh_dynamics is held to (INTEGRATION.md section AA).  Built on arap_ref.Reference: its dense Laplacian, its np.linalg.svd
rotations, its right-hand side.  The global step is exact (a dense solve of diag(mu) + L on the free rows: the inverse is formed once per
set of constraints and every solve is refined once against the matrix itself); `pcg` is the Jacobi-preconditioned conjugate-gradient
variant with the device's stopping rule.  The state is rounded to float32 at every step boundary.  numpy only."""
import numpy as np

import arap_ref


def vertex_masses(vertices, faces, density=1.0):
    """one third of each incident face's area, times density; float64 from the float32 vertices"""
    V = np.asarray(vertices, np.float32).astype(np.float64)
    m = np.zeros(len(V))
    for tri in np.asarray(faces, np.int64):
        a = 0.5 * np.linalg.norm(np.cross(V[tri[1]] - V[tri[0]], V[tri[2]] - V[tri[0]]))
        m[tri] += a / 3.0
    return m * density


class Dynamics:
    def __init__(self, rest_vertices, faces, mass, pinned=(), handles=(), dt=1.0 / 30.0, stiffness=10.0, damping=0.0, gravity=(0.0, 0.0, 0.0), iterations=3):
        self.ref = arap_ref.Reference(rest_vertices, faces, [])
        self.h, self.k, self.g, self.a, self.iterations = float(dt), float(stiffness), float(damping), np.asarray(gravity, np.float64), int(iterations)
        self.mu = np.asarray(mass, np.float64) / (2.0 * self.k * self.h * self.h)
        self.set_constraints(pinned, handles)

    def set_constraints(self, pinned=(), handles=()):
        r = self.ref
        self.handles = np.asarray(handles, np.int64).reshape(-1)
        held = r.pinned.copy()
        held[np.asarray(pinned, np.int64).reshape(-1)] = True
        held[self.handles] = True
        self.held, self.free = held, ~held
        f = self.free
        self.A = r.L[np.ix_(f, f)] + np.diag(self.mu[f])
        self.Ainv = np.linalg.inv(self.A) if f.any() else None
        self.Lfh = r.L[np.ix_(f, held)]

    def _rhs(self, X, y, R):
        """the right-hand side of the restricted system, [free,3]: mu y + the rotations' term, the held neighbours moved over"""
        f = self.free
        return self.mu[f, None] * y[f] + self.ref.rhs(R)[f] - self.Lfh @ X[self.held]

    def _global_exact(self, X, y, R):
        out = X.copy()
        if self.free.any():
            b = self._rhs(X, y, R)
            x = self.Ainv @ b
            x += self.Ainv @ (b - self.A @ x)
            out[self.free] = x
        return out, np.zeros(3), np.zeros(3)

    def _global_pcg(self, X, y, R, cg_iterations, cg_tolerance):
        f = self.free
        out, used, res = X.copy(), np.zeros(3), np.zeros(3)
        if not f.any():
            return out, used, res
        B, A, d = self._rhs(X, y, R), self.A, self.mu[f] + self.ref.deg[f]
        for c in range(3):
            b = B[:, c]
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

    def prediction(self, x, v):
        return x + self.h * v + self.h * self.h * self.a

    def solve_step(self, x, v, targets=None, pcg=None):
        """the float64 iterate X of one step from the float32 state, with (y, R of the last iteration, stats [6])"""
        x, v = np.asarray(x, np.float32).astype(np.float64), np.asarray(v, np.float32).astype(np.float64)
        y = self.prediction(x, v)
        X = np.where(self.free[:, None], y, x)
        if len(self.handles):
            X[self.handles] = np.asarray(targets, np.float32).astype(np.float64)
        for _ in range(self.iterations):
            R = self.ref.rotations(X)
            X, used, res = self._global_exact(X, y, R) if pcg is None else self._global_pcg(X, y, R, *pcg)
        return X, y, R, np.concatenate([used, res])

    def step(self, x, v, targets=None, pcg=None):
        """(x', v', stats [6]): the state after one step, float32"""
        X, _, _, stats = self.solve_step(x, v, targets, pcg)
        x64 = np.asarray(x, np.float32).astype(np.float64)
        vel = (X - x64) / self.h
        vel[self.free] *= 1.0 - self.g
        return X.astype(np.float32), vel.astype(np.float32), stats

    def run(self, x, v, steps, targets=None, pcg=None):
        """(positions [steps,Vm,3] float32, the last velocities [Vm,3] float32, stats [steps,6]); targets [steps,H,3]"""
        xs, stats = [], []
        for t in range(steps):
            x, v, s = self.step(x, v, None if targets is None else targets[t], pcg)
            xs.append(x)
            stats.append(s)
        return np.array(xs, np.float32).reshape(steps, -1, 3), v, np.array(stats).reshape(steps, 6)

    def objective_gradient(self, X, y, R):
        """d/dX of sum_i mass_i / (2 h^2) |X_i - y_i|^2 + (k / 2) E_arap(X, R) at fixed R, [Vm,3]:
        mass / h^2 (X - y) + (k / 2) 4 (L X - rhs(R)), and mass / h^2 = 2 k mu"""
        return 2.0 * self.k * (self.mu[:, None] * (X - y) + self.ref.L @ X - self.ref.rhs(R))

    def objective(self, X, y, R):
        return float((self.mu * 2.0 * self.k / 2.0 * ((X - y) ** 2).sum(axis=1)).sum() + 0.5 * self.k * self.ref.energy(X, R))
