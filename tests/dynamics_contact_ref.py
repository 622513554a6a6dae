"""Projective-dynamics steps with unilateral contact against analytic colliders, restated in float64 numpy: the definition
gm_mesh_dynamics_contact is held to (INTEGRATION.md section AB).  A subclass of dynamics_ref.Dynamics: everything of a step is its parent's,
and in each iteration every free row takes the collider of its smallest phi, is active iff that phi is negative, and then adds
kappa_i = mu_i kc h^2 to the matrix's diagonal and kappa_i c_i to the right-hand side.  The matrix changes with the active set, so the
exact global step is one np.linalg.solve per iteration (refined once against the matrix); `pcg` is the Jacobi-preconditioned CG with the
device's stopping rule and the diagonal (mu + kappa) + d.  An iteration in which no row is active IS the parent's (its arrays, exactly).
numpy only."""
import numpy as np

import dynamics_ref as dr

HALF_SPACE, SPHERE = 0, 1


def half_space(normal, offset=None, point=None, friction=0.0):
    """(kind, row float32 [4], friction): the solid is n . x < d; the normal is normalised here, d = offset or n . point"""
    n = np.asarray(normal, np.float64)
    n = n / np.linalg.norm(n)
    d = float(offset) if offset is not None else float(n @ np.asarray(point, np.float64))
    return HALF_SPACE, np.array([n[0], n[1], n[2], d], np.float32), float(friction)


def floor(height=0.0, up=(0.0, 1.0, 0.0), friction=0.0):
    return half_space(up, offset=height, friction=friction)


def sphere(center, radius, friction=0.0):
    c = np.asarray(center, np.float64)
    return SPHERE, np.array([c[0], c[1], c[2], radius], np.float32), float(friction)


def phis(kinds, rows, X):
    """phi of every collider at every row of X: [Vm,K] (NaN for a kind that is neither 0 nor 1)"""
    out = np.full((len(X), len(kinds)), np.nan)
    for k, kind in enumerate(kinds):
        r = np.asarray(rows[k], np.float32).astype(np.float64)
        if kind == HALF_SPACE:
            out[:, k] = X @ r[:3] - r[3]
        elif kind == SPHERE:
            out[:, k] = np.linalg.norm(X - r[:3], axis=1) - r[3]
    return out


class ContactDynamics(dr.Dynamics):
    """colliders: a sequence of (kind, row [4], friction) as half_space / floor / sphere make them; contact_stiffness kc.  run / step /
    solve_step take collider_rows ([steps,K,4] / [K,4]) for colliders that move; without it the colliders' own rows in every step.
    After run: contact [steps,Vm] int (1 + k* of the rows active in each step's last iteration, 0 elsewhere), phi_star [steps,Vm] (the
    smallest phi at that iterate; +inf on held rows and with no candidate) and gap [steps,Vm] (the second smallest phi minus the smallest;
    +inf with fewer than two).  What a row can touch is candidates(): a subclass adds to it."""

    def __init__(self, *args, colliders=(), contact_stiffness=1.0e4, **kw):
        super().__init__(*args, **kw)
        self.kinds = [int(c[0]) for c in colliders]
        self.rows = np.array([np.asarray(c[1], np.float32) for c in colliders], np.float32).reshape(len(self.kinds), 4)
        self.friction = np.array([float(c[2]) for c in colliders], np.float64)
        self.kc = float(contact_stiffness)
        self.contact = self.phi_star = self.gap = None

    def candidates(self, X, rows):
        """(phi [Vm,K'], friction [K'], normal(i, k) of candidate k at row i, per-row arrays run is to keep as well, by name)"""
        def normal(i, k):
            if self.kinds[k] == HALF_SPACE:
                return rows[k, :3]
            e = X[i] - rows[k, :3]
            s = np.linalg.norm(e)
            return e / s if s > 0.0 else np.array([0.0, 1.0, 0.0])
        return phis(self.kinds, rows, X), self.friction, normal, {}

    def contact_terms(self, X, xs, rows):
        """(kappa [Vm], c [Vm,3], which [Vm] int: 1 + k* or 0, phi_star [Vm], gap [Vm]) at the iterate X with the step's start xs"""
        Vm = len(X)
        kappa, c, which = np.zeros(Vm), np.zeros((Vm, 3)), np.zeros(Vm, np.int64)
        best, gap, kstar = np.full(Vm, np.inf), np.full(Vm, np.inf), np.full(Vm, -1)
        rows = np.asarray(rows, np.float32).astype(np.float64).reshape(len(self.kinds), 4)
        phi, friction, normal, also = self.candidates(X, rows)
        for k in range(phi.shape[1]):                                  # phi < best: ties to the lowest k, a NaN never
            take = phi[:, k] < best
            best[take], kstar[take] = phi[take, k], k
        if phi.shape[1] > 1:
            s = np.sort(np.where(np.isnan(phi), np.inf, phi), axis=1)
            with np.errstate(invalid="ignore"):
                gap = np.where(np.isfinite(s[:, 1]), s[:, 1] - s[:, 0], np.inf)
        best[self.held], gap[self.held] = np.inf, np.inf
        for i in np.flatnonzero(self.free & (best < 0.0)):
            k, p, n = kstar[i], best[i], normal(i, kstar[i])
            u = X[i] - xs[i]
            t = u - (n @ u) * n
            s, lim = np.linalg.norm(t), friction[k] * abs(p)
            scale = 1.0 if s <= lim else lim / s
            kappa[i], c[i], which[i] = self.mu[i] * (self.kc * self.h * self.h), X[i] - p * n - scale * t, 1 + k
        self.last = dict(also, contact=which, phi_star=best, gap=gap)
        return kappa, c, which, best, gap

    def _global_contact_exact(self, X, y, R, kappa, c):
        f = self.free
        A = self.A + np.diag(kappa[f])
        b = self._rhs(X, y, R) + kappa[f, None] * c[f]
        x = np.linalg.solve(A, b)
        x += np.linalg.solve(A, b - A @ x)
        out = X.copy()
        out[f] = x
        return out, np.zeros(3), np.zeros(3)

    def _global_contact_pcg(self, X, y, R, kappa, c, cg_iterations, cg_tolerance):
        f = self.free
        out, used, res = X.copy(), np.zeros(3), np.zeros(3)
        A = self.A + np.diag(kappa[f])
        B = self._rhs(X, y, R) + kappa[f, None] * c[f]
        d = (self.mu[f] + kappa[f]) + self.ref.deg[f]
        for col in range(3):
            b = B[:, col]
            x = X[f, col].copy()
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
                used[col] = it + 1
            out[f, col] = x
            res[col] = np.sqrt(rr / bb) if bb > 0 else (np.inf if rr > 0 else 0.0)
        return out, used, res

    def solve_step(self, x, v, targets=None, pcg=None, collider_rows=None):
        """the float64 iterate X of one step from the float32 state, with (y, R of the last iteration, stats [6]); the contact of the
        last iteration is left in self.last (contact_terms)"""
        rows = self.rows if collider_rows is None else np.asarray(collider_rows, np.float32).reshape(len(self.kinds), 4)
        x, v = np.asarray(x, np.float32).astype(np.float64), np.asarray(v, np.float32).astype(np.float64)
        y = self.prediction(x, v)
        X = np.where(self.free[:, None], y, x)
        if len(self.handles):
            X[self.handles] = np.asarray(targets, np.float32).astype(np.float64)
        for _ in range(self.iterations):
            R = self.ref.rotations(X)
            kappa, c, which, _, _ = self.contact_terms(X, x, rows)
            if not which.any():
                X, used, res = self._global_exact(X, y, R) if pcg is None else self._global_pcg(X, y, R, *pcg)
            elif pcg is None:
                X, used, res = self._global_contact_exact(X, y, R, kappa, c)
            else:
                X, used, res = self._global_contact_pcg(X, y, R, kappa, c, *pcg)
        return X, y, R, np.concatenate([used, res])

    def step(self, x, v, targets=None, pcg=None, collider_rows=None):
        """(x', v', stats [6]): the state after one step, float32"""
        X, _, _, stats = self.solve_step(x, v, targets, pcg, collider_rows)
        vel = (X - np.asarray(x, np.float32).astype(np.float64)) / self.h
        vel[self.free] *= 1.0 - self.g
        return X.astype(np.float32), vel.astype(np.float32), stats

    def run(self, x, v, steps, targets=None, pcg=None, collider_rows=None):
        """(positions [steps,Vm,3] float32, the last velocities [Vm,3] float32, stats [steps,6]); collider_rows [steps,K,4]"""
        xs, stats, trace = [], [], []
        for t in range(steps):
            x, v, s = self.step(x, v, None if targets is None else targets[t], pcg, None if collider_rows is None else collider_rows[t])
            xs.append(x)
            stats.append(s)
            trace.append(self.last)
        for name in trace[0]:                                          # contact, phi_star, gap, and what candidates() named
            setattr(self, name, np.array([a[name] for a in trace]).reshape(steps, -1))
        return np.array(xs, np.float32).reshape(steps, -1, 3), v, np.array(stats).reshape(steps, 6)
