"""Projective-dynamics steps with contact against the analytic colliders AND a sampled signed-distance grid, restated in float64 numpy:
the definition gm_mesh_dynamics_field is held to (INTEGRATION.md section AC).  A subclass of dynamics_contact_ref.ContactDynamics: only
contact_terms changes - the field is candidate K behind the K analytic colliders, with the same `phi < best` (ties to the analytic
collider, a NaN never), sampled as sdf_grid_ref.sample samples the prepared grid.  numpy only."""
import numpy as np

import dynamics_contact_ref as cr
import sdf_grid_ref as sg

PROBE = 1e-5                    # contact_terms' `fringe`: rows whose field value becomes or stops being a number within this distance


class FieldDynamics(cr.ContactDynamics):
    """field: (grid float32 [nz,ny,nx,4] as sdf_grid_ref.prepare makes it, origin [3], voxel); field_friction.  After run, next to
    ContactDynamics' contact / phi_star / gap (the field counted among the candidates, reported as 1 + K): fringe [steps,Vm] bool, the
    free rows that lie within PROBE of where the field's value changes between a number and NaN (the grid's border, an unknown sample)."""

    def __init__(self, *args, field=None, field_friction=0.0, **kw):
        super().__init__(*args, **kw)
        self.field, self.field_friction = field, float(field_friction)
        self.fringe = None

    def field_sample(self, X):
        grid, origin, voxel = self.field
        return sg.sample(grid, origin, voxel, X)

    def contact_terms(self, X, xs, rows):
        if self.field is None:
            self.last_fringe = np.zeros(len(X), bool)
            return super().contact_terms(X, xs, rows)
        Vm, K = len(X), len(self.kinds)
        kappa, c, which = np.zeros(Vm), np.zeros((Vm, 3)), np.zeros(Vm, np.int64)
        best = np.full(Vm, np.inf)
        rows = np.asarray(rows, np.float32).astype(np.float64).reshape(K, 4)
        fphi, fn = self.field_sample(X)
        phi = np.concatenate([cr.phis(self.kinds, rows, X), fphi[:, None]], axis=1)         # [Vm, K + 1]: the field last
        kstar = np.full(Vm, -1)
        with np.errstate(invalid="ignore"):
            for k in range(K + 1):
                take = phi[:, k] < best
                best[take], kstar[take] = phi[take, k], k
            s = np.sort(np.where(np.isnan(phi), np.inf, phi), axis=1)
            gap = np.where(np.isfinite(s[:, 1]), s[:, 1] - s[:, 0], np.inf) if K > 0 else np.full(Vm, np.inf)
        fringe = np.zeros(Vm, bool)
        for axis in range(3):
            for sign in (-1.0, 1.0):
                P = X.copy()
                P[:, axis] += sign * PROBE
                fringe |= np.isnan(self.field_sample(P)[0]) != np.isnan(fphi)
        best[self.held], gap[self.held], fringe[self.held] = np.inf, np.inf, False
        self.last_fringe = fringe
        for i in np.flatnonzero(self.free & (best < 0.0)):
            k, p = kstar[i], best[i]
            if k == K:
                n, mu = fn[i], self.field_friction
            elif self.kinds[k] == cr.HALF_SPACE:
                n, mu = rows[k, :3], self.friction[k]
            else:
                e = X[i] - rows[k, :3]
                s = np.linalg.norm(e)
                n, mu = (e / s if s > 0.0 else np.array([0.0, 1.0, 0.0])), self.friction[k]
            u = X[i] - xs[i]
            t = u - (n @ u) * n
            s, lim = np.linalg.norm(t), mu * abs(p)
            scale = 1.0 if s <= lim else lim / s
            kappa[i], c[i], which[i] = self.mu[i] * (self.kc * self.h * self.h), X[i] - p * n - scale * t, 1 + k
        return kappa, c, which, best, gap

    def run(self, x, v, steps, targets=None, pcg=None, collider_rows=None):
        """ContactDynamics.run; the fringe of every step's last iteration is kept as well"""
        xs, stats, trace, fr = [], [], [], []
        for t in range(steps):
            x, v, s = self.step(x, v, None if targets is None else targets[t], pcg, None if collider_rows is None else collider_rows[t])
            xs.append(x)
            stats.append(s)
            trace.append(self.last)
            fr.append(self.last_fringe)
        self.contact = np.array([a[0] for a in trace]).reshape(steps, -1)
        self.phi_star = np.array([a[1] for a in trace]).reshape(steps, -1)
        self.gap = np.array([a[2] for a in trace]).reshape(steps, -1)
        self.fringe = np.array(fr).reshape(steps, -1)
        return np.array(xs, np.float32).reshape(steps, -1, 3), v, np.array(stats).reshape(steps, 6)
