"""Projective-dynamics steps with contact against the analytic colliders AND a sampled signed-distance grid, restated in float64 numpy:
the definition gm_mesh_dynamics_field is held to (INTEGRATION.md section AC).  A subclass of dynamics_contact_ref.ContactDynamics: only
the candidates change - the field is candidate K behind the K analytic colliders, so contact_terms takes it with the same `phi < best`
(ties to the analytic collider, a NaN never) - sampled as sdf_grid_ref.sample samples the prepared grid.  numpy only."""
import numpy as np

import dynamics_contact_ref as cr
import sdf_grid_ref as sg

PROBE = 1e-5                    # candidates' `fringe`: rows whose field value becomes or stops being a number within this distance


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

    def candidates(self, X, rows):
        """ContactDynamics' candidates and, last, the field: its phi, its friction, the sampled normal; `fringe` for run to keep"""
        phi, friction, normal, also = super().candidates(X, rows)
        fringe = np.zeros(len(X), bool)
        if self.field is None:
            return phi, friction, normal, dict(also, fringe=fringe)
        K = len(self.kinds)
        fphi, fn = self.field_sample(X)
        for axis in range(3):
            for sign in (-1.0, 1.0):
                P = X.copy()
                P[:, axis] += sign * PROBE
                fringe |= np.isnan(self.field_sample(P)[0]) != np.isnan(fphi)
        fringe[self.held] = False
        return (np.concatenate([phi, fphi[:, None]], axis=1), np.append(friction, self.field_friction),         # [Vm, K + 1]: the field last
                lambda i, k: fn[i] if k == K else normal(i, k), dict(also, fringe=fringe))
