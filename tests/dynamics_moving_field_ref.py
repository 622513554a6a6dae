"""Projective-dynamics steps with contact against the analytic colliders AND up to four sampled signed-distance grids that move rigidly,
restated in float64 numpy: the definition gm_mesh_dynamics_fields is held to (INTEGRATION.md section AG).  A subclass of
dynamics_field_ref.FieldDynamics (built without its one static field): candidates() appends the F fields, field f as candidate K + f,
sampled through sdf_grid_ref.sample at R^T (X - t) with the normal rotated back; `fringe` is probed in each field's own frame; and
contact_terms carries the friction anchor of a row that a field wins with the obstacle: xs' = P_now(P_before^-1 xs).  A pose is (R | t)
[3,4], world = R local + t.  numpy only."""
import numpy as np

import dynamics_field_ref as fr
import sdf_grid_ref as sg

IDENTITY = np.eye(3, 4)


def carry(before, now, p):
    """the points p [N,3], fixed to a body that moved from pose `before` to pose `now`: P_now(P_before^-1 p)"""
    local = (p - before[:, 3]) @ before[:, :3]                         # R_b^T (p - t_b), row by row
    return local @ now[:, :3].T + now[:, 3]


class MovingFieldDynamics(fr.FieldDynamics):
    """fields: a sequence of (grid float32 [nz,ny,nx,4] as sdf_grid_ref.prepare makes it, origin [3], voxel); field_frictions: one number
    each.  run / step take field_poses ([steps,F,3,4] / [F,3,4]): every field's pose DURING the step; the pose before the first step is
    `poses` (the identity at first; run and step leave the last pose there, as MeshDynamics keeps it).  After run: FieldDynamics'
    contact (1 + K + f for field f) / phi_star / gap / fringe."""

    def __init__(self, *args, fields=(), field_frictions=None, **kw):
        super().__init__(*args, field=None, **kw)
        self.fields = list(fields)
        self.field_frictions = np.zeros(len(self.fields)) if field_frictions is None else np.asarray(field_frictions, np.float64)
        assert len(self.field_frictions) == len(self.fields)
        self.poses = np.tile(IDENTITY, (len(self.fields), 1, 1))
        self.before = self.now = self.poses

    def local(self, f, X):
        """world points in field f's frame during this step"""
        P = self.now[f]
        return (X - P[:, 3]) @ P[:, :3]

    def candidates(self, X, rows):
        phi, friction, normal, also = super().candidates(X, rows)      # the analytic colliders (the parent's own field is None)
        K, F = len(self.kinds), len(self.fields)
        if F == 0:
            return phi, friction, normal, also
        fringe = np.zeros(len(X), bool)
        fphis, fns = [], []
        for f, (grid, origin, voxel) in enumerate(self.fields):
            Xl = self.local(f, X)
            fphi, nl = sg.sample(grid, origin, voxel, Xl)
            for axis in range(3):
                for sign in (-1.0, 1.0):
                    P = Xl.copy()
                    P[:, axis] += sign * fr.PROBE
                    fringe |= np.isnan(sg.sample(grid, origin, voxel, P)[0]) != np.isnan(fphi)
            fphis.append(fphi)
            fns.append(nl @ self.now[f][:, :3].T)                      # n = R nl
        fringe[self.held] = False
        return (np.concatenate([phi] + [p[:, None] for p in fphis], axis=1), np.concatenate([friction, self.field_frictions]),
                lambda i, k: fns[k - K][i] if k >= K else normal(i, k), dict(also, fringe=fringe))

    def contact_terms(self, X, xs, rows):
        """FieldDynamics' terms with the anchor of every row a field wins carried by that field from the step's start to now; which
        candidate wins does not depend on the anchor, so it is found first"""
        K = len(self.kinds)
        which = super().contact_terms(X, xs, rows)[2]
        anchor = np.array(xs, np.float64, copy=True)
        for f in range(len(self.fields)):
            won = which == 1 + K + f
            if won.any() and not np.array_equal(self.before[f], self.now[f]):
                anchor[won] = carry(self.before[f], self.now[f], anchor[won])
        return super().contact_terms(X, anchor, rows)

    def step(self, x, v, targets=None, pcg=None, collider_rows=None, field_poses=None):
        self.before = self.poses
        self.now = self.poses if field_poses is None else np.asarray(field_poses, np.float64).reshape(len(self.fields), 3, 4)
        out = super().step(x, v, targets, pcg, collider_rows)
        self.poses = self.now
        return out

    def run(self, x, v, steps, targets=None, pcg=None, collider_rows=None, field_poses=None):
        """(positions [steps,Vm,3] float32, the last velocities [Vm,3] float32, stats [steps,6]); field_poses [steps,F,3,4]"""
        xs, stats, trace = [], [], []
        for t in range(steps):
            x, v, s = self.step(x, v, None if targets is None else targets[t], pcg, None if collider_rows is None else collider_rows[t],
                                None if field_poses is None else field_poses[t])
            xs.append(x)
            stats.append(s)
            trace.append(self.last)
        for name in trace[0]:
            setattr(self, name, np.array([a[name] for a in trace]).reshape(steps, -1))
        return np.array(xs, np.float32).reshape(steps, -1, 3), v, np.array(stats).reshape(steps, 6)
