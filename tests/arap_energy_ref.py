"""The ARAP energy of a pose as a function of the pose alone, its gradient, and the one-ring smoothing sweep, restated in float64
numpy: the definition gm_arap_energy_grad and gm_mesh_smooth_rows are held to.  Built on arap_ref.Reference
(its weights, rotations, energy, rhs, L, deg, scale); numpy only.

    E(x)      = Reference.energy(x, R(x))
    R(x)      = Reference.rotations(x), except that a row whose pose edges x_i - x_j equal its rest edges p_i - p_j bit for bit takes
                the identity itself (its exact optimum; the SVD returns it to 1e-15), so that the rest pose has E = 0 and g = 0 exactly
    g_i(x)    = 4 sum_j w_ij [ (x_i - x_j) - (R_i + R_j)(p_i - p_j) / 2 ]      (= 4 (L x - Reference.rhs(R)), summed edge by edge)
                rows whose weights sum to 0 have no edge: 0
    sweep     y_i <- (g_i + lam sum_j w_ij y_j) / (1 + lam d_i)
"""
import numpy as np


def rotations(ref, X):
    X = np.asarray(X, np.float64)
    R = ref.rotations(X)
    moved = np.zeros(len(ref.V0), bool)
    np.logical_or.at(moved, ref.I, ((X[ref.I] - X[ref.J]) != ref.E0).any(axis=1))
    R[~moved] = np.eye(3)
    return R


def energy(ref, X, R=None):
    X = np.asarray(X, np.float64)
    return ref.energy(X, rotations(ref, X) if R is None else R)


def gradient(ref, X, R=None):
    """[Vm,3]: the partial derivative of Reference.energy in X at fixed R (R None: the minimising rotations, where it is the total one)"""
    X = np.asarray(X, np.float64)
    R = rotations(ref, X) if R is None else R
    term = (X[ref.I] - X[ref.J]) - 0.5 * np.einsum("nab,nb->na", R[ref.I] + R[ref.J], ref.E0)
    g = np.zeros_like(ref.V0)
    np.add.at(g, ref.I, ref.w[:, None] * term)
    return 4.0 * g


def value_and_grad(ref, X):
    X = np.asarray(X, np.float64)
    R = rotations(ref, X)
    return ref.energy(X, R), gradient(ref, X, R)


def smooth(ref, g, lam, sweeps):
    """the state after `sweeps` sweeps from y = g; g [Vm,k] float64"""
    g = np.asarray(g, np.float64)
    y = g.copy()
    den = 1.0 + lam * ref.deg
    for _ in range(int(sweeps)):
        y = (g + lam * (ref.W @ y)) / den[:, None]
    return y


def fold(flat, idx, line, angle):
    """the flat grid `flat` [n,3] (z = 0, columns of idx along x) folded rigidly by `angle` about the vertex line idx[line, :]: the
    vertices beyond the line turn about the y-parallel axis through it; no edge changes its length"""
    X = np.asarray(flat, np.float64).copy()
    x0 = X[idx[line, 0], 0]
    far = X[:, 0] > x0
    dx = X[far, 0] - x0
    X[far, 0] = x0 + dx * np.cos(angle)
    X[far, 2] = dx * np.sin(angle)
    return X
