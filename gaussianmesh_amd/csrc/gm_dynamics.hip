// gm_dynamics.hip -- secondary motion of a proxy mesh (gm_mesh_dynamics): T implicit-Euler steps of an elastic mesh whose potential is the
// ARAP energy, solved by the local/global iteration of projective dynamics (Bouaziz, Martin, Liu, Kavan & Pauly, "Projective Dynamics:
// Fusing Constraint Projections for Fast Simulation", SIGGRAPH 2014, with the vertex-star energy of Sorkine & Alexa 2007 as the constraint
// set).  The reference has no such stage; the result is defined by arithmetic.
//
// DEFINITION.  The CSR, weights w_ij and rest vertices p of gm_arap_solve; mass_i > 0; held rows (held[i] != 0, and rows whose weights sum to
// 0); handle rows (held rows whose position is scripted: handle_targets[t] in step t); the state (x, v), float32, read as float64.  With
// h = dt, k = stiffness, g = damping, a = gravity, step t takes (x, v) to (x', v'):
//   y_i = x_i + h v_i + h^2 a                                  the prediction
//   X_i = y_i on free rows, handle_targets[t] on handle rows, x_i on the other held rows
//   `iterations` times:  R_i = arap_rotation(S_i), S_i = sum_j w_ij (X_i - X_j)(p_i - p_j)^T        (the local step of gm_arap.hip)
//                        for every free row and coordinate   mu_i X_i + sum_j w_ij (X_i - X_j) = mu_i y_i + sum_j (w_ij / 2)(R_i + R_j)(p_i - p_j),
//                        mu_i = mass_i / (2 k h^2): Jacobi-preconditioned CG (diagonal mu_i + d_i) warm-started from X, stopped at
//                        |r| <= cg_tolerance |b|, at p . A p <= 0 or after cg_iterations steps (arap_global_kernel's rules)
//   x' = float32(X);  v'_i = float32((1 - g)(X_i - x_i) / h) on free rows, float32((X_i - x_i) / h) on held rows
// - the local/global minimisation of sum_i mass_i / (2 h^2) |X_i - y_i|^2 + (k / 2) E_arap(X, R).  The matrix diag(mu) + L is positive
// definite with no held row at all: a free body is a valid input.  (x', v') are rounded to float32 at EVERY step boundary, so a call of T
// steps is bit for bit T calls of one step.
//
// KERNELS.  dyn_init (the state into the float64 columns, mu, the diagonal, which rows are unknowns, the first prediction), dyn_handles (the
// handle rows of the first start column), then per step 2 * iterations launches and none per CG step:
//   dyn_local    one thread per vertex: S_i, R_i - a copy of arap_local_kernel's row body (see dyn_local_row).
//   dyn_global   3 workgroups of 1024 threads, one per coordinate: the column of the right-hand side, then the WHOLE PCG of that column
//                (arap_pcg_steps<true>: the step loop of arap_global_kernel with the operator's extra diagonal mu).  The prediction is
//                separable by coordinate, so the launch of a step's LAST iteration also closes the step for its own coordinate: it writes
//                x', v' (X_out, the float64 state columns, v_out in the last step), the next step's y and start column, and the next
//                step's handle targets.  No workgroup reads what another wrote in the same launch.
// Sums in a fixed order (arap_block_sum), no atomics: the same bits from call to call.  One workgroup per column keeps the nine state
// columns of a proxy mesh (7.5 k vertices: 60 KB each) in L2; a whole-chip global step for meshes far above that is not built.
// CONTACT (gm_mesh_dynamics_contact, gm_mesh_dynamics_field; the block further down) is the same step with other kernels in the same two
// slots, each pair of kernels one templated source: dyn_contact_local / dyn_field_local are dyn_contact_local_body<FIELD> over the one
// contact row dyn_contact_row<FIELD>, and dyn_global / dyn_contact_global are dyn_global_body<CONTACT>.  Every kernel symbol is a one-line
// wrapper with a name and signature of its own, so two builds compare symbol by symbol (tools/kernel_disasm.sh).
// MOVING FIELDS (gm_mesh_dynamics_fields; the last block of kernels) add a third local kernel, dyn_fields_local: the same local body
// (dyn_contact_local_rows) over dyn_fields_contact_row, which samples up to four grids, each in its own posed frame, and carries the
// friction anchor with the obstacle; the row's tail (dyn_contact_target) is shared with dyn_contact_row.
// Conventions of gm_closest.hip: caller workspace, stream-ordered, no device allocation, no host wait anywhere in this file.
#include <math.h>
#include "gm_common.h"
#include "gm_check.h"
#include "gm_mat3.h"
#include "gm_arap_shared.h"
#include "gm_sdf.h"

namespace gm {

#define DYN_THREADS 1024      // dyn_global: one workgroup of ARAP_WAVES waves
#define DYN_ROW_THREADS 256   // dyn_init / dyn_handles / dyn_local: one thread per vertex (per handle)

struct DynWs {
  double* x;       // [3][Vm] the iterate X, one column per coordinate
  double* r;       // [3][Vm]
  double* p;       // [3][Vm]
  double* q;       // [3][Vm]
  double* y;       // [3][Vm] the step's prediction
  double* xs;      // [3][Vm] the state x at the step's start (float32 values)
  double* vs;      // [3][Vm] the state v at the step's start (float32 values)
  double* R;       // [3][Vm][3]: row c of R_i at (c Vm + i) 3
  double* mu;      // [Vm] mass_i / (2 k h^2)
  double* diag;    // [Vm] mu_i + sum_j w_ij
  int* free_row;   // [Vm] 1 = a row of the linear system
  char* end;
  static DynWs from(void* ws, size_t Vm) {
    char* p = reinterpret_cast<char*>(ws);
    DynWs k;
    k.x = carve<double>(p, 3 * Vm); k.r = carve<double>(p, 3 * Vm); k.p = carve<double>(p, 3 * Vm); k.q = carve<double>(p, 3 * Vm);
    k.y = carve<double>(p, 3 * Vm); k.xs = carve<double>(p, 3 * Vm); k.vs = carve<double>(p, 3 * Vm);
    k.R = carve<double>(p, 9 * Vm);
    k.mu = carve<double>(p, Vm); k.diag = carve<double>(p, Vm);
    k.free_row = carve<int>(p, Vm);
    k.end = p;
    return k;
  }
};

// y = x + h v + h^2 a with one spelled-out rounding order: dyn_init and dyn_global's step end must give the same bits
__device__ __forceinline__ double dyn_predict(double x, double v, double h, double h2a) { return fma(h, v, x) + h2a; }

struct DynGravity { double h2a[3]; };   // h^2 a per coordinate

__global__ __launch_bounds__(DYN_ROW_THREADS) void dyn_init_kernel(int Vm, const int* __restrict__ row_offsets, const double* __restrict__ weights,
                                                                   const double* __restrict__ mass, const unsigned char* __restrict__ held,
                                                                   const float* __restrict__ x_in, const float* v_in, double two_k_h2, double h,
                                                                   DynGravity grav, double* __restrict__ x, double* __restrict__ y,
                                                                   double* __restrict__ xs, double* __restrict__ vs, double* __restrict__ mu,
                                                                   double* __restrict__ diag, int* __restrict__ free_row) {
  const int i = blockIdx.x * DYN_ROW_THREADS + threadIdx.x;
  if (i >= Vm) return;
  const ArapRowSum row = arap_row_sum(row_offsets, weights, held, i);
  const double m = mass[i] / two_k_h2;
  mu[i] = m;
  diag[i] = m + row.d;
  free_row[i] = row.free_row;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const size_t o = (size_t)c * Vm + i;
    const double xi = (double)x_in[3 * (size_t)i + c], vi = (double)v_in[3 * (size_t)i + c];
    const double yi = dyn_predict(xi, vi, h, grav.h2a[c]);
    xs[o] = xi; vs[o] = vi; y[o] = yi;
    x[o] = row.free_row ? yi : xi;
  }
}

// the handle rows of the first step's start column (behind dyn_init: another thread wrote x_i there)
__global__ __launch_bounds__(DYN_ROW_THREADS) void dyn_handles_kernel(int Vm, int H, const int* __restrict__ handle_ids,
                                                                      const float* __restrict__ targets, double* __restrict__ x) {
  const int k = blockIdx.x * DYN_ROW_THREADS + threadIdx.x;
  if (k >= H) return;
  const int i = clamp_index(handle_ids[k], Vm);
#pragma unroll
  for (int c = 0; c < 3; c++) x[(size_t)c * Vm + i] = (double)targets[3 * (size_t)k + c];
}

// the local step of row i: S_i = sum_j w_ij (x_i - x_j)(p_i - p_j)^T from the float64 columns x ([3][Vm]), its rotation into R.  A copy of
// arap_local_kernel's row body (gm_arap.hip): moved into gm_arap_shared.h and called from both, that kernel compiled to other code (the
// operands of its multiply-adds changed places), and the solver's kernels are to stay the code they are.
__device__ __forceinline__ void dyn_local_row(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                               const double* __restrict__ weights, const float* __restrict__ V0, const double* __restrict__ x,
                                               double* __restrict__ R, int i) {
  double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, Q[3][3];
  const double pi[3] = {(double)V0[3 * (size_t)i], (double)V0[3 * (size_t)i + 1], (double)V0[3 * (size_t)i + 2]};
  const double xi[3] = {x[i], x[(size_t)Vm + i], x[2 * (size_t)Vm + i]};
  for (int k = row_offsets[i]; k < row_offsets[i + 1]; k++) {
    const int j = clamp_index(cols[k], Vm);
    const double w = weights[k];
    double e[3], d[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { e[c] = pi[c] - (double)V0[3 * (size_t)j + c]; d[c] = xi[c] - x[(size_t)c * Vm + j]; }
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) S[a][b] += w * d[a] * e[b];
  }
  arap_rotation(S, Q);
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int k = 0; k < 3; k++) R[((size_t)c * Vm + i) * 3 + k] = Q[c][k];
}

__global__ __launch_bounds__(DYN_ROW_THREADS) void dyn_local_kernel(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                                    const double* __restrict__ weights, const float* __restrict__ V0,
                                                                    const double* __restrict__ x, double* __restrict__ R) {
  const int i = blockIdx.x * DYN_ROW_THREADS + threadIdx.x;
  if (i >= Vm) return;
  dyn_local_row(Vm, row_offsets, cols, weights, V0, x, R, i);
}

// what closes a step (X_out != null: the launch of the step's last iteration)
struct DynStepEnd {
  float* X_out;                // [Vm][3] this step's row of X_out; null: not the step's last iteration
  float* v_out;                // [Vm][3], or null: not the call's last step
  double* stats_row;           // [6], or null
  const float* next_targets;   // [H][3] the next step's handle targets; null: none (the last step, or H == 0)
  const int* handle_ids;
  int H;
  double h, keep;              // dt, 1 - damping
  DynGravity grav;
};

// workgroup c: column c of the right-hand side, r and p with it in the one edge loop, the whole PCG of that column (arap_pcg_steps with
// the diagonal mu), and in a step's last iteration the step's end for this coordinate.  CONTACT (dyn_contact_global_kernel, below): the
// operator's diagonal part is shift = mu + kappa instead of mu, diag is its Jacobi diagonal, and the right-hand side gains kappa_i c_i;
// without it kappa, shift and ctall are not read, and dyn_global_kernel is the code it was before the body became a template.
static_assert(DYN_THREADS == ARAP_WAVES * 64, "dyn_global_kernel strides its rows as arap_pcg_steps does");
template <bool CONTACT>
__device__ __forceinline__ void dyn_global_body(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                const double* __restrict__ weights, const float* __restrict__ V0,
                                                const double* __restrict__ Rall, const double* __restrict__ mu,
                                                const double* __restrict__ kappa, const double* __restrict__ shift,
                                                const double* __restrict__ diag, const double* __restrict__ ctall,
                                                const int* __restrict__ free_row, double* xall, double* rall, double* pall, double* qall,
                                                double* yall, double* xsall, double* vsall, int cg_iterations, double tol2,
                                                const DynStepEnd& end, double (*partA)[ARAP_WAVES], double (*partB)[ARAP_WAVES]) {
  const int c = blockIdx.x;
  const double* R = Rall + (size_t)c * Vm * 3;
  double* x = xall + (size_t)c * Vm;
  double* r = rall + (size_t)c * Vm;
  double* p = pall + (size_t)c * Vm;
  double* q = qall + (size_t)c * Vm;
  double* y = yall + (size_t)c * Vm;
  double s3[3] = {0.0, 0.0, 0.0};                                  // |b|^2, |r|^2, r . z
  for (int i = threadIdx.x; i < Vm; i += DYN_THREADS) {
    double ri = 0.0, zi = 0.0;
    if (free_row[i]) {
      const double Ri[3] = {R[3 * (size_t)i], R[3 * (size_t)i + 1], R[3 * (size_t)i + 2]};
      const double xi = x[i], mi = mu[i];
      double b = 0.0, Lx = 0.0, bc = 0.0;
      for (int k = row_offsets[i]; k < row_offsets[i + 1]; k++) {
        const int j = clamp_index(cols[k], Vm);
        const double w = weights[k], xj = x[j];
        double t = 0.0;
#pragma unroll
        for (int a = 0; a < 3; a++) t += (Ri[a] + R[3 * (size_t)j + a]) * ((double)V0[3 * (size_t)i + a] - (double)V0[3 * (size_t)j + a]);
        b += 0.5 * w * t;
        Lx += w * (xi - xj);
        if (!free_row[j]) bc += w * xj;                            // a held neighbour moves to the right-hand side
      }
      b += mi * y[i];
      if constexpr (CONTACT) b += kappa[i] * ctall[(size_t)c * Vm + i];
      bc += b;
      if constexpr (CONTACT) ri = b - (shift[i] * xi + Lx);
      else ri = b - (mi * xi + Lx);
      zi = ri / diag[i];
      s3[0] += bc * bc; s3[1] += ri * ri; s3[2] += ri * zi;
    }
    r[i] = ri; p[i] = zi;                                          // held rows: r = p = 0, for the whole solve
  }
  const ArapPcgResult cg = arap_pcg_steps<true>(Vm, row_offsets, cols, weights, diag, free_row, x, r, p, q, cg_iterations, tol2, s3, partA, partB,
                                                CONTACT ? shift : mu);
  if (!end.X_out) return;
  // the step's end: each thread reads back its own rows of x
  double* xs = xsall + (size_t)c * Vm;
  double* vs = vsall + (size_t)c * Vm;
  for (int i = threadIdx.x; i < Vm; i += DYN_THREADS) {
    const double X = x[i], d = (X - xs[i]) / end.h;
    const int fr = free_row[i];
    const float xf = (float)X, vf = (float)(fr ? end.keep * d : d);
    end.X_out[3 * (size_t)i + c] = xf;
    if (end.v_out) end.v_out[3 * (size_t)i + c] = vf;
    const double xn = (double)xf, vn = (double)vf, yn = dyn_predict(xn, vn, end.h, end.grav.h2a[c]);
    xs[i] = xn; vs[i] = vn; y[i] = yn;
    x[i] = fr ? yn : xn;
  }
  if (end.stats_row && threadIdx.x == 0) {
    end.stats_row[c] = (double)cg.used;
    end.stats_row[3 + c] = arap_rel_residual(cg.bb, cg.rr);
  }
  if (!end.next_targets) return;                                   // uniform
  __syncthreads();                                                 // a handle row's x was written by the row's thread above
  for (int k = threadIdx.x; k < end.H; k += DYN_THREADS) x[clamp_index(end.handle_ids[k], Vm)] = (double)end.next_targets[3 * (size_t)k + c];
}

__global__ __launch_bounds__(DYN_THREADS) void dyn_global_kernel(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                                 const double* __restrict__ weights, const float* __restrict__ V0,
                                                                 const double* __restrict__ Rall, const double* __restrict__ mu,
                                                                 const double* __restrict__ diag, const int* __restrict__ free_row, double* xall,
                                                                 double* rall, double* pall, double* qall, double* yall, double* xsall,
                                                                 double* vsall, int cg_iterations, double tol2, DynStepEnd end) {
  __shared__ double partA[1][ARAP_WAVES], partB[3][ARAP_WAVES];
  dyn_global_body<false>(Vm, row_offsets, cols, weights, V0, Rall, mu, nullptr, nullptr, diag, nullptr, free_row, xall, rall, pall, qall, yall, xsall, vsall,
                         cg_iterations, tol2, end, partA, partB);
}

// ---------------------------------------------------------------------------------------------
// CONTACT (gm_mesh_dynamics_contact; INTEGRATION.md section AB): unilateral contact of the free rows with K analytic colliders, as a
// penalty in projective-dynamics form.  Collider k of step t is row (t K + k) of collider_rows: kind 0 a half-space (nx, ny, nz, d),
// phi = n . x - d, normal n as given; kind 1 a sphere (cx, cy, cz, r), phi = |x - c| - r, normal (x - c) / |x - c|, (0, 1, 0) at the
// centre; any other kind is never chosen.  In every iteration, at the iterate X the local step read, free row i takes the collider k* of
// the smallest phi (`phi < best` from best = +inf: ties to the lowest k, a NaN never), is ACTIVE iff phi* < 0, and then adds
// kappa_i = mu_i (kc h^2) to its diagonal and kappa_i c_i to its right-hand side, c_i = X_i - phi* n - scale t, with u = X_i - xs_i,
// t = u - (n . u) n, lim = friction_k* |phi*|, scale = |t| <= lim ? 1 : lim / |t|: the normal part of c_i is the surface point, the
// tangential part pulls back to where the row was at the step's start, capped by Coulomb's cone.  Inactive, held and handle rows:
// kappa_i = 0.  The rounding order is dyn_contact_phi's and dyn_contact_row's, spelled out there.
// FIELD CONTACT (gm_mesh_dynamics_field; INTEGRATION.md section AC): the same, with a prepared signed-distance grid (gm_sdf.hip), static
// over the call, as candidate K behind the K analytic colliders: (phi, n) = sdf_sample(grid, X), taken with the same phi < best, so a tie
// goes to the analytic collider and a NaN - a row outside the grid, next to an unknown sample, on a gradient without a direction - is
// never chosen.  The winner's (phi, n, friction) go through the one tail of dyn_contact_row; contact_out is 1 + K for the field.
// KERNELS.  dyn_contact_local / dyn_field_local (dyn_contact_local_body<FIELD>: dyn_local_row, then the row's contact
// dyn_contact_row<FIELD>: kappa, mu + kappa, mu + kappa + d, c into the workspace, and contact_out in a step's last iteration) and, for
// both, dyn_contact_global (dyn_global_body<true>: dyn_global_kernel's source with the effective diagonal and shift and kappa_i c_i on
// the right-hand side; dyn_global_kernel, the <false> instantiation, kept its code).  A step stays 2 * iterations launches; no workgroup
// reads what another wrote in the same launch; no atomics.

struct DynContactWs {
  double* kappa;   // [Vm] mu_i kc h^2 on active rows, 0 elsewhere
  double* shift;   // [Vm] mu_i + kappa_i
  double* diag;    // [Vm] (mu_i + kappa_i) + d_i
  double* c;       // [3][Vm] the contact targets, 0 on inactive rows
  char* end;
  static DynContactWs from(char* p, size_t Vm) {
    DynContactWs k;
    k.kappa = carve<double>(p, Vm); k.shift = carve<double>(p, Vm); k.diag = carve<double>(p, Vm); k.c = carve<double>(p, 3 * Vm);
    k.end = p;
    return k;
  }
};

struct DynColliders {
  int K;
  const int* kind;          // [K]
  const float* rows;        // [K][4] this step's
  const double* friction;   // [K]
  double kch2;              // contact_stiffness h^2
  int* contact_out;         // [Vm] this step's row of contact_out; null: not wanted, or not the step's last iteration
};

// phi of collider (kind, row) at X, in this order: half-space  fma(nz, X2, fma(ny, X1, nx X0)) - d;  sphere  e = X - c per coordinate,
// s = sqrt(fma(e2, e2, fma(e1, e1, e0 e0))), s - r.  NaN for a kind that is neither.
__device__ __forceinline__ double dyn_contact_phi(int kind, const float* __restrict__ row, const double (&X)[3]) {
  const double a = (double)row[0], b = (double)row[1], c = (double)row[2], d = (double)row[3];
  if (kind == 0) return fma(c, X[2], fma(b, X[1], a * X[0])) - d;
  if (kind == 1) {
    const double e0 = X[0] - a, e1 = X[1] - b, e2 = X[2] - c;
    return sqrt(fma(e2, e2, fma(e1, e1, e0 * e0))) - d;
  }
  return (double)NAN;
}

struct DynField {
  SdfGrid grid;
  double friction;
};

// the tail of a contact row: the target c of an active row from the winner's (phi, n, friction) and the friction anchor xs (the u .. c
// lines of dyn_contact_row's comment), shared with dyn_fields_contact_row
__device__ __forceinline__ void dyn_contact_target(const double (&X)[3], const double (&xs)[3], const double (&n)[3], double phi, double friction,
                                                   double (&c)[3]) {
  const double u[3] = {X[0] - xs[0], X[1] - xs[1], X[2] - xs[2]};
  const double nu = fma(n[2], u[2], fma(n[1], u[1], n[0] * u[0]));
  const double t[3] = {fma(-nu, n[0], u[0]), fma(-nu, n[1], u[1]), fma(-nu, n[2], u[2])};
  const double s = sqrt(fma(t[2], t[2], fma(t[1], t[1], t[0] * t[0])));
  const double lim = friction * fabs(phi);
  const double scale = s <= lim ? 1.0 : lim / s;
#pragma unroll
  for (int a = 0; a < 3; a++) c[a] = fma(-scale, t[a], fma(-phi, n[a], X[a]));
}

// The contact of one free row at the iterate X with the step's start xs: returns 1 + k* if the row is active (0 if not) and then its
// target in c.  FIELD: fld's grid is candidate K; without it fld is not read.  The order of every rounding:
//   phi_k      dyn_contact_phi, k ascending, kept iff phi_k < best
//   phi_K      FIELD only: sdf_sample (gm_sdf.h), behind the colliders, kept iff phi_K < best
//   n          the half-space's row as given; the sphere's e / s per coordinate with e, s as in dyn_contact_phi ((0, 1, 0) at s == 0);
//              the field's as sdf_sample gives it
//   u = X - xs per coordinate;  nu = fma(n2, u2, fma(n1, u1, n0 u0));  t = fma(-nu, n, u) per coordinate
//   s = sqrt(fma(t2, t2, fma(t1, t1, t0 t0)));  lim = friction fabs(phi);  scale = s <= lim ? 1 : lim / s
//   c = (X - phi n) - scale t per coordinate: two fused multiply-adds, the inner one first
template <bool FIELD>
__device__ __forceinline__ int dyn_contact_row(const DynColliders& col, const DynField& fld, const double (&X)[3], const double (&xs)[3], double (&c)[3]) {
  double best = (double)INFINITY;
  int which = -1;
  for (int k = 0; k < col.K; k++) {                                  // uniform addresses: every thread reads collider k
    const double phi = dyn_contact_phi(col.kind[k], col.rows + 4 * k, X);
    if (phi < best) { best = phi; which = k; }
  }
  double n[3] = {0.0, 0.0, 0.0}, friction = 0.0;
  if constexpr (FIELD) {
    const double fphi = sdf_sample(fld.grid, X, n);
    if (fphi < best) { best = fphi; which = col.K; }
    friction = fld.friction;
  }
  if (!(best < 0.0)) return 0;                                       // (which >= 0 here: best left +inf)
  if (!FIELD || which < col.K) {                                     // an analytic collider won
    const float* row = col.rows + 4 * which;
    n[0] = (double)row[0]; n[1] = (double)row[1]; n[2] = (double)row[2];
    if (col.kind[which] == 1) {
      const double e[3] = {X[0] - n[0], X[1] - n[1], X[2] - n[2]};
      const double s = sqrt(fma(e[2], e[2], fma(e[1], e[1], e[0] * e[0])));
      if (s == 0.0) { n[0] = 0.0; n[1] = 1.0; n[2] = 0.0; }
      else { n[0] = e[0] / s; n[1] = e[1] / s; n[2] = e[2] / s; }
    }
    friction = col.friction[which];
  }
  dyn_contact_target(X, xs, n, best, friction, c);
  return 1 + which;
}

// dyn_local_row, then row i's contact - contact_row(X, xs, c), one of the row functions - into the workspace
template <class ContactRow>
__device__ __forceinline__ void dyn_contact_local_rows(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                        const double* __restrict__ weights, const float* __restrict__ V0,
                                                        const double* __restrict__ x, const double* __restrict__ xs,
                                                        const double* __restrict__ mu, const int* __restrict__ free_row,
                                                        double* __restrict__ R, const DynColliders& col, ContactRow contact_row,
                                                        double* __restrict__ kappa, double* __restrict__ shift, double* __restrict__ diag,
                                                        double* __restrict__ ct) {
  const int i = blockIdx.x * DYN_ROW_THREADS + threadIdx.x;
  if (i >= Vm) return;
  dyn_local_row(Vm, row_offsets, cols, weights, V0, x, R, i);
  double d = 0.0;                                                    // arap_row_sum's order: with kappa = 0 the diagonal is dyn_init's
  for (int k = row_offsets[i]; k < row_offsets[i + 1]; k++) d += weights[k];
  const double m = mu[i];
  double c[3] = {0.0, 0.0, 0.0}, kap = 0.0;
  int hit = 0;
  if (free_row[i]) {
    const double X[3] = {x[i], x[(size_t)Vm + i], x[2 * (size_t)Vm + i]};
    const double s[3] = {xs[i], xs[(size_t)Vm + i], xs[2 * (size_t)Vm + i]};
    hit = contact_row(X, s, c);
    if (hit) kap = m * col.kch2;
    else c[0] = c[1] = c[2] = 0.0;
  }
  kappa[i] = kap;
  shift[i] = m + kap;
  diag[i] = (m + kap) + d;
#pragma unroll
  for (int a = 0; a < 3; a++) ct[(size_t)a * Vm + i] = c[a];
  if (col.contact_out) col.contact_out[i] = hit;
}

template <bool FIELD>
__device__ __forceinline__ void dyn_contact_local_body(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                        const double* __restrict__ weights, const float* __restrict__ V0,
                                                        const double* __restrict__ x, const double* __restrict__ xs,
                                                        const double* __restrict__ mu, const int* __restrict__ free_row,
                                                        double* __restrict__ R, const DynColliders& col, const DynField& fld,
                                                        double* __restrict__ kappa, double* __restrict__ shift, double* __restrict__ diag,
                                                        double* __restrict__ ct) {
  dyn_contact_local_rows(Vm, row_offsets, cols, weights, V0, x, xs, mu, free_row, R, col,
                         [&](const double (&X)[3], const double (&s)[3], double (&c)[3]) { return dyn_contact_row<FIELD>(col, fld, X, s, c); },
                         kappa, shift, diag, ct);
}

__global__ __launch_bounds__(DYN_ROW_THREADS) void dyn_contact_local_kernel(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                                            const double* __restrict__ weights, const float* __restrict__ V0,
                                                                            const double* __restrict__ x, const double* __restrict__ xs,
                                                                            const double* __restrict__ mu, const int* __restrict__ free_row,
                                                                            double* __restrict__ R, DynColliders col, double* __restrict__ kappa,
                                                                            double* __restrict__ shift, double* __restrict__ diag,
                                                                            double* __restrict__ ct) {
  dyn_contact_local_body<false>(Vm, row_offsets, cols, weights, V0, x, xs, mu, free_row, R, col, DynField(), kappa, shift, diag, ct);
}

// dyn_global_body with the contact terms: shift = mu + kappa is the operator's diagonal part (diag its Jacobi diagonal), the right-hand
// side gains kappa_i c_i
__global__ __launch_bounds__(DYN_THREADS) void dyn_contact_global_kernel(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                                         const double* __restrict__ weights, const float* __restrict__ V0,
                                                                         const double* __restrict__ Rall, const double* __restrict__ mu,
                                                                         const double* __restrict__ kappa, const double* __restrict__ shift,
                                                                         const double* __restrict__ diag, const double* __restrict__ ctall,
                                                                         const int* __restrict__ free_row, double* xall, double* rall, double* pall,
                                                                         double* qall, double* yall, double* xsall, double* vsall,
                                                                         int cg_iterations, double tol2, DynStepEnd end) {
  __shared__ double partA[1][ARAP_WAVES], partB[3][ARAP_WAVES];
  dyn_global_body<true>(Vm, row_offsets, cols, weights, V0, Rall, mu, kappa, shift, diag, ctall, free_row, xall, rall, pall, qall, yall, xsall, vsall,
                        cg_iterations, tol2, end, partA, partB);
}

__global__ __launch_bounds__(DYN_ROW_THREADS) void dyn_field_local_kernel(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                                          const double* __restrict__ weights, const float* __restrict__ V0,
                                                                          const double* __restrict__ x, const double* __restrict__ xs,
                                                                          const double* __restrict__ mu, const int* __restrict__ free_row,
                                                                          double* __restrict__ R, DynColliders col, DynField fld,
                                                                          double* __restrict__ kappa, double* __restrict__ shift,
                                                                          double* __restrict__ diag, double* __restrict__ ct) {
  dyn_contact_local_body<true>(Vm, row_offsets, cols, weights, V0, x, xs, mu, free_row, R, col, fld, kappa, shift, diag, ct);
}

// ---------------------------------------------------------------------------------------------
// MOVING FIELDS (gm_mesh_dynamics_fields; INTEGRATION.md section AG): up to GM_MESH_FIELDS_MAX prepared grids, each under a rigid pose
// (R | t), world = R local + t, of its own per step: `now` is the pose during this step (row t + 1 of field_poses), `before` the one of
// the step before (row t; row 0: at the state's time).  Field f is candidate K + f behind the analytic colliders.  One more local kernel,
// dyn_fields_local (dyn_contact_local_rows over dyn_fields_contact_row); the global kernel is dyn_contact_global itself.  The poses are
// read at addresses the whole wave shares; the grids' descriptions travel in the kernel's arguments and are indexed by unrolled loops,
// so nothing goes through scratch.
struct DynFields {
  int F;
  SdfGrid grid[GM_MESH_FIELDS_MAX];
  double friction[GM_MESH_FIELDS_MAX];
  const double* before;   // [F][3][4]
  const double* now;      // [F][3][4]
};

// the normal of analytic collider `which` at X into n (the n lines of dyn_contact_row's comment, and a copy of its code: called from
// there, dyn_contact_local_kernel compiled to other code - loads and moves changed places); returns its friction
__device__ __forceinline__ double dyn_collider_normal(const DynColliders& col, int which, const double (&X)[3], double (&n)[3]) {
  const float* row = col.rows + 4 * which;
  n[0] = (double)row[0]; n[1] = (double)row[1]; n[2] = (double)row[2];
  if (col.kind[which] == 1) {
    const double e[3] = {X[0] - n[0], X[1] - n[1], X[2] - n[2]};
    const double s = sqrt(fma(e[2], e[2], fma(e[1], e[1], e[0] * e[0])));
    if (s == 0.0) { n[0] = 0.0; n[1] = 1.0; n[2] = 0.0; }
    else { n[0] = e[0] / s; n[1] = e[1] / s; n[2] = e[2] / s; }
  }
  return col.friction[which];
}

// dyn_contact_row with the fields as candidates K .. K + F - 1.  The order of every rounding, beyond dyn_contact_row's (float64, no
// contraction; P = (R | t) = now[f], R_ab = P[4 a + b], t_a = P[4 a + 3]):
//   phi_k      dyn_contact_phi, k ascending, kept iff phi_k < best
//   d = X - t per coordinate: one subtraction;  Xl_a = fma(R_2a, d_2, fma(R_1a, d_1, R_0a d_0))                  (R^T d)
//   phi_K+f    sdf_sample(grid[f], Xl) with its normal nl, f ascending, kept iff phi_K+f < best
//   n          an analytic winner's: dyn_collider_normal;  field f's: n_a = fma(R_a2, nl_2, fma(R_a1, nl_1, R_a0 nl_0))    (R nl)
//   the anchor an analytic winner's: xs.  Field f's: xs itself if before[f] and now[f] compare equal in all twelve numbers; else, with
//              (Rb | tb) = before[f]:  e = xs - tb per coordinate;  q_a = fma(Rb_2a, e_2, fma(Rb_1a, e_1, Rb_0a e_0));
//              xs'_a = fma(R_a2, q_2, fma(R_a1, q_1, fma(R_a0, q_0, t_a)))
//   the rest   dyn_contact_target with the anchor in the place of xs
// Returns 1 + K + f for field f.  With an identity pose Xl = X and n = nl (products with 0 and 1 are exact), so the bits are
// dyn_contact_row<true>'s.
__device__ __forceinline__ int dyn_fields_contact_row(const DynColliders& col, const DynFields& fl, const double (&X)[3], const double (&xs)[3],
                                                      double (&c)[3]) {
#pragma clang fp contract(off)
  double best = (double)INFINITY;
  int which = -1;
  for (int k = 0; k < col.K; k++) {                                  // uniform addresses: every thread reads collider k
    const double phi = dyn_contact_phi(col.kind[k], col.rows + 4 * k, X);
    if (phi < best) { best = phi; which = k; }
  }
  double nl[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int f = 0; f < GM_MESH_FIELDS_MAX; f++) {
    if (f < fl.F) {                                                  // uniform
      const double* P = fl.now + 12 * f;
      const double d[3] = {X[0] - P[3], X[1] - P[7], X[2] - P[11]};
      double Xl[3], m[3];
#pragma unroll
      for (int a = 0; a < 3; a++) Xl[a] = fma(P[8 + a], d[2], fma(P[4 + a], d[1], P[a] * d[0]));
      const double phi = sdf_sample(fl.grid[f], Xl, m);
      if (phi < best) { best = phi; which = col.K + f; nl[0] = m[0]; nl[1] = m[1]; nl[2] = m[2]; }
    }
  }
  if (!(best < 0.0)) return 0;
  double n[3] = {0.0, 0.0, 0.0}, anchor[3] = {xs[0], xs[1], xs[2]}, friction = 0.0;
  if (which < col.K) friction = dyn_collider_normal(col, which, X, n);
#pragma unroll
  for (int f = 0; f < GM_MESH_FIELDS_MAX; f++) {
    if (which == col.K + f) {                                        // (which < K + F: only a field below F was a candidate)
      const double* P = fl.now + 12 * f;
      const double* B = fl.before + 12 * f;
#pragma unroll
      for (int a = 0; a < 3; a++) n[a] = fma(P[4 * a + 2], nl[2], fma(P[4 * a + 1], nl[1], P[4 * a] * nl[0]));
      friction = fl.friction[f];
      bool same = true;
#pragma unroll
      for (int j = 0; j < 12; j++) same = same && P[j] == B[j];
      if (!same) {                                                   // uniform
        const double e[3] = {xs[0] - B[3], xs[1] - B[7], xs[2] - B[11]};
        double q[3];
#pragma unroll
        for (int a = 0; a < 3; a++) q[a] = fma(B[8 + a], e[2], fma(B[4 + a], e[1], B[a] * e[0]));
#pragma unroll
        for (int a = 0; a < 3; a++) anchor[a] = fma(P[4 * a + 2], q[2], fma(P[4 * a + 1], q[1], fma(P[4 * a], q[0], P[4 * a + 3])));
      }
    }
  }
  dyn_contact_target(X, anchor, n, best, friction, c);
  return 1 + which;
}

__global__ __launch_bounds__(DYN_ROW_THREADS) void dyn_fields_local_kernel(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                                           const double* __restrict__ weights, const float* __restrict__ V0,
                                                                           const double* __restrict__ x, const double* __restrict__ xs,
                                                                           const double* __restrict__ mu, const int* __restrict__ free_row,
                                                                           double* __restrict__ R, DynColliders col, DynFields fl,
                                                                           double* __restrict__ kappa, double* __restrict__ shift,
                                                                           double* __restrict__ diag, double* __restrict__ ct) {
  dyn_contact_local_rows(Vm, row_offsets, cols, weights, V0, x, xs, mu, free_row, R, col,
                         [&](const double (&X)[3], const double (&s)[3], double (&c)[3]) { return dyn_fields_contact_row(col, fl, X, s, c); },
                         kappa, shift, diag, ct);
}

}  // namespace gm

// ---------------------------------------------------------------------------------------------
// the entry points (include/gmesh_hip.h): their refusals, then the launches
using namespace gm;

static bool dyn_finite(double v) { return v - v == 0.0; }

extern "C" {

size_t gm_mesh_dynamics_workspace_bytes(int Vm) {
  if (Vm < 1) return 0;
  return (size_t)DynWs::from(nullptr, (size_t)Vm).end + 256;
}

// the checks and launches of the three entries.  col == null: gm_mesh_dynamics; with col->K == 0 and no field the same launches, so the
// same bits.  fld != null (gm_mesh_dynamics_field; col is there too): the field's local kernel in every iteration, for every K.
// fls != null with fls->F > 0 (gm_mesh_dynamics_fields; col is there too, fld is not): the moving fields' local kernel, for every K; with
// F == 0 the launches of col alone.
struct DynContactArgs { int K; const int* kind; const float* rows; const double* friction; double kc; int* contact_out; };
struct DynFieldArgs { int nx, ny, nz; const float* origin; float voxel; const float* grid; double friction; };
struct DynFieldsArgs { int F; const gm_dynamics_field* fields; const double* poses; };

static int dyn_run(const char* fn, const DynContactArgs* col, const DynFieldArgs* fld, const DynFieldsArgs* fls, int T, int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0,
                   const double* mass, const unsigned char* held, int H, const int* handle_ids, const float* handle_targets, const float* x_in,
                   const float* v_in, double dt, double stiffness, double damping, double gx, double gy, double gz, int iterations, int cg_iterations,
                   double cg_tolerance, float* X_out, float* v_out, double* stats, void* workspace, size_t workspace_bytes, void* stream) {
  if (T < 1 || T > GM_MESH_DYNAMICS_STEPS_MAX) { set_error("%s: T = %d (1 .. %d)", fn, T, GM_MESH_DYNAMICS_STEPS_MAX); return GM_ERR_INVALID_ARG; }
  if (Vm < 1) { set_error("%s: Vm = %d (must be positive)", fn, Vm); return GM_ERR_INVALID_ARG; }
  if (H < 0 || H > Vm) { set_error("%s: H = %d (0 .. Vm = %d)", fn, H, Vm); return GM_ERR_INVALID_ARG; }
  if (!dyn_finite(dt) || !(dt > 0.0)) { set_error("%s: dt must be finite and positive", fn); return GM_ERR_INVALID_ARG; }
  if (!dyn_finite(stiffness) || !(stiffness > 0.0)) { set_error("%s: stiffness must be finite and positive", fn); return GM_ERR_INVALID_ARG; }
  if (!(damping >= 0.0) || !(damping < 1.0)) { set_error("%s: damping must lie in [0, 1)", fn); return GM_ERR_INVALID_ARG; }
  if (!dyn_finite(gx) || !dyn_finite(gy) || !dyn_finite(gz)) { set_error("%s: gravity must be finite", fn); return GM_ERR_INVALID_ARG; }
  const double two_k_h2 = 2.0 * stiffness * dt * dt;
  if (!dyn_finite(two_k_h2) || !(two_k_h2 > 0.0)) { set_error("%s: 2 stiffness dt^2 must be finite and positive", fn); return GM_ERR_INVALID_ARG; }
  if (iterations < 1) { set_error("%s: iterations = %d (at least 1)", fn, iterations); return GM_ERR_INVALID_ARG; }
  if (cg_iterations < 1) { set_error("%s: cg_iterations = %d (at least 1)", fn, cg_iterations); return GM_ERR_INVALID_ARG; }
  if (!(cg_tolerance >= 0.0) || !dyn_finite(cg_tolerance)) { set_error("%s: cg_tolerance must be finite and not negative", fn); return GM_ERR_INVALID_ARG; }
  const int K = col ? col->K : 0;
  if (col) {
    if (K < 0 || K > GM_MESH_CONTACT_COLLIDERS_MAX) { set_error("%s: K = %d (0 .. %d)", fn, K, GM_MESH_CONTACT_COLLIDERS_MAX); return GM_ERR_INVALID_ARG; }
    if (!dyn_finite(col->kc) || !(col->kc > 0.0)) { set_error("%s: contact_stiffness must be finite and positive", fn); return GM_ERR_INVALID_ARG; }
    if (K > 0 && (!col->kind || !col->rows || !col->friction)) { set_error("%s: null pointer (K = %d colliders)", fn, K); return GM_ERR_INVALID_ARG; }
  }
  if (fld) {
    if (int rc = check_sdf_grid(fn, fld->nx, fld->ny, fld->nz, fld->origin, fld->voxel, fld->grid)) return rc;
    if (!(fld->friction >= 0.0)) { set_error("%s: field_friction must not be negative", fn); return GM_ERR_INVALID_ARG; }
  }
  const int F = fls ? fls->F : 0;
  if (fls) {
    if (F < 0 || F > GM_MESH_FIELDS_MAX) { set_error("%s: F = %d (0 .. %d)", fn, F, GM_MESH_FIELDS_MAX); return GM_ERR_INVALID_ARG; }
    if (F > 0 && !fls->fields) { set_error("%s: null pointer (fields, F = %d)", fn, F); return GM_ERR_INVALID_ARG; }
    for (int f = 0; f < F; f++) {
      const gm_dynamics_field& g = fls->fields[f];
      if (int rc = check_sdf_grid(fn, g.nx, g.ny, g.nz, g.origin, g.voxel, g.grid)) return rc;
      if (!(g.friction >= 0.0)) { set_error("%s: the friction of field %d must not be negative", fn, f); return GM_ERR_INVALID_ARG; }
    }
    if (F > 0 && !fls->poses) { set_error("%s: null pointer (field_poses, F = %d)", fn, F); return GM_ERR_INVALID_ARG; }
  }
  if (!row_offsets || !cols || !weights || !V0 || !mass || !held || !x_in || !v_in || !X_out || !v_out || !workspace ||
      (H > 0 && (!handle_ids || !handle_targets))) {
    set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG;
  }
  // the inputs are only read and may alias one another; an output or the workspace meets nothing, except that v_out may be v_in (v_in
  // stands for both: it is read once, by the first launch)
  const size_t row = 12 * (size_t)Vm;
  ByteRange rg[17 + GM_MESH_FIELDS_MAX] = {{V0, row, "V0", false}, {mass, 8 * (size_t)Vm, "mass", false}, {held, (size_t)Vm, "held", false},
                            {H > 0 ? handle_ids : nullptr, 4 * (size_t)H, "handle_ids", false},
                            {H > 0 ? handle_targets : nullptr, 12 * (size_t)H * T, "handle_targets", false}, {x_in, row, "x_in", false},
                            {v_in, row, "v_in", v_out == v_in}, {X_out, row * T, "X_out", true}, {v_out == v_in ? nullptr : v_out, row, "v_out", true},
                            {stats, 48 * (size_t)T, "stats", true}, {workspace, workspace_bytes, "workspace", true},
                            {K > 0 ? col->kind : nullptr, 4 * (size_t)K, "collider_kind", false},
                            {K > 0 ? col->rows : nullptr, 16 * (size_t)K * T, "collider_rows", false},
                            {K > 0 ? col->friction : nullptr, 8 * (size_t)K, "collider_friction", false},
                            {col ? col->contact_out : nullptr, 4 * (size_t)Vm * T, "contact_out", true},
                            {fld ? fld->grid : nullptr, fld ? 16 * (size_t)fld->nx * fld->ny * fld->nz : 0, "field_grid", false},
                            {F > 0 ? fls->poses : nullptr, 96 * (size_t)F * ((size_t)T + 1), "field_poses", false}};
  static const char* const grid_names[GM_MESH_FIELDS_MAX] = {"the grid of field 0", "the grid of field 1", "the grid of field 2", "the grid of field 3"};
  for (int f = 0; f < F; f++) {                                       // (the entries past F stay empty: they overlap nothing)
    const gm_dynamics_field& g = fls->fields[f];
    rg[17 + f] = {g.grid, 16 * (size_t)g.nx * g.ny * g.nz, grid_names[f], false};
  }
  if (int rc = check_ranges(fn, rg)) return rc;
  const size_t need = col ? gm_mesh_dynamics_contact_workspace_bytes(Vm) : gm_mesh_dynamics_workspace_bytes(Vm);
  if (workspace_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need); return GM_ERR_BUFFER; }
  const DynWs k = DynWs::from(workspace, (size_t)Vm);
  const DynContactWs kc = DynContactWs::from(k.end, (size_t)Vm);   // (pointers only: not touched when K == 0)
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 rows((Vm + DYN_ROW_THREADS - 1) / DYN_ROW_THREADS), threads(DYN_ROW_THREADS);
  const DynGravity grav = {{dt * dt * gx, dt * dt * gy, dt * dt * gz}};
  hipLaunchKernelGGL(dyn_init_kernel, rows, threads, 0, s, Vm, row_offsets, weights, mass, held, x_in, v_in, two_k_h2, dt, grav, k.x, k.y, k.xs, k.vs, k.mu,
                     k.diag, k.free_row);
  if (H > 0) hipLaunchKernelGGL(dyn_handles_kernel, dim3((H + DYN_ROW_THREADS - 1) / DYN_ROW_THREADS), threads, 0, s, Vm, H, handle_ids, handle_targets, k.x);
  if (K == 0 && !fld && F == 0 && col && col->contact_out) GM_HIP(hipMemsetAsync(col->contact_out, 0, 4 * (size_t)Vm * T, s));
  const double tol2 = cg_tolerance * cg_tolerance;
  for (int t = 0; t < T; t++)
    for (int it = 0; it < iterations; it++) {
      DynStepEnd end = {nullptr, nullptr, nullptr, nullptr, handle_ids, H, dt, 1.0 - damping, grav};
      const bool last = it == iterations - 1;
      if (last) {
        end.X_out = X_out + 3 * (size_t)Vm * t;
        end.v_out = t == T - 1 ? v_out : nullptr;
        end.stats_row = stats ? stats + 6 * (size_t)t : nullptr;
        end.next_targets = (H > 0 && t + 1 < T) ? handle_targets + 3 * (size_t)H * (t + 1) : nullptr;
      }
      if (K == 0 && !fld && F == 0) {
        hipLaunchKernelGGL(dyn_local_kernel, rows, threads, 0, s, Vm, row_offsets, cols, weights, V0, k.x, k.R);
        hipLaunchKernelGGL(dyn_global_kernel, dim3(3), dim3(DYN_THREADS), 0, s, Vm, row_offsets, cols, weights, V0, k.R, k.mu, k.diag, k.free_row, k.x, k.r,
                           k.p, k.q, k.y, k.xs, k.vs, cg_iterations, tol2, end);
        continue;
      }
      const DynColliders dc = {K, col->kind, col->rows + 4 * (size_t)K * t, col->friction, col->kc * dt * dt,
                               (last && col->contact_out) ? col->contact_out + (size_t)Vm * t : nullptr};
      if (fld) {
        const DynField df = {{reinterpret_cast<const float4*>(fld->grid), fld->nx, fld->ny, fld->nz, {fld->origin[0], fld->origin[1], fld->origin[2]}, fld->voxel},
                             fld->friction};
        hipLaunchKernelGGL(dyn_field_local_kernel, rows, threads, 0, s, Vm, row_offsets, cols, weights, V0, k.x, k.xs, k.mu, k.free_row, k.R, dc, df,
                           kc.kappa, kc.shift, kc.diag, kc.c);
      } else if (F > 0) {
        DynFields df = {};
        df.F = F;
        for (int f = 0; f < F; f++) {
          const gm_dynamics_field& g = fls->fields[f];
          df.grid[f] = {reinterpret_cast<const float4*>(g.grid), g.nx, g.ny, g.nz, {g.origin[0], g.origin[1], g.origin[2]}, g.voxel};
          df.friction[f] = g.friction;
        }
        df.before = fls->poses + 12 * (size_t)F * t;
        df.now = df.before + 12 * (size_t)F;
        hipLaunchKernelGGL(dyn_fields_local_kernel, rows, threads, 0, s, Vm, row_offsets, cols, weights, V0, k.x, k.xs, k.mu, k.free_row, k.R, dc, df,
                           kc.kappa, kc.shift, kc.diag, kc.c);
      } else {
        hipLaunchKernelGGL(dyn_contact_local_kernel, rows, threads, 0, s, Vm, row_offsets, cols, weights, V0, k.x, k.xs, k.mu, k.free_row, k.R, dc, kc.kappa,
                           kc.shift, kc.diag, kc.c);
      }
      hipLaunchKernelGGL(dyn_contact_global_kernel, dim3(3), dim3(DYN_THREADS), 0, s, Vm, row_offsets, cols, weights, V0, k.R, k.mu, kc.kappa, kc.shift,
                         kc.diag, kc.c, k.free_row, k.x, k.r, k.p, k.q, k.y, k.xs, k.vs, cg_iterations, tol2, end);
    }
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_mesh_dynamics(int T, int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0, const double* mass,
                     const unsigned char* held, int H, const int* handle_ids, const float* handle_targets, const float* x_in, const float* v_in,
                     double dt, double stiffness, double damping, double gx, double gy, double gz, int iterations, int cg_iterations,
                     double cg_tolerance, float* X_out, float* v_out, double* stats, void* workspace, size_t workspace_bytes, void* stream) {
  return dyn_run("gm_mesh_dynamics", nullptr, nullptr, nullptr, T, Vm, row_offsets, cols, weights, V0, mass, held, H, handle_ids, handle_targets, x_in, v_in, dt, stiffness,
                 damping, gx, gy, gz, iterations, cg_iterations, cg_tolerance, X_out, v_out, stats, workspace, workspace_bytes, stream);
}

size_t gm_mesh_dynamics_contact_workspace_bytes(int Vm) {
  if (Vm < 1) return 0;
  return (size_t)DynContactWs::from(DynWs::from(nullptr, (size_t)Vm).end, (size_t)Vm).end + 256;
}

int gm_mesh_dynamics_contact(int T, int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0, const double* mass,
                             const unsigned char* held, int H, const int* handle_ids, const float* handle_targets, const float* x_in,
                             const float* v_in, double dt, double stiffness, double damping, double gx, double gy, double gz, int iterations,
                             int cg_iterations, double cg_tolerance, int K, const int* collider_kind, const float* collider_rows,
                             const double* collider_friction, double contact_stiffness, float* X_out, float* v_out, int* contact_out,
                             double* stats, void* workspace, size_t workspace_bytes, void* stream) {
  const DynContactArgs col = {K, collider_kind, collider_rows, collider_friction, contact_stiffness, contact_out};
  return dyn_run("gm_mesh_dynamics_contact", &col, nullptr, nullptr, T, Vm, row_offsets, cols, weights, V0, mass, held, H, handle_ids, handle_targets, x_in, v_in, dt,
                 stiffness, damping, gx, gy, gz, iterations, cg_iterations, cg_tolerance, X_out, v_out, stats, workspace, workspace_bytes, stream);
}

int gm_mesh_dynamics_field(int T, int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0, const double* mass,
                           const unsigned char* held, int H, const int* handle_ids, const float* handle_targets, const float* x_in, const float* v_in,
                           double dt, double stiffness, double damping, double gx, double gy, double gz, int iterations, int cg_iterations,
                           double cg_tolerance, int K, const int* collider_kind, const float* collider_rows, const double* collider_friction,
                           double contact_stiffness, int nx, int ny, int nz, const float* origin, float voxel, const float* field_grid,
                           double field_friction, float* X_out, float* v_out, int* contact_out, double* stats, void* workspace, size_t workspace_bytes,
                           void* stream) {
  const DynContactArgs col = {K, collider_kind, collider_rows, collider_friction, contact_stiffness, contact_out};
  const DynFieldArgs fld = {nx, ny, nz, origin, voxel, field_grid, field_friction};
  return dyn_run("gm_mesh_dynamics_field", &col, &fld, nullptr, T, Vm, row_offsets, cols, weights, V0, mass, held, H, handle_ids, handle_targets, x_in, v_in, dt,
                 stiffness, damping, gx, gy, gz, iterations, cg_iterations, cg_tolerance, X_out, v_out, stats, workspace, workspace_bytes, stream);
}

int gm_mesh_dynamics_fields(int T, int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0, const double* mass,
                            const unsigned char* held, int H, const int* handle_ids, const float* handle_targets, const float* x_in, const float* v_in,
                            double dt, double stiffness, double damping, double gx, double gy, double gz, int iterations, int cg_iterations,
                            double cg_tolerance, int K, const int* collider_kind, const float* collider_rows, const double* collider_friction,
                            double contact_stiffness, int F, const gm_dynamics_field* fields, const double* field_poses, float* X_out, float* v_out,
                            int* contact_out, double* stats, void* workspace, size_t workspace_bytes, void* stream) {
  const DynContactArgs col = {K, collider_kind, collider_rows, collider_friction, contact_stiffness, contact_out};
  const DynFieldsArgs fls = {F, fields, field_poses};
  return dyn_run("gm_mesh_dynamics_fields", &col, nullptr, &fls, T, Vm, row_offsets, cols, weights, V0, mass, held, H, handle_ids, handle_targets, x_in, v_in, dt,
                 stiffness, damping, gx, gy, gz, iterations, cg_iterations, cg_tolerance, X_out, v_out, stats, workspace, workspace_bytes, stream);
}

}  // extern "C"
