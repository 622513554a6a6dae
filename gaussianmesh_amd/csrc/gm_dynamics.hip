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
// Conventions of gm_closest.hip: caller workspace, stream-ordered, no device allocation, no host wait anywhere in this file.
#include <math.h>
#include "gm_common.h"
#include "gm_check.h"
#include "gm_mat3.h"
#include "gm_arap_shared.h"

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
// the diagonal mu), and in a step's last iteration the step's end for this coordinate
static_assert(DYN_THREADS == ARAP_WAVES * 64, "dyn_global_kernel strides its rows as arap_pcg_steps does");
__global__ __launch_bounds__(DYN_THREADS) void dyn_global_kernel(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                                 const double* __restrict__ weights, const float* __restrict__ V0,
                                                                 const double* __restrict__ Rall, const double* __restrict__ mu,
                                                                 const double* __restrict__ diag, const int* __restrict__ free_row, double* xall,
                                                                 double* rall, double* pall, double* qall, double* yall, double* xsall,
                                                                 double* vsall, int cg_iterations, double tol2, DynStepEnd end) {
  __shared__ double partA[1][ARAP_WAVES], partB[3][ARAP_WAVES];
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
      bc += b;
      ri = b - (mi * xi + Lx); zi = ri / diag[i];
      s3[0] += bc * bc; s3[1] += ri * ri; s3[2] += ri * zi;
    }
    r[i] = ri; p[i] = zi;                                          // held rows: r = p = 0, for the whole solve
  }
  const ArapPcgResult cg = arap_pcg_steps<true>(Vm, row_offsets, cols, weights, diag, free_row, x, r, p, q, cg_iterations, tol2, s3, partA, partB, mu);
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

int gm_mesh_dynamics(int T, int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0, const double* mass,
                     const unsigned char* held, int H, const int* handle_ids, const float* handle_targets, const float* x_in, const float* v_in,
                     double dt, double stiffness, double damping, double gx, double gy, double gz, int iterations, int cg_iterations,
                     double cg_tolerance, float* X_out, float* v_out, double* stats, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "gm_mesh_dynamics";
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
  if (!row_offsets || !cols || !weights || !V0 || !mass || !held || !x_in || !v_in || !X_out || !v_out || !workspace ||
      (H > 0 && (!handle_ids || !handle_targets))) {
    set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG;
  }
  // the inputs are only read and may alias one another; an output or the workspace meets nothing, except that v_out may be v_in (v_in
  // stands for both: it is read once, by the first launch)
  const size_t row = 12 * (size_t)Vm;
  const ByteRange rg[11] = {{V0, row, "V0", false}, {mass, 8 * (size_t)Vm, "mass", false}, {held, (size_t)Vm, "held", false},
                            {H > 0 ? handle_ids : nullptr, 4 * (size_t)H, "handle_ids", false},
                            {H > 0 ? handle_targets : nullptr, 12 * (size_t)H * T, "handle_targets", false}, {x_in, row, "x_in", false},
                            {v_in, row, "v_in", v_out == v_in}, {X_out, row * T, "X_out", true}, {v_out == v_in ? nullptr : v_out, row, "v_out", true},
                            {stats, 48 * (size_t)T, "stats", true}, {workspace, workspace_bytes, "workspace", true}};
  if (int rc = check_ranges(fn, rg)) return rc;
  const size_t need = gm_mesh_dynamics_workspace_bytes(Vm);
  if (workspace_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need); return GM_ERR_BUFFER; }
  const DynWs k = DynWs::from(workspace, (size_t)Vm);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 rows((Vm + DYN_ROW_THREADS - 1) / DYN_ROW_THREADS), threads(DYN_ROW_THREADS);
  const DynGravity grav = {{dt * dt * gx, dt * dt * gy, dt * dt * gz}};
  hipLaunchKernelGGL(dyn_init_kernel, rows, threads, 0, s, Vm, row_offsets, weights, mass, held, x_in, v_in, two_k_h2, dt, grav, k.x, k.y, k.xs, k.vs, k.mu,
                     k.diag, k.free_row);
  if (H > 0) hipLaunchKernelGGL(dyn_handles_kernel, dim3((H + DYN_ROW_THREADS - 1) / DYN_ROW_THREADS), threads, 0, s, Vm, H, handle_ids, handle_targets, k.x);
  const double tol2 = cg_tolerance * cg_tolerance;
  for (int t = 0; t < T; t++)
    for (int it = 0; it < iterations; it++) {
      DynStepEnd end = {nullptr, nullptr, nullptr, nullptr, handle_ids, H, dt, 1.0 - damping, grav};
      if (it == iterations - 1) {
        end.X_out = X_out + 3 * (size_t)Vm * t;
        end.v_out = t == T - 1 ? v_out : nullptr;
        end.stats_row = stats ? stats + 6 * (size_t)t : nullptr;
        end.next_targets = (H > 0 && t + 1 < T) ? handle_targets + 3 * (size_t)H * (t + 1) : nullptr;
      }
      hipLaunchKernelGGL(dyn_local_kernel, rows, threads, 0, s, Vm, row_offsets, cols, weights, V0, k.x, k.R);
      hipLaunchKernelGGL(dyn_global_kernel, dim3(3), dim3(DYN_THREADS), 0, s, Vm, row_offsets, cols, weights, V0, k.R, k.mu, k.diag, k.free_row, k.x, k.r,
                         k.p, k.q, k.y, k.xs, k.vs, cg_iterations, tol2, end);
    }
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // extern "C"
