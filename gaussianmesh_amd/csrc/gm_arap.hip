// gm_arap.hip -- as-rigid-as-possible deformation of a proxy mesh from dragged handle vertices (gm_arap_solve, gm_arap_solve_grid): the stage that
// MAKES the deformed mesh gm_mesh_rs then reads (R, S) from.  The reference delegates it to pyACAP, a binary outside its tree;
// restated from the published algorithm (Sorkine & Alexa, "As-Rigid-As-Possible Surface Modeling", SGP 2007).
//
// DEFINITION.  Rest vertices p (float32, read as float64), symmetric positive edge weights w_ij (the caller's CSR: the clamped
// cotangent weights of mesh_rs_kernel, arap.edge_csr), unknown positions p'.
//   E(P', R) = sum_i sum_{j in N(i)} w_ij |(p'_i - p'_j) - R_i (p_i - p_j)|^2
//   local step:  S_i = sum_j w_ij (p'_i - p'_j)(p_i - p_j)^T,  R_i = U diag(1, 1, det(U V^T)) V^T for S_i = U Sigma V^T: the proper
//     rotation that maximises tr(R^T S_i).  Formed by the eigen-route of gm_mesh.hip: S^T S = E diag E^T gives the right singular
//     directions only; the two strongest columns S e_k are normalised (the second orthogonalised against the first), the third column
//     is their cross product and the third direction the cross product of the first two - so det R = +1 by construction and a planar
//     one-ring (rank-2 S_i) gets its unique rotation.  Second singular value <= 1e-12 of the first (rank <= 1): R_i = I.
//     WHAT IS GUARANTEED.  S^T S squares the condition number.  With singular values s0 >= s1 >= s2, d = det(U V^T) and
//     gap = (s1 + d s2) / s0:  gap >= 1e-2: R_i is the SVD's rotation element by element (to eps / gap^2) and loses at most 64 eps s0 of
//     tr(R^T S_i).  A one-ring whose second singular value is below about 1e-3 of the first (a needle), or a reflected one with
//     s1 ~ s2: R_i is a proper rotation that maximises tr(R^T S_i) only to within 8 sqrt(eps) s0 = 1.2e-7 s0 - it is NOT element by
//     element the SVD's rotation; the difference is a turn about the strongest direction (of any angle for s1 < 1e-8 s0) and costs E
//     at most twice that bar.  tests/polar_route_cases.py, test_gpu_polar_routes.py.
//   global step: for every free vertex  sum_j w_ij (p'_i - p'_j) = sum_j (w_ij / 2)(R_i + R_j)(p_i - p_j);  rows with fixed[i] != 0
//     (handles, pinned vertices) and rows whose weights sum to 0 keep their V_init position.
//   The three coordinate columns are independent systems with one symmetric positive definite matrix (the Laplacian restricted to
//   the free rows).  Each is solved by Jacobi-preconditioned conjugate gradients warm-started from the current positions and stopped
//   at |r|_2 <= cg_tolerance |b|_2 (b the right-hand side of the restricted system) or after cg_iterations steps.  CG minimises the
//   column's share of E over a growing subspace from the warm start, so no number of steps can raise E.
//
// KERNELS.  arap_init (positions to the float64 state, row sums), then per outer iteration TWO launches and none per CG step:
//   arap_local   one thread per vertex: S_i, R_i.
//   arap_global  3 workgroups of 1024 threads, one per coordinate; a workgroup forms its column of the right-hand side (it needs
//                the neighbours' R_j: hence a launch boundary after arap_local) and runs the WHOLE PCG of that column, rows strided
//                over the threads, x / r / p / q in the workspace (L2-resident: 7.5 k rows x 8 B).  No workgroup waits on another.
//                The step loop behind the right-hand side is arap_pcg_steps (gm_arap_shared.h), which gm_pose_interp.hip runs too.
//   Dot products: butterfly inside each wave, 16 wave partials in LDS, then EVERY thread adds the 16 in index order - all threads
//   hold the same bits, so the loop's exit tests are uniform, and the result is the same from run to run (no atomics anywhere).
//   With stats, arap_energy (one workgroup, same reduction) runs after the local and after the global step; without, E is never formed.
// A SECOND GLOBAL STEP (gm_arap_solve_grid, below arap_global_kernel) spreads the rows over ceil(Vm / 256) workgroups that meet only at
//   kernel boundaries: arap_grid_rhs once per outer iteration, then arap_grid_product + arap_grid_update per CG step.  Same definition,
//   same stopping rule, same stats; only the order of the sums differs.  init, local and energy kernels are shared.  No workgroup waits
//   on another there either, and the sums are again taken in a fixed order (of Vm alone), with no atomics.
// A BATCH (gm_arap_solve_batch) is the second grid dimension of every kernel: workgroup (., b) runs item b - its own V_init / V_out, stats
//   rows and workspace slab (state columns, R, slots, carry), `slab` doubles from item b - 1's - on the one mesh: CSR, weights, V0, diag
//   and free_row are shared (item 0's workgroups write the last two, in arap_init).  The single solves are a batch of one, through the
//   same kernels, the same workspace carve and the same host loop (arap_chain, with the column launch or the grid launch sequence as
//   its global step): an item's bits do not depend on the batch it rides in.  No workgroup reads what another item's wrote.
// THE ENERGY OF A POSE (gm_arap_energy_grad) and ONE-RING SMOOTHING of rows (gm_mesh_smooth_rows) are at the end of the namespace: E as a
//   function of the pose alone with its gradient, over ceil(Vm / 256) workgroups, and Jacobi sweeps of (I + lambda L) y = g - what an
//   optimiser of the vertices (pose_fit.py) takes as a rigidity term and as a preconditioner of its gradient.  They share arap_rotation,
//   arap_block_sum and arap_slot_sum with the solver and none of its kernels.  (arap_rotation, arap_row_sum, arap_block_sum,
//   arap_pcg_steps and arap_rel_residual live in gm_arap_shared.h: gm_pose_interp.hip uses them too.)
// Conventions of gm_closest.hip: caller workspace, stream-ordered, no device allocation, no host wait anywhere in this file.
#include "gm_common.h"
#include "gm_check.h"
#include "gm_mat3.h"
#include "gm_arap_shared.h"

namespace gm {

#define ARAP_THREADS 1024     // arap_global / arap_energy: one workgroup of 16 waves
#define ARAP_ROW_THREADS 256  // arap_init / arap_local: one thread per vertex

// B items (the single solve: B = 1): per item a slab of `slab` doubles (x, r, p, q, R), then the mesh's own diag and free_row once.  The
// pointers are item 0's; slab is a multiple of 256 bytes, so every item's arrays are aligned as item 0's.  The slabs come first so
// that x lies at the workspace's base whatever B (a single solve's arrays are where they were before there was a batch).
struct ArapWs {
  double* x;       // [3][Vm] positions, one column per coordinate
  double* r;       // [3][Vm]
  double* p;       // [3][Vm]
  double* q;       // [3][Vm]
  double* R;       // [3][Vm][3]: row c of R_i at (c Vm + i) 3
  size_t slab;
  double* diag;    // [Vm] sum_j w_ij
  int* free_row;   // [Vm] 1 = a row of the linear system
  char* end;
  static ArapWs from(void* ws, size_t Vm, size_t B) {
    char* p = reinterpret_cast<char*>(ws);
    ArapWs k;
    k.x = carve<double>(p, 3 * Vm); k.r = carve<double>(p, 3 * Vm); k.p = carve<double>(p, 3 * Vm); k.q = carve<double>(p, 3 * Vm);
    k.R = carve<double>(p, 9 * Vm);
    k.slab = (size_t)(carve<double>(p, 0) - k.x);
    p = reinterpret_cast<char*>(k.x + B * k.slab);
    k.diag = carve<double>(p, Vm);
    k.free_row = carve<int>(p, Vm);
    k.end = p;
    return k;
  }
};

// positions into the float64 state, row sums, which rows are unknowns.  copy_only: V_out = V_init (outer_iterations == 0).
__global__ __launch_bounds__(ARAP_ROW_THREADS) void arap_init_kernel(int Vm, const int* __restrict__ row_offsets, const double* __restrict__ weights,
                                                                     const unsigned char* __restrict__ fixed, const float* V_init, float* V_out,
                                                                     double* __restrict__ x, double* __restrict__ diag, int* __restrict__ free_row,
                                                                     int copy_only, size_t slab) {
  const int i = blockIdx.x * ARAP_ROW_THREADS + threadIdx.x;
  if (i >= Vm) return;
  V_init += (size_t)blockIdx.y * 3 * Vm; V_out += (size_t)blockIdx.y * 3 * Vm; x += blockIdx.y * slab;
  const float v[3] = {V_init[3 * (size_t)i], V_init[3 * (size_t)i + 1], V_init[3 * (size_t)i + 2]};
  if (copy_only) {
#pragma unroll
    for (int c = 0; c < 3; c++) V_out[3 * (size_t)i + c] = v[c];
    return;
  }
#pragma unroll
  for (int c = 0; c < 3; c++) x[(size_t)c * Vm + i] = (double)v[c];
  if (blockIdx.y) return;                                          // the mesh's own words have one writer: item 0
  const ArapRowSum row = arap_row_sum(row_offsets, weights, fixed, i);
  diag[i] = row.d;
  free_row[i] = row.free_row;
}

__global__ __launch_bounds__(ARAP_ROW_THREADS) void arap_local_kernel(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                                      const double* __restrict__ weights, const float* __restrict__ V0,
                                                                      const double* __restrict__ x, double* __restrict__ R, size_t slab) {
  const int i = blockIdx.x * ARAP_ROW_THREADS + threadIdx.x;
  if (i >= Vm) return;
  x += blockIdx.y * slab; R += blockIdx.y * slab;
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

// E(P', R) of the state, into *out; one workgroup per item (out_stride: doubles between two items' stats)
__global__ __launch_bounds__(ARAP_THREADS) void arap_energy_kernel(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                                   const double* __restrict__ weights, const float* __restrict__ V0,
                                                                   const double* __restrict__ x, const double* __restrict__ R, double* out,
                                                                   size_t slab, size_t out_stride) {
  __shared__ double part[1][ARAP_WAVES];
  double acc[1] = {0.0};
  x += blockIdx.y * slab; R += blockIdx.y * slab; out += blockIdx.y * out_stride;
  for (int i = threadIdx.x; i < Vm; i += ARAP_THREADS) {
    double Ri[3][3];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int k = 0; k < 3; k++) Ri[c][k] = R[((size_t)c * Vm + i) * 3 + k];
    double e_i = 0.0;
    for (int k = row_offsets[i]; k < row_offsets[i + 1]; k++) {
      const int j = clamp_index(cols[k], Vm);
      double e[3];
#pragma unroll
      for (int c = 0; c < 3; c++) e[c] = (double)V0[3 * (size_t)i + c] - (double)V0[3 * (size_t)j + c];
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const double t = (x[(size_t)c * Vm + i] - x[(size_t)c * Vm + j]) - (Ri[c][0] * e[0] + Ri[c][1] * e[1] + Ri[c][2] * e[2]);
        s += t * t;
      }
      e_i += weights[k] * s;
    }
    acc[0] += e_i;
  }
  arap_block_sum<1>(acc, part);
  if (threadIdx.x == 0) *out = acc[0];
}

// workgroup (c, b): column c of item b's right-hand side, r and p with it in the one edge loop, then the whole PCG of that column
// (arap_pcg_steps)
static_assert(ARAP_THREADS == ARAP_WAVES * 64, "arap_global_kernel strides its rows as arap_pcg_steps does");
__global__ __launch_bounds__(ARAP_THREADS) void arap_global_kernel(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                                   const double* __restrict__ weights, const float* __restrict__ V0,
                                                                   const double* __restrict__ Rall, const double* __restrict__ diag,
                                                                   const int* __restrict__ free_row, double* xall, double* rall, double* pall,
                                                                   double* qall, int cg_iterations, double tol2, float* V_out,
                                                                   double* stats_row, size_t slab, size_t stats_stride) {
  __shared__ double partA[1][ARAP_WAVES], partB[3][ARAP_WAVES];
  const int c = blockIdx.x;
  const size_t item = blockIdx.y * slab;
  const double* R = Rall + item + (size_t)c * Vm * 3;
  double* x = xall + item + (size_t)c * Vm;
  double* r = rall + item + (size_t)c * Vm;
  double* p = pall + item + (size_t)c * Vm;
  double* q = qall + item + (size_t)c * Vm;
  if (V_out) V_out += (size_t)blockIdx.y * 3 * Vm;
  if (stats_row) stats_row += blockIdx.y * stats_stride;
  double s3[3] = {0.0, 0.0, 0.0};                                  // |b|^2, |r|^2, r . z
  for (int i = threadIdx.x; i < Vm; i += ARAP_THREADS) {
    double ri = 0.0, zi = 0.0;
    if (free_row[i]) {
      const double Ri[3] = {R[3 * (size_t)i], R[3 * (size_t)i + 1], R[3 * (size_t)i + 2]};
      const double xi = x[i];
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
      bc += b;
      ri = b - Lx; zi = ri / diag[i];
      s3[0] += bc * bc; s3[1] += ri * ri; s3[2] += ri * zi;
    }
    r[i] = ri; p[i] = zi;                                          // held rows: r = p = 0, for the whole solve
  }
  const ArapPcgResult cg = arap_pcg_steps(Vm, row_offsets, cols, weights, diag, free_row, x, r, p, q, cg_iterations, tol2, s3, partA, partB);
  if (V_out)                                                       // the last outer iteration: each thread reads back its own rows
    for (int i = threadIdx.x; i < Vm; i += ARAP_THREADS) V_out[3 * (size_t)i + c] = (float)x[i];
  if (stats_row && threadIdx.x == 0) {
    stats_row[2 + c] = (double)cg.used;
    stats_row[5 + c] = arap_rel_residual(cg.bb, cg.rr);
  }
}

// ---- the whole-chip global step (gm_arap_solve_grid): the same systems, the same stopping rule, rows over G = ceil(Vm / 256) workgroups ----
// One row per thread, all three coordinates in that thread (the CSR row is read once for three products).  The ONLY synchronisation
// between workgroups is the kernel boundary, so a CG step costs launches; the single-reduction recurrences of Chronopoulos & Gear
// ("s-step iterative methods for symmetric linear systems", 1989) need two per step where the classic ones need three:
//   u = r / diag, w = A u, gamma = r . u, delta = w . u;   beta = gamma / gamma_prev, p . A p = delta - beta gamma / alpha_prev,
//   alpha = gamma / (p . A p);   p = u + beta p, s = w + beta s (= A p), x += alpha p, r -= alpha s.
//   arap_grid_rhs      r = b - L x, u, |b|^2 partials (once per outer iteration, behind arap_local)
//   arap_grid_product  w = A u and the workgroup's partial sums of r . u, w . u, r . r: one slot per workgroup, quantity and coordinate
//   arap_grid_update   every workgroup adds the G slots (arap_slot_sum: the same bits everywhere), makes the column kernel's two exit
//                      tests per coordinate, and updates p, s, x, r, u of its rows
// The host cannot see convergence without a wait, so product / update pairs are enqueued for the full cg_iterations; a coordinate that
// has stopped is frozen (its steps and |r|^2 are carried), and once all three have stopped a launch reads its state and changes nothing.
// WHO WRITES WHAT.  rhs and product write slots and read none; update reads slots and writes none.  The carried scalars are read and
// written by update, so they live in a pair: launch k reads carry[k & 1] and workgroup 0 writes carry[(k + 1) & 1] - no workgroup can
// overwrite what a slower one of the same launch still reads.  Every other array is written by the thread that owns the row.
#define ARAP_ROW_WAVES 4
#define ARAP_EDGE_BATCH 8     // arap_grid_product: edges of a row in flight together (a closed triangle mesh has 6 per vertex on average)
#define ARAP_CARRY 6          // per coordinate: alpha and gamma of the previous step, |b|^2, |r|^2, steps used, stopped (0 / 1)

// B items, as ArapWs: per item a slab (the six state columns, R, both slot arrays, the carry pair), then diag and free_row once
struct ArapGridWs {
  double *x, *r, *u, *w, *p, *s;   // [3][Vm] each
  double* R;                       // [3][Vm][3]
  double* bb_slots;                // [3][G]
  double* slots;                   // [3 quantities][3][G]
  double* carry;                   // [2][3][ARAP_CARRY]
  size_t slab;
  double* diag;                    // [Vm]
  int* free_row;                   // [Vm]
  char* end;
  static ArapGridWs from(void* ws, size_t Vm, size_t B) {
    char* p = reinterpret_cast<char*>(ws);
    const size_t G = (Vm + ARAP_ROW_THREADS - 1) / ARAP_ROW_THREADS;
    ArapGridWs k;
    k.x = carve<double>(p, 3 * Vm); k.r = carve<double>(p, 3 * Vm); k.u = carve<double>(p, 3 * Vm);
    k.w = carve<double>(p, 3 * Vm); k.p = carve<double>(p, 3 * Vm); k.s = carve<double>(p, 3 * Vm);
    k.R = carve<double>(p, 9 * Vm);
    k.bb_slots = carve<double>(p, 3 * G);
    k.slots = carve<double>(p, 9 * G);
    k.carry = carve<double>(p, 2 * 3 * ARAP_CARRY);
    k.slab = (size_t)(carve<double>(p, 0) - k.x);
    p = reinterpret_cast<char*>(k.x + B * k.slab);
    k.diag = carve<double>(p, Vm);
    k.free_row = carve<int>(p, Vm);
    k.end = p;
    return k;
  }
};

// the sums of N rows of G workgroup slots, the same bits in every thread of every workgroup: each wave adds all G for itself, lane l
// the slots l, l + 64, ... in ascending order, then the butterfly.  The order depends on G alone.  Reached by whole waves only.
// (The N loads of a pass are in flight together: one memory round trip per 64 workgroups, not one per quantity.)
template <int N>
__device__ __forceinline__ void arap_slot_sum(const double* __restrict__ slots, int G, double (&v)[N]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < N; k++) v[k] = 0.0;
  for (int g = lane; g < G; g += 64)
#pragma unroll
    for (int k = 0; k < N; k++) v[k] += slots[(size_t)k * G + g];
#pragma unroll
  for (int k = 0; k < N; k++)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d);
}

// r = b - L x and u = r / diag of the free rows (held rows: r = u = 0 for the whole solve), |b|^2 partials.  The row arithmetic of
// arap_global_kernel's first loop, three coordinates at once.
__global__ __launch_bounds__(ARAP_ROW_THREADS) void arap_grid_rhs_kernel(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                                         const double* __restrict__ weights, const float* __restrict__ V0,
                                                                         const double* __restrict__ R, const double* __restrict__ diag,
                                                                         const int* __restrict__ free_row, const double* __restrict__ x,
                                                                         double* __restrict__ r, double* __restrict__ u, double* __restrict__ bb_slots,
                                                                         size_t slab) {
  __shared__ double part[3][ARAP_ROW_WAVES];
  const int i = blockIdx.x * ARAP_ROW_THREADS + threadIdx.x;
  const size_t item = blockIdx.y * slab;
  R += item; x += item; r += item; u += item; bb_slots += item;
  double bb[3] = {0.0, 0.0, 0.0};
  if (i < Vm) {
    double ri[3] = {0.0, 0.0, 0.0}, ui[3] = {0.0, 0.0, 0.0};
    if (free_row[i]) {
      double Ri[3][3], xi[3], pi[3], b[3] = {0.0, 0.0, 0.0}, Lx[3] = {0.0, 0.0, 0.0}, bc[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int c = 0; c < 3; c++) {
        xi[c] = x[(size_t)c * Vm + i]; pi[c] = (double)V0[3 * (size_t)i + c];
#pragma unroll
        for (int a = 0; a < 3; a++) Ri[c][a] = R[((size_t)c * Vm + i) * 3 + a];
      }
      for (int k = row_offsets[i]; k < row_offsets[i + 1]; k++) {
        const int j = clamp_index(cols[k], Vm);
        const double wk = weights[k];
        const int held = !free_row[j];
        double e[3];
#pragma unroll
        for (int a = 0; a < 3; a++) e[a] = pi[a] - (double)V0[3 * (size_t)j + a];
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const double xj = x[(size_t)c * Vm + j];
          double t = 0.0;
#pragma unroll
          for (int a = 0; a < 3; a++) t += (Ri[c][a] + R[((size_t)c * Vm + j) * 3 + a]) * e[a];
          b[c] += 0.5 * wk * t;
          Lx[c] += wk * (xi[c] - xj);
          if (held) bc[c] += wk * xj;                              // a held neighbour moves to the right-hand side
        }
      }
      const double d = diag[i];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        bc[c] += b[c];
        ri[c] = b[c] - Lx[c]; ui[c] = ri[c] / d;
        bb[c] = bc[c] * bc[c];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) { r[(size_t)c * Vm + i] = ri[c]; u[(size_t)c * Vm + i] = ui[c]; }
  }
  arap_block_sum<3, ARAP_ROW_WAVES>(bb, part);
  if (threadIdx.x == 0)
#pragma unroll
    for (int c = 0; c < 3; c++) bb_slots[(size_t)c * gridDim.x + blockIdx.x] = bb[c];
}

// w = A u of the free rows; slots [0..3) r . u, [3..6) w . u, [6..9) r . r.  carry: null in the first launch of an outer iteration.
// The early return is item b's own: all three of ITS columns have stopped, whatever the other items do.
__global__ __launch_bounds__(ARAP_ROW_THREADS) void arap_grid_product_kernel(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                                             const double* __restrict__ weights, const int* __restrict__ free_row,
                                                                             const double* __restrict__ r, const double* __restrict__ u,
                                                                             double* __restrict__ w, const double* __restrict__ carry,
                                                                             double* __restrict__ slots, size_t slab) {
  __shared__ double part[9][ARAP_ROW_WAVES];
  const size_t item = blockIdx.y * slab;
  r += item; u += item; w += item; slots += item;
  if (carry) carry += item;
  // the row's own loads are issued ahead of the carry test, so that the test costs no memory round trip of its own
  // (a thread past the last row reads the last row and adds nothing)
  const int i = min(blockIdx.x * ARAP_ROW_THREADS + threadIdx.x, Vm - 1);
  const bool row = blockIdx.x * ARAP_ROW_THREADS + threadIdx.x < Vm;
  const int k0 = row_offsets[i], k1 = row_offsets[i + 1], fr = free_row[i];
  double ui[3], ri[3];
#pragma unroll
  for (int c = 0; c < 3; c++) { ui[c] = u[(size_t)c * Vm + i]; ri[c] = r[(size_t)c * Vm + i]; }
  if (carry && carry[ARAP_CARRY - 1] != 0.0 && carry[2 * ARAP_CARRY - 1] != 0.0 && carry[3 * ARAP_CARRY - 1] != 0.0) return;   // all stopped: the same in every thread of the item
  double s9[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (row && fr) {
    double q[3] = {0.0, 0.0, 0.0};
    // ARAP_EDGE_BATCH edges at a time: their column ids and weights are asked for together, then their u together.  An edge at a time
    // compiled to a wait after the column id and another after u[j] in every trip of the loop.  Past the row's end the last edge is
    // read again and not added.  Added in CSR order.  (Measured only together with the hoisted loads: INTEGRATION.md section Q.)
    for (int kb = k0; kb < k1; kb += ARAP_EDGE_BATCH) {
      int j[ARAP_EDGE_BATCH];
      double wk[ARAP_EDGE_BATCH], uj[ARAP_EDGE_BATCH][3];
#pragma unroll
      for (int t = 0; t < ARAP_EDGE_BATCH; t++) {
        const int k = min(kb + t, k1 - 1);
        j[t] = clamp_index(cols[k], Vm); wk[t] = weights[k];
      }
#pragma unroll
      for (int t = 0; t < ARAP_EDGE_BATCH; t++)
#pragma unroll
        for (int c = 0; c < 3; c++) uj[t][c] = u[(size_t)c * Vm + j[t]];
#pragma unroll
      for (int t = 0; t < ARAP_EDGE_BATCH; t++)
        if (kb + t < k1)
#pragma unroll
          for (int c = 0; c < 3; c++) q[c] += wk[t] * (ui[c] - uj[t][c]);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
      w[(size_t)c * Vm + i] = q[c];
      s9[c] = ri[c] * ui[c]; s9[3 + c] = q[c] * ui[c]; s9[6 + c] = ri[c] * ri[c];
    }
  }
  arap_block_sum<9, ARAP_ROW_WAVES>(s9, part);
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < 9; k++) slots[(size_t)k * gridDim.x + blockIdx.x] = s9[k];
}

// step `first ? 0 : k` of all three columns: the sums, the exit tests, the update of this thread's row.  last: the launch behind the
// final product - it only closes the books (|r|^2 of the columns still running) and writes stats_row.  V_out: written when not null.
__global__ __launch_bounds__(ARAP_ROW_THREADS) void arap_grid_update_kernel(int Vm, const double* __restrict__ diag, const int* __restrict__ free_row,
                                                                            double* __restrict__ x, double* __restrict__ r, double* __restrict__ u,
                                                                            const double* __restrict__ w, double* __restrict__ p, double* __restrict__ s,
                                                                            const double* __restrict__ bb_slots, const double* __restrict__ slots,
                                                                            const double* __restrict__ carry_in, double* __restrict__ carry_out,
                                                                            int first, int last, double tol2, float* __restrict__ V_out,
                                                                            double* __restrict__ stats_row, size_t slab, size_t stats_stride) {
  const size_t item = blockIdx.y * slab;
  x += item; r += item; u += item; w += item; p += item; s += item; bb_slots += item; slots += item; carry_in += item; carry_out += item;
  if (V_out) V_out += (size_t)blockIdx.y * 3 * Vm;
  if (stats_row) stats_row += blockIdx.y * stats_stride;
  // Everything this thread reads is asked for before anything is decided: the row, the slots and the carry arrive in one memory round
  // trip instead of three in a row.  (p and s of the first step are read and not used.)
  // (A thread past the last row reads the last row and writes nothing.)
  const int G = gridDim.x;
  const int i = min(blockIdx.x * ARAP_ROW_THREADS + threadIdx.x, Vm - 1);
  const bool row = blockIdx.x * ARAP_ROW_THREADS + threadIdx.x < Vm;
  const int fr = free_row[i];
  const double d = diag[i];
  double xi[3], ri[3], ui[3], wi[3], pi[3], si[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const size_t o = (size_t)c * Vm + i;
    xi[c] = x[o]; ri[c] = r[o]; ui[c] = u[o]; wi[c] = w[o]; pi[c] = p[o]; si[c] = s[o];
  }
  double st[3][ARAP_CARRY], t9[9], alpha[3] = {0.0, 0.0, 0.0}, beta[3] = {0.0, 0.0, 0.0};
  int act[3] = {0, 0, 0};                                          // this launch updates the column
  arap_slot_sum<9>(slots, G, t9);
  if (first) {
    double bb[3];
    arap_slot_sum<3>(bb_slots, G, bb);
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
      for (int k = 0; k < ARAP_CARRY; k++) st[c][k] = 0.0;
      st[c][2] = bb[c];
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int k = 0; k < ARAP_CARRY; k++) st[c][k] = carry_in[c * ARAP_CARRY + k];
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {                                    // uniform over the item: all its workgroups hold the same sums and the same carry
    if (st[c][5] != 0.0) continue;                                 // stopped: frozen, the slots of this column are not looked at
    const double gamma = t9[c], delta = t9[3 + c], rr = t9[6 + c];
    st[c][3] = rr;
    const double bt = first ? 0.0 : gamma / st[c][1];
    const double pq = first ? delta : delta - bt * gamma / st[c][0];
    if (!(rr > tol2 * st[c][2]) || !(pq > 0.0)) {                  // converged (or not finite), or p = 0: the column kernel's two exits
      st[c][5] = 1.0;
    } else if (!last) {
      beta[c] = bt; alpha[c] = gamma / pq; act[c] = 1;
      st[c][0] = alpha[c]; st[c][1] = gamma; st[c][4] += 1.0;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
      for (int k = 0; k < ARAP_CARRY; k++) carry_out[c * ARAP_CARRY + k] = st[c][k];
      if (stats_row) {
        const double bb = st[c][2], rr = st[c][3];
        stats_row[2 + c] = st[c][4];
        stats_row[5 + c] = arap_rel_residual(bb, rr);
      }
    }
  }
  if (!row) return;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const size_t o = (size_t)c * Vm + i;
    double xv = xi[c];
    if (fr && act[c]) {
      const double pc = first ? ui[c] : ui[c] + beta[c] * pi[c];
      const double sc = first ? wi[c] : wi[c] + beta[c] * si[c];
      const double rv = ri[c] - alpha[c] * sc;
      xv += alpha[c] * pc;
      p[o] = pc; s[o] = sc; x[o] = xv; r[o] = rv; u[o] = rv / d;
    }
    if (V_out) V_out[3 * (size_t)i + c] = (float)xv;
  }
}

// ---- the energy of a pose and its gradient (gm_arap_energy_grad): E(x) = min_R E(x, R) as a function of the pose alone ----
//   R_i(x): the local step (arap_rotation of S_i, above), so E(x) = E(x, R(x)); the R_i minimise E, hence the total derivative is the
//   partial one at fixed R:   dE/dx_i = 4 sum_j w_ij [ (x_i - x_j) - (R_i + R_j)(p_i - p_j) / 2 ]   (w symmetric: the neighbour's share
//   of the edge is its own term of row i, nothing is scattered) - the residual of the global step's equation, times 4.
//   A row whose pose edges x_i - x_j equal its rest edges p_i - p_j bit for bit (the rest pose, a translate of it that float32 holds)
//   takes R_i = I itself and not the eigen-route's I + O(1e-16): the rest pose then has E = 0 and dE/dx = 0 exactly.
// Three launches, rows over G = ceil(Vm / 256) workgroups that meet only at the kernel boundaries:
//   arap_pose_local    one thread per vertex: R_i from the float32 pose, into the workspace as [Vm][9] (one gather per neighbour)
//   arap_energy_grad   one thread per vertex: g_i, the row's energy; the workgroup's energies into its slot (arap_block_sum)
//   arap_energy_total  one wave adds the G slots in index order (arap_slot_sum)
// Both row kernels ask for ARAP_POSE_BATCH edges of a row together, as arap_grid_product does: at these sizes (one workgroup per CU
// or fewer) a row's time is its chain of dependent gathers, not its bytes.  Sums in CSR order, no atomics: two calls give the same bits.
#define ARAP_POSE_BATCH 8

struct ArapEnergyWs {
  double* R;       // [Vm][9]: R_i row-major
  double* slots;   // [G] the workgroups' energies
  char* end;
  static ArapEnergyWs from(void* ws, size_t Vm) {
    char* p = reinterpret_cast<char*>(ws);
    ArapEnergyWs k;
    k.R = carve<double>(p, 9 * Vm);
    k.slots = carve<double>(p, (Vm + ARAP_ROW_THREADS - 1) / ARAP_ROW_THREADS);
    k.end = p;
    return k;
  }
};

__global__ __launch_bounds__(ARAP_ROW_THREADS) void arap_pose_local_kernel(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                                           const double* __restrict__ weights, const float* __restrict__ V0,
                                                                           const float* __restrict__ V1, double* __restrict__ R) {
  const int i = blockIdx.x * ARAP_ROW_THREADS + threadIdx.x;
  if (i >= Vm) return;
  const int k0 = row_offsets[i], k1 = row_offsets[i + 1];
  double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, Q[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, pi[3], xi[3];
#pragma unroll
  for (int c = 0; c < 3; c++) { pi[c] = (double)V0[3 * (size_t)i + c]; xi[c] = (double)V1[3 * (size_t)i + c]; }
  bool unmoved = true;
  for (int kb = k0; kb < k1; kb += ARAP_POSE_BATCH) {               // past the row's end the last edge is read again and not added
    int j[ARAP_POSE_BATCH];
    double w[ARAP_POSE_BATCH];
    float pj[ARAP_POSE_BATCH][3], xj[ARAP_POSE_BATCH][3];
#pragma unroll
    for (int t = 0; t < ARAP_POSE_BATCH; t++) {
      const int k = min(kb + t, k1 - 1);
      j[t] = clamp_index(cols[k], Vm); w[t] = weights[k];
    }
#pragma unroll
    for (int t = 0; t < ARAP_POSE_BATCH; t++)
#pragma unroll
      for (int c = 0; c < 3; c++) { pj[t][c] = V0[3 * (size_t)j[t] + c]; xj[t][c] = V1[3 * (size_t)j[t] + c]; }
#pragma unroll
    for (int t = 0; t < ARAP_POSE_BATCH; t++)
      if (kb + t < k1) {
        double e[3], d[3];
#pragma unroll
        for (int c = 0; c < 3; c++) { e[c] = pi[c] - (double)pj[t][c]; d[c] = xi[c] - (double)xj[t][c]; unmoved = unmoved && d[c] == e[c]; }
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
          for (int b = 0; b < 3; b++) S[a][b] += w[t] * d[a] * e[b];
      }
  }
  if (!unmoved) arap_rotation(S, Q);
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) R[9 * (size_t)i + 3 * a + b] = Q[a][b];
}

// grad: null when only the energy is wanted (the same arithmetic: the same energy bits)
__global__ __launch_bounds__(ARAP_ROW_THREADS) void arap_energy_grad_kernel(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                                            const double* __restrict__ weights, const float* __restrict__ V0,
                                                                            const float* __restrict__ V1, const double* __restrict__ R,
                                                                            double* __restrict__ grad, double* __restrict__ slots) {
  __shared__ double part[1][ARAP_ROW_WAVES];
  // (a thread past the last row reads the last row, adds nothing and writes nothing: every thread reaches the sum's barrier)
  const int i = min(blockIdx.x * ARAP_ROW_THREADS + threadIdx.x, Vm - 1);
  const bool row = blockIdx.x * ARAP_ROW_THREADS + threadIdx.x < Vm;
  const int k0 = row_offsets[i], k1 = row_offsets[i + 1];
  double Ri[3][3], pi[3], xi[3], g[3] = {0.0, 0.0, 0.0}, e_i = 0.0, deg = 0.0;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    pi[c] = (double)V0[3 * (size_t)i + c]; xi[c] = (double)V1[3 * (size_t)i + c];
#pragma unroll
    for (int a = 0; a < 3; a++) Ri[c][a] = R[9 * (size_t)i + 3 * c + a];
  }
  for (int kb = k0; kb < k1; kb += ARAP_POSE_BATCH) {
    int j[ARAP_POSE_BATCH];
    double w[ARAP_POSE_BATCH], Rj[ARAP_POSE_BATCH][9];
    float pj[ARAP_POSE_BATCH][3], xj[ARAP_POSE_BATCH][3];
#pragma unroll
    for (int t = 0; t < ARAP_POSE_BATCH; t++) {
      const int k = min(kb + t, k1 - 1);
      j[t] = clamp_index(cols[k], Vm); w[t] = weights[k];
    }
#pragma unroll
    for (int t = 0; t < ARAP_POSE_BATCH; t++) {
#pragma unroll
      for (int c = 0; c < 3; c++) { pj[t][c] = V0[3 * (size_t)j[t] + c]; xj[t][c] = V1[3 * (size_t)j[t] + c]; }
#pragma unroll
      for (int a = 0; a < 9; a++) Rj[t][a] = R[9 * (size_t)j[t] + a];
    }
#pragma unroll
    for (int t = 0; t < ARAP_POSE_BATCH; t++)
      if (kb + t < k1) {
        double e[3], s = 0.0;
#pragma unroll
        for (int c = 0; c < 3; c++) e[c] = pi[c] - (double)pj[t][c];
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const double d = xi[c] - (double)xj[t][c];
          const double own = Ri[c][0] * e[0] + Ri[c][1] * e[1] + Ri[c][2] * e[2];
          const double both = (Ri[c][0] + Rj[t][3 * c]) * e[0] + (Ri[c][1] + Rj[t][3 * c + 1]) * e[1] + (Ri[c][2] + Rj[t][3 * c + 2]) * e[2];
          g[c] += w[t] * (d - 0.5 * both);
          s += (d - own) * (d - own);
        }
        e_i += w[t] * s;
        deg += w[t];
      }
  }
  double acc[1] = {row && deg > 0.0 ? e_i : 0.0};                  // a pinned row (its weights sum to 0) contributes nothing
  if (row && grad)
#pragma unroll
    for (int c = 0; c < 3; c++) grad[3 * (size_t)i + c] = deg > 0.0 ? 4.0 * g[c] : 0.0;
  arap_block_sum<1, ARAP_ROW_WAVES>(acc, part);
  if (threadIdx.x == 0) slots[blockIdx.x] = acc[0];
}

// one wave: the G slots in the order of arap_slot_sum, into *out
__global__ __launch_bounds__(64) void arap_energy_total_kernel(const double* __restrict__ slots, int G, double* __restrict__ out) {
  double v[1];
  arap_slot_sum<1>(slots, G, v);
  if (threadIdx.x == 0) *out = v[0];
}

// ---- one-ring smoothing of per-vertex rows (gm_mesh_smooth_rows): T Jacobi sweeps of (I + lambda L) y = g from y = g ----
//   y_i <- (g_i + lambda sum_j w_ij y_j) / (1 + lambda d_i): a convex combination of g_i and the neighbours' values, so nothing grows, a
//   constant field stays, a row with d_i = 0 keeps g_i.  One thread per vertex, one launch per sweep between two copies of the state
//   (the scheme of gm_tsdf_fill): a sweep reads only what the previous launch wrote.  smooth_init: d_i once (as 1 + lambda d_i), g into
//   the first copy; the last sweep writes `out`, which may be g itself - a thread reads g_i before it writes row i, and no other row of g.
__global__ __launch_bounds__(ARAP_ROW_THREADS) void smooth_init_kernel(int Vm, const int* __restrict__ row_offsets, const double* __restrict__ weights,
                                                                       const double* g, double lambda, double* __restrict__ denom,
                                                                       double* __restrict__ state, double* out) {
  const int i = blockIdx.x * ARAP_ROW_THREADS + threadIdx.x;
  if (i >= Vm) return;
  const double gi[3] = {g[3 * (size_t)i], g[3 * (size_t)i + 1], g[3 * (size_t)i + 2]};
  double d = 0.0;
  for (int k = row_offsets[i]; k < row_offsets[i + 1]; k++) d += weights[k];
  denom[i] = 1.0 + lambda * d;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    state[3 * (size_t)i + c] = gi[c];
    if (out) out[3 * (size_t)i + c] = gi[c];                         // sweeps == 0: the copy
  }
}

__global__ __launch_bounds__(ARAP_ROW_THREADS) void smooth_sweep_kernel(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                                        const double* __restrict__ weights, const double* g,
                                                                        const double* __restrict__ denom, double lambda, const double* __restrict__ y,
                                                                        double* y_next) {
  const int i = blockIdx.x * ARAP_ROW_THREADS + threadIdx.x;
  if (i >= Vm) return;
  const int k0 = row_offsets[i], k1 = row_offsets[i + 1];
  const double gi[3] = {g[3 * (size_t)i], g[3 * (size_t)i + 1], g[3 * (size_t)i + 2]}, den = denom[i];
  double acc[3] = {0.0, 0.0, 0.0};
  for (int kb = k0; kb < k1; kb += ARAP_POSE_BATCH) {               // past the row's end the last edge is read again and not added
    int j[ARAP_POSE_BATCH];
    double w[ARAP_POSE_BATCH], yj[ARAP_POSE_BATCH][3];
#pragma unroll
    for (int t = 0; t < ARAP_POSE_BATCH; t++) {
      const int k = min(kb + t, k1 - 1);
      j[t] = clamp_index(cols[k], Vm); w[t] = weights[k];
    }
#pragma unroll
    for (int t = 0; t < ARAP_POSE_BATCH; t++)
#pragma unroll
      for (int c = 0; c < 3; c++) yj[t][c] = y[3 * (size_t)j[t] + c];
#pragma unroll
    for (int t = 0; t < ARAP_POSE_BATCH; t++)
      if (kb + t < k1)
#pragma unroll
        for (int c = 0; c < 3; c++) acc[c] += w[t] * yj[t][c];
  }
#pragma unroll
  for (int c = 0; c < 3; c++) y_next[3 * (size_t)i + c] = (gi[c] + lambda * acc[c]) / den;
}

struct SmoothWs {
  double* denom;      // [Vm] 1 + lambda d_i
  double* state[2];   // [Vm][3] each
  char* end;
  static SmoothWs from(void* ws, size_t Vm) {
    char* p = reinterpret_cast<char*>(ws);
    SmoothWs k;
    k.denom = carve<double>(p, Vm);
    k.state[0] = carve<double>(p, 3 * Vm); k.state[1] = carve<double>(p, 3 * Vm);
    k.end = p;
    return k;
  }
};

}  // namespace gm

// ---------------------------------------------------------------------------------------------
// the entry points (include/gmesh_hip.h): their refusals, then the launches
using namespace gm;

// gm_arap_solve, gm_arap_solve_grid and gm_arap_solve_batch: one set of refusals (B items: V_init, V_out and stats span B solves' worth;
// need: the workspace the chosen chain takes)
static int arap_args_checked(const char* fn, int B, int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0,
                             const unsigned char* fixed, const float* V_init, int outer_iterations, int cg_iterations, double cg_tolerance, float* V_out,
                             double* stats, void* workspace, size_t workspace_bytes, size_t need) {
  if (Vm <= 0) { set_error("%s: Vm = %d (must be positive)", fn, Vm); return GM_ERR_INVALID_ARG; }
  if (outer_iterations < 0) { set_error("%s: outer_iterations = %d (negative)", fn, outer_iterations); return GM_ERR_INVALID_ARG; }
  if (cg_iterations < 1) { set_error("%s: cg_iterations = %d (at least 1)", fn, cg_iterations); return GM_ERR_INVALID_ARG; }
  if (!(cg_tolerance >= 0.0) || cg_tolerance > 1.7976931348623157e308) {
    set_error("%s: cg_tolerance must be finite and not negative", fn); return GM_ERR_INVALID_ARG;
  }
  if (!row_offsets || !cols || !weights || !V0 || !fixed || !V_init || !V_out || !workspace) { set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG; }
  // every meeting of two of these ranges is refused, the read-only ones included; V_out == V_init is the in-place call (V_init stands for both)
  const ByteRange rg[5] = {{V0, 12 * (size_t)Vm, "V0", true}, {V_init, 12 * (size_t)Vm * B, "V_init", true},
                           {V_out == V_init ? nullptr : V_out, 12 * (size_t)Vm * B, "V_out", true},
                           {stats, 64 * (size_t)outer_iterations * B, "stats", true}, {workspace, workspace_bytes, "workspace", true}};
  if (int rc = check_ranges(fn, rg)) return rc;
  if (workspace_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need); return GM_ERR_BUFFER; }
  return GM_OK;
}

// the launch chain of a solve over B items: init, then per outer iteration local, [energy], the global step, [energy] (the energies
// only with stats).  global_step(out, row, stride) enqueues one global step on k's state: out is V_out in the last outer iteration and
// null before, row the iteration's stats row or null, stride the doubles between two items' stats.
template <class Ws, class GlobalStep>
static void arap_chain(int B, const Ws& k, int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0, const unsigned char* fixed,
                       const float* V_init, int outer_iterations, float* V_out, double* stats, hipStream_t s, GlobalStep global_step) {
  const dim3 rows((Vm + ARAP_ROW_THREADS - 1) / ARAP_ROW_THREADS, B), threads(ARAP_ROW_THREADS);
  const size_t stride = 8 * (size_t)outer_iterations;
  hipLaunchKernelGGL(arap_init_kernel, rows, threads, 0, s, Vm, row_offsets, weights, fixed, V_init, V_out, k.x, k.diag, k.free_row,
                     outer_iterations == 0 ? 1 : 0, k.slab);
  for (int it = 0; it < outer_iterations; it++) {
    double* row = stats ? stats + 8 * (size_t)it : nullptr;
    hipLaunchKernelGGL(arap_local_kernel, rows, threads, 0, s, Vm, row_offsets, cols, weights, V0, k.x, k.R, k.slab);
    if (row) hipLaunchKernelGGL(arap_energy_kernel, dim3(1, B), dim3(ARAP_THREADS), 0, s, Vm, row_offsets, cols, weights, V0, k.x, k.R, row, k.slab, stride);
    global_step(it == outer_iterations - 1 ? V_out : nullptr, row, stride);
    if (row) hipLaunchKernelGGL(arap_energy_kernel, dim3(1, B), dim3(ARAP_THREADS), 0, s, Vm, row_offsets, cols, weights, V0, k.x, k.R, row + 1, k.slab, stride);
  }
}

static size_t arap_workspace_bytes(int Vm, int B, int global_step) {
  if (Vm < 1) Vm = 1;                                              // the public sizes are defined for every Vm; a solve refuses Vm <= 0
  return (size_t)(global_step ? ArapGridWs::from(nullptr, (size_t)Vm, (size_t)B).end : ArapWs::from(nullptr, (size_t)Vm, (size_t)B).end) + 256;
}

// gm_arap_solve, gm_arap_solve_grid (B = 1) and gm_arap_solve_batch behind their own refusals: the shared ones, then the chain with the
// column step (global_step 0) or the grid step (1)
static int arap_solve(const char* fn, int B, int global_step, int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0,
                      const unsigned char* fixed, const float* V_init, int outer_iterations, int cg_iterations, double cg_tolerance, float* V_out,
                      double* stats, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = arap_args_checked(fn, B, Vm, row_offsets, cols, weights, V0, fixed, V_init, outer_iterations, cg_iterations, cg_tolerance, V_out, stats,
                                 workspace, workspace_bytes, arap_workspace_bytes(Vm, B, global_step)))
    return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const double tol2 = cg_tolerance * cg_tolerance;
  if (global_step) {
    const ArapGridWs k = ArapGridWs::from(workspace, (size_t)Vm, (size_t)B);
    const dim3 rows((Vm + ARAP_ROW_THREADS - 1) / ARAP_ROW_THREADS, B), threads(ARAP_ROW_THREADS);
    arap_chain(B, k, Vm, row_offsets, cols, weights, V0, fixed, V_init, outer_iterations, V_out, stats, s, [&](float* out, double* row, size_t stride) {
      hipLaunchKernelGGL(arap_grid_rhs_kernel, rows, threads, 0, s, Vm, row_offsets, cols, weights, V0, k.R, k.diag, k.free_row, k.x, k.r, k.u, k.bb_slots, k.slab);
      // steps 0 .. cg_iterations - 1 update; the pair behind them only forms the final |r|^2, which nothing but stats reads
      // (Unlike the column step, whose loop leaves on the device, a cap costs 2 * cg_iterations host launches per outer iteration whether
      // or not the solve stops early: a cap far above the steps needed is paid for.  64-bit, so that cap + 1 cannot overflow.)
      const long long pairs = (long long)cg_iterations + (row ? 1 : 0);
      for (long long step = 0; step < pairs; step++) {
        const double* carry_in = k.carry + (step & 1) * 3 * ARAP_CARRY;
        double* carry_out = k.carry + ((step + 1) & 1) * 3 * ARAP_CARRY;
        const int last = step == cg_iterations;
        hipLaunchKernelGGL(arap_grid_product_kernel, rows, threads, 0, s, Vm, row_offsets, cols, weights, k.free_row, k.r, k.u, k.w, step ? carry_in : nullptr,
                           k.slots, k.slab);
        hipLaunchKernelGGL(arap_grid_update_kernel, rows, threads, 0, s, Vm, k.diag, k.free_row, k.x, k.r, k.u, k.w, k.p, k.s, k.bb_slots, k.slots, carry_in,
                           carry_out, step == 0 ? 1 : 0, last, tol2, step == pairs - 1 ? out : nullptr, last ? row : nullptr, k.slab, stride);
      }
    });
  } else {
    const ArapWs k = ArapWs::from(workspace, (size_t)Vm, (size_t)B);
    arap_chain(B, k, Vm, row_offsets, cols, weights, V0, fixed, V_init, outer_iterations, V_out, stats, s, [&](float* out, double* row, size_t stride) {
      hipLaunchKernelGGL(arap_global_kernel, dim3(3, B), dim3(ARAP_THREADS), 0, s, Vm, row_offsets, cols, weights, V0, k.R, k.diag, k.free_row, k.x, k.r,
                         k.p, k.q, cg_iterations, tol2, out, row, k.slab, stride);
    });
  }
  GM_HIP(hipGetLastError());
  return GM_OK;
}

extern "C" {

size_t gm_arap_workspace_bytes(int Vm) { return arap_workspace_bytes(Vm, 1, 0); }

int gm_arap_solve(int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0, const unsigned char* fixed,
                  const float* V_init, int outer_iterations, int cg_iterations, double cg_tolerance, float* V_out, double* stats,
                  void* workspace, size_t workspace_bytes, void* stream) {
  return arap_solve("gm_arap_solve", 1, 0, Vm, row_offsets, cols, weights, V0, fixed, V_init, outer_iterations, cg_iterations, cg_tolerance, V_out, stats,
                    workspace, workspace_bytes, stream);
}

size_t gm_arap_grid_workspace_bytes(int Vm) { return arap_workspace_bytes(Vm, 1, 1); }

int gm_arap_solve_grid(int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0, const unsigned char* fixed,
                       const float* V_init, int outer_iterations, int cg_iterations, double cg_tolerance, float* V_out, double* stats,
                       void* workspace, size_t workspace_bytes, void* stream) {
  return arap_solve("gm_arap_solve_grid", 1, 1, Vm, row_offsets, cols, weights, V0, fixed, V_init, outer_iterations, cg_iterations, cg_tolerance, V_out,
                    stats, workspace, workspace_bytes, stream);
}

// ---- B solves in one chain (gm_arap_solve_batch): the batch is the second grid dimension of every kernel ----
size_t gm_arap_batch_workspace_bytes(int Vm, int B, int global_step) {
  if (Vm <= 0 || B < 1 || B > GM_ARAP_BATCH_MAX || (global_step != 0 && global_step != 1)) return 0;
  return arap_workspace_bytes(Vm, B, global_step);
}

int gm_arap_solve_batch(int B, int global_step, int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0,
                        const unsigned char* fixed, const float* V_init, int outer_iterations, int cg_iterations, double cg_tolerance, float* V_out,
                        double* stats, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "gm_arap_solve_batch";
  if (B < 1 || B > GM_ARAP_BATCH_MAX) { set_error("%s: B = %d (1 .. %d)", fn, B, GM_ARAP_BATCH_MAX); return GM_ERR_INVALID_ARG; }
  if (global_step != 0 && global_step != 1) { set_error("%s: global_step = %d (0 column, 1 grid)", fn, global_step); return GM_ERR_INVALID_ARG; }
  return arap_solve(fn, B, global_step, Vm, row_offsets, cols, weights, V0, fixed, V_init, outer_iterations, cg_iterations, cg_tolerance, V_out, stats,
                    workspace, workspace_bytes, stream);
}

// ---- E(x) and dE/dx of a pose (gm_arap_energy_grad), one-ring smoothing of rows (gm_mesh_smooth_rows) ----
size_t gm_arap_energy_workspace_bytes(int Vm) {
  ArapEnergyWs k = ArapEnergyWs::from(nullptr, (size_t)(Vm > 0 ? Vm : 1));
  return (size_t)k.end + 256;
}

int gm_arap_energy_grad(int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0, const float* V1,
                        double* energy_out, double* grad_out, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "gm_arap_energy_grad";
  if (Vm <= 0) { set_error("%s: Vm = %d (must be positive)", fn, Vm); return GM_ERR_INVALID_ARG; }
  if (!row_offsets || !cols || !weights || !V0 || !V1 || !energy_out || !workspace) { set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG; }
  // V0 and V1 are only read and may be one array (the rest pose); every meeting of an output or the workspace with anything is refused
  const ByteRange rg[5] = {{V0, 12 * (size_t)Vm, "V0", false}, {V1, 12 * (size_t)Vm, "V1", false}, {energy_out, 8, "energy_out", true},
                           {grad_out, 24 * (size_t)Vm, "grad_out", true}, {workspace, workspace_bytes, "workspace", true}};
  if (int rc = check_ranges(fn, rg)) return rc;
  const size_t need = gm_arap_energy_workspace_bytes(Vm);
  if (workspace_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need); return GM_ERR_BUFFER; }
  const ArapEnergyWs k = ArapEnergyWs::from(workspace, (size_t)Vm);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int G = (Vm + ARAP_ROW_THREADS - 1) / ARAP_ROW_THREADS;
  hipLaunchKernelGGL(arap_pose_local_kernel, dim3(G), dim3(ARAP_ROW_THREADS), 0, s, Vm, row_offsets, cols, weights, V0, V1, k.R);
  hipLaunchKernelGGL(arap_energy_grad_kernel, dim3(G), dim3(ARAP_ROW_THREADS), 0, s, Vm, row_offsets, cols, weights, V0, V1, k.R, grad_out, k.slots);
  hipLaunchKernelGGL(arap_energy_total_kernel, dim3(1), dim3(64), 0, s, k.slots, G, energy_out);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

size_t gm_mesh_smooth_workspace_bytes(int Vm) {
  SmoothWs k = SmoothWs::from(nullptr, (size_t)(Vm > 0 ? Vm : 1));
  return (size_t)k.end + 256;
}

int gm_mesh_smooth_rows(int Vm, const int* row_offsets, const int* cols, const double* weights, const double* g_in, double lambda, int sweeps,
                        double* out, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "gm_mesh_smooth_rows";
  if (Vm <= 0) { set_error("%s: Vm = %d (must be positive)", fn, Vm); return GM_ERR_INVALID_ARG; }
  if (sweeps < 0) { set_error("%s: sweeps = %d (negative)", fn, sweeps); return GM_ERR_INVALID_ARG; }
  if (!(lambda >= 0.0) || lambda > 1.7976931348623157e308) { set_error("%s: lambda must be finite and not negative", fn); return GM_ERR_INVALID_ARG; }
  if (!row_offsets || !cols || !weights || !g_in || !out || !workspace) { set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG; }
  // out == g_in is the in-place call (g_in stands for both); any other meeting of g_in, out and the workspace is refused
  const ByteRange rg[3] = {{g_in, 24 * (size_t)Vm, "g_in", true}, {out == g_in ? nullptr : out, 24 * (size_t)Vm, "out", true},
                           {workspace, workspace_bytes, "workspace", true}};
  if (int rc = check_ranges(fn, rg)) return rc;
  const size_t need = gm_mesh_smooth_workspace_bytes(Vm);
  if (workspace_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need); return GM_ERR_BUFFER; }
  const SmoothWs k = SmoothWs::from(workspace, (size_t)Vm);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 rows((Vm + ARAP_ROW_THREADS - 1) / ARAP_ROW_THREADS), threads(ARAP_ROW_THREADS);
  hipLaunchKernelGGL(smooth_init_kernel, rows, threads, 0, s, Vm, row_offsets, weights, g_in, lambda, k.denom, k.state[0], sweeps == 0 ? out : nullptr);
  for (int t = 0; t < sweeps; t++)                                   // sweep t reads copy t & 1; the last one writes out
    hipLaunchKernelGGL(smooth_sweep_kernel, rows, threads, 0, s, Vm, row_offsets, cols, weights, g_in, k.denom, lambda, k.state[t & 1],
                       t == sweeps - 1 ? out : k.state[(t + 1) & 1]);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // extern "C"
