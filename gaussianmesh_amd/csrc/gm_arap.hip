// gm_arap.hip -- as-rigid-as-possible deformation of a proxy mesh from dragged handle vertices (gm_arap_solve): the stage that
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
//   Dot products: butterfly inside each wave, 16 wave partials in LDS, then EVERY thread adds the 16 in index order - all threads
//   hold the same bits, so the loop's exit tests are uniform, and the result is the same from run to run (no atomics anywhere).
//   With stats, arap_energy (one workgroup, same reduction) runs after the local and after the global step; without, E is never formed.
// Conventions of gm_closest.hip: caller workspace, stream-ordered, no device allocation, no host wait anywhere in this file.
#include "gm_common.h"

namespace gm {

#define ARAP_THREADS 1024     // arap_global / arap_energy: one workgroup of 16 waves
#define ARAP_WAVES 16
#define ARAP_ROW_THREADS 256  // arap_init / arap_local: one thread per vertex

struct ArapWs {
  double* x;       // [3][Vm] positions, one column per coordinate
  double* r;       // [3][Vm]
  double* p;       // [3][Vm]
  double* q;       // [3][Vm]
  double* R;       // [3][Vm][3]: row c of R_i at (c Vm + i) 3
  double* diag;    // [Vm] sum_j w_ij
  int* free_row;   // [Vm] 1 = a row of the linear system
  char* end;
  static ArapWs from(void* ws, size_t Vm) {
    char* p = reinterpret_cast<char*>(ws);
    ArapWs k;
    k.x = carve<double>(p, 3 * Vm); k.r = carve<double>(p, 3 * Vm); k.p = carve<double>(p, 3 * Vm); k.q = carve<double>(p, 3 * Vm);
    k.R = carve<double>(p, 9 * Vm);
    k.diag = carve<double>(p, Vm);
    k.free_row = carve<int>(p, Vm);
    k.end = p;
    return k;
  }
};

size_t arap_workspace_bytes(int Vm) {
  ArapWs k = ArapWs::from(nullptr, (size_t)(Vm > 0 ? Vm : 1));
  return (size_t)k.end + 256;
}

__device__ __forceinline__ void arap_cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// eigen-decomposition of a symmetric 3x3 (cyclic Jacobi): gm_mesh.hip's jacobi3 line for line (sweeps and threshold included), restated
// because sharing it would have to leave mesh_rs_kernel's machine code unchanged.  A -> diagonal in place, V columns = eigenvectors
__device__ __forceinline__ void arap_jacobi3(double A[3][3], double V[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) V[i][j] = i == j ? 1.0 : 0.0;
  const double scale = fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]) + 1e-300;
  for (int sweep = 0; sweep < 10; sweep++) {
    const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
    if (off <= 1e-16 * scale) break;
#pragma unroll
    for (int pq = 0; pq < 3; pq++) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      const double apq = A[p][q];
      if (fabs(apq) <= 1e-300) continue;
      const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
      const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
      const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
      const int r = 3 - p - q;
      const double arp = A[r][p], arq = A[r][q];
      A[p][p] -= t * apq; A[q][q] += t * apq; A[p][q] = A[q][p] = 0.0;
      A[r][p] = A[p][r] = cs * arp - sn * arq;
      A[r][q] = A[q][r] = sn * arp + cs * arq;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const double vp = V[k][p], vq = V[k][q];
        V[k][p] = cs * vp - sn * vq; V[k][q] = sn * vp + cs * vq;
      }
    }
  }
}

// the proper rotation closest to F (max tr(Q^T F)); identity for rank <= 1
__device__ __forceinline__ void arap_rotation(const double F[3][3], double Q[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) Q[i][j] = i == j ? 1.0 : 0.0;
  double C[3][3], E[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) C[i][j] = F[0][i] * F[0][j] + F[1][i] * F[1][j] + F[2][i] * F[2][j];   // F^T F
  arap_jacobi3(C, E);
  double FE[3][3], sig[3];                                        // F E and its column lengths: the singular values (never sqrt(lambda))
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int k = 0; k < 3; k++) FE[i][k] = F[i][0] * E[0][k] + F[i][1] * E[1][k] + F[i][2] * E[2][k];
#pragma unroll
  for (int k = 0; k < 3; k++) sig[k] = sqrt(FE[0][k] * FE[0][k] + FE[1][k] * FE[1][k] + FE[2][k] * FE[2][k]);
#pragma unroll
  for (int pass = 0; pass < 3; pass++) {                          // sig[0] >= sig[1] >= sig[2]
    const int a = pass == 1 ? 1 : 0, b = a + 1;
    if (sig[a] < sig[b]) {
      double t = sig[a]; sig[a] = sig[b]; sig[b] = t;
#pragma unroll
      for (int i = 0; i < 3; i++) {
        t = FE[i][a]; FE[i][a] = FE[i][b]; FE[i][b] = t;
        t = E[i][a]; E[i][a] = E[i][b]; E[i][b] = t;
      }
    }
  }
  if (!(sig[1] > 1e-12 * sig[0])) return;                         // a line or a point (or F = 0, or not finite): no rotation is singled out
  const double ep[3] = {E[0][0], E[1][0], E[2][0]}, eq[3] = {E[0][1], E[1][1], E[2][1]};
  double em[3], up[3], uq[3], um[3];
  arap_cross3(ep, eq, em);                                        // right-handed (ep, eq, em) and (up, uq, um): det Q = +1
  double dpq = 0.0, lq = 0.0;
#pragma unroll
  for (int i = 0; i < 3; i++) { up[i] = FE[i][0] / sig[0]; dpq += up[i] * FE[i][1]; }
#pragma unroll
  for (int i = 0; i < 3; i++) { uq[i] = FE[i][1] - dpq * up[i]; lq += uq[i] * uq[i]; }
  lq = sqrt(lq);
#pragma unroll
  for (int i = 0; i < 3; i++) uq[i] /= lq;
  arap_cross3(up, uq, um);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) Q[i][j] = up[i] * ep[j] + uq[i] * eq[j] + um[i] * em[j];
}

// a column index forced into [0, Vm): an index outside cannot be reported without a read-back, but it must not fault
__device__ __forceinline__ int arap_col(const int* cols, int k, int Vm) { return min(max(cols[k], 0), Vm - 1); }

// sum of N values over the workgroup, the same bits in every thread: wave butterfly, ARAP_WAVES partials in LDS, fixed-order sum.
// The barrier inside is reached by all threads; `part` must not be the array of the previous call (a slow thread may still read it).
template <int N>
__device__ __forceinline__ void arap_block_sum(double (&v)[N], double (*part)[ARAP_WAVES]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; k++) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d);
    if (lane == 0) part[k][wave] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; k++) {
    double s = part[k][0];
#pragma unroll
    for (int w = 1; w < ARAP_WAVES; w++) s += part[k][w];
    v[k] = s;
  }
}

// positions into the float64 state, row sums, which rows are unknowns.  copy_only: V_out = V_init (outer_iterations == 0).
__global__ __launch_bounds__(ARAP_ROW_THREADS) void arap_init_kernel(int Vm, const int* __restrict__ row_offsets, const double* __restrict__ weights,
                                                                     const unsigned char* __restrict__ fixed, const float* V_init, float* V_out,
                                                                     double* __restrict__ x, double* __restrict__ diag, int* __restrict__ free_row,
                                                                     int copy_only) {
  const int i = blockIdx.x * ARAP_ROW_THREADS + threadIdx.x;
  if (i >= Vm) return;
  const float v[3] = {V_init[3 * (size_t)i], V_init[3 * (size_t)i + 1], V_init[3 * (size_t)i + 2]};
  if (copy_only) {
#pragma unroll
    for (int c = 0; c < 3; c++) V_out[3 * (size_t)i + c] = v[c];
    return;
  }
  double d = 0.0;
  for (int k = row_offsets[i]; k < row_offsets[i + 1]; k++) d += weights[k];
#pragma unroll
  for (int c = 0; c < 3; c++) x[(size_t)c * Vm + i] = (double)v[c];
  diag[i] = d;
  free_row[i] = (fixed[i] == 0 && d > 0.0) ? 1 : 0;
}

__global__ __launch_bounds__(ARAP_ROW_THREADS) void arap_local_kernel(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                                      const double* __restrict__ weights, const float* __restrict__ V0,
                                                                      const double* __restrict__ x, double* __restrict__ R) {
  const int i = blockIdx.x * ARAP_ROW_THREADS + threadIdx.x;
  if (i >= Vm) return;
  double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, Q[3][3];
  const double pi[3] = {(double)V0[3 * (size_t)i], (double)V0[3 * (size_t)i + 1], (double)V0[3 * (size_t)i + 2]};
  const double xi[3] = {x[i], x[(size_t)Vm + i], x[2 * (size_t)Vm + i]};
  for (int k = row_offsets[i]; k < row_offsets[i + 1]; k++) {
    const int j = arap_col(cols, k, Vm);
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

// E(P', R) of the state, into *out; one workgroup
__global__ __launch_bounds__(ARAP_THREADS) void arap_energy_kernel(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                                   const double* __restrict__ weights, const float* __restrict__ V0,
                                                                   const double* __restrict__ x, const double* __restrict__ R, double* out) {
  __shared__ double part[1][ARAP_WAVES];
  double acc[1] = {0.0};
  for (int i = threadIdx.x; i < Vm; i += ARAP_THREADS) {
    double Ri[3][3];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int k = 0; k < 3; k++) Ri[c][k] = R[((size_t)c * Vm + i) * 3 + k];
    double e_i = 0.0;
    for (int k = row_offsets[i]; k < row_offsets[i + 1]; k++) {
      const int j = arap_col(cols, k, Vm);
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

// workgroup c: column c of the right-hand side, then the whole PCG of that column.  Every test that leaves a loop holding a
// barrier is made on sums that arap_block_sum left identical in all threads.
__global__ __launch_bounds__(ARAP_THREADS) void arap_global_kernel(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                                   const double* __restrict__ weights, const float* __restrict__ V0,
                                                                   const double* __restrict__ Rall, const double* __restrict__ diag,
                                                                   const int* __restrict__ free_row, double* xall, double* rall, double* pall,
                                                                   double* qall, int cg_iterations, double tol2, float* V_out,
                                                                   double* stats_row) {
  __shared__ double partA[1][ARAP_WAVES], partB[3][ARAP_WAVES];
  const int c = blockIdx.x;
  const double* R = Rall + (size_t)c * Vm * 3;
  double* x = xall + (size_t)c * Vm;
  double* r = rall + (size_t)c * Vm;
  double* p = pall + (size_t)c * Vm;
  double* q = qall + (size_t)c * Vm;
  double s3[3] = {0.0, 0.0, 0.0};                                  // |b|^2, |r|^2, r . z
  for (int i = threadIdx.x; i < Vm; i += ARAP_THREADS) {
    double ri = 0.0, zi = 0.0;
    if (free_row[i]) {
      const double Ri[3] = {R[3 * (size_t)i], R[3 * (size_t)i + 1], R[3 * (size_t)i + 2]};
      const double xi = x[i];
      double b = 0.0, Lx = 0.0, bc = 0.0;
      for (int k = row_offsets[i]; k < row_offsets[i + 1]; k++) {
        const int j = arap_col(cols, k, Vm);
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
  arap_block_sum<3>(s3, partB);                                    // (its barrier also publishes p)
  const double bb = s3[0];
  double rr = s3[1], rz = s3[2];
  int used = 0;
  for (int it = 0; it < cg_iterations; it++) {
    if (!(rr > tol2 * bb)) break;                                  // converged (or not finite): uniform
    double s1[1] = {0.0};
    for (int i = threadIdx.x; i < Vm; i += ARAP_THREADS) {
      if (!free_row[i]) continue;
      const double pi = p[i];
      double qi = 0.0;
      for (int k = row_offsets[i]; k < row_offsets[i + 1]; k++) qi += weights[k] * (pi - p[arap_col(cols, k, Vm)]);
      q[i] = qi;
      s1[0] += pi * qi;
    }
    arap_block_sum<1>(s1, partA);
    if (!(s1[0] > 0.0)) break;                                     // p = 0: nothing left to do; uniform
    const double alpha = rz / s1[0];
    double s2[2] = {0.0, 0.0};                                     // |r|^2, r . z
    for (int i = threadIdx.x; i < Vm; i += ARAP_THREADS) {
      if (!free_row[i]) continue;
      x[i] += alpha * p[i];
      const double ri = r[i] - alpha * q[i];
      r[i] = ri;
      s2[0] += ri * ri; s2[1] += ri * (ri / diag[i]);
    }
    arap_block_sum<2>(s2, partB);
    rr = s2[0];
    const double beta = s2[1] / rz;
    rz = s2[1];
    for (int i = threadIdx.x; i < Vm; i += ARAP_THREADS)
      if (free_row[i]) p[i] = r[i] / diag[i] + beta * p[i];
    used = it + 1;
    __syncthreads();                                               // p complete before the next product reads the neighbours'
  }
  if (V_out)                                                       // the last outer iteration: each thread reads back its own rows
    for (int i = threadIdx.x; i < Vm; i += ARAP_THREADS) V_out[3 * (size_t)i + c] = (float)x[i];
  if (stats_row && threadIdx.x == 0) {
    stats_row[2 + c] = (double)used;
    stats_row[5 + c] = bb > 0.0 ? sqrt(rr / bb) : (rr > 0.0 ? (double)INFINITY : 0.0);
  }
}

int launch_arap_solve(int Vm, const int* row_offsets, const int* cols, const double* weights, const float* V0, const unsigned char* fixed,
                      const float* V_init, int outer_iterations, int cg_iterations, double cg_tolerance, float* V_out, double* stats, void* ws,
                      size_t ws_bytes, hipStream_t s) {
  const size_t need = arap_workspace_bytes(Vm);
  if (ws_bytes < need) { set_error("gm_arap_solve: workspace too small (%zu < %zu)", ws_bytes, need); return 3; }
  ArapWs k = ArapWs::from(ws, (size_t)Vm);
  const dim3 rows((Vm + ARAP_ROW_THREADS - 1) / ARAP_ROW_THREADS);
  hipLaunchKernelGGL(arap_init_kernel, rows, dim3(ARAP_ROW_THREADS), 0, s, Vm, row_offsets, weights, fixed, V_init, V_out, k.x, k.diag, k.free_row,
                     outer_iterations == 0 ? 1 : 0);
  for (int it = 0; it < outer_iterations; it++) {
    double* row = stats ? stats + 8 * (size_t)it : nullptr;
    hipLaunchKernelGGL(arap_local_kernel, rows, dim3(ARAP_ROW_THREADS), 0, s, Vm, row_offsets, cols, weights, V0, k.x, k.R);
    if (row) hipLaunchKernelGGL(arap_energy_kernel, dim3(1), dim3(ARAP_THREADS), 0, s, Vm, row_offsets, cols, weights, V0, k.x, k.R, row);
    hipLaunchKernelGGL(arap_global_kernel, dim3(3), dim3(ARAP_THREADS), 0, s, Vm, row_offsets, cols, weights, V0, k.R, k.diag, k.free_row, k.x, k.r,
                       k.p, k.q, cg_iterations, cg_tolerance * cg_tolerance, it == outer_iterations - 1 ? V_out : nullptr, row);
    if (row) hipLaunchKernelGGL(arap_energy_kernel, dim3(1), dim3(ARAP_THREADS), 0, s, Vm, row_offsets, cols, weights, V0, k.x, k.R, row + 1);
  }
  GM_HIP(hipGetLastError());
  return 0;
}

}  // namespace gm
