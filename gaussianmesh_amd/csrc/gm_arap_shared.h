// gm_arap_shared.h -- the device primitives gm_arap.hip, gm_pose_interp.hip and gm_dynamics.hip share: the polar rotation of a 3 x 3
// matrix, the sum of a CSR row's weights, the workgroup sum that leaves the same bits in every thread, and on top of it the step loop of
// the one-workgroup column PCG (arap_global_kernel, pi_solve_kernel, dyn_global_kernel).  Device code only; all are inlined where they are
// used.
#pragma once
#include "gm_common.h"
#include "gm_mat3.h"

namespace gm {

#define ARAP_WAVES 16         // waves of the 1024-thread workgroups (arap_global / arap_energy / pi_solve)

// the proper rotation closest to F (max tr(Q^T F)); identity for rank <= 1.  Always a proper rotation (to 1e-14).  With singular values
// s0 >= s1 >= s2 of F and gap = (s1 + sign(det F) s2) / s0:  gap >= 1e-2: the SVD's U diag(1, 1, det) V^T element by element, tr(Q^T F)
// within 64 eps s0 of its maximum.  Below (a needle: s1 under about 1e-3 s0; a reflection with s1 ~ s2): F^T F has squared the condition
// number, and Q maximises tr(Q^T F) only to within 8 sqrt(eps) s0 - it is not element by element the SVD's rotation but differs from it
// by a turn about the strongest direction, which the trace barely sees (an ARAP row's energy: at most twice that bar).
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
  jacobi3(C, E);
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
  cross3(ep, eq, em);                                        // right-handed (ep, eq, em) and (up, uq, um): det Q = +1
  double dpq = 0.0, lq = 0.0;
#pragma unroll
  for (int i = 0; i < 3; i++) { up[i] = FE[i][0] / sig[0]; dpq += up[i] * FE[i][1]; }
#pragma unroll
  for (int i = 0; i < 3; i++) { uq[i] = FE[i][1] - dpq * up[i]; lq += uq[i] * uq[i]; }
  lq = sqrt(lq);
#pragma unroll
  for (int i = 0; i < 3; i++) uq[i] /= lq;
  cross3(up, uq, um);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) Q[i][j] = up[i] * ep[j] + uq[i] * eq[j] + um[i] * em[j];
}

// d_i = sum_j w_ij of CSR row i, and whether the row is an unknown of the linear systems: not held and d_i > 0
struct ArapRowSum { double d; int free_row; };
__device__ __forceinline__ ArapRowSum arap_row_sum(const int* __restrict__ row_offsets, const double* __restrict__ weights,
                                                   const unsigned char* __restrict__ held, int i) {
  double d = 0.0;
  for (int k = row_offsets[i]; k < row_offsets[i + 1]; k++) d += weights[k];
  return {d, (held[i] == 0 && d > 0.0) ? 1 : 0};
}

// |r| / |b| as the stats rows report it
__device__ __forceinline__ double arap_rel_residual(double bb, double rr) {
  return bb > 0.0 ? sqrt(rr / bb) : (rr > 0.0 ? (double)INFINITY : 0.0);
}

// sum of N values over the workgroup of W waves, the same bits in every thread: wave butterfly, W partials in LDS, fixed-order sum.
// The barrier inside is reached by all threads; `part` must not be the array of the previous call (a slow thread may still read it).
template <int N, int W = ARAP_WAVES>
__device__ __forceinline__ void arap_block_sum(double (&v)[N], double (*part)[W]) {
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
    for (int w = 1; w < W; w++) s += part[k][w];
    v[k] = s;
  }
}

// The Jacobi-preconditioned CG of one column (x, r, p, q: [Vm]) by one workgroup of ARAP_WAVES waves, rows strided over the threads.  The
// caller has written r = b - L x and p = r / diag (0 in held rows, for the whole solve) and holds this thread's share of |b|^2, |r|^2,
// r . z in s3; partA and partB are two LDS arrays of its own.  Stops at |r|^2 <= tol2 |b|^2, at p . A p <= 0 or after cg_iterations
// steps.  Every test that leaves the loop, which holds barriers, is made on sums that arap_block_sum left identical in all threads.
// Returns bb = |b|^2, rr = the last |r|^2, used = steps taken.
// SHIFTED: the operator is diag(shift) + L (gm_dynamics.hip: the mass term of an implicit step), and diag is then its diagonal,
// shift_i + d_i; the default is the plain Laplacian, and shift is not read.
struct ArapPcgResult { double bb, rr; int used; };
template <bool SHIFTED = false>
__device__ __forceinline__ ArapPcgResult arap_pcg_steps(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                        const double* __restrict__ weights, const double* __restrict__ diag,
                                                        const int* __restrict__ free_row, double* x, double* r, double* p, double* q,
                                                        int cg_iterations, double tol2, double (&s3)[3], double (*partA)[ARAP_WAVES],
                                                        double (*partB)[ARAP_WAVES], const double* __restrict__ shift = nullptr) {
  constexpr int THREADS = ARAP_WAVES * 64;
  arap_block_sum<3>(s3, partB);                                    // (its barrier also publishes p)
  const double bb = s3[0];
  double rr = s3[1], rz = s3[2];
  int used = 0;
  for (int it = 0; it < cg_iterations; it++) {
    if (!(rr > tol2 * bb)) break;                                  // converged (or not finite): uniform
    double s1[1] = {0.0};
    for (int i = threadIdx.x; i < Vm; i += THREADS) {
      if (!free_row[i]) continue;
      const double pi = p[i];
      double qi = 0.0;
      for (int k = row_offsets[i]; k < row_offsets[i + 1]; k++) qi += weights[k] * (pi - p[clamp_index(cols[k], Vm)]);
      if constexpr (SHIFTED) qi += shift[i] * pi;
      q[i] = qi;
      s1[0] += pi * qi;
    }
    arap_block_sum<1>(s1, partA);
    if (!(s1[0] > 0.0)) break;                                     // p = 0: nothing left to do; uniform
    const double alpha = rz / s1[0];
    double s2[2] = {0.0, 0.0};                                     // |r|^2, r . z
    for (int i = threadIdx.x; i < Vm; i += THREADS) {
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
    for (int i = threadIdx.x; i < Vm; i += THREADS)
      if (free_row[i]) p[i] = r[i] / diag[i] + beta * p[i];
    used = it + 1;
    __syncthreads();                                               // p complete before the next product reads the neighbours'
  }
  return {bb, rr, used};
}

}  // namespace gm
