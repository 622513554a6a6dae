// gm_mat3.h -- the double-precision 3x3 helpers of the polar decompositions (gm_mesh.hip mesh_rs_kernel, gm_arap.hip arap_rotation).
#pragma once
#include "gm_common.h"

namespace gm {

__device__ __forceinline__ void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// eigen-decomposition of a symmetric 3x3 (cyclic Jacobi): A -> diagonal in place, V columns = eigenvectors
__device__ __forceinline__ void jacobi3(double A[3][3], double V[3][3]) {
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

}  // namespace gm
