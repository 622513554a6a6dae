// gm_pose_interp.hip -- the meshes BETWEEN two key poses of a proxy mesh (gm_pose_interp): every face's deformation gradient is
// interpolated in polar form and the vertices are recovered from one Poisson solve per coordinate (Alexa, Cohen-Or & Levin, "As-Rigid-
// As-Possible Shape Interpolation", SIGGRAPH 2000; Xu, Zhang, Wang & Bao, "Poisson Shape Interpolation", SPM 2005).  The reference has no
// such stage; the result is defined by arithmetic.  A linear blend of two poses collapses whatever rotates between them; this does not.
//
// DEFINITION.  Rest vertices V0 (float32, read as float64), faces, key poses A and B ([Vm,3] float32, read as float64), parameters
// t[0 .. T) (float64, each in [0, 1]).  All arithmetic is float64; the result is rounded to float32 once, at the end.
//   Per face f = (a, b, c) with three distinct ids and |u x w| > 1e-30 at rest (u = b - a, w = c - a; edge_csr's rule - a face that fails
//   it adds nothing anywhere):
//     D(V) = [u | w | n], n = (u x w) / |u x w|, n = 0 where the deformed |u x w| <= 1e-30;   F_A = D(A) D(V0)^-1, likewise F_B.
//     R_A = the proper rotation closest to F_A (arap_rotation: identity for rank <= 1), S_A = sym(R_A^T F_A) as six entries; R_B, S_B.
//     omega = log(R_A^T R_B), a rotation vector of angle in [0, pi]:  with Rrel = R_A^T R_B, v = vee(Rrel - Rrel^T) / 2, s = |v|,
//       c = (tr Rrel - 1) / 2, theta = atan2(s, c):   s >= 1e-6: omega = v theta / s;   s < 1e-6 and c > 0: omega = v;
//       s < 1e-6 and c <= 0: omega = theta axis, axis = the column of sym(Rrel) - c I with the largest diagonal entry, normalised and
//       signed so that axis . v >= 0.  Within 1e-3 rad of a half turn the side a face turns to is not specified (the two geodesics
//       are equally long): the user adds a key.
//     T_f(t) = R_A exp(t omega) ((1 - t) S_A + t S_B), exp by Rodrigues' formula.  T_f(0) = F_A and T_f(1) = F_B.
//   For every free vertex i:   sum_j w_ij (x_i - x_j) = sum_{f holding i} sum_{j in f, j != i} w^f_ij T_f(t) (p_i - p_j),
//     w^f_ij = max(0.5 cot(angle of f opposite edge ij), 1e-3) from V0 as arap.edge_csr forms it, so sum_f w^f_ij = w_ij (the caller's
//     CSR: the matrix of the ARAP global step) and each key solves its own system exactly.
//   Held rows (held[i] != 0, and rows whose weights sum to 0) stay at (1 - t) A_i + t B_i.  With C > 0 components (the caller's CSR of
//     their rows, label[i] = the component of vertex i or -1) every component is then translated so that the mean of its vertices is
//     (1 - t) mean_A + t mean_B of that component: a spin about the centroid comes out as a spin.  C = 0: nothing is translated.
//   Each (frame, coordinate) is one Jacobi-preconditioned CG solve warm-started from (1 - t) A + t B, stopped at
//     |r|_2 <= cg_tolerance |b|_2 (b the right-hand side of the system restricted to the free rows) or after cg_iterations steps; the
//     test is made before the first step too.
//
// KERNELS.  Six launches whatever T; the frame is the second grid dimension of all but the first.
//   pi_face_keys  one thread per face: the cotangent weights and the key pair's record R_A, omega, S_A, S_B (24 doubles).  Once per call.
//   pi_transform  one thread per (face, frame): T_f(t), 9 doubles - the sincos runs once per face and frame, not once per corner.
//   pi_rhs        one thread per (vertex, frame): gathers the vertex's faces through the vertex -> face CSR (deform.vertex_face_adjacency)
//                 into the three right-hand-side entries, writes the warm start; frame 0's threads write diag and free_row.
//   pi_solve      grid (3, T) of 1024 threads: workgroup (c, t) runs the WHOLE PCG of coordinate c of frame t, rows strided over the
//                 threads, no launch per step.  The step loop is arap_pcg_steps (gm_arap_shared.h), the one arap_global_kernel runs:
//                 dot products through arap_block_sum, so every exit test is uniform.  No workgroup waits on another.
//   pi_shift      one workgroup per (component, frame): the component's sums of x, A and B in a fixed order, the translation.
//   pi_finish     one thread per (vertex, frame): adds the translation of the vertex's component, rounds, writes V_out.
// A frame reads nothing another frame wrote and every sum has one fixed order: a frame's bits do not depend on the batch it rides in,
// on where it stands in it or on the call.  No atomics.  One workgroup per system keeps x / r / p / q / b (5 x 8 B x Vm) in L2 up to
// the sizes of a proxy mesh (7.5 k vertices: 300 KB per coordinate); a whole-chip solve for meshes far above that is not built.
// Conventions of gm_closest.hip: caller workspace, stream-ordered, no device allocation, no host wait anywhere in this file.
#include "gm_common.h"
#include "gm_check.h"
#include "gm_mat3.h"
#include "gm_arap_shared.h"

namespace gm {

#define PI_THREADS 1024       // pi_solve: one workgroup of ARAP_WAVES waves
#define PI_ROW_THREADS 256    // every other kernel
#define PI_ROW_WAVES 4
#define PI_KEY 24             // doubles of a face's record: R_A [9] row-major, omega [3], S_A [6], S_B [6] (xx xy xz yy yz zz)

struct PoseInterpWs {
  double* keys;    // [F][PI_KEY]
  double* fw;      // [F][3] weight of the corner k of face f (the edge opposite it); 0 0 0 for a face that adds nothing
  double* Tf;      // [T][F][9] row-major
  double* diag;    // [Vm] sum_j w_ij
  int* free_row;   // [Vm] 1 = a row of the linear system
  double* x;       // frame 0's slab: x, r, p, q, b, each [3][Vm]; frame t's starts t * slab doubles later
  size_t slab;     // (after the solve a frame's r holds its components' translations, [C][3])
  char* end;
  static PoseInterpWs from(void* ws, size_t Vm, size_t F, size_t T) {
    char* p = reinterpret_cast<char*>(ws);
    PoseInterpWs k;
    k.keys = carve<double>(p, PI_KEY * F);
    k.fw = carve<double>(p, 3 * F);
    k.Tf = carve<double>(p, 9 * F * T);
    k.diag = carve<double>(p, Vm);
    k.free_row = carve<int>(p, Vm);
    k.x = carve<double>(p, 0);
    for (int a = 0; a < 5; a++) carve<double>(p, 3 * Vm);
    k.slab = (size_t)(carve<double>(p, 0) - k.x);
    k.end = reinterpret_cast<char*>(k.x + T * k.slab);
    return k;
  }
};

__device__ __forceinline__ void pi_load3(const float* __restrict__ V, size_t i, double o[3]) {
  o[0] = (double)V[3 * i]; o[1] = (double)V[3 * i + 1]; o[2] = (double)V[3 * i + 2];
}

// D = [u | w | n] of the corner (a, b, c) of V; returns |u x w| (n = 0 where it is <= 1e-30)
__device__ __forceinline__ double pi_frame(const float* __restrict__ V, size_t a, size_t b, size_t c, double D[3][3]) {
  double pa[3], pb[3], pc[3], u[3], w[3], n[3];
  pi_load3(V, a, pa); pi_load3(V, b, pb); pi_load3(V, c, pc);
#pragma unroll
  for (int k = 0; k < 3; k++) { u[k] = pb[k] - pa[k]; w[k] = pc[k] - pa[k]; }
  cross3(u, w, n);
  const double area2 = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  const double inv = area2 > 1e-30 ? 1.0 / area2 : 0.0;
#pragma unroll
  for (int k = 0; k < 3; k++) { D[k][0] = u[k]; D[k][1] = w[k]; D[k][2] = area2 > 1e-30 ? n[k] * inv : 0.0; }
  return area2;
}

__device__ __forceinline__ void pi_mul(const double A[3][3], const double B[3][3], double O[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) O[i][j] = A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j];
}

// O = A^T B
__device__ __forceinline__ void pi_mul_tn(const double A[3][3], const double B[3][3], double O[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) O[i][j] = A[0][i] * B[0][j] + A[1][i] * B[1][j] + A[2][i] * B[2][j];
}

// F = D(V) Dinv, R = its polar rotation, S = sym(R^T F) as six entries
__device__ __forceinline__ void pi_polar(const float* __restrict__ V, size_t a, size_t b, size_t c, const double Dinv[3][3], double R[3][3], double S[6]) {
  double D[3][3], Fm[3][3], M[3][3];
  pi_frame(V, a, b, c, D);
  pi_mul(D, Dinv, Fm);
  arap_rotation(Fm, R);
  pi_mul_tn(R, Fm, M);
  S[0] = M[0][0]; S[1] = 0.5 * (M[0][1] + M[1][0]); S[2] = 0.5 * (M[0][2] + M[2][0]);
  S[3] = M[1][1]; S[4] = 0.5 * (M[1][2] + M[2][1]); S[5] = M[2][2];
}

// the rotation vector of Rrel, angle in [0, pi] (the rule of the DEFINITION)
__device__ __forceinline__ void pi_log(const double Q[3][3], double omega[3]) {
  const double v[3] = {0.5 * (Q[2][1] - Q[1][2]), 0.5 * (Q[0][2] - Q[2][0]), 0.5 * (Q[1][0] - Q[0][1])};
  const double s = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  const double c = 0.5 * (Q[0][0] + Q[1][1] + Q[2][2] - 1.0);
  const double theta = atan2(s, c);
  if (s >= 1e-6) {
#pragma unroll
    for (int k = 0; k < 3; k++) omega[k] = v[k] * (theta / s);
    return;
  }
  if (c > 0.0) {
#pragma unroll
    for (int k = 0; k < 3; k++) omega[k] = v[k];
    return;
  }
  double M[3][3];                                                  // sym(Q) - c I = (1 - c) axis axis^T
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) M[i][j] = 0.5 * (Q[i][j] + Q[j][i]) - (i == j ? c : 0.0);
  int m = 0;
  if (M[1][1] > M[m][m]) m = 1;
  if (M[2][2] > M[m][m]) m = 2;
  double ax[3] = {M[0][m], M[1][m], M[2][m]};
  const double l = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
  const double sign = (ax[0] * v[0] + ax[1] * v[1] + ax[2] * v[2]) >= 0.0 ? 1.0 : -1.0;
#pragma unroll
  for (int k = 0; k < 3; k++) omega[k] = l > 0.0 ? sign * theta * ax[k] / l : 0.0;
}

__global__ __launch_bounds__(PI_ROW_THREADS) void pi_face_keys_kernel(int Vm, int F, const float* __restrict__ V0, const int* __restrict__ faces,
                                                                      const float* __restrict__ A, const float* __restrict__ B,
                                                                      double* __restrict__ keys, double* __restrict__ fw) {
  const int f = blockIdx.x * PI_ROW_THREADS + threadIdx.x;
  if (f >= F) return;
  double* rec = keys + (size_t)f * PI_KEY;
  double* wk = fw + 3 * (size_t)f;
  const size_t id[3] = {face_vertex(faces, 3 * (size_t)f, Vm), face_vertex(faces, 3 * (size_t)f + 1, Vm), face_vertex(faces, 3 * (size_t)f + 2, Vm)};
  double D0[3][3];
  const double area2 = pi_frame(V0, id[0], id[1], id[2], D0);
  if (id[0] == id[1] || id[1] == id[2] || id[0] == id[2] || !(area2 > 1e-30)) {
#pragma unroll
    for (int k = 0; k < PI_KEY; k++) rec[k] = 0.0;
    wk[0] = wk[1] = wk[2] = 0.0;
    return;
  }
  double P[3][3];
#pragma unroll
  for (int k = 0; k < 3; k++) pi_load3(V0, id[k], P[k]);
#pragma unroll
  for (int k = 0; k < 3; k++) {                                    // corner k: u, w to the two other vertices, as edge_csr takes them
    const int ia = (k + 1) % 3, ib = (k + 2) % 3;
    double u[3], w[3], n[3];
#pragma unroll
    for (int a = 0; a < 3; a++) { u[a] = P[ia][a] - P[k][a]; w[a] = P[ib][a] - P[k][a]; }
    cross3(u, w, n);
    const double ar = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const double cot = 0.5 * (u[0] * w[0] + u[1] * w[1] + u[2] * w[2]) / ar;
    wk[k] = ar > 1e-30 ? fmax(cot, 1e-3) : 0.0;
  }
  // D0^-1 by cofactors: row k = (column k+1 x column k+2) / det, det = |u x w| (n is the unit normal)
  double col[3][3], Dinv[3][3];
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int a = 0; a < 3; a++) col[k][a] = D0[a][k];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    double r[3];
    cross3(col[(k + 1) % 3], col[(k + 2) % 3], r);
#pragma unroll
    for (int a = 0; a < 3; a++) Dinv[k][a] = r[a] / area2;
  }
  double RA[3][3], RB[3][3], SA[6], SB[6], Rrel[3][3], omega[3];
  pi_polar(A, id[0], id[1], id[2], Dinv, RA, SA);
  pi_polar(B, id[0], id[1], id[2], Dinv, RB, SB);
  pi_mul_tn(RA, RB, Rrel);
  pi_log(Rrel, omega);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) rec[3 * i + j] = RA[i][j];
#pragma unroll
  for (int k = 0; k < 3; k++) rec[9 + k] = omega[k];
#pragma unroll
  for (int k = 0; k < 6; k++) { rec[12 + k] = SA[k]; rec[18 + k] = SB[k]; }
}

__global__ __launch_bounds__(PI_ROW_THREADS) void pi_transform_kernel(int F, const double* __restrict__ keys, const double* __restrict__ ts,
                                                                      double* __restrict__ Tf) {
  const int f = blockIdx.x * PI_ROW_THREADS + threadIdx.x;
  if (f >= F) return;
  const double t = ts[blockIdx.y];
  const double* rec = keys + (size_t)f * PI_KEY;
  double* out = Tf + ((size_t)blockIdx.y * F + f) * 9;
  double RA[3][3], E[3][3], S[3][3], RE[3][3], O[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) RA[i][j] = rec[3 * i + j];
  const double k[3] = {t * rec[9], t * rec[10], t * rec[11]};
  const double th = sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2]);
  double a = 1.0, b = 0.5;                                         // sin(th) / th and (1 - cos th) / th^2 = (sin(th/2) / (th/2))^2 / 2
  if (th > 1e-8) {
    const double h = sin(0.5 * th) / (0.5 * th);
    a = sin(th) / th; b = 0.5 * h * h;
  }
  const double K[3][3] = {{0.0, -k[2], k[1]}, {k[2], 0.0, -k[0]}, {-k[1], k[0], 0.0}};
  double K2[3][3];
  pi_mul(K, K, K2);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) E[i][j] = (i == j ? 1.0 : 0.0) + a * K[i][j] + b * K2[i][j];
  double s[6];
#pragma unroll
  for (int e = 0; e < 6; e++) s[e] = (1.0 - t) * rec[12 + e] + t * rec[18 + e];
  S[0][0] = s[0]; S[0][1] = S[1][0] = s[1]; S[0][2] = S[2][0] = s[2]; S[1][1] = s[3]; S[1][2] = S[2][1] = s[4]; S[2][2] = s[5];
  pi_mul(RA, E, RE);
  pi_mul(RE, S, O);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) out[3 * i + j] = O[i][j];
}

__global__ __launch_bounds__(PI_ROW_THREADS) void pi_rhs_kernel(int Vm, int F, const int* __restrict__ row_offsets, const double* __restrict__ weights,
                                                                const float* __restrict__ V0, const int* __restrict__ faces,
                                                                const int* __restrict__ vf_offsets, const int* __restrict__ vf_faces,
                                                                const unsigned char* __restrict__ held, const float* __restrict__ A,
                                                                const float* __restrict__ B, const double* __restrict__ ts,
                                                                const double* __restrict__ fw, const double* __restrict__ Tf, double* xall,
                                                                double* __restrict__ diag, int* __restrict__ free_row, size_t slab) {
  const int i = blockIdx.x * PI_ROW_THREADS + threadIdx.x;
  if (i >= Vm) return;
  const double t = ts[blockIdx.y];
  double* x = xall + blockIdx.y * slab;
  double* bcol = x + 12 * (size_t)Vm;
  const double* T = Tf + (size_t)blockIdx.y * F * 9;
  double pi[3], pa[3], pb[3], rhs[3] = {0.0, 0.0, 0.0};
  pi_load3(V0, (size_t)i, pi); pi_load3(A, (size_t)i, pa); pi_load3(B, (size_t)i, pb);
  for (int k = vf_offsets[i]; F > 0 && k < vf_offsets[i + 1]; k++) {
    const size_t f = (size_t)clamp_index(vf_faces[k], F);
    const double w[3] = {fw[3 * f], fw[3 * f + 1], fw[3 * f + 2]};
    if (!(w[0] > 0.0)) continue;                                   // a face that adds nothing
    const size_t id[3] = {face_vertex(faces, 3 * f, Vm), face_vertex(faces, 3 * f + 1, Vm), face_vertex(faces, 3 * f + 2, Vm)};
    const int m = id[0] == (size_t)i ? 0 : (id[1] == (size_t)i ? 1 : 2);
    if (id[m] != (size_t)i) continue;                              // (an adjacency that names a face without this vertex)
    const int m1 = (m + 1) % 3, m2 = (m + 2) % 3;
    double p1[3], p2[3], e[3];
    pi_load3(V0, id[m1], p1); pi_load3(V0, id[m2], p2);
#pragma unroll
    for (int a = 0; a < 3; a++) e[a] = w[m2] * (pi[a] - p1[a]) + w[m1] * (pi[a] - p2[a]);   // edge (i, m1) lies opposite corner m2
#pragma unroll
    for (int a = 0; a < 3; a++) rhs[a] += T[9 * f + 3 * a] * e[0] + T[9 * f + 3 * a + 1] * e[1] + T[9 * f + 3 * a + 2] * e[2];
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    x[(size_t)c * Vm + i] = (1.0 - t) * pa[c] + t * pb[c];
    bcol[(size_t)c * Vm + i] = rhs[c];
  }
  if (blockIdx.y) return;                                          // the mesh's own words have one writer: frame 0
  const ArapRowSum row = arap_row_sum(row_offsets, weights, held, i);
  diag[i] = row.d;
  free_row[i] = row.free_row;
}

// workgroup (c, t): the whole PCG of coordinate c of frame t: r, p and the first sums from the stored b, then arap_pcg_steps
static_assert(PI_THREADS == ARAP_WAVES * 64, "pi_solve_kernel strides its rows as arap_pcg_steps does");
__global__ __launch_bounds__(PI_THREADS) void pi_solve_kernel(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                              const double* __restrict__ weights, const double* __restrict__ diag,
                                                              const int* __restrict__ free_row, double* xall, int cg_iterations, double tol2,
                                                              double* stats, size_t slab) {
  __shared__ double partA[1][ARAP_WAVES], partB[3][ARAP_WAVES];
  const int c = blockIdx.x;
  double* x = xall + blockIdx.y * slab + (size_t)c * Vm;
  double* r = x + 3 * (size_t)Vm;
  double* p = x + 6 * (size_t)Vm;
  double* q = x + 9 * (size_t)Vm;
  const double* b = x + 12 * (size_t)Vm;
  double s3[3] = {0.0, 0.0, 0.0};                                  // |b|^2, |r|^2, r . z
  for (int i = threadIdx.x; i < Vm; i += PI_THREADS) {
    double ri = 0.0, zi = 0.0;
    if (free_row[i]) {
      const double xi = x[i];
      double Lx = 0.0, bc = b[i];
      for (int k = row_offsets[i]; k < row_offsets[i + 1]; k++) {
        const int j = clamp_index(cols[k], Vm);
        const double w = weights[k], xj = x[j];
        Lx += w * (xi - xj);
        if (!free_row[j]) bc += w * xj;                            // a held neighbour moves to the right-hand side
      }
      ri = b[i] - Lx; zi = ri / diag[i];
      s3[0] += bc * bc; s3[1] += ri * ri; s3[2] += ri * zi;
    }
    r[i] = ri; p[i] = zi;                                          // held rows: r = p = 0, for the whole solve
  }
  const ArapPcgResult cg = arap_pcg_steps(Vm, row_offsets, cols, weights, diag, free_row, x, r, p, q, cg_iterations, tol2, s3, partA, partB);
  if (stats && threadIdx.x == 0) {
    double* row = stats + 6 * (size_t)blockIdx.y;
    row[c] = (double)cg.used;
    row[3 + c] = arap_rel_residual(cg.bb, cg.rr);
  }
}

// workgroup (k, t): the translation of component k in frame t, into the frame's r (the solve is over): shift[k][3]
__global__ __launch_bounds__(PI_ROW_THREADS) void pi_shift_kernel(int Vm, const int* __restrict__ comp_offsets, const int* __restrict__ comp_rows,
                                                                  const float* __restrict__ A, const float* __restrict__ B,
                                                                  const double* __restrict__ ts, double* xall, size_t slab) {
  __shared__ double part[9][PI_ROW_WAVES];
  const double t = ts[blockIdx.y];
  const double* x = xall + blockIdx.y * slab;
  double* shift = xall + blockIdx.y * slab + 3 * (size_t)Vm;
  const int lo = comp_offsets[blockIdx.x], hi = comp_offsets[blockIdx.x + 1];
  double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};                       // sums of x, A, B
  for (int k = lo + (int)threadIdx.x; k < hi; k += PI_ROW_THREADS) {
    const size_t i = (size_t)clamp_index(comp_rows[k], Vm);
#pragma unroll
    for (int c = 0; c < 3; c++) { s[c] += x[(size_t)c * Vm + i]; s[3 + c] += (double)A[3 * i + c]; s[6 + c] += (double)B[3 * i + c]; }
  }
  arap_block_sum<9, PI_ROW_WAVES>(s, part);
  if (threadIdx.x < 3 && hi > lo) {
    const int c = threadIdx.x;
    const double n = (double)(hi - lo);
    shift[3 * (size_t)blockIdx.x + c] = ((1.0 - t) * (s[3 + c] / n) + t * (s[6 + c] / n)) - s[c] / n;
  }
}

__global__ __launch_bounds__(PI_ROW_THREADS) void pi_finish_kernel(int Vm, int C, const int* __restrict__ label, const double* __restrict__ xall,
                                                                   float* __restrict__ V_out, size_t slab) {
  const int i = blockIdx.x * PI_ROW_THREADS + threadIdx.x;
  if (i >= Vm) return;
  const double* x = xall + blockIdx.y * slab;
  const double* shift = x + 3 * (size_t)Vm;
  float* out = V_out + (size_t)blockIdx.y * 3 * Vm;
  const int l = C > 0 ? label[i] : -1;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    double v = x[(size_t)c * Vm + i];
    if (l >= 0 && l < C) v += shift[3 * (size_t)l + c];
    out[3 * (size_t)i + c] = (float)v;
  }
}

}  // namespace gm

// ---------------------------------------------------------------------------------------------
// the entry points (include/gmesh_hip.h): their refusals, then the launches
using namespace gm;

extern "C" {

size_t gm_pose_interp_workspace_bytes(int Vm, int F, int T) {
  if (Vm < 1 || F < 0 || T < 1 || T > GM_POSE_INTERP_BATCH_MAX) return 0;
  return (size_t)PoseInterpWs::from(nullptr, (size_t)Vm, (size_t)F, (size_t)T).end + 256;
}

int gm_pose_interp(int T, int Vm, int F, const int* row_offsets, const int* cols, const double* weights, const float* V0, const int* faces,
                   const int* vf_offsets, const int* vf_faces, const unsigned char* held, int C, const int* comp_offsets, const int* comp_rows,
                   const int* label, const float* A, const float* B, const double* ts, int cg_iterations, double cg_tolerance, float* V_out,
                   double* stats, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "gm_pose_interp";
  if (T < 1 || T > GM_POSE_INTERP_BATCH_MAX) { set_error("%s: T = %d (1 .. %d)", fn, T, GM_POSE_INTERP_BATCH_MAX); return GM_ERR_INVALID_ARG; }
  if (Vm < 1) { set_error("%s: Vm = %d (must be positive)", fn, Vm); return GM_ERR_INVALID_ARG; }
  if (F < 0) { set_error("%s: F = %d (negative)", fn, F); return GM_ERR_INVALID_ARG; }
  if (C < 0 || C > Vm) { set_error("%s: C = %d (0 .. Vm = %d)", fn, C, Vm); return GM_ERR_INVALID_ARG; }
  if (cg_iterations < 1) { set_error("%s: cg_iterations = %d (at least 1)", fn, cg_iterations); return GM_ERR_INVALID_ARG; }
  if (!(cg_tolerance >= 0.0) || cg_tolerance > 1.7976931348623157e308) {
    set_error("%s: cg_tolerance must be finite and not negative", fn); return GM_ERR_INVALID_ARG;
  }
  if (!row_offsets || !cols || !weights || !V0 || !vf_offsets || !held || !A || !B || !ts || !V_out || !workspace || (F > 0 && (!faces || !vf_faces)) ||
      (C > 0 && (!comp_offsets || !comp_rows || !label))) {
    set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG;
  }
  // V0, A and B are only read and may be one array (a key may be the rest pose); an output or the workspace meets nothing
  const ByteRange rg[7] = {{V0, 12 * (size_t)Vm, "V0", false}, {A, 12 * (size_t)Vm, "A", false}, {B, 12 * (size_t)Vm, "B", false},
                           {ts, 8 * (size_t)T, "ts", false}, {V_out, 12 * (size_t)Vm * T, "V_out", true}, {stats, 48 * (size_t)T, "stats", true},
                           {workspace, workspace_bytes, "workspace", true}};
  if (int rc = check_ranges(fn, rg)) return rc;
  const size_t need = gm_pose_interp_workspace_bytes(Vm, F, T);
  if (workspace_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need); return GM_ERR_BUFFER; }
  const PoseInterpWs k = PoseInterpWs::from(workspace, (size_t)Vm, (size_t)F, (size_t)T);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 threads(PI_ROW_THREADS), rows((Vm + PI_ROW_THREADS - 1) / PI_ROW_THREADS, T);
  if (F > 0) {
    const int G = (F + PI_ROW_THREADS - 1) / PI_ROW_THREADS;
    hipLaunchKernelGGL(pi_face_keys_kernel, dim3(G), threads, 0, s, Vm, F, V0, faces, A, B, k.keys, k.fw);
    hipLaunchKernelGGL(pi_transform_kernel, dim3(G, T), threads, 0, s, F, k.keys, ts, k.Tf);
  }
  hipLaunchKernelGGL(pi_rhs_kernel, rows, threads, 0, s, Vm, F, row_offsets, weights, V0, faces, vf_offsets, vf_faces, held, A, B, ts, k.fw, k.Tf, k.x,
                     k.diag, k.free_row, k.slab);
  hipLaunchKernelGGL(pi_solve_kernel, dim3(3, T), dim3(PI_THREADS), 0, s, Vm, row_offsets, cols, weights, k.diag, k.free_row, k.x, cg_iterations,
                     cg_tolerance * cg_tolerance, stats, k.slab);
  if (C > 0) hipLaunchKernelGGL(pi_shift_kernel, dim3(C, T), threads, 0, s, Vm, comp_offsets, comp_rows, A, B, ts, k.x, k.slab);
  hipLaunchKernelGGL(pi_finish_kernel, rows, threads, 0, s, Vm, C, label, k.x, V_out, k.slab);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // extern "C"
