// gm_skin.hip -- the proxy mesh posed from a skeleton: bone-heat skinning weights (gm_skin_weights; Baran & Popovic, "Automatic Rigging and
// Animation of 3D Characters", SIGGRAPH 2007) and the per-frame skinning of the rest mesh by bone transforms (gm_skin_pose), linear or by
// dual quaternions (Kavan, Collins, Zara & O'Sullivan, "Geometric Skinning with Approximate Dual Quaternion Blending", TOG 2008).  The
// reference has no such stage; the result is defined by arithmetic.
//
// DEFINITION, WEIGHTS.  Rest vertices V0 (float32, read as float64), J bones as rest segments bone_a[j] -> bone_b[j] (float32, read as
// float64), area float64 [Vm] (dynamics.vertex_masses at density 1), the cotangent CSR of arap.edge_csr (L: d_i = sum_j w_ij).
//   d2_ij = |V0_i - (a_j + s (b_j - a_j))|^2, s = clamp(((V0_i - a_j) . (b_j - a_j)) / |b_j - a_j|^2, 0, 1), s = 0 for a bone of no length.
//   d2min_i = max(min_j d2_ij, (1e-3 D)^2), D the diagonal of the bounding box of all rows of V0 (float32 min / max, the rest float64).
//   N(i) = { j : d2_ij <= (1 + 1e-4)^2 d2min_i }   (Pinocchio's rule: a vertex at a joint is shared by the bones that meet there).
//   h_i = heat area_i / d2min_i (0 where area_i is not positive);  p_ij = 1 / |N(i)| on N(i), 0 elsewhere.
//   Row i is an UNKNOWN iff h_i + d_i > 0 (an unreferenced vertex is none).  Column j solves (diag(h) + L) w_j = h o p_j over the unknowns
//   by Jacobi-preconditioned CG from x0 = p_j, stopped at |r|_2 <= cg_tolerance |b|_2 or after cg_iterations steps, the test made before
//   the first step too (arap_pcg_steps<true>, shift = h).  Rows that are no unknowns keep p_ij.  Every cotangent weight is positive, so
//   the matrix is an M-matrix: in exact arithmetic 0 <= w_ij <= 1 and sum_j w_ij = 1 on every unknown row.
//   COMPACTION.  Per vertex v_j = max(w_ij, 0); slot s = 0 .. max_influences - 1 takes the largest v_j not taken yet (`v > best` from
//   best = -1 over ascending j: ties to the lower bone, a NaN never).  sum = ((v_0 + v_1) + v_2) + v_3 over the taken slots in float64;
//   bone_w[s] = (float)(v_s / sum), bone_ids[s] its bone; a slot that took nothing or whose v is 0 is UNUSED: slot 0's id, weight 0.  A row
//   that is no unknown, or whose sum is not positive: the lowest bone of N(i) with weight 1 in slot 0.
// DEFINITION, POSE.  transforms float32 [T,J,3,4] (M = [A | t], read as float64), ids int32 [Vm,4] forced into [0, J), w float32 [Vm,4].
//   Linear:  x' = (sum_k w_k (A_k x + t_k)) / (sum_k w_k), sums over the slots in order.  A row whose weights sum to 0 keeps x.
//   Dual quaternion: per (frame, bone) q_r = the unit quaternion of A by Shepperd's branch (the largest of trace, A00, A11, A22), negated
//   where its scalar part is negative; q_d = (-(t . v) / 2, (w t + t x v) / 2) for q_r = (w, v).  Per vertex b = sum_k w_k s_k q_k,
//   s_k = -1 where q_r,k . q_r,0 < 0 else +1; b /= |b_r|; |b_r| < 1e-12 (before the division): the linear blend.  Then
//   x' = x + 2 b_v x (b_v x x + b_w x) + 2 (b_w d_v - d_w b_v + b_v x d_v).
//   All arithmetic float64, rounded to float32 once.  A frame reads its own transforms only: its bits depend on neither T nor its place.
//
// KERNELS.  gm_skin_weights is four launches, gm_skin_pose one per 32768 frames.  No atomics; every sum has one fixed order.
//   skin_box            one workgroup: the bounding box of V0 (min / max: exact in any order), the floor (1e-3 D)^2.
//   skin_bone_distance  one thread per vertex, a wave-uniform loop over the bones, twice (the minimum, then the near set): h, diag,
//                       free_row, |N(i)| and the near set as a [J,Vm] byte plane (a bone's column is what its solve reads, coalesced).
//   skin_heat_solve     grid (J) of ARAP_WAVES waves: workgroup j runs the whole PCG of bone j, rows strided over the threads.
//   skin_compact        one thread per vertex over the J columns.
//   skin_pose<BLEND>    grid (ceil(Vm / 256), T).  BLEND 1: the block's prologue turns the frame's J transforms into dual quaternions in
//                       LDS ([J][8] float64, 16 KB at 256 bones), one bone per thread.
// Conventions of gm_closest.hip: caller workspace, stream-ordered, no device allocation, no host wait anywhere in this file.
#include "gm_common.h"
#include "gm_check.h"
#include "gm_arap_shared.h"

namespace gm {

#define SKIN_THREADS 1024     // skin_heat_solve: one workgroup of ARAP_WAVES waves
#define SKIN_ROW_THREADS 256  // every other kernel
#define SKIN_POSE_FRAMES 32768   // frames of one skin_pose launch (the grid's y)

struct SkinWs {
  double* floor2;           // [1] (1e-3 D)^2
  double* h;                // [Vm]
  double* diag;             // [Vm] h_i + d_i
  int* free_row;            // [Vm]
  int* count;               // [Vm] |N(i)|
  unsigned char* near_set;  // [J][Vm]
  double* x;                // [J][Vm] the columns (out_full stands for it where the caller gives one)
  double* r;                // [J][Vm]
  double* p;                // [J][Vm]
  double* q;                // [J][Vm]
  char* end;
  static SkinWs from(void* ws, size_t Vm, size_t J) {
    char* c = reinterpret_cast<char*>(ws);
    SkinWs k;
    k.floor2 = carve<double>(c, 1);
    k.h = carve<double>(c, Vm);
    k.diag = carve<double>(c, Vm);
    k.free_row = carve<int>(c, Vm);
    k.count = carve<int>(c, Vm);
    k.near_set = carve<unsigned char>(c, J * Vm);
    k.x = carve<double>(c, J * Vm);
    k.r = carve<double>(c, J * Vm);
    k.p = carve<double>(c, J * Vm);
    k.q = carve<double>(c, J * Vm);
    k.end = c;
    return k;
  }
};

__device__ __forceinline__ void skin_load3(const float* __restrict__ V, size_t i, double o[3]) {
  o[0] = (double)V[3 * i]; o[1] = (double)V[3 * i + 1]; o[2] = (double)V[3 * i + 2];
}

__global__ __launch_bounds__(SKIN_ROW_THREADS) void skin_box_kernel(int Vm, const float* __restrict__ V0, double* __restrict__ floor2) {
  __shared__ float lo[3][SKIN_ROW_THREADS], hi[3][SKIN_ROW_THREADS];
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int i = threadIdx.x; i < Vm; i += SKIN_ROW_THREADS)
#pragma unroll
    for (int c = 0; c < 3; c++) { const float v = V0[3 * (size_t)i + c]; mn[c] = fminf(mn[c], v); mx[c] = fmaxf(mx[c], v); }
#pragma unroll
  for (int c = 0; c < 3; c++) { lo[c][threadIdx.x] = mn[c]; hi[c][threadIdx.x] = mx[c]; }
  __syncthreads();
  for (int s = SKIN_ROW_THREADS / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        lo[c][threadIdx.x] = fminf(lo[c][threadIdx.x], lo[c][threadIdx.x + s]);
        hi[c][threadIdx.x] = fmaxf(hi[c][threadIdx.x], hi[c][threadIdx.x + s]);
      }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double e[3] = {(double)hi[0][0] - (double)lo[0][0], (double)hi[1][0] - (double)lo[1][0], (double)hi[2][0] - (double)lo[2][0]};
    const double fl = 1e-3 * sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    floor2[0] = fl * fl;
  }
}

// |x - segment(a, b)|^2, the foot parameter clamped to [0, 1]
__device__ __forceinline__ double skin_segment_d2(const double x[3], const float* __restrict__ bone_a, const float* __restrict__ bone_b, int j) {
  double a[3], b[3];
  skin_load3(bone_a, (size_t)j, a); skin_load3(bone_b, (size_t)j, b);
  const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ax[3] = {x[0] - a[0], x[1] - a[1], x[2] - a[2]};
  const double ll = ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2];
  double s = ll > 0.0 ? (ax[0] * ab[0] + ax[1] * ab[1] + ax[2] * ab[2]) / ll : 0.0;
  s = fmin(fmax(s, 0.0), 1.0);
  const double e[3] = {ax[0] - s * ab[0], ax[1] - s * ab[1], ax[2] - s * ab[2]};
  return e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
}

__global__ __launch_bounds__(SKIN_ROW_THREADS) void skin_bone_distance_kernel(int Vm, int J, const int* __restrict__ row_offsets,
                                                                              const double* __restrict__ weights, const float* __restrict__ V0,
                                                                              const double* __restrict__ area, const float* __restrict__ bone_a,
                                                                              const float* __restrict__ bone_b, double heat,
                                                                              const double* __restrict__ floor2, double* __restrict__ h,
                                                                              double* __restrict__ diag, int* __restrict__ free_row,
                                                                              int* __restrict__ count, unsigned char* __restrict__ near_set) {
  const int i = blockIdx.x * SKIN_ROW_THREADS + threadIdx.x;
  if (i >= Vm) return;
  double x[3];
  skin_load3(V0, (size_t)i, x);
  double d2min = INFINITY;
  for (int j = 0; j < J; j++) d2min = fmin(d2min, skin_segment_d2(x, bone_a, bone_b, j));
  d2min = fmax(d2min, floor2[0]);
  const double bar = (1.0 + 1e-4) * (1.0 + 1e-4) * d2min;
  int n = 0;
  for (int j = 0; j < J; j++) {
    const int in = skin_segment_d2(x, bone_a, bone_b, j) <= bar ? 1 : 0;
    near_set[(size_t)j * Vm + i] = (unsigned char)in;
    n += in;
  }
  const double ar = area[i];
  const double hi = ar > 0.0 ? heat * ar / d2min : 0.0;
  double d = 0.0;
  for (int k = row_offsets[i]; k < row_offsets[i + 1]; k++) d += weights[k];
  h[i] = hi;
  diag[i] = hi + d;
  free_row[i] = hi + d > 0.0 ? 1 : 0;
  count[i] = n;
}

__device__ __forceinline__ double skin_p(const unsigned char* __restrict__ near_col, const int* __restrict__ count, int i) {
  return near_col[i] ? 1.0 / (double)count[i] : 0.0;
}

// workgroup j: the whole PCG of bone j.  A row that is no unknown has no edge (h_i + d_i = 0 means d_i = 0, and the CSR is symmetric), so
// no neighbour moves to the right-hand side.
static_assert(SKIN_THREADS == ARAP_WAVES * 64, "skin_heat_solve_kernel strides its rows as arap_pcg_steps does");
__global__ __launch_bounds__(SKIN_THREADS) void skin_heat_solve_kernel(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                                       const double* __restrict__ weights, const double* __restrict__ h,
                                                                       const double* __restrict__ diag, const int* __restrict__ free_row,
                                                                       const int* __restrict__ count, const unsigned char* __restrict__ near_set,
                                                                       double* xall, double* rall, double* pall, double* qall,
                                                                       int cg_iterations, double tol2, double* stats) {
  __shared__ double partA[1][ARAP_WAVES], partB[3][ARAP_WAVES];
  const size_t col = (size_t)blockIdx.x * Vm;
  const unsigned char* near_col = near_set + col;
  double* x = xall + col;
  double* r = rall + col;
  double* p = pall + col;
  double* q = qall + col;
  double s3[3] = {0.0, 0.0, 0.0};                                  // |b|^2, |r|^2, r . z
  for (int i = threadIdx.x; i < Vm; i += SKIN_THREADS) {
    const double xi = skin_p(near_col, count, i);
    double ri = 0.0, zi = 0.0;
    if (free_row[i]) {
      double Lx = 0.0;
      for (int k = row_offsets[i]; k < row_offsets[i + 1]; k++) Lx += weights[k] * (xi - skin_p(near_col, count, clamp_index(cols[k], Vm)));
      const double b = h[i] * xi;
      ri = b - (h[i] * xi + Lx); zi = ri / diag[i];
      s3[0] += b * b; s3[1] += ri * ri; s3[2] += ri * zi;
    }
    x[i] = xi; r[i] = ri; p[i] = zi;                               // rows that are no unknowns: x = p_j, r = p = 0, for the whole solve
  }
  const ArapPcgResult cg = arap_pcg_steps<true>(Vm, row_offsets, cols, weights, diag, free_row, x, r, p, q, cg_iterations, tol2, s3, partA, partB, h);
  if (stats && threadIdx.x == 0) {
    stats[2 * (size_t)blockIdx.x] = (double)cg.used;
    stats[2 * (size_t)blockIdx.x + 1] = arap_rel_residual(cg.bb, cg.rr);
  }
}

__global__ __launch_bounds__(SKIN_ROW_THREADS) void skin_compact_kernel(int Vm, int J, int keep, const double* __restrict__ full,
                                                                        const int* __restrict__ free_row, const unsigned char* __restrict__ near_set,
                                                                        int* __restrict__ out_ids, float* __restrict__ out_w) {
  const int i = blockIdx.x * SKIN_ROW_THREADS + threadIdx.x;
  if (i >= Vm) return;
  int id[4] = {-1, -1, -1, -1};
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int s = 0; s < keep; s++) {
    double best = -1.0;
    int at = -1;
    for (int j = 0; j < J; j++) {
      if (j == id[0] || j == id[1] || j == id[2]) continue;
      const double w = fmax(full[(size_t)j * Vm + i], 0.0);        // (fmax drops a NaN: it counts as 0)
      if (w > best) { best = w; at = j; }
    }
    if (at < 0) break;
    id[s] = at; v[s] = best;
  }
  const double sum = ((v[0] + v[1]) + v[2]) + v[3];
  int* oi = out_ids + 4 * (size_t)i;
  float* ow = out_w + 4 * (size_t)i;
  if (!free_row[i] || !(sum > 0.0)) {
    int low = 0;
    for (int j = J - 1; j >= 0; j--)
      if (near_set[(size_t)j * Vm + i]) low = j;
    oi[0] = oi[1] = oi[2] = oi[3] = low;
    ow[0] = 1.f; ow[1] = ow[2] = ow[3] = 0.f;
    return;
  }
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const bool used = id[s] >= 0 && v[s] > 0.0;
    oi[s] = used ? id[s] : id[0];
    ow[s] = used ? (float)(v[s] / sum) : 0.f;
  }
}

// the unit dual quaternion (w, x, y, z; dw, dx, dy, dz) of the rigid motion M = [A | t] (row-major 3 x 4, float32)
__device__ __forceinline__ void skin_dual_quaternion(const float* __restrict__ M, double o[8]) {
  double A[3][3], t[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int b = 0; b < 3; b++) A[a][b] = (double)M[4 * a + b];
    t[a] = (double)M[4 * a + 3];
  }
  const double tr = A[0][0] + A[1][1] + A[2][2];
  double qw, qx, qy, qz;
  if (tr >= A[0][0] && tr >= A[1][1] && tr >= A[2][2]) {
    const double s = 2.0 * sqrt(1.0 + tr);
    qw = 0.25 * s; qx = (A[2][1] - A[1][2]) / s; qy = (A[0][2] - A[2][0]) / s; qz = (A[1][0] - A[0][1]) / s;
  } else if (A[0][0] >= A[1][1] && A[0][0] >= A[2][2]) {
    const double s = 2.0 * sqrt(1.0 + A[0][0] - A[1][1] - A[2][2]);
    qw = (A[2][1] - A[1][2]) / s; qx = 0.25 * s; qy = (A[0][1] + A[1][0]) / s; qz = (A[0][2] + A[2][0]) / s;
  } else if (A[1][1] >= A[2][2]) {
    const double s = 2.0 * sqrt(1.0 + A[1][1] - A[0][0] - A[2][2]);
    qw = (A[0][2] - A[2][0]) / s; qx = (A[0][1] + A[1][0]) / s; qy = 0.25 * s; qz = (A[1][2] + A[2][1]) / s;
  } else {
    const double s = 2.0 * sqrt(1.0 + A[2][2] - A[0][0] - A[1][1]);
    qw = (A[1][0] - A[0][1]) / s; qx = (A[0][2] + A[2][0]) / s; qy = (A[1][2] + A[2][1]) / s; qz = 0.25 * s;
  }
  const double n = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  const double f = (qw < 0.0 ? -1.0 : 1.0) / n;
  qw *= f; qx *= f; qy *= f; qz *= f;
  o[0] = qw; o[1] = qx; o[2] = qy; o[3] = qz;
  o[4] = -0.5 * (t[0] * qx + t[1] * qy + t[2] * qz);
  o[5] = 0.5 * (qw * t[0] + (t[1] * qz - t[2] * qy));
  o[6] = 0.5 * (qw * t[1] + (t[2] * qx - t[0] * qz));
  o[7] = 0.5 * (qw * t[2] + (t[0] * qy - t[1] * qx));
}

template <int BLEND>
__global__ __launch_bounds__(SKIN_ROW_THREADS) void skin_pose_kernel(int Vm, int J, const float* __restrict__ V0, const int* __restrict__ ids,
                                                                     const float* __restrict__ w, const float* __restrict__ transforms,
                                                                     float* __restrict__ out) {
  const float* M = transforms + (size_t)blockIdx.y * J * 12;
  __shared__ double dq[BLEND ? GM_SKIN_BONES_MAX : 1][8];
  if constexpr (BLEND) {
    for (int j = threadIdx.x; j < J; j += SKIN_ROW_THREADS) skin_dual_quaternion(M + 12 * (size_t)j, dq[j]);
    __syncthreads();
  }
  const int i = blockIdx.x * SKIN_ROW_THREADS + threadIdx.x;
  if (i >= Vm) return;
  double x[3];
  skin_load3(V0, (size_t)i, x);
  int id[4];
  double wk[4];
#pragma unroll
  for (int k = 0; k < 4; k++) { id[k] = clamp_index(ids[4 * (size_t)i + k], J); wk[k] = (double)w[4 * (size_t)i + k]; }
  double y[3] = {x[0], x[1], x[2]};
  bool linear = true;
  if constexpr (BLEND) {
    double b[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const double* qk = dq[id[k]];
      const double* q0 = dq[id[0]];
      const double dot = qk[0] * q0[0] + qk[1] * q0[1] + qk[2] * q0[2] + qk[3] * q0[3];
      const double s = dot < 0.0 ? -wk[k] : wk[k];
#pragma unroll
      for (int e = 0; e < 8; e++) b[e] += s * qk[e];
    }
    const double n = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3]);
    if (!(n < 1e-12)) {
      linear = false;
#pragma unroll
      for (int e = 0; e < 8; e++) b[e] /= n;
      const double bw = b[0], bv[3] = {b[1], b[2], b[3]}, dw = b[4], dv[3] = {b[5], b[6], b[7]};
      double c1[3], u[3], c2[3], c3[3];
      cross3(bv, x, c1);
#pragma unroll
      for (int a = 0; a < 3; a++) u[a] = c1[a] + bw * x[a];
      cross3(bv, u, c2);
      cross3(bv, dv, c3);
#pragma unroll
      for (int a = 0; a < 3; a++) y[a] = x[a] + 2.0 * c2[a] + 2.0 * (bw * dv[a] - dw * bv[a] + c3[a]);
    }
  }
  if (linear) {
    double acc[3] = {0.0, 0.0, 0.0}, sum = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float* Mk = M + 12 * (size_t)id[k];
#pragma unroll
      for (int a = 0; a < 3; a++)
        acc[a] += wk[k] * ((double)Mk[4 * a] * x[0] + (double)Mk[4 * a + 1] * x[1] + (double)Mk[4 * a + 2] * x[2] + (double)Mk[4 * a + 3]);
      sum += wk[k];
    }
    if (sum != 0.0) {
#pragma unroll
      for (int a = 0; a < 3; a++) y[a] = acc[a] / sum;
    }
  }
  float* o = out + ((size_t)blockIdx.y * Vm + i) * 3;
  o[0] = (float)y[0]; o[1] = (float)y[1]; o[2] = (float)y[2];
}

// ---------------------------------------------------------------------------------------------
// gm_skin_pose_bwd: the vector-Jacobian product of DEFINITION, POSE with respect to the transforms, float64 throughout from the float32
// inputs (g_out float32, read as float64).  The forward's decisions are constants: the Shepperd branch and the sign that makes q_w >= 0
// of each (frame, bone), the slots' signs s_k, the |b_r| < 1e-12 fallback, the sum == 0 row.
//   Linear (and the rows of dqs that fell back):  g_M[k][a][:] += w_k (g[a] / sum) (x, 1) for every (vertex, slot) of bone k; nothing from
//   a row whose weights sum to 0.
//   Dual quaternion, per vertex with G = 2 g, u = b_v x x + b_w x (b normalised):
//     g_bv = u x G + x x (G x b_v) - d_w G + d_v x G;  g_bw = (G x b_v) . x + G . d_v;  g_dv = b_w G + G x b_v;  g_dw = -G . b_v;
//     g_b[f] = g_bh[f] / n - [f < 4] bh_f (sum_e g_bh[e] bh_e) / n;  g_q_k = sum over the bone's (vertex, slot) of s_k w_k g_b.
//   Per (frame, bone), back through skin_dual_quaternion: q_d = (-(t . v) / 2, (w t + t x v) / 2) gives g_t and adds to g_q_r; the
//   normalisation q = sg raw / |raw|: g_raw = sg (g_q - q (q . g_q)) / |raw|; the branch: its pivot is s / 4, the others N_i / s with
//   s = 2 sqrt(D), D = 1 +- A00 +- A11 +- A22, N_i = A_ab +- A_ba: g_s = g_pivot / 4 - sum_i raw_i g_raw_i / s, g_D = 2 g_s / s.
//   Off the rotation manifold the gradient is what this arithmetic's extension gives (tests/skin_bwd_ref.py states it through autograd).
// Two launches per 32768 frames, no atomics (the shape of gm_deform_bwd.hip):
//   rows   grid (ceil(Vm / 256), T), one thread per (frame, vertex): workspace row [T][Vm][ROW] float64 - linear ROW = 3: g / sum (zeros
//          where sum == 0); dqs ROW = 12: g_b [8] (zeros on a fallback row) | g / sum [3] (fallback rows only, else zeros) | the slots'
//          signs as bits 0 .. 3 of an integer kept in the 12th double.  Every element of a row is written.
//   bones  grid (ceil(J / 4), T), one wave per (frame, bone) over its incidence list (CSR: bone_offsets [J+1], bone_entries = 4 vertex +
//          slot, ascending): lane l takes entries l, l + 64, .. in that order, then a fixed xor butterfly; lane 0 turns g_dq into g_M and
//          writes the bone's 12 doubles.  An empty list gives exact zeros; an entry outside [0, 4 Vm) is skipped; offsets are forced
//          into [0, 4 Vm] (the list's consistency with ids is the caller's contract; this only keeps the reads in bounds).
// A frame reads its own transforms, g_out and workspace rows only: its bits depend on neither T nor its place.
// Contraction is off from here on: the restated forward decides s_k and the fallback by plain IEEE products and sums.
#pragma clang fp contract(off)

constexpr int SKIN_BWD_ROW_LINEAR = 3;
constexpr int SKIN_BWD_ROW_DQS = 12;

template <int BLEND>
__global__ __launch_bounds__(SKIN_ROW_THREADS) void skin_pose_bwd_rows_kernel(int Vm, int J, const float* __restrict__ V0,
                                                                              const int* __restrict__ ids, const float* __restrict__ w,
                                                                              const float* __restrict__ transforms,
                                                                              const float* __restrict__ g_out, double* __restrict__ rows) {
  constexpr int ROW = BLEND ? SKIN_BWD_ROW_DQS : SKIN_BWD_ROW_LINEAR;
  __shared__ double dq[BLEND ? GM_SKIN_BONES_MAX : 1][8];
  if constexpr (BLEND) {
    const float* M = transforms + (size_t)blockIdx.y * J * 12;
    for (int j = threadIdx.x; j < J; j += SKIN_ROW_THREADS) skin_dual_quaternion(M + 12 * (size_t)j, dq[j]);
    __syncthreads();
  }
  const int i = blockIdx.x * SKIN_ROW_THREADS + threadIdx.x;
  if (i >= Vm) return;
  const size_t at = (size_t)blockIdx.y * Vm + i;
  double* o = rows + at * ROW;
  double x[3], g[3], wk[4];
  skin_load3(V0, (size_t)i, x);
  skin_load3(g_out, at, g);
#pragma unroll
  for (int k = 0; k < 4; k++) wk[k] = (double)w[4 * (size_t)i + k];
  if constexpr (BLEND) {
    int id[4];
#pragma unroll
    for (int k = 0; k < 4; k++) id[k] = clamp_index(ids[4 * (size_t)i + k], J);
    double b[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    long long bits = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const double* qk = dq[id[k]];
      const double* q0 = dq[id[0]];
      const double dot = qk[0] * q0[0] + qk[1] * q0[1] + qk[2] * q0[2] + qk[3] * q0[3];
      const double s = dot < 0.0 ? -wk[k] : wk[k];
      if (dot < 0.0) bits |= 1ll << k;
#pragma unroll
      for (int e = 0; e < 8; e++) b[e] += s * qk[e];
    }
    o[11] = __longlong_as_double(bits);
    const double n = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3]);
    if (!(n < 1e-12)) {
#pragma unroll
      for (int e = 0; e < 8; e++) b[e] /= n;
      const double bw = b[0], bv[3] = {b[1], b[2], b[3]}, dw = b[4], dv[3] = {b[5], b[6], b[7]};
      const double G[3] = {2.0 * g[0], 2.0 * g[1], 2.0 * g[2]};
      double c1[3], u[3], gu[3], t1[3], t2[3], t3[3], gh[8];
      cross3(bv, x, c1);
#pragma unroll
      for (int a = 0; a < 3; a++) u[a] = c1[a] + bw * x[a];
      cross3(G, bv, gu);                           // g_u: also the gradient the cross product b_v x d_v hands to d_v
      cross3(u, G, t1);
      cross3(x, gu, t2);
      cross3(dv, G, t3);
      gh[0] = (gu[0] * x[0] + gu[1] * x[1] + gu[2] * x[2]) + (G[0] * dv[0] + G[1] * dv[1] + G[2] * dv[2]);
      gh[4] = -(G[0] * bv[0] + G[1] * bv[1] + G[2] * bv[2]);
#pragma unroll
      for (int a = 0; a < 3; a++) {
        gh[1 + a] = ((t1[a] + t2[a]) - dw * G[a]) + t3[a];
        gh[5 + a] = bw * G[a] + gu[a];
      }
      double S = 0.0;
#pragma unroll
      for (int e = 0; e < 8; e++) S += gh[e] * b[e];
      S /= n;
#pragma unroll
      for (int e = 0; e < 8; e++) o[e] = e < 4 ? gh[e] / n - b[e] * S : gh[e] / n;
      o[8] = 0.0; o[9] = 0.0; o[10] = 0.0;
      return;
    }
#pragma unroll
    for (int e = 0; e < 8; e++) o[e] = 0.0;
  }
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < 4; k++) sum += wk[k];
  double* l = o + (BLEND ? 8 : 0);
#pragma unroll
  for (int a = 0; a < 3; a++) l[a] = sum != 0.0 ? g[a] / sum : 0.0;
}

// gM [12] += the gradient of M = [A | t] (row-major 3 x 4) from G = g_dq [8]: skin_dual_quaternion restated with what its backward needs.
// Branch P: raw[P] = s / 4, raw[i] = (A[IA][IB] + SG A[IB][IA]) / s for the others, s = 2 sqrt(1 + DD . diag A).
template <int P>
__device__ __forceinline__ void skin_dual_quaternion_bwd_branch(const double A[9], const double t[3], const double G[8], double gM[12]) {
  constexpr int IA[4][4] = {{0, 2, 0, 1}, {2, 0, 0, 0}, {0, 0, 0, 1}, {1, 0, 1, 0}};
  constexpr int IB[4][4] = {{0, 1, 2, 0}, {1, 0, 1, 2}, {2, 1, 0, 2}, {0, 2, 2, 0}};
  constexpr double SG[4][4] = {{0.0, -1.0, -1.0, -1.0}, {-1.0, 0.0, 1.0, 1.0}, {-1.0, 1.0, 0.0, 1.0}, {-1.0, 1.0, 1.0, 0.0}};
  constexpr double DD[4][3] = {{1.0, 1.0, 1.0}, {1.0, -1.0, -1.0}, {-1.0, 1.0, -1.0}, {-1.0, -1.0, 1.0}};
  const double s = 2.0 * sqrt(((1.0 + DD[P][0] * A[0]) + DD[P][1] * A[4]) + DD[P][2] * A[8]);
  double raw[4];
#pragma unroll
  for (int i = 0; i < 4; i++) raw[i] = i == P ? 0.25 * s : (A[3 * IA[P][i] + IB[P][i]] + SG[P][i] * A[3 * IB[P][i] + IA[P][i]]) / s;
  const double nn = sqrt(raw[0] * raw[0] + raw[1] * raw[1] + raw[2] * raw[2] + raw[3] * raw[3]);
  const double f = (raw[0] < 0.0 ? -1.0 : 1.0) / nn;
  const double q[4] = {raw[0] * f, raw[1] * f, raw[2] * f, raw[3] * f};
  // q_d = (-(t . v) / 2, (q_w t + t x v) / 2)
  const double Gd[3] = {G[5], G[6], G[7]};
  double vG[3], Gt[3], gq[4];
  cross3(q + 1, Gd, vG);
  cross3(Gd, t, Gt);
  gq[0] = G[0] + 0.5 * (Gd[0] * t[0] + Gd[1] * t[1] + Gd[2] * t[2]);
#pragma unroll
  for (int a = 0; a < 3; a++) {
    gM[4 * a + 3] += (0.5 * q[0] * Gd[a] - 0.5 * G[4] * q[1 + a]) + 0.5 * vG[a];
    gq[1 + a] = (G[1 + a] - 0.5 * G[4] * t[a]) + 0.5 * Gt[a];
  }
  // q = f raw, f = sign / |raw|
  const double qg = q[0] * gq[0] + q[1] * gq[1] + q[2] * gq[2] + q[3] * gq[3];
  double gs = 0.0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const double graw = f * (gq[i] - q[i] * qg);
    if (i == P) { gs += 0.25 * graw; continue; }
    gs -= raw[i] * graw / s;
    gM[4 * IA[P][i] + IB[P][i]] += graw / s;
    gM[4 * IB[P][i] + IA[P][i]] += SG[P][i] * (graw / s);
  }
  const double gD = 2.0 * gs / s;
#pragma unroll
  for (int a = 0; a < 3; a++) gM[5 * a] += DD[P][a] * gD;
}

__device__ __forceinline__ void skin_dual_quaternion_bwd(const float* __restrict__ M, const double G[8], double gM[12]) {
  double A[9], t[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int b = 0; b < 3; b++) A[3 * a + b] = (double)M[4 * a + b];
    t[a] = (double)M[4 * a + 3];
  }
  const double tr = A[0] + A[4] + A[8];
  if (tr >= A[0] && tr >= A[4] && tr >= A[8]) skin_dual_quaternion_bwd_branch<0>(A, t, G, gM);
  else if (A[0] >= A[4] && A[0] >= A[8]) skin_dual_quaternion_bwd_branch<1>(A, t, G, gM);
  else if (A[4] >= A[8]) skin_dual_quaternion_bwd_branch<2>(A, t, G, gM);
  else skin_dual_quaternion_bwd_branch<3>(A, t, G, gM);
}

// one wave per (frame, bone), four bones per workgroup
template <int BLEND>
__global__ __launch_bounds__(256) void skin_pose_bwd_bones_kernel(int Vm, int J, const float* __restrict__ V0, const float* __restrict__ w,
                                                                  const float* __restrict__ transforms, const int* __restrict__ bone_offsets,
                                                                  const int* __restrict__ bone_entries, const double* __restrict__ rows,
                                                                  double* __restrict__ g_transforms) {
  constexpr int ROW = BLEND ? SKIN_BWD_ROW_DQS : SKIN_BWD_ROW_LINEAR;
  constexpr int NACC = BLEND ? 20 : 12;              // g_M [12] | g_dq [8]
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= J) return;                              // (wave-uniform)
  const int lane = threadIdx.x & 63;
  const long long n4 = 4ll * Vm;
  long long lo = bone_offsets[j], hi = bone_offsets[j + 1];
  lo = lo < 0 ? 0 : lo; hi = hi > n4 ? n4 : hi;
  const double* frame_rows = rows + (size_t)blockIdx.y * Vm * ROW;
  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; k++) acc[k] = 0.0;
  for (long long jj = lo + lane; jj < hi; jj += 64) {
    const int e = bone_entries[jj];
    if (e < 0 || e >= n4) continue;
    const size_t v = (size_t)(e >> 2);
    const double we = (double)w[e];
    const double* r = frame_rows + v * ROW;
    const double* l = r + (BLEND ? 8 : 0);
    double x[3];
    skin_load3(V0, v, x);
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const double c = we * l[a];
#pragma unroll
      for (int b = 0; b < 3; b++) acc[4 * a + b] = acc[4 * a + b] + c * x[b];
      acc[4 * a + 3] = acc[4 * a + 3] + c;
    }
    if constexpr (BLEND) {
      const double s = ((__double_as_longlong(r[11]) >> (e & 3)) & 1) ? -we : we;
#pragma unroll
      for (int k = 0; k < 8; k++) acc[12 + k] = acc[12 + k] + s * r[k];
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < NACC; k++) acc[k] = acc[k] + __shfl_xor(acc[k], off);
  if (lane == 0) {
    const size_t at = (size_t)blockIdx.y * J + j;
    if constexpr (BLEND) skin_dual_quaternion_bwd(transforms + at * 12, acc + 12, acc);
    double* o = g_transforms + at * 12;
#pragma unroll
    for (int k = 0; k < 12; k++) o[k] = acc[k];
  }
}

}  // namespace gm

// ---------------------------------------------------------------------------------------------
// the entry points (include/gmesh_hip.h): their refusals, then the launches
using namespace gm;

extern "C" {

size_t gm_skin_weights_workspace_bytes(int Vm, int J) {
  if (Vm < 1 || J < 1 || J > GM_SKIN_BONES_MAX) return 0;
  return (size_t)SkinWs::from(nullptr, (size_t)Vm, (size_t)J).end + 256;
}

int gm_skin_weights(int Vm, int J, const int* row_offsets, const int* cols, const double* weights, const float* V0, const double* area,
                    const float* bone_a, const float* bone_b, double heat, int cg_iterations, double cg_tolerance, int max_influences,
                    int* out_ids, float* out_w, double* out_full, double* out_stats, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "gm_skin_weights";
  if (Vm < 1) { set_error("%s: Vm = %d (must be positive)", fn, Vm); return GM_ERR_INVALID_ARG; }
  if (J < 1 || J > GM_SKIN_BONES_MAX) { set_error("%s: J = %d bones (1 .. %d)", fn, J, GM_SKIN_BONES_MAX); return GM_ERR_INVALID_ARG; }
  if (!(heat > 0.0) || heat > 1.7976931348623157e308) { set_error("%s: heat must be positive and finite", fn); return GM_ERR_INVALID_ARG; }
  if (cg_iterations < 1) { set_error("%s: cg_iterations = %d (at least 1)", fn, cg_iterations); return GM_ERR_INVALID_ARG; }
  if (!(cg_tolerance >= 0.0) || cg_tolerance > 1.7976931348623157e308) {
    set_error("%s: cg_tolerance must be finite and not negative", fn); return GM_ERR_INVALID_ARG;
  }
  if (max_influences < 1 || max_influences > 4) { set_error("%s: max_influences = %d (1 .. 4)", fn, max_influences); return GM_ERR_INVALID_ARG; }
  if (!row_offsets || !cols || !weights || !V0 || !area || !bone_a || !bone_b || !out_ids || !out_w || !workspace) {
    set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG;
  }
  const ByteRange rg[9] = {{V0, 12 * (size_t)Vm, "V0", false}, {area, 8 * (size_t)Vm, "area", false}, {bone_a, 12 * (size_t)J, "bone_a", false},
                           {bone_b, 12 * (size_t)J, "bone_b", false}, {out_ids, 16 * (size_t)Vm, "out_ids", true}, {out_w, 16 * (size_t)Vm, "out_w", true},
                           {out_full, 8 * (size_t)Vm * J, "out_full", true}, {out_stats, 16 * (size_t)J, "out_stats", true},
                           {workspace, workspace_bytes, "workspace", true}};
  if (int rc = check_ranges(fn, rg)) return rc;
  const size_t need = gm_skin_weights_workspace_bytes(Vm, J);
  if (workspace_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need); return GM_ERR_BUFFER; }
  const SkinWs k = SkinWs::from(workspace, (size_t)Vm, (size_t)J);
  double* x = out_full ? out_full : k.x;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 threads(SKIN_ROW_THREADS), rows((Vm + SKIN_ROW_THREADS - 1) / SKIN_ROW_THREADS);
  hipLaunchKernelGGL(skin_box_kernel, dim3(1), threads, 0, s, Vm, V0, k.floor2);
  hipLaunchKernelGGL(skin_bone_distance_kernel, rows, threads, 0, s, Vm, J, row_offsets, weights, V0, area, bone_a, bone_b, heat, k.floor2, k.h, k.diag,
                     k.free_row, k.count, k.near_set);
  hipLaunchKernelGGL(skin_heat_solve_kernel, dim3(J), dim3(SKIN_THREADS), 0, s, Vm, row_offsets, cols, weights, k.h, k.diag, k.free_row, k.count,
                     k.near_set, x, k.r, k.p, k.q, cg_iterations, cg_tolerance * cg_tolerance, out_stats);
  hipLaunchKernelGGL(skin_compact_kernel, rows, threads, 0, s, Vm, J, max_influences, x, k.free_row, k.near_set, out_ids, out_w);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_skin_pose(int T, int Vm, int J, const float* V0, const int* ids, const float* w, const float* transforms, int blend, float* out,
                 void* stream) {
  const char* fn = "gm_skin_pose";
  if (T < 1) { set_error("%s: T = %d (must be positive)", fn, T); return GM_ERR_INVALID_ARG; }
  if (Vm < 1) { set_error("%s: Vm = %d (must be positive)", fn, Vm); return GM_ERR_INVALID_ARG; }
  if (J < 1 || J > GM_SKIN_BONES_MAX) { set_error("%s: J = %d bones (1 .. %d)", fn, J, GM_SKIN_BONES_MAX); return GM_ERR_INVALID_ARG; }
  if (blend != GM_SKIN_BLEND_LINEAR && blend != GM_SKIN_BLEND_DQS) { set_error("%s: blend = %d (0 linear, 1 dual quaternion)", fn, blend); return GM_ERR_INVALID_ARG; }
  if (!V0 || !ids || !w || !transforms || !out) { set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG; }
  const ByteRange rg[5] = {{V0, 12 * (size_t)Vm, "V0", false}, {ids, 16 * (size_t)Vm, "ids", false}, {w, 16 * (size_t)Vm, "w", false},
                           {transforms, 48 * (size_t)T * J, "transforms", false}, {out, 12 * (size_t)Vm * T, "out", true}};
  if (int rc = check_ranges(fn, rg)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int G = (Vm + SKIN_ROW_THREADS - 1) / SKIN_ROW_THREADS;
  for (int t0 = 0; t0 < T; t0 += SKIN_POSE_FRAMES) {
    const int n = T - t0 < SKIN_POSE_FRAMES ? T - t0 : SKIN_POSE_FRAMES;
    const float* M = transforms + (size_t)t0 * J * 12;
    float* o = out + (size_t)t0 * Vm * 3;
    if (blend == GM_SKIN_BLEND_DQS) hipLaunchKernelGGL(skin_pose_kernel<1>, dim3(G, n), dim3(SKIN_ROW_THREADS), 0, s, Vm, J, V0, ids, w, M, o);
    else hipLaunchKernelGGL(skin_pose_kernel<0>, dim3(G, n), dim3(SKIN_ROW_THREADS), 0, s, Vm, J, V0, ids, w, M, o);
  }
  GM_HIP(hipGetLastError());
  return GM_OK;
}

size_t gm_skin_pose_bwd_workspace_bytes(int T, int Vm, int J, int blend) {
  if (T < 1 || Vm < 1 || J < 1 || J > GM_SKIN_BONES_MAX || (blend != GM_SKIN_BLEND_LINEAR && blend != GM_SKIN_BLEND_DQS)) return 0;
  const size_t row = blend == GM_SKIN_BLEND_DQS ? SKIN_BWD_ROW_DQS : SKIN_BWD_ROW_LINEAR;
  return ((size_t)T * Vm * row * sizeof(double) + 255) & ~(size_t)255;
}

int gm_skin_pose_bwd(int T, int Vm, int J, const float* V0, const int* ids, const float* w, const float* transforms, int blend,
                     const float* g_out, const int* bone_offsets, const int* bone_entries, double* g_transforms, void* workspace,
                     size_t workspace_bytes, void* stream) {
  const char* fn = "gm_skin_pose_bwd";
  if (T < 1) { set_error("%s: T = %d (must be positive)", fn, T); return GM_ERR_INVALID_ARG; }
  if (Vm < 1) { set_error("%s: Vm = %d (must be positive)", fn, Vm); return GM_ERR_INVALID_ARG; }
  if (J < 1 || J > GM_SKIN_BONES_MAX) { set_error("%s: J = %d bones (1 .. %d)", fn, J, GM_SKIN_BONES_MAX); return GM_ERR_INVALID_ARG; }
  if (blend != GM_SKIN_BLEND_LINEAR && blend != GM_SKIN_BLEND_DQS) { set_error("%s: blend = %d (0 linear, 1 dual quaternion)", fn, blend); return GM_ERR_INVALID_ARG; }
  if (!V0 || !ids || !w || !transforms || !g_out || !bone_offsets || !bone_entries || !g_transforms || !workspace) {
    set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG;
  }
  const size_t need = gm_skin_pose_bwd_workspace_bytes(T, Vm, J, blend);
  // (bone_entries holds bone_offsets[J] ints, a number on the device: its first element stands for it)
  const ByteRange rg[9] = {{g_transforms, 96 * (size_t)T * J, "g_transforms", true}, {workspace, workspace_bytes, "workspace", true},
                           {V0, 12 * (size_t)Vm, "V0", false}, {ids, 16 * (size_t)Vm, "ids", false}, {w, 16 * (size_t)Vm, "w", false},
                           {transforms, 48 * (size_t)T * J, "transforms", false}, {g_out, 12 * (size_t)Vm * T, "g_out", false},
                           {bone_offsets, 4 * ((size_t)J + 1), "bone_offsets", false}, {bone_entries, 4, "bone_entries", false}};
  if (int rc = check_ranges(fn, rg)) return rc;
  if (workspace_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need); return GM_ERR_BUFFER; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int G = (Vm + SKIN_ROW_THREADS - 1) / SKIN_ROW_THREADS, B = (J + 3) / 4;
  const bool dqs = blend == GM_SKIN_BLEND_DQS;
  const size_t row = dqs ? SKIN_BWD_ROW_DQS : SKIN_BWD_ROW_LINEAR;
  for (int t0 = 0; t0 < T; t0 += SKIN_POSE_FRAMES) {
    const int n = T - t0 < SKIN_POSE_FRAMES ? T - t0 : SKIN_POSE_FRAMES;
    const float* M = transforms + (size_t)t0 * J * 12;
    const float* g = g_out + (size_t)t0 * Vm * 3;
    double* rows = reinterpret_cast<double*>(workspace) + (size_t)t0 * Vm * row;
    double* o = g_transforms + (size_t)t0 * J * 12;
    if (dqs) {
      hipLaunchKernelGGL(skin_pose_bwd_rows_kernel<1>, dim3(G, n), dim3(SKIN_ROW_THREADS), 0, s, Vm, J, V0, ids, w, M, g, rows);
      hipLaunchKernelGGL(skin_pose_bwd_bones_kernel<1>, dim3(B, n), dim3(256), 0, s, Vm, J, V0, w, M, bone_offsets, bone_entries, rows, o);
    } else {
      hipLaunchKernelGGL(skin_pose_bwd_rows_kernel<0>, dim3(G, n), dim3(SKIN_ROW_THREADS), 0, s, Vm, J, V0, ids, w, M, g, rows);
      hipLaunchKernelGGL(skin_pose_bwd_bones_kernel<0>, dim3(B, n), dim3(256), 0, s, Vm, J, V0, w, M, bone_offsets, bone_entries, rows, o);
    }
  }
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // extern "C"
