// gm_deform_bwd.hip -- backward of the fused deform / shade pass (gm_deform_shade_bwd): from the rasterizer's dL/dmeans3D, dL/dcov3D [N,6]
// and dL/dcolors to the gradients of the per-vertex tables (dV, R, S) a mesh pose is made of, and optionally of the SH rows, the rest
// covariances and the rest positions (deform.deform_shade_differentiable, pose_fit.py).
//
// Forward per row (gm_deform.hip: deform_kernel / deform_cov / shade_rotated, restated below with their parenthesisation, contraction off, so
// the clamp gate r + 0.5 > 0 recomputed here is the one behind the rgb the forward wrote):
//   d, Rb, Sb = blend_w(dV, Rv, Sv)[tri];  Rt = Rb^T;  RS = Rt Sb;  O = RS C RS^T;  npos = p + d;
//   dir = (npos - cam) / |npos - cam|;  (x, y, z) = Rb dir;  rgb = max(SH_deg(x, y, z) + 0.5, 0)
// Backward per row, G the 3x3 with g_cov6 in its upper triangle:
//   g_RS = G (RS C^T) + G^T (RS C);  g_C = RS^T (G RS);  g_Rt = g_RS Sb^T;  g_Sb = Rt^T g_RS;
//   g_r = gated g_rgb;  g_xyz = sum_ch g_r[ch] dSH/d(x,y,z);  g_Rb = g_Rt^T + g_xyz (x) dir;  g_dir = Rb^T g_xyz;
//   g_npos = g_pos + (g_dir - dir (dir . g_dir)) / len;  g_d = g_rest_pos = g_npos
// A NULL g_cov6 / g_rgb stands for zeros and runs the same arithmetic on them: the same bits as an all-zero tensor.
//
// Two launches, no atomics:
//   rows      one thread per row: the 21 unweighted floats (g_d | g_Rb | g_Sb) -> workspace [N][21], and the optional per-row outputs;
//   vertices  one wave per vertex over its incidence list (CSR: inc_offsets [Vm+1], inc_entries = 3 row + corner, which is also the index
//             of the corner's weight in w): lane l takes entries l, l + 64, .. in that order, then a fixed xor butterfly over the lanes.
//             A vertex's sum is a function of its list alone: the same bits every run; an empty list gives exact zeros; every element of
//             g_dV / g_Rv / g_Sv is written.
// (Measured against a fused variant, one launch in which each wave recomputes its vertex's rows: 0.28 against 0.45 ms at 1 M rows on 7.5 k
// vertices - the rows' 312 B of inputs are read three times instead of once; NOTEBOOK.md "Deform / shade backward".)
// An entry outside [0, 3N) is skipped (the list's consistency with tri is the caller's contract; this only keeps the reads in bounds).
#include "gm_common.h"
#include "gm_check.h"
#pragma clang fp contract(off)
#include "gm_sh.h"

namespace gm {

constexpr int DB_ROW = 21;                         // floats per workspace row: g_d 3 | g_Rb 9 | g_Sb 9

// c[a][b] = sum_k a[a][k] b[k][b], (t0 + t1) + t2
__device__ __forceinline__ void mm(const float* A, const float* B, float* C) {
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) C[3 * a + b] = (A[3 * a] * B[b] + A[3 * a + 1] * B[3 + b]) + A[3 * a + 2] * B[6 + b];
}
// c[a][b] = sum_k a[a][k] b[b][k]
__device__ __forceinline__ void mm_nt(const float* A, const float* B, float* C) {
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) C[3 * a + b] = (A[3 * a] * B[3 * b] + A[3 * a + 1] * B[3 * b + 1]) + A[3 * a + 2] * B[3 * b + 2];
}
// c[a][b] = sum_k a[k][a] b[k][b]
__device__ __forceinline__ void mm_tn(const float* A, const float* B, float* C) {
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) C[3 * a + b] = (A[a] * B[b] + A[3 + a] * B[3 + b]) + A[6 + a] * B[6 + b];
}

__global__ __launch_bounds__(256) void deform_shade_bwd_rows_kernel(int N, int deg, int M, const int* __restrict__ tri, const float* __restrict__ w,
                                                                    const float* __restrict__ dV, const float* __restrict__ Rv,
                                                                    const float* __restrict__ Sv, const float* __restrict__ cov,
                                                                    const float* __restrict__ pos, const float* __restrict__ shs,
                                                                    const float* __restrict__ campos, const float* __restrict__ g_pos,
                                                                    const float* __restrict__ g_cov6, const float* __restrict__ g_rgb,
                                                                    float* __restrict__ rows, float* __restrict__ g_shs, float* __restrict__ g_cov,
                                                                    float* __restrict__ g_rest_pos) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= N) return;
  const size_t i = (size_t)idx;
  // ---- the forward, as deform_kernel / deform_shade_kernel<false, ..> state it
  const int t0 = tri[3 * i], t1 = tri[3 * i + 1], t2 = tri[3 * i + 2];
  const float w0 = w[3 * i], w1 = w[3 * i + 1], w2 = w[3 * i + 2];
  float d[3], Rb[9], Sb[9];
#pragma unroll
  for (int k = 0; k < 3; k++) d[k] = (w0 * dV[3 * (size_t)t0 + k] + w1 * dV[3 * (size_t)t1 + k]) + w2 * dV[3 * (size_t)t2 + k];
#pragma unroll
  for (int k = 0; k < 9; k++) {
    Rb[k] = (w0 * Rv[9 * (size_t)t0 + k] + w1 * Rv[9 * (size_t)t1 + k]) + w2 * Rv[9 * (size_t)t2 + k];
    Sb[k] = (w0 * Sv[9 * (size_t)t0 + k] + w1 * Sv[9 * (size_t)t1 + k]) + w2 * Sv[9 * (size_t)t2 + k];
  }
  float npos[3];
#pragma unroll
  for (int k = 0; k < 3; k++) npos[k] = pos[3 * i + k] + d[k];
  float dir[3] = {npos[0] - campos[0], npos[1] - campos[1], npos[2] - campos[2]};
  const float len = sqrtf(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
  dir[0] = dir[0] / len; dir[1] = dir[1] / len; dir[2] = dir[2] / len;
  // (x, y, z) = Rt^T dir = Rb dir (shade_rotated)
  const float x = (Rb[0] * dir[0] + Rb[1] * dir[1]) + Rb[2] * dir[2];
  const float y = (Rb[3] * dir[0] + Rb[4] * dir[1]) + Rb[5] * dir[2];
  const float z = (Rb[6] * dir[0] + Rb[7] * dir[1]) + Rb[8] * dir[2];
  // ---- colour route: the gate, dSH/d(x, y, z) (computeColorFromSH's backward, as gm_preprocess.hip states it), the SH rows' gradient
  float gxyz[3];
  {
    const int ncoef = (deg + 1) * (deg + 1);
    float sh[48];
    load_sh(shs, i, M, ncoef, sh);
    float gr[3], wgt[16];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const float r = sh_channel(deg, [&](int k) { return sh[3 * k + ch]; }, x, y, z);
      const float g = g_rgb ? g_rgb[3 * i + ch] : 0.f;
      gr[ch] = (r + 0.5f > 0.f) ? g : 0.f;
    }
    float ddx[3] = {0.f, 0.f, 0.f}, ddy[3] = {0.f, 0.f, 0.f}, ddz[3] = {0.f, 0.f, 0.f};
#define S(k, ch) sh[3 * (k) + (ch)]
    wgt[0] = SH_C0;
    if (deg > 0) {
      wgt[1] = -SH_C1 * y; wgt[2] = SH_C1 * z; wgt[3] = -SH_C1 * x;
#pragma unroll
      for (int ch = 0; ch < 3; ch++) { ddx[ch] = -SH_C1 * S(3, ch); ddy[ch] = -SH_C1 * S(1, ch); ddz[ch] = SH_C1 * S(2, ch); }
      if (deg > 1) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        wgt[4] = SH_C2[0] * xy; wgt[5] = SH_C2[1] * yz; wgt[6] = SH_C2[2] * (2.f * zz - xx - yy);
        wgt[7] = SH_C2[3] * xz; wgt[8] = SH_C2[4] * (xx - yy);
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
          ddx[ch] += SH_C2[0] * y * S(4, ch) + SH_C2[2] * 2.f * -x * S(6, ch) + SH_C2[3] * z * S(7, ch) + SH_C2[4] * 2.f * x * S(8, ch);
          ddy[ch] += SH_C2[0] * x * S(4, ch) + SH_C2[1] * z * S(5, ch) + SH_C2[2] * 2.f * -y * S(6, ch) + SH_C2[4] * 2.f * -y * S(8, ch);
          ddz[ch] += SH_C2[1] * y * S(5, ch) + SH_C2[2] * 2.f * 2.f * z * S(6, ch) + SH_C2[3] * x * S(7, ch);
        }
        if (deg > 2) {
          wgt[9] = SH_C3[0] * y * (3.f * xx - yy); wgt[10] = SH_C3[1] * xy * z;
          wgt[11] = SH_C3[2] * y * (4.f * zz - xx - yy); wgt[12] = SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy);
          wgt[13] = SH_C3[4] * x * (4.f * zz - xx - yy); wgt[14] = SH_C3[5] * z * (xx - yy);
          wgt[15] = SH_C3[6] * x * (xx - 3.f * yy);
#pragma unroll
          for (int ch = 0; ch < 3; ch++) {
            ddx[ch] += (SH_C3[0] * S(9, ch) * 3.f * 2.f * xy + SH_C3[1] * S(10, ch) * yz + SH_C3[2] * S(11, ch) * -2.f * xy +
                        SH_C3[3] * S(12, ch) * -3.f * 2.f * xz + SH_C3[4] * S(13, ch) * (-3.f * xx + 4.f * zz - yy) +
                        SH_C3[5] * S(14, ch) * 2.f * xz + SH_C3[6] * S(15, ch) * 3.f * (xx - yy));
            ddy[ch] += (SH_C3[0] * S(9, ch) * 3.f * (xx - yy) + SH_C3[1] * S(10, ch) * xz +
                        SH_C3[2] * S(11, ch) * (-3.f * yy + 4.f * zz - xx) + SH_C3[3] * S(12, ch) * -3.f * 2.f * yz +
                        SH_C3[4] * S(13, ch) * -2.f * xy + SH_C3[5] * S(14, ch) * -2.f * yz + SH_C3[6] * S(15, ch) * -3.f * 2.f * xy);
            ddz[ch] += (SH_C3[1] * S(10, ch) * xy + SH_C3[2] * S(11, ch) * 4.f * 2.f * yz +
                        SH_C3[3] * S(12, ch) * 3.f * (2.f * zz - xx - yy) + SH_C3[4] * S(13, ch) * 4.f * 2.f * xz +
                        SH_C3[5] * S(14, ch) * (xx - yy));
          }
        }
      }
    }
#undef S
    gxyz[0] = (gr[0] * ddx[0] + gr[1] * ddx[1]) + gr[2] * ddx[2];
    gxyz[1] = (gr[0] * ddy[0] + gr[1] * ddy[1]) + gr[2] * ddy[2];
    gxyz[2] = (gr[0] * ddz[0] + gr[1] * ddz[1]) + gr[2] * ddz[2];
    if (g_shs) {                                   // coefficients beyond the degree: 0
      float* o = g_shs + i * (size_t)M * 3;
#pragma unroll
      for (int k = 0; k < 16; k++) {
        if (k < M) {
          const bool on = k < ncoef;
#pragma unroll
          for (int ch = 0; ch < 3; ch++) o[3 * k + ch] = on ? wgt[k] * gr[ch] : 0.f;
        }
      }
      for (int k = 48; k < 3 * M; k++) o[k] = 0.f;
    }
  }
  // ---- covariance route
  float C[9], G[9], Rt[9], RS[9];
#pragma unroll
  for (int k = 0; k < 9; k++) C[k] = cov[9 * i + k];
  {
    float g6[6];
#pragma unroll
    for (int k = 0; k < 6; k++) g6[k] = g_cov6 ? g_cov6[6 * i + k] : 0.f;
    G[0] = g6[0]; G[1] = g6[1]; G[2] = g6[2]; G[3] = 0.f; G[4] = g6[3]; G[5] = g6[4]; G[6] = 0.f; G[7] = 0.f; G[8] = g6[5];
  }
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) Rt[3 * a + b] = Rb[3 * b + a];
  mm(Rt, Sb, RS);                                  // deform_cov's RS
  float P[9], Q[9], T1[9], T2[9], gRS[9], U[9];
  mm_nt(RS, C, P);                                 // RS C^T
  mm(RS, C, Q);                                    // RS C (deform_cov's A)
  mm(G, P, T1);                                    // G (RS C^T)
  mm_tn(G, Q, T2);                                 // G^T (RS C)
#pragma unroll
  for (int k = 0; k < 9; k++) gRS[k] = T1[k] + T2[k];
  if (g_cov) {
    float gC[9];
    mm(G, RS, U);
    mm_tn(RS, U, gC);                              // RS^T (G RS)
#pragma unroll
    for (int k = 0; k < 9; k++) g_cov[9 * i + k] = gC[k];
  }
  float gRt[9], gSb[9];
  mm_nt(gRS, Sb, gRt);                             // g_RS Sb^T
  mm_tn(Rt, gRS, gSb);                             // Rt^T g_RS
  // ---- the blended rotation collects both routes; the direction's gradient reaches the position
  float* o = rows + DB_ROW * i;
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) o[3 + 3 * a + b] = gRt[3 * b + a] + gxyz[a] * dir[b];
#pragma unroll
  for (int k = 0; k < 9; k++) o[12 + k] = gSb[k];
  float gdir[3];
#pragma unroll
  for (int b = 0; b < 3; b++) gdir[b] = (Rb[b] * gxyz[0] + Rb[3 + b] * gxyz[1]) + Rb[6 + b] * gxyz[2];
  const float s = (gdir[0] * dir[0] + gdir[1] * dir[1]) + gdir[2] * dir[2];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float gn = g_pos[3 * i + k] + (gdir[k] - dir[k] * s) / len;
    o[k] = gn;
    if (g_rest_pos) g_rest_pos[3 * i + k] = gn;
  }
}

// one wave per vertex, four vertices per workgroup
__global__ __launch_bounds__(256) void deform_shade_bwd_vertices_kernel(int N, int Vm, const float* __restrict__ w, const int* __restrict__ inc_offsets,
                                                                        const int* __restrict__ inc_entries, const float* __restrict__ rows,
                                                                        float* __restrict__ g_dV, float* __restrict__ g_Rv, float* __restrict__ g_Sv) {
  const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (v >= Vm) return;                             // (wave-uniform)
  const int lane = threadIdx.x & 63;
  const long long n3 = 3ll * N;
  long long lo = inc_offsets[v], hi = inc_offsets[v + 1];
  lo = lo < 0 ? 0 : lo; hi = hi > n3 ? n3 : hi;
  float acc[DB_ROW];
#pragma unroll
  for (int k = 0; k < DB_ROW; k++) acc[k] = 0.f;
  for (long long j = lo + lane; j < hi; j += 64) {
    const int e = inc_entries[j];
    if (e < 0 || e >= n3) continue;
    const float we = w[e];
    const float* r = rows + DB_ROW * (size_t)(e / 3);
#pragma unroll
    for (int k = 0; k < DB_ROW; k++) acc[k] = acc[k] + we * r[k];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < DB_ROW; k++) acc[k] = acc[k] + __shfl_xor(acc[k], off);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 3; k++) g_dV[3 * (size_t)v + k] = acc[k];
#pragma unroll
    for (int k = 0; k < 9; k++) { g_Rv[9 * (size_t)v + k] = acc[3 + k]; g_Sv[9 * (size_t)v + k] = acc[12 + k]; }
  }
}

}  // namespace gm

// ---------------------------------------------------------------------------------------------
// the entry points (include/gmesh_hip.h): their refusals, then the launches
using namespace gm;

extern "C" {

size_t gm_deform_shade_bwd_workspace_bytes(int N, int Vm) {
  (void)Vm;
  if (N <= 0) return 0;
  return ((size_t)N * DB_ROW * sizeof(float) + 255) & ~(size_t)255;
}

int gm_deform_shade_bwd(int N, int deg, int M, int Vm, const int* tri, const float* w, const float* dV, const float* Rv, const float* Sv,
                        const float* cov, const float* pos, const float* shs, const float* campos, const int* inc_offsets,
                        const int* inc_entries, const float* g_pos, const float* g_cov6, const float* g_rgb, float* g_dV, float* g_Rv,
                        float* g_Sv, float* g_shs, float* g_cov, float* g_rest_pos, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "gm_deform_shade_bwd";
  if (N < 0 || Vm < 0) { set_error("%s: negative N = %d or Vm = %d", fn, N, Vm); return GM_ERR_INVALID_ARG; }
  if (deg < 0 || deg > 3) { set_error("%s: degree %d out of range 0..3", fn, deg); return GM_ERR_INVALID_ARG; }
  if (M < (deg + 1) * (deg + 1)) { set_error("%s: rows of M = %d coefficients hold no degree %d", fn, M, deg); return GM_ERR_INVALID_ARG; }
  if (Vm == 0 && N > 0) { set_error("%s: N = %d rows bound to Vm = 0 vertices", fn, N); return GM_ERR_INVALID_ARG; }
  if (Vm == 0) return GM_OK;
  if (!inc_offsets || !g_dV || !g_Rv || !g_Sv) { set_error("%s: null pointer (inc_offsets / g_dV / g_Rv / g_Sv)", fn); return GM_ERR_INVALID_ARG; }
  if (N > 0 && (!tri || !w || !dV || !Rv || !Sv || !cov || !pos || !shs || !campos || !inc_entries || !g_pos || !workspace)) {
    set_error("%s: null pointer (a forward input, inc_entries, g_pos or the workspace)", fn); return GM_ERR_INVALID_ARG;
  }
  if (!g_cov6 && !g_rgb && g_shs) { set_error("%s: g_shs asked for with neither g_rgb nor g_cov6", fn); return GM_ERR_INVALID_ARG; }
  const size_t need = gm_deform_shade_bwd_workspace_bytes(N, Vm);
  if (workspace_bytes < need) { set_error("%s: workspace of %zu bytes, needs %zu", fn, workspace_bytes, need); return GM_ERR_INVALID_ARG; }
  const size_t n = (size_t)N, vm = (size_t)Vm, row = (size_t)M * 12;
  const ByteRange rg[21] = {{g_dV, 12 * vm, "g_dV", true}, {g_Rv, 36 * vm, "g_Rv", true}, {g_Sv, 36 * vm, "g_Sv", true},
                            {g_shs, row * n, "g_shs", true}, {g_cov, 36 * n, "g_cov", true}, {g_rest_pos, 12 * n, "g_rest_pos", true},
                            {workspace, need, "workspace", true},
                            {tri, 12 * n, "tri", false}, {w, 12 * n, "w", false}, {dV, 12 * vm, "dV", false}, {Rv, 36 * vm, "Rv", false},
                            {Sv, 36 * vm, "Sv", false}, {cov, 36 * n, "cov", false}, {pos, 12 * n, "pos", false}, {shs, row * n, "shs", false},
                            {campos, 12, "campos", false}, {inc_offsets, 4 * (vm + 1), "inc_offsets", false}, {inc_entries, 12 * n, "inc_entries", false},
                            {g_pos, 12 * n, "g_pos", false}, {g_cov6, 24 * n, "g_cov6", false}, {g_rgb, 12 * n, "g_rgb", false}};
  if (int rc = check_ranges(fn, rg)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  StageScope sc(ST_DEFORM, s);
  float* rows = reinterpret_cast<float*>(workspace);
  if (N > 0)
    hipLaunchKernelGGL(deform_shade_bwd_rows_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, deg, M, tri, w, dV, Rv, Sv, cov, pos, shs, campos,
                       g_pos, g_cov6, g_rgb, rows, g_shs, g_cov, g_rest_pos);
  hipLaunchKernelGGL(deform_shade_bwd_vertices_kernel, dim3((Vm + 3) / 4), dim3(256), 0, s, N, Vm, w, inc_offsets, inc_entries, rows, g_dV, g_Rv,
                     g_Sv);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // extern "C"
