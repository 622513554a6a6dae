// gm_sdf.h -- sampling a prepared signed-distance grid (gm_sdf.hip): the one device function gm_sdf_grid_sample and the field contact of
// gm_mesh_dynamics_field (gm_dynamics.hip) share, and the host checks of a grid's description.
//
// THE GRID.  float32 [nz,ny,nx,4]: sample (ix, iy, iz), at origin + (i + 0.5) voxel, holds (phi, gx, gy, gz) - the distance and the
// gradient gm_sdf_grid_prepare took over the sample's known neighbours - or four NaNs where nothing is known.
//
// sdf_sample(g, X) -> phi, n, every step in float64 and in this order:
//   per axis a   g_a = (X_a - origin_a) / voxel - 0.5 (origin and voxel widened from float32);  the row is OUTSIDE unless
//                0 <= g_a < n_a - 1 on all three axes (a NaN coordinate compares false: outside);  i_a = floor(g_a), f_a = g_a - i_a
//   the corners  q[dz][dy][dx] = sample (ix + dx, iy + dy, iz + dz): eight 16-byte loads; a corner whose phi is NaN: phi = NaN
//   per channel  (phi, gx, gy, gz widened to double) along x: a_dzdy = fma(fx, q[dz][dy][1] - q[dz][dy][0], q[dz][dy][0]);
//                along y: b_dz = fma(fy, a_dz1 - a_dz0, a_dz0);  along z: fma(fz, b_1 - b_0, b_0)
//   the normal   s = sqrt(fma(g2, g2, fma(g1, g1, g0 g0)));  !(s > 0) or s not finite: phi = NaN;  else n = g / s per coordinate
// Outside, phi = NaN and n is not written.  The gradient channels are interpolated like phi itself, so the normal is continuous across
// cell faces; the gradient of the trilinear interpolant is not.
#pragma once
#include <math.h>
#include "gm_common.h"
#include "gm_check.h"

namespace gm {

struct SdfGrid {
  const float4* grid;   // [nz][ny][nx] (phi, gx, gy, gz), 16-byte aligned
  int nx, ny, nz;
  float origin[3];
  float voxel;
};

__device__ __forceinline__ double sdf_lerp3(const double (&q)[2][2][2], double fx, double fy, double fz) {
  double b[2];
#pragma unroll
  for (int dz = 0; dz < 2; dz++) {
    const double a0 = fma(fx, q[dz][0][1] - q[dz][0][0], q[dz][0][0]);
    const double a1 = fma(fx, q[dz][1][1] - q[dz][1][0], q[dz][1][0]);
    b[dz] = fma(fy, a1 - a0, a0);
  }
  return fma(fz, b[1] - b[0], b[0]);
}

// phi at X (NaN: outside, next to an unknown sample, or on a gradient without a direction) and, where phi is a number, the unit normal
__device__ __forceinline__ double sdf_sample(const SdfGrid& g, const double (&X)[3], double (&n)[3]) {
#pragma clang fp contract(off)
  const int dims[3] = {g.nx, g.ny, g.nz};
  int i[3];
  double f[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const double ga = (X[a] - (double)g.origin[a]) / (double)g.voxel - 0.5;
    if (!(ga >= 0.0 && ga < (double)(dims[a] - 1))) return (double)NAN;
    const double fl = floor(ga);
    i[a] = (int)fl;                                                  // 0 .. n_a - 2
    f[a] = ga - fl;
  }
  float4 c[2][2][2];
#pragma unroll
  for (int dz = 0; dz < 2; dz++)
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
      for (int dx = 0; dx < 2; dx++) c[dz][dy][dx] = g.grid[((size_t)(i[2] + dz) * g.ny + (i[1] + dy)) * g.nx + (i[0] + dx)];
  double q[2][2][2], grad[3];
  bool known = true;
#pragma unroll
  for (int dz = 0; dz < 2; dz++)
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
      for (int dx = 0; dx < 2; dx++) { q[dz][dy][dx] = (double)c[dz][dy][dx].x; known = known && !(c[dz][dy][dx].x != c[dz][dy][dx].x); }
  if (!known) return (double)NAN;
  const double phi = sdf_lerp3(q, f[0], f[1], f[2]);
#pragma unroll
  for (int dz = 0; dz < 2; dz++)
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
      for (int dx = 0; dx < 2; dx++) q[dz][dy][dx] = (double)c[dz][dy][dx].y;
  grad[0] = sdf_lerp3(q, f[0], f[1], f[2]);
#pragma unroll
  for (int dz = 0; dz < 2; dz++)
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
      for (int dx = 0; dx < 2; dx++) q[dz][dy][dx] = (double)c[dz][dy][dx].z;
  grad[1] = sdf_lerp3(q, f[0], f[1], f[2]);
#pragma unroll
  for (int dz = 0; dz < 2; dz++)
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
      for (int dx = 0; dx < 2; dx++) q[dz][dy][dx] = (double)c[dz][dy][dx].w;
  grad[2] = sdf_lerp3(q, f[0], f[1], f[2]);
  const double s = sqrt(fma(grad[2], grad[2], fma(grad[1], grad[1], grad[0] * grad[0])));
  if (!(s > 0.0) || !(s - s == 0.0)) return (double)NAN;
  n[0] = grad[0] / s; n[1] = grad[1] / s; n[2] = grad[2] / s;
  return phi;
}

// the host checks every entry that takes a prepared grid shares: check_tsdf_grid's rules (sides at least 2: a cell needs two samples),
// the pointer and its alignment for the 16-byte loads
static inline int check_sdf_grid(const char* fn, int nx, int ny, int nz, const float* origin, float voxel, const float* grid) {
  if (int rc = check_tsdf_grid(fn, nx, ny, nz, 2, origin, voxel)) return rc;
  if (!grid) { set_error("%s: null pointer (field_grid)", fn); return GM_ERR_INVALID_ARG; }
  if (reinterpret_cast<uintptr_t>(grid) % 16) { set_error("%s: field_grid must be 16-byte aligned", fn); return GM_ERR_INVALID_ARG; }
  return GM_OK;
}

}  // namespace gm
