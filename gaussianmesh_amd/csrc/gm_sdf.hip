// gm_sdf.hip -- a sampled signed-distance field for contact (dynamics.SdfGrid; INTEGRATION.md section AC): gm_sdf_grid_prepare turns a
// float32 volume of distances (a TsdfVolume's tsdf / weight pair, or any [nz,ny,nx] tensor with NaN for "unknown") into the grid
// sdf_sample (gm_sdf.h) reads, gm_sdf_grid_sample exposes that function row by row.  The reference has no such stage: both results are
// defined by arithmetic.
//
// PREPARE.  One thread per sample, no atomics, float32 throughout, no contraction, correctly rounded division.  Sample (ix, iy, iz) is
// VALID iff its value is not NaN and (weight == null or weight >= min_weight; a NaN weight fails).  An invalid sample writes four NaNs.
// A valid one writes
//   phi = value * scale                                               one multiply
//   per axis, with phi- / phi+ the phi of the neighbour one sample down / up that axis (valid and inside the grid, or absent):
//     both      (phi+ - phi-) / (2 voxel)                             2 voxel = 2.f * voxel, rounded once
//     only +    (phi+ - phi) / voxel
//     only -    (phi - phi-) / voxel
//     neither   0
// Every neighbour's phi is its own value * scale again, so the result does not depend on the order in which samples are written.
// Conventions of gm_closest.hip: stream-ordered, no device allocation, no host wait.
#include <math.h>
#include "gm_common.h"
#include "gm_check.h"
#include "gm_sdf.h"
#pragma clang fp contract(off)   // every product, difference and quotient rounds on its own, as the definition above says

namespace gm {

#define SDF_THREADS 256

struct SdfSource {
  const float* values;
  const float* weight;   // or null
  float min_weight, scale;
  int nx, ny, nz;
};

// phi of sample (x, y, z) if it is inside the grid and valid; false otherwise
__device__ __forceinline__ bool sdf_known(const SdfSource& s, int x, int y, int z, float& phi) {
  if (x < 0 || y < 0 || z < 0 || x >= s.nx || y >= s.ny || z >= s.nz) return false;
  const size_t o = ((size_t)z * s.ny + y) * s.nx + x;
  const float v = s.values[o];
  if (v != v) return false;
  if (s.weight && !(s.weight[o] >= s.min_weight)) return false;
  phi = v * s.scale;
  return true;
}

__device__ __forceinline__ float sdf_gradient(bool lo, float pm, bool hi, float pp, float phi, float voxel, float two_voxel) {
  if (lo && hi) return (pp - pm) / two_voxel;
  if (hi) return (pp - phi) / voxel;
  if (lo) return (phi - pm) / voxel;
  return 0.f;
}

__global__ __launch_bounds__(SDF_THREADS) void sdf_prepare_kernel(SdfSource s, float voxel, float4* __restrict__ out) {
  const size_t total = (size_t)s.nx * s.ny * s.nz;
  const size_t o = (size_t)blockIdx.x * SDF_THREADS + threadIdx.x;
  if (o >= total) return;
  const int x = (int)(o % s.nx), y = (int)((o / s.nx) % s.ny), z = (int)(o / ((size_t)s.nx * s.ny));
  float phi;
  if (!sdf_known(s, x, y, z, phi)) { out[o] = make_float4(NAN, NAN, NAN, NAN); return; }
  const float two_voxel = 2.f * voxel;
  float g[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    float pm = 0.f, pp = 0.f;
    const bool lo = sdf_known(s, x - (a == 0), y - (a == 1), z - (a == 2), pm);
    const bool hi = sdf_known(s, x + (a == 0), y + (a == 1), z + (a == 2), pp);
    g[a] = sdf_gradient(lo, pm, hi, pp, phi, voxel, two_voxel);
  }
  out[o] = make_float4(phi, g[0], g[1], g[2]);
}

__global__ __launch_bounds__(SDF_THREADS) void sdf_sample_kernel(int N, const float* __restrict__ points, SdfGrid g, double* __restrict__ phi_out,
                                                                 double* __restrict__ n_out) {
  const int i = blockIdx.x * SDF_THREADS + threadIdx.x;
  if (i >= N) return;
  const double X[3] = {(double)points[3 * (size_t)i], (double)points[3 * (size_t)i + 1], (double)points[3 * (size_t)i + 2]};
  double n[3] = {(double)NAN, (double)NAN, (double)NAN};
  const double phi = sdf_sample(g, X, n);
  phi_out[i] = phi;
#pragma unroll
  for (int a = 0; a < 3; a++) n_out[3 * (size_t)i + a] = phi != phi ? (double)NAN : n[a];
}

}  // namespace gm

using namespace gm;

extern "C" {

int gm_sdf_grid_prepare(int nx, int ny, int nz, const float* values, const float* weight, float min_weight, float scale, float voxel,
                        float* grid_out, void* stream) {
  const char* fn = "gm_sdf_grid_prepare";
  static const float no_origin[3] = {0.f, 0.f, 0.f};                 // (prepare does not read an origin)
  if (int rc = check_tsdf_grid(fn, nx, ny, nz, 2, no_origin, voxel)) return rc;
  if (!(scale - scale == 0.f)) { set_error("%s: scale must be finite", fn); return GM_ERR_INVALID_ARG; }
  if (!values || !grid_out) { set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG; }
  if (reinterpret_cast<uintptr_t>(grid_out) % 16) { set_error("%s: grid_out must be 16-byte aligned", fn); return GM_ERR_INVALID_ARG; }
  const size_t total = (size_t)nx * ny * nz;
  const ByteRange rg[3] = {{values, 4 * total, "values", false}, {weight, 4 * total, "weight", false}, {grid_out, 16 * total, "grid_out", true}};
  if (int rc = check_ranges(fn, rg)) return rc;
  const SdfSource src = {values, weight, min_weight, scale, nx, ny, nz};
  hipLaunchKernelGGL(sdf_prepare_kernel, dim3((unsigned)((total + SDF_THREADS - 1) / SDF_THREADS)), dim3(SDF_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), src, voxel, reinterpret_cast<float4*>(grid_out));
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_sdf_grid_sample(int N, const float* points, int nx, int ny, int nz, const float* origin, float voxel, const float* grid, double* phi_out,
                       double* n_out, void* stream) {
  const char* fn = "gm_sdf_grid_sample";
  if (N < 1) { set_error("%s: N = %d (must be positive)", fn, N); return GM_ERR_INVALID_ARG; }
  if (int rc = check_sdf_grid(fn, nx, ny, nz, origin, voxel, grid)) return rc;
  if (!points || !phi_out || !n_out) { set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG; }
  const ByteRange rg[4] = {{points, 12 * (size_t)N, "points", false}, {grid, 16 * (size_t)nx * ny * nz, "field_grid", false},
                           {phi_out, 8 * (size_t)N, "phi_out", true}, {n_out, 24 * (size_t)N, "n_out", true}};
  if (int rc = check_ranges(fn, rg)) return rc;
  const SdfGrid g = {reinterpret_cast<const float4*>(grid), nx, ny, nz, {origin[0], origin[1], origin[2]}, voxel};
  hipLaunchKernelGGL(sdf_sample_kernel, dim3((N + SDF_THREADS - 1) / SDF_THREADS), dim3(SDF_THREADS), 0, reinterpret_cast<hipStream_t>(stream), N, points, g,
                     phi_out, n_out);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // extern "C"
