// gm_spatial.hip -- the host side of the Morton front end of gm_knn, gm_knn_nearest (gm_knn.hip) and gm_closest_face (gm_closest.hip):
// the bounding box of a point set, a 30-bit Morton code per point, and the radix sort (gm_sort.hip) of (code, index) pairs, which
// returns its own result.  Stream-ordered, caller workspace (MortonWs / MortonSet, gm_common.h), no host wait.
#include "gm_common.h"
#include "gm_spatial.h"
#include "gm_wave.h"
#include <cfloat>
#pragma clang fp contract(off)

namespace gm {

// bounding box of n points, seeded with +-FLT_MAX (the true box): per-workgroup partials, then one workgroup
__global__ __launch_bounds__(256) void point_bbox_partial(int n, const float* __restrict__ pts, float* __restrict__ partial) {
  __shared__ float sm[4][6];
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
#pragma unroll
    for (int k = 0; k < 3; k++) { const float v = pts[3 * (size_t)i + k]; mn[k] = fminf(mn[k], v); mx[k] = fmaxf(mx[k], v); }
  }
  block_minmax3(mn, mx, sm);
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < 3; k++) { partial[6 * blockIdx.x + k] = mn[k]; partial[6 * blockIdx.x + 3 + k] = mx[k]; }
}

__global__ __launch_bounds__(256) void point_bbox_final(int nb, const float* __restrict__ partial, float* __restrict__ bbox) {
  __shared__ float sm[4][6];
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (int i = threadIdx.x; i < nb; i += 256)
#pragma unroll
    for (int k = 0; k < 3; k++) { mn[k] = fminf(mn[k], partial[6 * i + k]); mx[k] = fmaxf(mx[k], partial[6 * i + 3 + k]); }
  block_minmax3(mn, mx, sm);
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < 3; k++) { bbox[k] = mn[k]; bbox[3 + k] = mx[k]; }
}

__global__ __launch_bounds__(256) void point_morton(int n, const float* __restrict__ pts, const float* __restrict__ bbox,
                                                    uint32_t* __restrict__ codes) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  codes[i] = morton_code30(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], bbox);
}

int launch_point_bbox(int n, const float* pts, float* partial, float* bbox, hipStream_t s) {
  const int nb = min(GM_BBOX_PARTIALS, (n + 255) / 256);
  hipLaunchKernelGGL(point_bbox_partial, dim3(nb), dim3(256), 0, s, n, pts, partial);
  hipLaunchKernelGGL(point_bbox_final, dim3(1), dim3(256), 0, s, nb, partial, bbox);
  GM_HIP(hipGetLastError());
  return 0;
}

int launch_point_morton(int n, const float* pts, const float* bbox, uint32_t* codes, hipStream_t s) {
  hipLaunchKernelGGL(point_morton, dim3((n + 255) / 256), dim3(256), 0, s, n, pts, bbox, codes);
  GM_HIP(hipGetLastError());
  return 0;
}

int morton_sort(MortonSet& set, const MortonWs& w, size_t n, MortonSorted* out, hipStream_t s) {
  const int rc = radix_sort_pairs(set.keys, set.idx, w.hist, w.digit_total, n, 30, true, 0, s);
  const int slot = radix_final_slot(30);
  out->keys = set.keys[slot];
  out->idx = set.idx[slot];
  return rc;
}

}  // namespace gm
