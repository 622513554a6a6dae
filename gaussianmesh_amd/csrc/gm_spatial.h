// gm_spatial.h -- the device side of the Morton front end the geometry queries share (gm_knn.hip, gm_closest.hip; host side in
// gm_spatial.hip, declared in gm_common.h): the 30-bit code of a point against a bounding box, and the search in the sorted codes.
// The codes fix an ORDER only; what a query returns is defined by its own arithmetic and does not depend on them.
#pragma once
#include "gm_common.h"

namespace gm {

// 10 bits -> every third bit (simple_knn.cu:45-61)
__device__ __forceinline__ uint32_t morton_spread10(uint32_t x) {
  x = (x | (x << 16)) & 0x030000FF;
  x = (x | (x << 8)) & 0x0300F00F;
  x = (x | (x << 4)) & 0x030C30C3;
  x = (x | (x << 2)) & 0x09249249;
  return x;
}

// 30-bit Morton code against the box bb = (min xyz, max xyz); a point outside is clamped onto it, a flat axis maps to 0
__device__ __forceinline__ uint32_t morton_code30(float x, float y, float z, const float* bb) {
  const float v[3] = {x, y, z};
  uint32_t c[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float ext = bb[3 + k] - bb[k];
    float t = ext > 0.f ? (v[k] - bb[k]) / ext : 0.f;
    t = fminf(fmaxf(t, 0.f), 1.f);               // (NaN -> 0)
    c[k] = morton_spread10((uint32_t)(t * ((1 << 10) - 1)));
  }
  return c[0] | (c[1] << 1) | (c[2] << 2);
}

// the first position of the sorted keys [0, n) whose key is not below code (n if there is none)
__device__ __forceinline__ int morton_lower_bound(const uint32_t* __restrict__ keys, int n, uint32_t code) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < code) lo = mid + 1; else hi = mid;
  }
  return lo;
}

}  // namespace gm
