// gm_wave.h -- the wave64 / workgroup primitives of the ordering kernels (gm_bucket.hip, gm_sort.hip, gm_binning.hip, gm_tile_order.h,
// gm_tsdf.hip), one copy each: wave reductions, the stable match-any rank of a radix pass, the workgroup exclusive scan and the
// per-wave digit counts -> per-wave offsets step, all uint32_t and exact; and the float min / max reductions of the geometry queries
// (gm_spatial.hip, gm_knn.hip, gm_closest.hip), exact as well.  The float SUMS of other files fix their own order and stay where they are.
#pragma once
#include "gm_common.h"

namespace gm {

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
  return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
  return v;
}
__device__ __forceinline__ float wave_min_f32(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
  return v;
}

// min of mn[3] and max of mx[3] over the workgroup (a bounding box); the result is valid in thread 0.  Every thread calls it (ONE
// __syncthreads inside); sm holds a row per wave.
__device__ __forceinline__ void block_minmax3(float* mn, float* mx, float (*sm)[6]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; k++) { mn[k] = wave_min_f32(mn[k]); mx[k] = wave_max_f32(mx[k]); }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 3; k++) { sm[wave][k] = mn[k]; sm[wave][3 + k] = mx[k]; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < (int)(blockDim.x >> 6); w++)
#pragma unroll
      for (int k = 0; k < 3; k++) { mn[k] = fminf(mn[k], sm[w][k]); mx[k] = fmaxf(mx[k], sm[w][3 + k]); }
  }
}

// match-any over the low DB bits of the digit among the valid lanes: the lanes of the wave whose key has this lane's digit (DB + 1
// ballots; an invalid lane's mask means nothing)
template <int DB>
__device__ __forceinline__ uint64_t wave_match_peers(uint32_t d, bool valid) {
  uint64_t peers = __ballot(valid);
#pragma unroll
  for (int b = 0; b < DB; b++) {
    const uint64_t bal = __ballot((d >> b) & 1u);
    peers &= ((d >> b) & 1u) ? bal : ~bal;
  }
  return peers;
}

// Stable rank of this lane's key among the keys of the same digit the wave has ranked so far: cnt [digits] are THIS wave's running
// digit counts in LDS; the first lane of each peer group adds the group's size and hands the old count to its peers, a lane's rank is
// that plus the peers in lower lanes.  Every lane of the wave calls it (ballots), round after round in key order.
template <int DB, class CNT>
__device__ __forceinline__ uint32_t wave_match_rank(uint32_t d, bool valid, CNT* cnt, int lane) {
  const uint64_t peers = wave_match_peers<DB>(d, valid);
  const uint32_t before = lanes_below(peers);
  const int leader = __ffsll((unsigned long long)peers) - 1;
  uint32_t old = 0;
  if (valid && lane == leader) {
    old = cnt[d];
    cnt[d] = (CNT)(old + __popcll(peers));
  }
  old = __shfl(old, leader < 0 ? 0 : leader);
  __builtin_amdgcn_wave_barrier();             // keep the per-wave LDS counter updates of successive rounds in order
  return old + before;
}

// Exclusive scan of one value per thread over the WAVES * 64 threads of the workgroup; total = the sum of all.  Every thread calls it
// (ONE __syncthreads inside); wsum [WAVES] is shared, and the caller synchronises before it is written again.
template <int WAVES>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* wsum, uint32_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(incl, d);
    if (lane >= d) incl += t;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint32_t woff = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < WAVES; w++) {
    const uint32_t s = wsum[w];
    woff += (w < wave) ? s : 0;
    tot += s;
  }
  total = tot;
  return woff + incl - v;
}

// One digit's per-wave counts, cnt[w * stride] for wave w (cnt = &wcnt[0][digit], stride = counters per wave), turned in place into
// the waves' exclusive offsets inside the digit's run; returns the digit's total.
template <int WAVES, class CNT>
__device__ __forceinline__ uint32_t wave_counts_to_offsets(CNT* cnt, int stride) {
  uint32_t run = 0;
#pragma unroll
  for (int w = 0; w < WAVES; w++) {
    const uint32_t c = cnt[w * stride];
    cnt[w * stride] = (CNT)run;
    run += c;
  }
  return run;
}

}  // namespace gm
