// gm_knn.hip -- mean squared distance to the 3 nearest neighbours (model initialisation helper), and the nearest point of a
// second cloud (knn_nearest, below: the neighbour pruning of train_bg_gaussian.py:129-137).
//
// Replaces SimpleKNN::knn (scene/simple_knn/cuda_headers/simple_knn.cu:185-221; python entry
// scene/simple_knn/__init__.py:15-28 distCUDA2).  Same algorithm family: Morton order, 1024-point boxes,
// exact 3-NN with box-distance pruning; the result (mean of the three smallest squared distances to other
// points, duplicates count as distance 0) does not depend on the acceleration structure.
// Differences by design: no internal allocation (caller workspace), no host readback of the bounding box
// (it stays on the device), our own radix sort (gm_sort.hip).
#include "gm_common.h"
#include "gm_check.h"
#include "gm_spatial.h"
#include "gm_wave.h"
#include <cfloat>
#pragma clang fp contract(off)   // squared distances evaluated exactly as the CPU oracle does

namespace gm {

#define KNN_BOX 1024

struct KnnWs {
  MortonWs front;        // bbox = the true bounding box (the reference seeds its reduction with 0, simple_knn.cu:191-200: no output depends on it)
  MortonSet set;
  float* boxes;          // [nboxes][6]
  char* end;
  static KnnWs from(void* ws, size_t P) {
    char* p = reinterpret_cast<char*>(ws);
    KnnWs k;
    k.front = MortonWs::carve_from(p, P);
    k.set = MortonSet::carve_from(p, P);
    k.boxes = carve<float>(p, 6 * ((P + KNN_BOX - 1) / KNN_BOX));
    k.end = p;
    return k;
  }
};

// one workgroup per box of 1024 Morton-consecutive points (simple_knn.cu:78-117)
__global__ __launch_bounds__(256) void knn_box_minmax(int P, const float* __restrict__ pts, const uint32_t* __restrict__ idx,
                                                      float* __restrict__ boxes) {
  __shared__ float sm[4][6];
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
#pragma unroll
  for (int r = 0; r < KNN_BOX / 256; r++) {
    const int i = blockIdx.x * KNN_BOX + r * 256 + threadIdx.x;
    if (i < P) {
      const uint32_t g = idx[i];
#pragma unroll
      for (int k = 0; k < 3; k++) { const float v = pts[3 * (size_t)g + k]; mn[k] = fminf(mn[k], v); mx[k] = fmaxf(mx[k], v); }
    }
  }
  block_minmax3(mn, mx, sm);
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < 3; k++) { boxes[6 * blockIdx.x + k] = mn[k]; boxes[6 * blockIdx.x + 3 + k] = mx[k]; }
}

__device__ __forceinline__ void update3(float dist, float* best) {   // updateKBest<3>, simple_knn.cu:131-145
#pragma unroll
  for (int j = 0; j < 3; j++)
    if (best[j] > dist) { const float t = best[j]; best[j] = dist; dist = t; }
}
__device__ __forceinline__ float dist2(const float* a, const float* b) {
  const float dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
  return dx * dx + dy * dy + dz * dz;
}

// one thread per Morton-sorted point (simple_knn.cu:147-183)
__global__ __launch_bounds__(256) void knn_box_mean_dist(int P, const float* __restrict__ pts, const uint32_t* __restrict__ idx,
                                                         const float* __restrict__ boxes, float* __restrict__ dists) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const uint32_t self = idx[i];
  const float p[3] = {pts[3 * (size_t)self], pts[3 * (size_t)self + 1], pts[3 * (size_t)self + 2]};
  float best[3] = {FLT_MAX, FLT_MAX, FLT_MAX};
  for (int j = max(0, i - 3); j <= min(P - 1, i + 3); j++) {
    if (j == i) continue;
    const uint32_t g = idx[j];
    const float q[3] = {pts[3 * (size_t)g], pts[3 * (size_t)g + 1], pts[3 * (size_t)g + 2]};
    update3(dist2(p, q), best);
  }
  const float reject = best[2];
  best[0] = best[1] = best[2] = FLT_MAX;
  const int nboxes = (P + KNN_BOX - 1) / KNN_BOX;
  for (int b = 0; b < nboxes; b++) {
    const float* bx = boxes + 6 * b;
    float d0 = 0.f, d1 = 0.f, d2 = 0.f;      // distBoxPoint, simple_knn.cu:119-129
    if (p[0] < bx[0] || p[0] > bx[3]) d0 = fminf(fabsf(p[0] - bx[0]), fabsf(p[0] - bx[3]));
    if (p[1] < bx[1] || p[1] > bx[4]) d1 = fminf(fabsf(p[1] - bx[1]), fabsf(p[1] - bx[4]));
    if (p[2] < bx[2] || p[2] > bx[5]) d2 = fminf(fabsf(p[2] - bx[2]), fabsf(p[2] - bx[5]));
    const float dist = d0 * d0 + d1 * d1 + d2 * d2;
    if (dist > reject || dist > best[2]) continue;
    const int e = min(P, (b + 1) * KNN_BOX);
    for (int j = b * KNN_BOX; j < e; j++) {
      if (j == i) continue;
      const uint32_t g = idx[j];
      const float q[3] = {pts[3 * (size_t)g], pts[3 * (size_t)g + 1], pts[3 * (size_t)g + 2]};
      update3(dist2(p, q), best);
    }
  }
  dists[self] = (best[0] + best[1] + best[2]) / 3.0f;
}

// ---------------------------------------------------------------------------------------------
// knn_nearest: for every query point the nearest reference point (k = 1), squared distance and index.
//   d2 = (dx*dx + dy*dy) + dz*dz in float32, no contraction (file pragma), ties -> lowest reference index: the result is that of
//   a float32 brute force bit for bit, whatever the search structure.
// Structure: the reference points in Morton order (bbox and radix sort as gm_knn) cut into boxes of NN_BOX points with their
// bounding boxes; the queries in Morton order too, so that the 64 queries of a wave are neighbours and visit the same boxes.
// A query starts from the NN_WIN sorted reference points around its own Morton code, then visits every box whose distance
// to it is <= the best so far.  The float distance to a box never exceeds the float distance to a point inside it (rounding
// is monotonic), so no box holding the answer - or a tie with a lower index - is skipped.
#define NN_BOX 256
#define NN_WIN 8

struct NnWs {
  MortonWs front;        // bbox of the reference points; sort scratch for the larger of the two sets
  MortonSet rset, qset;
  float4* rsorted;       // [Pr] x, y, z, original index (bits)
  float4* boxes;         // [nboxes][2] min xyz, max xyz
  char* end;
  static NnWs from(void* ws, size_t Pq, size_t Pr) {
    char* p = reinterpret_cast<char*>(ws);
    NnWs k;
    k.front = MortonWs::carve_from(p, Pq > Pr ? Pq : Pr);
    k.rset = MortonSet::carve_from(p, Pr);
    k.qset = MortonSet::carve_from(p, Pq);
    k.rsorted = carve<float4>(p, Pr);
    k.boxes = carve<float4>(p, 2 * ((Pr + NN_BOX - 1) / NN_BOX));
    k.end = p;
    return k;
  }
};

// sorted reference points as float4 (w = original index) and the bounding box of every NN_BOX of them (one workgroup per box)
__global__ __launch_bounds__(NN_BOX) void nn_gather_boxes(int Pr, const float* __restrict__ ref, const uint32_t* __restrict__ idx,
                                                          float4* __restrict__ rsorted, float4* __restrict__ boxes) {
  __shared__ float sm[NN_BOX / 64][6];
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  const int i = blockIdx.x * NN_BOX + threadIdx.x;
  if (i < Pr) {
    const uint32_t g = idx[i];
    const float x = ref[3 * (size_t)g], y = ref[3 * (size_t)g + 1], z = ref[3 * (size_t)g + 2];
    rsorted[i] = make_float4(x, y, z, __uint_as_float(g));
    mn[0] = mx[0] = x; mn[1] = mx[1] = y; mn[2] = mx[2] = z;
  }
  block_minmax3(mn, mx, sm);
  if (threadIdx.x == 0) {
    boxes[2 * blockIdx.x] = make_float4(mn[0], mn[1], mn[2], 0.f);
    boxes[2 * blockIdx.x + 1] = make_float4(mx[0], mx[1], mx[2], 0.f);
  }
}

__device__ __forceinline__ float nn_d2(float px, float py, float pz, const float4 r) {
  const float dx = px - r.x, dy = py - r.y, dz = pz - r.z;
  return (dx * dx + dy * dy) + dz * dz;
}
__device__ __forceinline__ void nn_take(float d, uint32_t id, float& best, uint32_t& bid) {
  if (d < best || (d == best && id < bid)) { best = d; bid = id; }
}
__device__ __forceinline__ float nn_axis(float p, float lo, float hi) { return p < lo ? lo - p : (p > hi ? p - hi : 0.f); }

// one thread per Morton-sorted query
__global__ __launch_bounds__(256) void nn_query(int Pq, const float* __restrict__ query, const uint32_t* __restrict__ qidx, int Pr,
                                                const uint32_t* __restrict__ rkeys, const float4* __restrict__ rsorted,
                                                const float4* __restrict__ boxes, int nboxes, const float* __restrict__ bbox,
                                                float* __restrict__ out_d2, int* __restrict__ out_idx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Pq) return;
  const uint32_t q = qidx[i];
  const float px = query[3 * (size_t)q], py = query[3 * (size_t)q + 1], pz = query[3 * (size_t)q + 2];
  // start: the sorted reference points around the query's own Morton code (a query outside the reference box is clamped onto it)
  const int lo = morton_lower_bound(rkeys, Pr, morton_code30(px, py, pz, bbox));
  float best = INFINITY;                         // (an infinite distance is still taken, lowest index first)
  uint32_t bid = 0xFFFFFFFFu;
  const int j0 = max(0, lo - NN_WIN), j1 = min(Pr, lo + NN_WIN);
  for (int j = j0; j < j1; j++) {
    const float4 r = rsorted[j];
    nn_take(nn_d2(px, py, pz, r), __float_as_uint(r.w), best, bid);
  }
  for (int b = 0; b < nboxes; b++) {
    const float4 bmn = boxes[2 * b], bmx = boxes[2 * b + 1];
    const float d0 = nn_axis(px, bmn.x, bmx.x), d1 = nn_axis(py, bmn.y, bmx.y), d2 = nn_axis(pz, bmn.z, bmx.z);
    if ((d0 * d0 + d1 * d1) + d2 * d2 > best) continue;
    const int e = min(Pr, (b + 1) * NN_BOX);
    for (int j = b * NN_BOX; j < e; j++) {
      const float4 r = rsorted[j];
      nn_take(nn_d2(px, py, pz, r), __float_as_uint(r.w), best, bid);
    }
  }
  out_d2[q] = best;
  out_idx[q] = (int)bid;
}

}  // namespace gm

// ---------------------------------------------------------------------------------------------
// the entry points (include/gmesh_hip.h): their refusals, then the launches
using namespace gm;

extern "C" {

size_t gm_knn_workspace_bytes(int P) {
  KnnWs k = KnnWs::from(nullptr, (size_t)(P > 0 ? P : 1));
  return (size_t)k.end + 256;
}

int gm_knn(int P, const float* points, float* meanDists, void* workspace, size_t workspace_bytes, void* stream) {
  if (P < 0 || (P > 0 && (!points || !meanDists || !workspace))) { set_error("gm_knn: bad args"); return GM_ERR_INVALID_ARG; }
  if (P == 0) return GM_OK;
  const size_t need = gm_knn_workspace_bytes(P);
  if (workspace_bytes < need) { set_error("gm_knn: workspace too small (%zu < %zu)", workspace_bytes, need); return GM_ERR_BUFFER; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  KnnWs k = KnnWs::from(workspace, (size_t)P);
  if (int rc = launch_point_bbox(P, points, k.front.bbox_partial, k.front.bbox, s)) return rc;
  if (int rc = launch_point_morton(P, points, k.front.bbox, k.set.keys[0], s)) return rc;
  MortonSorted sorted;
  if (int rc = morton_sort(k.set, k.front, (size_t)P, &sorted, s)) return rc;
  const int nboxes = (P + KNN_BOX - 1) / KNN_BOX;
  hipLaunchKernelGGL(knn_box_minmax, dim3(nboxes), dim3(256), 0, s, P, points, sorted.idx, k.boxes);
  hipLaunchKernelGGL(knn_box_mean_dist, dim3((P + 255) / 256), dim3(256), 0, s, P, points, sorted.idx, k.boxes, meanDists);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

size_t gm_knn_nearest_workspace_bytes(int Pq, int Pr) {
  NnWs k = NnWs::from(nullptr, (size_t)(Pq > 0 ? Pq : 1), (size_t)(Pr > 0 ? Pr : 1));
  return (size_t)k.end + 256;
}

int gm_knn_nearest(int Pq, const float* query, int Pr, const float* ref, float* out_d2, int* out_idx, void* workspace, size_t workspace_bytes,
                   void* stream) {
  if (Pq < 0 || Pr < 0) { set_error("gm_knn_nearest: negative size"); return GM_ERR_INVALID_ARG; }
  if (Pr == 0) { set_error("gm_knn_nearest: empty reference set (Pr == 0)"); return GM_ERR_INVALID_ARG; }
  if (Pq == 0) return GM_OK;
  if (!query || !ref || !out_d2 || !out_idx || !workspace) { set_error("gm_knn_nearest: null pointer"); return GM_ERR_INVALID_ARG; }
  const size_t need = gm_knn_nearest_workspace_bytes(Pq, Pr);
  if (workspace_bytes < need) { set_error("gm_knn_nearest: workspace too small (%zu < %zu)", workspace_bytes, need); return GM_ERR_BUFFER; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  NnWs k = NnWs::from(workspace, (size_t)Pq, (size_t)Pr);
  if (int rc = launch_point_bbox(Pr, ref, k.front.bbox_partial, k.front.bbox, s)) return rc;
  if (int rc = launch_point_morton(Pr, ref, k.front.bbox, k.rset.keys[0], s)) return rc;
  if (int rc = launch_point_morton(Pq, query, k.front.bbox, k.qset.keys[0], s)) return rc;
  MortonSorted r, q;
  if (int rc = morton_sort(k.rset, k.front, (size_t)Pr, &r, s)) return rc;
  if (int rc = morton_sort(k.qset, k.front, (size_t)Pq, &q, s)) return rc;
  const int nboxes = (Pr + NN_BOX - 1) / NN_BOX;
  hipLaunchKernelGGL(nn_gather_boxes, dim3(nboxes), dim3(NN_BOX), 0, s, Pr, ref, r.idx, k.rsorted, k.boxes);
  hipLaunchKernelGGL(nn_query, dim3((Pq + 255) / 256), dim3(256), 0, s, Pq, query, q.idx, Pr, r.keys, k.rsorted, k.boxes, nboxes,
                     k.front.bbox, out_d2, out_idx);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // extern "C"
