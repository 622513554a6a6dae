// gm_closest.hip -- closest triangle of a proxy mesh for every point of a cloud (gm_closest_face): the search behind
// mesh_bind.closest_faces / bind_points, which binds a plain Gaussian cloud to a mesh (the branch of SingleObjectDeform.load_mesh
// that runs when the file carries no face ids, edittool/__init__.py:68-85: igl.point_mesh_squared_distance there).
//
// THE RESULT IS DEFINED BY ARITHMETIC, not by the search structure (the contract gm_knn_nearest has, gm_knn.hip):
//   per (point p, face f = (a, b, c)), everything in float32, no contraction (file pragma), correctly rounded divisions,
//   dot(u, w) = (u.x*w.x + u.y*w.y) + u.z*w.z, and in this order (Ericson, "Real-Time Collision Detection" 5.1.5, as
//   edittool.point_mesh_squared_distance evaluates it):
//     ab = b - a, ac = c - a, cb = c - b
//     ap = p - a: d1 = dot(ab, ap), d2 = dot(ac, ap);  bp = p - b: d3 = dot(ab, bp), d4 = dot(ac, bp);  cp = p - c: d5 = dot(ab, cp), d6 = dot(ac, cp)
//     vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6, va = d3*d6 - d5*d4
//     denom = 1 / ((va + vb) + vc), v = vb*denom, w = vc*denom
//     t_ab = d1 / (d1 - d3), t_ac = d2 / (d2 - d6), x = d4 - d3, y = d5 - d6, t_bc = x / (x + y)
//     q = (a + ab*v) + ac*w                                            interior, unless one of the following holds; the LAST that holds wins:
//     q = b + cb*t_bc   if va <= 0 and x >= 0 and y >= 0               edge bc
//     q = a + ac*t_ac   if vb <= 0 and d2 >= 0 and d6 <= 0             edge ac
//     q = a + ab*t_ab   if vc <= 0 and d1 >= 0 and d3 <= 0             edge ab
//     q = c             if d6 >= 0 and d5 <= d6                        vertex c
//     q = b             if d3 >= 0 and d4 <= d3                        vertex b
//     q = a             if d1 <= 0 and d2 <= 0                         vertex a
//     (each product and sum of a vector expression per component: q.x = (a.x + ab.x*v) + ac.x*w, ...)
//     e = p - q, dist2 = (e.x*e.x + e.y*e.y) + e.z*e.z
//   winner: the smallest dist2, ties to the lowest face index, a NaN dist2 (a degenerate face: 0 / 0) never wins; if every face gives
//   NaN: out_face = -1, out_d2 = +inf, out_closest = NaN.  out_closest is the winner's q.
//   Taking the minimum of (dist2, index) pairs does not depend on the order of evaluation, and a face may be evaluated twice: the output
//   equals that of a float32 brute force over all F faces bit for bit provided no face that could win is skipped.
//
// Search structure: the faces in Morton order of their centroids ((a + b) + c) / 3 against the bounding box of the vertices (our radix
// sort, gm_sort.hip), re-packed as 48-byte records (a, b, c, original index) and cut into boxes of CF_BOX = 64 faces, the boxes into
// super-boxes of 64 boxes.  The queries in Morton order too (clamped onto the same box), one per lane, so that a wave's 64 queries are
// neighbours.  A lane starts from the CF_WIN sorted faces around its own Morton code.  The box loops are WAVE-UNIFORM: a (super-)box is
// entered when any lane of the wave still needs it (ballot); its records then come by uniform-address loads and every lane evaluates
// them - an extra evaluation never changes a result.  Per query: F / 4096 super-box tests, 64 box tests per super-box entered.
//
// WHEN A BOX MAY BE SKIPPED.  A box record holds lo / hi = the bounding box of all vertices of its faces, M = the largest |coordinate| of
// lo / hi, and tau = max over its faces of L^3 / S with L^2 = the longest squared edge and S = |ab x ac|^2 (inf for a face without area).
// A lane skips a box iff  LB > best  (strictly: a face as far as the best so far but with a lower index is still visited), where, with
// eps = 2^-24,
//     m     = 2^-19 (|p|_inf + M)  +  2^-17 tau Dfar^2,        Dfar^2 = sum_k max(|p_k - lo_k|, |p_k - hi_k|)^2
//     g_k   = max(lo_k - p_k, p_k - hi_k, 0),  LB = (1 - 2^-20) sum_k max(g_k - m, 0)^2 .
// Claim: for every face f of the box the float32 dist2_f(p) is NaN or >= LB (no overflow / underflow).  Then dist2_f >= LB > best: f can
// neither win nor tie, whatever its index.  The argument goes through the branch that produced q; by a <= b below we mean the float values.
//   vertex branches: q is a vertex, exactly: inside [lo, hi].
//   edge ab: taken only if d1 >= 0 and d3 <= 0.  Then d1 - d3 >= d1 exactly and rounding is monotonic, so fl(d1 - d3) >= d1 >= 0 and
//     t_ab = fl(d1 / fl(d1 - d3)) lies in [0, 1] - or is 0 / 0 = NaN, and then so is dist2.  The exact a_k + (b_k - a_k) t lies between
//     a_k and b_k; the three roundings of fl(a_k + fl(fl(b_k - a_k) t)) move it by at most (2 + 2 + 1) eps M (1 + o(1)) < 6 eps M.
//     Edge ac (d2 >= 0, d6 <= 0) and edge bc (x >= 0, y >= 0: fl(x + y) >= x) are the same statement.
//   interior with va, vb, vc >= 0: s = fl(fl(va + vb) + vc) >= max(vb, vc) by monotonicity, so v, w in [0, 1 + 2.1 eps] and
//     v + w <= (1 + eps)^4; s = 0 gives inf or NaN, and an infinite dist2 is >= every LB.  a (1 - v - w) + b v + c w is a convex
//     combination of the vertices moved by at most 4.1 eps |r - a| <= 8.2 eps M; the roundings of (a + ab*v) + ac*w add < 15 eps M.
//     So q_k in [lo_k - 23 eps M, hi_k + 23 eps M]; the first term of m is 32 eps (|p|_inf + M).
//   interior with a negative va, vb or vc: in exact arithmetic the chain is complete - the interior is reached only with all three
//     positive - so this needs a rounding error to flip a test.  d1 .. d6 carry errors <= 7 eps L D (D >= |p - vertex|), va, vb, vc errors
//     <= E = 31 eps L^2 D^2, while their exact sum is S.  A value that the chain let through although it is negative is within E of zero, so
//     v, w >= -2 E / S and v + w <= 1 + 2 E / S, which moves q by at most 2 L * 2 E / S < 128 eps (L^3 / S) D^2 off the triangle: the second
//     term of m, with Dfar >= D.  (When E exceeds S / 2 - a sliver, or a point thousands of edge lengths away - the float32 formula itself
//     stops meaning anything; there the term is as large as the distances and nothing is skipped.  A face with S = 0 has tau = inf: its
//     box is never skipped.)  This last case is an argument about the size of the rounding noise, not a branch-by-branch derivation as the
//     cases above.
//   distance: e_k = fl(p_k - q_k) has relative error eps, and |p_k - q_k| >= g_k - (the bound above) where g_k > 0; three squares and two
//     sums lose a factor (1 - eps)^5 at most; on the other side g_k, m, the squares and sums of LB gain at most (1 + eps)^6: the factor
//     1 - 2^-20 = 1 - 16 eps covers both.  A NaN in LB (inf - inf) fails "LB > best": the box is visited.
// The same holds for a super-box (lo / hi the union, M and tau the maxima of its boxes).
//
// Conventions of gm_knn_nearest: caller workspace, stream-ordered, no device allocation, no host wait anywhere in this file.
#include "gm_common.h"
#include "gm_check.h"
#include "gm_spatial.h"
#include "gm_wave.h"
#include <cfloat>
#pragma clang fp contract(off)   // every product and sum rounds on its own, as the definition above says

namespace gm {

#define CF_BOX 64        // faces per box
#define CF_SUPER 64      // boxes per super-box
#define CF_WIN 4         // sorted faces on either side of a query's own Morton code evaluated first

struct CfWs {
  MortonWs front;        // bbox of the vertices; sort scratch for the larger of the two sets
  MortonSet fset, qset;
  float4* recs;          // [F][3] ax ay az bx | by bz cx cy | cz index(bits) 0 0, in Morton order
  float4* boxes;         // [nboxes][2] lo xyz, tau | hi xyz, M
  float4* sboxes;        // [nsuper][2]
  char* end;
  static CfWs from(void* ws, size_t N, size_t F) {
    char* p = reinterpret_cast<char*>(ws);
    const size_t nboxes = (F + CF_BOX - 1) / CF_BOX;
    CfWs k;
    k.front = MortonWs::carve_from(p, N > F ? N : F);
    k.fset = MortonSet::carve_from(p, F);
    k.qset = MortonSet::carve_from(p, N);
    k.recs = carve<float4>(p, 3 * F);
    k.boxes = carve<float4>(p, 2 * nboxes);
    k.sboxes = carve<float4>(p, 2 * ((nboxes + CF_SUPER - 1) / CF_SUPER));
    k.end = p;
    return k;
  }
};

// Morton code of a face: that of its centroid against the vertices' bounding box
__global__ __launch_bounds__(256) void cf_face_morton(int F, int Vm, const float* __restrict__ verts, const int* __restrict__ faces,
                                                      const float* __restrict__ bbox, uint32_t* __restrict__ codes) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const size_t ia = face_vertex(faces, 3 * (size_t)f, Vm), ib = face_vertex(faces, 3 * (size_t)f + 1, Vm), ic = face_vertex(faces, 3 * (size_t)f + 2, Vm);
  float c[3];
#pragma unroll
  for (int k = 0; k < 3; k++) c[k] = ((verts[3 * ia + k] + verts[3 * ib + k]) + verts[3 * ic + k]) / 3.0f;
  codes[f] = morton_code30(c[0], c[1], c[2], bbox);
}

// one wave per box: the sorted face records, and the box record (lo, tau | hi, M)
__global__ __launch_bounds__(CF_BOX) void cf_gather_boxes(int F, int Vm, const float* __restrict__ verts, const int* __restrict__ faces,
                                                          const uint32_t* __restrict__ idx, float4* __restrict__ recs, float4* __restrict__ boxes) {
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  float tau = 0.f;
  const int i = blockIdx.x * CF_BOX + threadIdx.x;
  if (i < F) {
    const uint32_t g = idx[i];
    const size_t ia = face_vertex(faces, 3 * (size_t)g, Vm), ib = face_vertex(faces, 3 * (size_t)g + 1, Vm), ic = face_vertex(faces, 3 * (size_t)g + 2, Vm);
    float a[3], b[3], c[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      a[k] = verts[3 * ia + k]; b[k] = verts[3 * ib + k]; c[k] = verts[3 * ic + k];
      mn[k] = fminf(a[k], fminf(b[k], c[k])); mx[k] = fmaxf(a[k], fmaxf(b[k], c[k]));
    }
    recs[3 * (size_t)i] = make_float4(a[0], a[1], a[2], b[0]);
    recs[3 * (size_t)i + 1] = make_float4(b[1], b[2], c[0], c[1]);
    recs[3 * (size_t)i + 2] = make_float4(c[2], __uint_as_float(g), 0.f, 0.f);
    const float ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]}, cb[3] = {c[0] - b[0], c[1] - b[1], c[2] - b[2]};
    const float n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
    const float S = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    const float L2 = fmaxf(ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2],
                           fmaxf(ac[0] * ac[0] + ac[1] * ac[1] + ac[2] * ac[2], cb[0] * cb[0] + cb[1] * cb[1] + cb[2] * cb[2]));
    tau = 1.0625f * (L2 * sqrtf(L2)) / S;        // (1.0625: S and L2 are computed values, a few eps off)
    if (!(tau < FLT_MAX)) tau = INFINITY;        // no area (S == 0, or 0 / 0 for three equal vertices): the box is never skipped
  }
#pragma unroll
  for (int k = 0; k < 3; k++) { mn[k] = wave_min_f32(mn[k]); mx[k] = wave_max_f32(mx[k]); }
  tau = wave_max_f32(tau);
  if (threadIdx.x == 0) {
    float M = 0.f;
#pragma unroll
    for (int k = 0; k < 3; k++) M = fmaxf(M, fmaxf(fabsf(mn[k]), fabsf(mx[k])));
    boxes[2 * blockIdx.x] = make_float4(mn[0], mn[1], mn[2], tau);
    boxes[2 * blockIdx.x + 1] = make_float4(mx[0], mx[1], mx[2], M);
  }
}

// one wave per super-box: union of its boxes, maxima of tau and M
__global__ __launch_bounds__(CF_SUPER) void cf_super_boxes(int nboxes, const float4* __restrict__ boxes, float4* __restrict__ sboxes) {
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  float tau = 0.f, M = 0.f;
  const int b = blockIdx.x * CF_SUPER + threadIdx.x;
  if (b < nboxes) {
    const float4 lo = boxes[2 * b], hi = boxes[2 * b + 1];
    mn[0] = lo.x; mn[1] = lo.y; mn[2] = lo.z; tau = lo.w;
    mx[0] = hi.x; mx[1] = hi.y; mx[2] = hi.z; M = hi.w;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) { mn[k] = wave_min_f32(mn[k]); mx[k] = wave_max_f32(mx[k]); }
  tau = wave_max_f32(tau); M = wave_max_f32(M);
  if (threadIdx.x == 0) {
    sboxes[2 * blockIdx.x] = make_float4(mn[0], mn[1], mn[2], tau);
    sboxes[2 * blockIdx.x + 1] = make_float4(mx[0], mx[1], mx[2], M);
  }
}

// the definition at the top of this file, line by line
__device__ __forceinline__ float cf_dot(float ux, float uy, float uz, float wx, float wy, float wz) { return (ux * wx + uy * wy) + uz * wz; }
__device__ __forceinline__ void cf_eval(float px, float py, float pz, const float4 r0, const float4 r1, const float4 r2, float& best, uint32_t& bid,
                                        float& bqx, float& bqy, float& bqz) {
  const float ax = r0.x, ay = r0.y, az = r0.z, bx = r0.w, by = r1.x, bz = r1.y, cx = r1.z, cy = r1.w, cz = r2.x;
  const uint32_t id = __float_as_uint(r2.y);
  const float abx = bx - ax, aby = by - ay, abz = bz - az, acx = cx - ax, acy = cy - ay, acz = cz - az, cbx = cx - bx, cby = cy - by, cbz = cz - bz;
  const float apx = px - ax, apy = py - ay, apz = pz - az;
  const float d1 = cf_dot(abx, aby, abz, apx, apy, apz), d2 = cf_dot(acx, acy, acz, apx, apy, apz);
  const float bpx = px - bx, bpy = py - by, bpz = pz - bz;
  const float d3 = cf_dot(abx, aby, abz, bpx, bpy, bpz), d4 = cf_dot(acx, acy, acz, bpx, bpy, bpz);
  const float cpx = px - cx, cpy = py - cy, cpz = pz - cz;
  const float d5 = cf_dot(abx, aby, abz, cpx, cpy, cpz), d6 = cf_dot(acx, acy, acz, cpx, cpy, cpz);
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const float denom = 1.0f / ((va + vb) + vc);
  const float v = vb * denom, w = vc * denom;
  const float t_ab = d1 / (d1 - d3), t_ac = d2 / (d2 - d6);
  const float x = d4 - d3, y = d5 - d6;
  const float t_bc = x / (x + y);
  float qx = (ax + abx * v) + acx * w, qy = (ay + aby * v) + acy * w, qz = (az + abz * v) + acz * w;
  if (va <= 0.f && x >= 0.f && y >= 0.f) { qx = bx + cbx * t_bc; qy = by + cby * t_bc; qz = bz + cbz * t_bc; }
  if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { qx = ax + acx * t_ac; qy = ay + acy * t_ac; qz = az + acz * t_ac; }
  if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { qx = ax + abx * t_ab; qy = ay + aby * t_ab; qz = az + abz * t_ab; }
  if (d6 >= 0.f && d5 <= d6) { qx = cx; qy = cy; qz = cz; }
  if (d3 >= 0.f && d4 <= d3) { qx = bx; qy = by; qz = bz; }
  if (d1 <= 0.f && d2 <= 0.f) { qx = ax; qy = ay; qz = az; }
  const float ex = px - qx, ey = py - qy, ez = pz - qz;
  const float d = (ex * ex + ey * ey) + ez * ez;
  if (d < best || (d == best && id < bid)) { best = d; bid = id; bqx = qx; bqy = qy; bqz = qz; }     // (NaN: neither)
}

// LB of the header comment: a lower bound of the float32 dist2 of every face of the box
__device__ __forceinline__ float cf_lower(float px, float py, float pz, float pinf, const float4 lo, const float4 hi) {
  const float fx = fmaxf(fabsf(px - lo.x), fabsf(px - hi.x)), fy = fmaxf(fabsf(py - lo.y), fabsf(py - hi.y)), fz = fmaxf(fabsf(pz - lo.z), fabsf(pz - hi.z));
  const float dfar2 = (fx * fx + fy * fy) + fz * fz;
  const float m = 0x1p-19f * (pinf + hi.w) + (0x1p-17f * lo.w) * dfar2;
  const float gx = fmaxf(fmaxf(fmaxf(lo.x - px, px - hi.x), 0.f) - m, 0.f);
  const float gy = fmaxf(fmaxf(fmaxf(lo.y - py, py - hi.y), 0.f) - m, 0.f);
  const float gz = fmaxf(fmaxf(fmaxf(lo.z - pz, pz - hi.z), 0.f) - m, 0.f);
  return ((gx * gx + gy * gy) + gz * gz) * (1.0f - 0x1p-20f);
}

// one lane per Morton-sorted query; the box loops are wave-uniform
__global__ __launch_bounds__(256) void cf_query(int N, const float* __restrict__ points, const uint32_t* __restrict__ qidx, int F,
                                                const uint32_t* __restrict__ fkeys, const float4* __restrict__ recs,
                                                const float4* __restrict__ boxes, int nboxes, const float4* __restrict__ sboxes, int nsuper,
                                                const float* __restrict__ bbox, float* __restrict__ out_d2, int* __restrict__ out_face,
                                                float* __restrict__ out_closest) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < N;
  const uint32_t q = qidx[live ? i : N - 1];       // a lane past the end repeats the last query (it needs no box of its own) and stores nothing
  const float px = points[3 * (size_t)q], py = points[3 * (size_t)q + 1], pz = points[3 * (size_t)q + 2];
  const float pinf = fmaxf(fabsf(px), fmaxf(fabsf(py), fabsf(pz)));
  float best = INFINITY, bqx = __uint_as_float(0x7FC00000u), bqy = bqx, bqz = bqx;     // (an infinite dist2 is still taken, lowest index first)
  uint32_t bid = 0xFFFFFFFFu;
  // start: the sorted faces around the query's own Morton code (a query outside the vertices' box is clamped onto it)
  const int lo = morton_lower_bound(fkeys, F, morton_code30(px, py, pz, bbox));
  const int j0 = max(0, lo - CF_WIN), j1 = min(F, lo + CF_WIN);
  for (int j = j0; j < j1; j++) cf_eval(px, py, pz, recs[3 * (size_t)j], recs[3 * (size_t)j + 1], recs[3 * (size_t)j + 2], best, bid, bqx, bqy, bqz);
  for (int sb = 0; sb < nsuper; sb++) {
    const bool need_sb = !(cf_lower(px, py, pz, pinf, sboxes[2 * sb], sboxes[2 * sb + 1]) > best);
    if (!__any(need_sb)) continue;
    const int b1 = min(nboxes, (sb + 1) * CF_SUPER);
    for (int b = sb * CF_SUPER; b < b1; b++) {
      const bool need = need_sb && !(cf_lower(px, py, pz, pinf, boxes[2 * b], boxes[2 * b + 1]) > best);
      if (!__any(need)) continue;
      const int e = min(F, (b + 1) * CF_BOX);
#pragma unroll 2
      for (int j = b * CF_BOX; j < e; j++)         // every lane evaluates: one more candidate never changes a result
        cf_eval(px, py, pz, recs[3 * (size_t)j], recs[3 * (size_t)j + 1], recs[3 * (size_t)j + 2], best, bid, bqx, bqy, bqz);
    }
  }
  if (!live) return;
  out_d2[q] = best;
  out_face[q] = (int)bid;
  if (out_closest) { out_closest[3 * (size_t)q] = bqx; out_closest[3 * (size_t)q + 1] = bqy; out_closest[3 * (size_t)q + 2] = bqz; }
}

}  // namespace gm

// ---------------------------------------------------------------------------------------------
// the entry points (include/gmesh_hip.h): their refusals, then the launches
using namespace gm;

extern "C" {

size_t gm_closest_face_workspace_bytes(int N, int F) {
  CfWs k = CfWs::from(nullptr, (size_t)(N > 0 ? N : 1), (size_t)(F > 0 ? F : 1));
  return (size_t)k.end + 256;
}

int gm_closest_face(int N, const float* points, int Vm, const float* vertices, int F, const int* faces, float* out_d2, int* out_face,
                    float* out_closest, void* workspace, size_t workspace_bytes, void* stream) {
  if (N < 0 || Vm < 0 || F < 0) { set_error("gm_closest_face: negative size N=%d Vm=%d F=%d", N, Vm, F); return GM_ERR_INVALID_ARG; }
  if (N == 0) return GM_OK;
  if (F == 0 || Vm == 0) { set_error("gm_closest_face: empty mesh (F == %d, Vm == %d)", F, Vm); return GM_ERR_INVALID_ARG; }
  if (!points || !vertices || !faces || !out_d2 || !out_face || !workspace) { set_error("gm_closest_face: null pointer"); return GM_ERR_INVALID_ARG; }
  const size_t need = gm_closest_face_workspace_bytes(N, F);
  if (workspace_bytes < need) { set_error("gm_closest_face: workspace too small (%zu < %zu)", workspace_bytes, need); return GM_ERR_BUFFER; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  CfWs k = CfWs::from(workspace, (size_t)N, (size_t)F);
  if (int rc = launch_point_bbox(Vm, vertices, k.front.bbox_partial, k.front.bbox, s)) return rc;
  hipLaunchKernelGGL(cf_face_morton, dim3((F + 255) / 256), dim3(256), 0, s, F, Vm, vertices, faces, k.front.bbox, k.fset.keys[0]);
  if (int rc = launch_point_morton(N, points, k.front.bbox, k.qset.keys[0], s)) return rc;
  MortonSorted f, q;
  if (int rc = morton_sort(k.fset, k.front, (size_t)F, &f, s)) return rc;
  if (int rc = morton_sort(k.qset, k.front, (size_t)N, &q, s)) return rc;
  const int nboxes = (F + CF_BOX - 1) / CF_BOX, nsuper = (nboxes + CF_SUPER - 1) / CF_SUPER;
  hipLaunchKernelGGL(cf_gather_boxes, dim3(nboxes), dim3(CF_BOX), 0, s, F, Vm, vertices, faces, f.idx, k.recs, k.boxes);
  hipLaunchKernelGGL(cf_super_boxes, dim3(nsuper), dim3(CF_SUPER), 0, s, nboxes, k.boxes, k.sboxes);
  hipLaunchKernelGGL(cf_query, dim3((N + 255) / 256), dim3(256), 0, s, N, points, q.idx, F, f.keys, k.recs, k.boxes, nboxes, k.sboxes,
                     nsuper, k.front.bbox, out_d2, out_face, out_closest);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // extern "C"
