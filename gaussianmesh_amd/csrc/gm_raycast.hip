// gm_raycast.hip -- first hit of every ray on a proxy mesh (gm_ray_mesh): the stage behind mesh_pick.ray_mesh_hits / pick /
// visible_vertices, which takes an editor from a pixel to a vertex id of the current, deformed mesh.
//
// THE RESULT IS DEFINED BY ARITHMETIC (the contract gm_closest_face has, gm_closest.hip):
//   per (ray (o, d), face f = (a, b, c)), everything in float32, no contraction (file pragma), correctly rounded division,
//   dot(x, y) = (x.x*y.x + x.y*y.y) + x.z*y.z, (x cross y).x = x.y*y.z - x.z*y.y and so on (Moeller & Trumbore 1997, two-sided):
//     e1 = b - a, e2 = c - a, p = d cross e2, det = dot(e1, p), s = o - a, q = s cross e1, inv = 1 / det
//     u = dot(s, p) * inv, v = dot(d, q) * inv, t = dot(e2, q) * inv
//     hit  iff  u >= 0 and v >= 0 and (u + v) <= 1 and t >= t_min and t <= t_max          (every comparison false on NaN)
//   There is no epsilon on det: det == 0 gives inf or NaN, which fail the comparisons by themselves.
//   winner: the smallest t, ties to the lowest face index; outputs t + 0.0f (-0 reported as +0), the index, (u, v).
//   No hit: face = -1, t = +inf, u = v = NaN.
//   A minimum of (t, index) pairs does not depend on the order of evaluation, so the outputs equal a float32 brute force over all F
//   faces bit for bit.  NO FACE IS SKIPPED: every (ray, face) pair is evaluated, there is no hierarchy and no early reject.
//
// Structure: rc_prepare writes one 48-byte record per face (a, e1, e2 - the differences are the definition's own, rounded once) and
// arms one 64-bit slot per ray.  rc_cast runs on a grid of ray blocks x face chunks (flattened: consecutive workgroups share a
// chunk), one lane per ray; the face loop is wave-uniform, the records come by uniform-address loads and are scalar operands.  A lane
// keeps its best hit as the key (bits(t + 0.0f) << 32) | face: an accepted t is >= +0 and never NaN, so the unsigned order of the
// keys is the order of (t, face).  A lane that hit something merges its key into the ray's slot with one 64-bit atomicMin - a minimum
// is order-independent: same bits every run.  rc_finish recomputes (u, v) of the winning face with the same function.
// A pick (a few rays x 10^5 faces) fills the chip through the face chunks, a selection (10^4 .. 10^6 rays) through the ray blocks.
//
// Conventions of gm_closest_face: caller workspace, stream-ordered, no device allocation, no host wait anywhere in this file.
#include "gm_common.h"
#include "gm_check.h"
#pragma clang fp contract(off)   // every product and sum rounds on its own, as the definition above says

namespace gm {

#define RC_CHUNK 64      // faces per workgroup of rc_cast
#define RC_MISS 0xFFFFFFFFFFFFFFFFull

struct RcWs {
  float4* recs;                  // [F][3] ax ay az e1x | e1y e1z e2x e2y | e2z 0 0 0, in face order
  unsigned long long* slots;     // [R] the smallest key so far
  char* end;
  static RcWs from(void* ws, size_t R, size_t F) {
    char* p = reinterpret_cast<char*>(ws);
    RcWs k;
    k.recs = carve<float4>(p, 3 * F);
    k.slots = carve<unsigned long long>(p, R);
    k.end = p;
    return k;
  }
};

static inline int rc_div_up(int n, int d) { return n > 0 ? (n - 1) / d + 1 : 0; }      // (no overflow near INT_MAX)

// workgroups of rc_cast; more than a grid holds is refused by gm_ray_mesh
static inline unsigned long long ray_mesh_blocks(int R, int F) { return (unsigned long long)rc_div_up(R, 256) * (unsigned long long)rc_div_up(F, RC_CHUNK); }

__global__ __launch_bounds__(256) void rc_prepare(int F, int Vm, const float* __restrict__ verts, const int* __restrict__ faces,
                                                  float4* __restrict__ recs, int R, unsigned long long* __restrict__ slots) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < R) slots[i] = RC_MISS;
  if (i >= F) return;
  const size_t ia = face_vertex(faces, 3 * (size_t)i, Vm), ib = face_vertex(faces, 3 * (size_t)i + 1, Vm), ic = face_vertex(faces, 3 * (size_t)i + 2, Vm);
  const float ax = verts[3 * ia], ay = verts[3 * ia + 1], az = verts[3 * ia + 2];
  recs[3 * (size_t)i] = make_float4(ax, ay, az, verts[3 * ib] - ax);
  recs[3 * (size_t)i + 1] = make_float4(verts[3 * ib + 1] - ay, verts[3 * ib + 2] - az, verts[3 * ic] - ax, verts[3 * ic + 1] - ay);
  recs[3 * (size_t)i + 2] = make_float4(verts[3 * ic + 2] - az, 0.f, 0.f, 0.f);
}

// the definition at the top of this file, line by line
__device__ __forceinline__ float rc_dot(float xx, float xy, float xz, float yx, float yy, float yz) { return (xx * yx + xy * yy) + xz * yz; }
__device__ __forceinline__ bool rc_eval(float ox, float oy, float oz, float dx, float dy, float dz, const float4 r0, const float4 r1, const float4 r2,
                                        float t_min, float t_max, float& t, float& u, float& v) {
  const float ax = r0.x, ay = r0.y, az = r0.z, e1x = r0.w, e1y = r1.x, e1z = r1.y, e2x = r1.z, e2y = r1.w, e2z = r2.x;
  const float px = dy * e2z - dz * e2y, py = dz * e2x - dx * e2z, pz = dx * e2y - dy * e2x;
  const float det = rc_dot(e1x, e1y, e1z, px, py, pz);
  const float sx = ox - ax, sy = oy - ay, sz = oz - az;
  const float qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
  const float inv = 1.0f / det;
  u = rc_dot(sx, sy, sz, px, py, pz) * inv;
  v = rc_dot(dx, dy, dz, qx, qy, qz) * inv;
  t = rc_dot(e2x, e2y, e2z, qx, qy, qz) * inv;
  return u >= 0.f && v >= 0.f && (u + v) <= 1.0f && t >= t_min && t <= t_max;      // (NaN: false)
}

// workgroup w: ray block w % ray_blocks, face chunk w / ray_blocks; one lane per ray, the face loop wave-uniform
__global__ __launch_bounds__(256) void rc_cast(int R, const float* __restrict__ origins, const float* __restrict__ dirs, int F,
                                               const float4* __restrict__ recs, int ray_blocks, float t_min, float t_max,
                                               unsigned long long* __restrict__ slots) {
  const int rb = blockIdx.x % ray_blocks, chunk = blockIdx.x / ray_blocks;
  const int i = rb * 256 + threadIdx.x;
  if (i - (int)(threadIdx.x & 63) >= R) return;    // a whole wave past the end
  const bool live = i < R;
  const size_t r = (size_t)(live ? i : R - 1);     // a lane past the end repeats the last ray and merges nothing
  const float ox = origins[3 * r], oy = origins[3 * r + 1], oz = origins[3 * r + 2];
  const float dx = dirs[3 * r], dy = dirs[3 * r + 1], dz = dirs[3 * r + 2];
  unsigned long long best = RC_MISS;
  const int f0 = chunk * RC_CHUNK, f1 = f0 + min(F - f0, RC_CHUNK);
#pragma unroll 4
  for (int f = f0; f < f1; f++) {
    float t, u, v;
    const bool hit = rc_eval(ox, oy, oz, dx, dy, dz, recs[3 * (size_t)f], recs[3 * (size_t)f + 1], recs[3 * (size_t)f + 2], t_min, t_max, t, u, v);
    const unsigned long long key = ((unsigned long long)__float_as_uint(t + 0.0f) << 32) | (unsigned)f;
    if (hit && key < best) best = key;
  }
  if (live && best != RC_MISS) atomicMin(&slots[r], best);
}

__global__ __launch_bounds__(256) void rc_finish(int R, const float* __restrict__ origins, const float* __restrict__ dirs,
                                                 const float4* __restrict__ recs, const unsigned long long* __restrict__ slots, float t_min,
                                                 float t_max, float* __restrict__ out_t, int* __restrict__ out_face, float* __restrict__ out_uv) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= R) return;
  const unsigned long long key = slots[i];
  const float nan = __uint_as_float(0x7FC00000u);
  float t = INFINITY, u = nan, v = nan;
  int face = -1;
  if (key != RC_MISS) {
    face = (int)(unsigned)key;
    const size_t r = (size_t)i, f = (size_t)face;
    rc_eval(origins[3 * r], origins[3 * r + 1], origins[3 * r + 2], dirs[3 * r], dirs[3 * r + 1], dirs[3 * r + 2], recs[3 * f], recs[3 * f + 1],
            recs[3 * f + 2], t_min, t_max, t, u, v);
    t = t + 0.0f;
  }
  out_t[i] = t;
  out_face[i] = face;
  if (out_uv) { out_uv[2 * (size_t)i] = u; out_uv[2 * (size_t)i + 1] = v; }
}

}  // namespace gm

// ---------------------------------------------------------------------------------------------
// the entry points (include/gmesh_hip.h): their refusals, then the launches
using namespace gm;

extern "C" {

size_t gm_ray_mesh_workspace_bytes(int R, int F) {
  RcWs k = RcWs::from(nullptr, (size_t)(R > 0 ? R : 1), (size_t)(F > 0 ? F : 1));
  return (size_t)k.end + 256;
}

int gm_ray_mesh(int R, const float* origins, const float* dirs, int Vm, const float* vertices, int F, const int* faces, float t_min, float t_max,
                float* out_t, int* out_face, float* out_uv, void* workspace, size_t workspace_bytes, void* stream) {
  if (R < 0 || Vm < 0 || F < 0) { set_error("gm_ray_mesh: negative size R=%d Vm=%d F=%d", R, Vm, F); return GM_ERR_INVALID_ARG; }
  if (!(t_min >= 0.f) || t_max != t_max) { set_error("gm_ray_mesh: t_min must be >= 0 and neither bound NaN"); return GM_ERR_INVALID_ARG; }
  if (R == 0) return GM_OK;
  if (F == 0 || Vm == 0) { set_error("gm_ray_mesh: empty mesh (F == %d, Vm == %d)", F, Vm); return GM_ERR_INVALID_ARG; }
  if (!origins || !dirs || !vertices || !faces || !out_t || !out_face || !workspace) { set_error("gm_ray_mesh: null pointer"); return GM_ERR_INVALID_ARG; }
  if (ray_mesh_blocks(R, F) > 0x7FFFFFFFull) {
    set_error("gm_ray_mesh: R x F too large for one launch (%llu workgroups); split the rays", ray_mesh_blocks(R, F)); return GM_ERR_INVALID_ARG;
  }
  const size_t need = gm_ray_mesh_workspace_bytes(R, F);
  if (workspace_bytes < need) { set_error("gm_ray_mesh: workspace too small (%zu < %zu)", workspace_bytes, need); return GM_ERR_BUFFER; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  RcWs k = RcWs::from(workspace, (size_t)R, (size_t)F);
  const int ray_blocks = rc_div_up(R, 256);
  hipLaunchKernelGGL(rc_prepare, dim3(rc_div_up(R > F ? R : F, 256)), dim3(256), 0, s, F, Vm, vertices, faces, k.recs, R, k.slots);
  hipLaunchKernelGGL(rc_cast, dim3((unsigned)ray_mesh_blocks(R, F)), dim3(256), 0, s, R, origins, dirs, F, k.recs, ray_blocks, t_min, t_max, k.slots);
  hipLaunchKernelGGL(rc_finish, dim3(ray_blocks), dim3(256), 0, s, R, origins, dirs, k.recs, k.slots, t_min, t_max, out_t, out_face, out_uv);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // extern "C"
