// gm_winding.hip -- the generalized winding number of a triangle mesh at every point of a set (gm_mesh_winding), and the signed
// distance composed from it and gm_closest_face (gm_mesh_signed_distance): the operator behind mesh_sdf.winding_numbers / inside /
// signed_distances / grid_values and dynamics.SdfGrid.from_mesh, which lets a simulated mesh collide with another mesh.
// Jacobson, Kavan & Sorkine-Hornung 2013: the sum of the faces' signed solid angles over 4 pi is 1 inside a closed mesh, 0 outside, and
// degrades gracefully where the mesh is open, non-manifold or self-intersecting - which a pseudonormal or a ray parity does not.
//
// THE RESULT IS DEFINED BY ARITHMETIC (the contract gm_closest_face and gm_ray_mesh have):
//   per (point p, face f = (v0, v1, v2)): the seven float32 triples are widened to float64 and EVERY operation after that is float64,
//   no contraction (file pragma), dot(x, y) = (x.x*y.x + x.y*y.y) + x.z*y.z, (x cross y).x = x.y*y.z - x.z*y.y and so on
//   (Van Oosterom & Strackee 1983):
//     a = v0 - p, b = v1 - p, c = v2 - p;  la = sqrt(dot(a, a)), lb = sqrt(dot(b, b)), lc = sqrt(dot(c, c))
//     det = dot(a, b cross c)
//     den = ((la*lb*lc + dot(a, b)*lc) + dot(b, c)*la) + dot(c, a)*lb           (la*lb*lc = (la*lb)*lc)
//     omega_f = 2 atan2(det, den)
//   atan2(+-0, +0) = +-0 (den is a sum that starts from a product of lengths: it is never -0), so a point on a vertex of the face
//   (a zero length: det = den = 0) and a face with two equal corners (b cross c = 0 exactly, den >= 0) contribute nothing.
//   ORDER OF SUMMATION, part of the definition: the faces in chunks of WN_CHUNK = 1024, chunk k = faces [1024 k, min(F, 1024 (k + 1)));
//     S_k = (((0.0 + omega_f0) + omega_f1) + ...) in face order,   T = (((0.0 + S_0) + S_1) + ...) in chunk order,   w = T / (4 pi)
//   with 4 pi = 4 * 0x1.921fb54442d18p+1 and a correctly rounded division.  The chunking depends on F alone - not on N, on how the
//   caller batches its points, or on the device: a point's w has the same bits in every run.  No float atomics anywhere.
//   sqrt and the division are correctly rounded; atan2 is the device library's double atan2 (about 1 ulp), which is why a host
//   restatement agrees to a few 1e-16 per face and not bit for bit.
//
// gm_mesh_signed_distance: (d2, face, closest) = gm_closest_face's, w as above, and per point
//     phi = NaN                 if w is NaN or face == -1 (no face could claim the point)
//     phi = +0                  if d2 == 0
//     phi = s * sqrtf(d2)       otherwise, s = -1 iff fabs(w) > 0.5, else +1; the float32 square root correctly rounded.
//   fabs: a mesh wound inwards (w = -1 inside) is solid inside all the same.
//
// Structure (rc_prepare / rc_cast / rc_finish of gm_raycast.hip): wn_prepare writes one 48-byte record per face, the nine raw float32
// corner coordinates in face order.  wn_accumulate runs on a grid of point blocks x face chunks (flattened: consecutive workgroups
// share a chunk, so its 48 KiB of records stay in L2), one lane per point; the face loop is wave-uniform, the records come by
// uniform-address loads (scalar loads: no vector memory traffic in the loop) and are widened in the loop; a lane writes its chunk's
// S_k as one double into partial[k][point].  wn_finish, one thread per point, adds the partials in chunk order.
//
// Conventions of gm_closest_face: caller workspace, stream-ordered, no device allocation, no host wait anywhere in this file.
#include "gm_common.h"
#include "gm_check.h"
#pragma clang fp contract(off)   // every product and sum rounds on its own, as the definition above says

namespace gm {

#define WN_CHUNK 1024    // faces per partial sum: part of the definition of w
#define WN_FOUR_PI (4.0 * 0x1.921fb54442d18p+1)

struct WnWs {
  float4* recs;          // [F][3] v0x v0y v0z v1x | v1y v1z v2x v2y | v2z 0 0 0, in face order
  double* partial;       // [chunks][N]
  char* end;
  static WnWs from(void* ws, size_t N, size_t F) {
    char* p = reinterpret_cast<char*>(ws);
    WnWs k;
    k.recs = carve<float4>(p, 3 * F);
    k.partial = carve<double>(p, N * ((F + WN_CHUNK - 1) / WN_CHUNK));
    k.end = p;
    return k;
  }
};

// gm_mesh_signed_distance: gm_closest_face's workspace, the winding chain's, and the intermediates the caller did not ask for
struct SdWs {
  char* closest;
  char* winding;
  float* d2;             // [N]
  int* face;             // [N]
  double* w;             // [N]
  char* end;
  static SdWs from(void* ws, size_t N, size_t F, size_t closest_bytes, size_t winding_bytes) {
    char* p = reinterpret_cast<char*>(ws);
    SdWs k;
    k.closest = carve<char>(p, closest_bytes);
    k.winding = carve<char>(p, winding_bytes);
    k.d2 = carve<float>(p, N);
    k.face = carve<int>(p, N);
    k.w = carve<double>(p, N);
    k.end = p;
    return k;
  }
};

static inline int wn_div_up(int n, int d) { return n > 0 ? (n - 1) / d + 1 : 0; }      // (no overflow near INT_MAX)

// workgroups of wn_accumulate; more than a grid holds is refused by the entry points
static inline unsigned long long winding_blocks(int N, int F) { return (unsigned long long)wn_div_up(N, 256) * (unsigned long long)wn_div_up(F, WN_CHUNK); }

__global__ __launch_bounds__(256) void wn_prepare(int F, int Vm, const float* __restrict__ verts, const int* __restrict__ faces,
                                                  float4* __restrict__ recs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= F) return;
  const size_t ia = face_vertex(faces, 3 * (size_t)i, Vm), ib = face_vertex(faces, 3 * (size_t)i + 1, Vm), ic = face_vertex(faces, 3 * (size_t)i + 2, Vm);
  recs[3 * (size_t)i] = make_float4(verts[3 * ia], verts[3 * ia + 1], verts[3 * ia + 2], verts[3 * ib]);
  recs[3 * (size_t)i + 1] = make_float4(verts[3 * ib + 1], verts[3 * ib + 2], verts[3 * ic], verts[3 * ic + 1]);
  recs[3 * (size_t)i + 2] = make_float4(verts[3 * ic + 2], 0.f, 0.f, 0.f);
}

// the definition at the top of this file, line by line
__device__ __forceinline__ double wn_dot(double xx, double xy, double xz, double yx, double yy, double yz) { return (xx * yx + xy * yy) + xz * yz; }
__device__ __forceinline__ double wn_omega(double px, double py, double pz, const float4 r0, const float4 r1, const float4 r2) {
  const double ax = (double)r0.x - px, ay = (double)r0.y - py, az = (double)r0.z - pz;
  const double bx = (double)r0.w - px, by = (double)r1.x - py, bz = (double)r1.y - pz;
  const double cx = (double)r1.z - px, cy = (double)r1.w - py, cz = (double)r2.x - pz;
  const double la = sqrt(wn_dot(ax, ay, az, ax, ay, az)), lb = sqrt(wn_dot(bx, by, bz, bx, by, bz)), lc = sqrt(wn_dot(cx, cy, cz, cx, cy, cz));
  const double nx = by * cz - bz * cy, ny = bz * cx - bx * cz, nz = bx * cy - by * cx;
  const double det = wn_dot(ax, ay, az, nx, ny, nz);
  const double den = (((la * lb) * lc + wn_dot(ax, ay, az, bx, by, bz) * lc) + wn_dot(bx, by, bz, cx, cy, cz) * la) + wn_dot(cx, cy, cz, ax, ay, az) * lb;
  return 2.0 * atan2(det, den);
}

// workgroup g: point block g % point_blocks, face chunk g / point_blocks; one lane per point, the face loop wave-uniform
__global__ __launch_bounds__(256) void wn_accumulate(int N, const float* __restrict__ points, int F, const float4* __restrict__ recs, int point_blocks,
                                                     double* __restrict__ partial) {
  const int pb = blockIdx.x % point_blocks, chunk = blockIdx.x / point_blocks;
  const int i = pb * 256 + threadIdx.x;
  if (i - (int)(threadIdx.x & 63) >= N) return;    // a whole wave past the end
  const bool live = i < N;
  const size_t r = (size_t)(live ? i : N - 1);     // a lane past the end repeats the last point and stores nothing
  const double px = (double)points[3 * r], py = (double)points[3 * r + 1], pz = (double)points[3 * r + 2];
  const int f0 = chunk * WN_CHUNK, f1 = f0 + min(F - f0, WN_CHUNK);
  double sum = 0.0;
#pragma unroll 2
  for (int f = f0; f < f1; f++) sum += wn_omega(px, py, pz, recs[3 * (size_t)f], recs[3 * (size_t)f + 1], recs[3 * (size_t)f + 2]);
  if (live) partial[(size_t)chunk * (size_t)N + r] = sum;
}

__global__ __launch_bounds__(256) void wn_finish(int N, int chunks, const double* __restrict__ partial, double* __restrict__ out_w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double total = 0.0;
  for (int k = 0; k < chunks; k++) total += partial[(size_t)k * (size_t)N + (size_t)i];
  out_w[i] = total / WN_FOUR_PI;
}

// phi of the header comment
__global__ __launch_bounds__(256) void sd_finish(int N, const float* __restrict__ d2, const int* __restrict__ face, const double* __restrict__ w,
                                                 float* __restrict__ out_phi) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const double wi = w[i];
  const float d = d2[i];
  float phi;
  if (wi != wi || face[i] < 0) phi = __uint_as_float(0x7FC00000u);
  else if (d == 0.f) phi = 0.f;
  else phi = fabs(wi) > 0.5 ? -sqrtf(d) : sqrtf(d);       // (sqrtf: correctly rounded; the __fsqrt_rn intrinsic is the 1-ulp native root here)
  out_phi[i] = phi;
}

// what both entry points refuse about the sizes, the mesh and the launch; 1: N == 0, nothing to do
static int wn_check_sizes(const char* fn, int N, int Vm, int F, int* rc) {
  *rc = GM_OK;
  if (N < 0 || Vm < 0 || F < 0) { set_error("%s: negative size N=%d Vm=%d F=%d", fn, N, Vm, F); *rc = GM_ERR_INVALID_ARG; return 1; }
  if (N == 0) return 1;
  if (F == 0 || Vm == 0) { set_error("%s: empty mesh (F == %d, Vm == %d)", fn, F, Vm); *rc = GM_ERR_INVALID_ARG; return 1; }
  if (winding_blocks(N, F) > 0x7FFFFFFFull) {
    set_error("%s: N x F too large for one launch (%llu workgroups); split the points", fn, winding_blocks(N, F)); *rc = GM_ERR_INVALID_ARG; return 1;
  }
  return 0;
}

// the three launches; everything was checked
static int wn_launch(int N, const float* points, int Vm, const float* vertices, int F, const int* faces, double* out_w, void* workspace, hipStream_t s) {
  WnWs k = WnWs::from(workspace, (size_t)N, (size_t)F);
  const int point_blocks = wn_div_up(N, 256), chunks = wn_div_up(F, WN_CHUNK);
  hipLaunchKernelGGL(wn_prepare, dim3(wn_div_up(F, 256)), dim3(256), 0, s, F, Vm, vertices, faces, k.recs);
  hipLaunchKernelGGL(wn_accumulate, dim3((unsigned)winding_blocks(N, F)), dim3(256), 0, s, N, points, F, k.recs, point_blocks, k.partial);
  hipLaunchKernelGGL(wn_finish, dim3(point_blocks), dim3(256), 0, s, N, chunks, k.partial, out_w);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // namespace gm

// ---------------------------------------------------------------------------------------------
// the entry points (include/gmesh_hip.h): their refusals, then the launches
using namespace gm;

extern "C" {

size_t gm_mesh_winding_workspace_bytes(int N, int F) {
  WnWs k = WnWs::from(nullptr, (size_t)(N > 0 ? N : 1), (size_t)(F > 0 ? F : 1));
  return (size_t)k.end + 256;
}

int gm_mesh_winding(int N, const float* points, int Vm, const float* vertices, int F, const int* faces, double* out_w, void* workspace,
                    size_t workspace_bytes, void* stream) {
  const char* fn = "gm_mesh_winding";
  int rc;
  if (wn_check_sizes(fn, N, Vm, F, &rc)) return rc;
  if (!points || !vertices || !faces || !out_w || !workspace) { set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG; }
  const size_t need = gm_mesh_winding_workspace_bytes(N, F);
  if (workspace_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need); return GM_ERR_INVALID_ARG; }
  const ByteRange rg[] = {{out_w, (size_t)N * 8, "out_w", true}, {workspace, need, "workspace", true}, {points, (size_t)N * 12, "points", false},
                          {vertices, (size_t)Vm * 12, "vertices", false}, {faces, (size_t)F * 12, "faces", false}};
  if (int bad = check_ranges(fn, rg)) return bad;
  return wn_launch(N, points, Vm, vertices, F, faces, out_w, workspace, reinterpret_cast<hipStream_t>(stream));
}

size_t gm_mesh_signed_distance_workspace_bytes(int N, int F) {
  const size_t n = (size_t)(N > 0 ? N : 1), f = (size_t)(F > 0 ? F : 1);
  SdWs k = SdWs::from(nullptr, n, f, gm_closest_face_workspace_bytes(N, F), gm_mesh_winding_workspace_bytes(N, F));
  return (size_t)k.end + 256;
}

int gm_mesh_signed_distance(int N, const float* points, int Vm, const float* vertices, int F, const int* faces, float* out_phi, int* out_face,
                            float* out_closest, double* out_w, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "gm_mesh_signed_distance";
  int rc;
  if (wn_check_sizes(fn, N, Vm, F, &rc)) return rc;
  if (!points || !vertices || !faces || !out_phi || !workspace) { set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG; }
  const size_t need = gm_mesh_signed_distance_workspace_bytes(N, F);
  if (workspace_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need); return GM_ERR_INVALID_ARG; }
  const ByteRange rg[] = {{out_phi, (size_t)N * 4, "out_phi", true}, {out_face, (size_t)N * 4, "out_face", true},
                          {out_closest, (size_t)N * 12, "out_closest", true}, {out_w, (size_t)N * 8, "out_w", true},
                          {workspace, need, "workspace", true}, {points, (size_t)N * 12, "points", false},
                          {vertices, (size_t)Vm * 12, "vertices", false}, {faces, (size_t)F * 12, "faces", false}};
  if (int bad = check_ranges(fn, rg)) return bad;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t closest_bytes = gm_closest_face_workspace_bytes(N, F), winding_bytes = gm_mesh_winding_workspace_bytes(N, F);
  SdWs k = SdWs::from(workspace, (size_t)N, (size_t)F, closest_bytes, winding_bytes);
  int* face = out_face ? out_face : k.face;
  double* w = out_w ? out_w : k.w;
  if (int bad = gm_closest_face(N, points, Vm, vertices, F, faces, k.d2, face, out_closest, k.closest, closest_bytes, stream)) return bad;
  if (int bad = wn_launch(N, points, Vm, vertices, F, faces, w, k.winding, s)) return bad;
  hipLaunchKernelGGL(sd_finish, dim3(wn_div_up(N, 256)), dim3(256), 0, s, N, k.d2, face, w, out_phi);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // extern "C"
