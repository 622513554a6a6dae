// gm_mesh_color.hip -- colour on the proxy mesh: gm_mesh_vertex_normals gives every vertex its area-weighted normal, gm_mesh_color_integrate
// fuses the views' own renders (colour, depth and opacity maps of the rasterizer, return_aux) into one colour per vertex, weighted by the
// squared cosine of the viewing angle and gated by the depth map (what the view does not see adds nothing), gm_mesh_color_spread gives the
// vertices no view coloured a value from their neighbours.  The stage behind mesh_color.VertexColors / color_from_cloud and
// proxy_mesh.from_cloud(vertex_colors=True); gm_tsdf.hip's per-view rule for voxels is the rule for vertices here.
//
// THE RESULT IS DEFINED BY ARITHMETIC, as everything around gm_tsdf.hip is: float32, no contraction (file pragma), correctly rounded
// division, the order of operations as written here; tests/mesh_color_ref.py restates all three in numpy, bit for bit.
//
// gm_mesh_vertex_normals, per vertex i over the CSR of deform.vertex_face_adjacency, N = 0, then for j = adj_offsets[i] .. adj_offsets[i + 1] - 1
// in this order, f = adj_faces[j], (a, b, c) = faces[f]:
//     e1 = V[b] - V[a], e2 = V[c] - V[a] per component
//     cr = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z, e1.x e2.y - e1.y e2.x)         each product rounds, then the difference
//     N = N + cr
//   Unnormalised: its length is twice the area around the vertex.  A vertex without faces gets (0, 0, 0).
//
// gm_mesh_color_integrate, per vertex P with normal N and per view k = 0 .. K-1 in this order (v = the view's world_view_transform, stored
// transposed: v[4 r + c]; (tx, ty) its tan(FoV/2) pair; csum[3], wsum the vertex's running sums):
//     1. xv = ((P.x v[0] + P.y v[4]) + P.z v[8]) + v[12], yv with v[1 + ..], zv with v[2 + ..]; not (zv > 0): skip the view
//     2. px = ((xv / (zv tx) + 1) W - 1) 0.5, py = ((yv / (zv ty) + 1) H - 1) 0.5, fx = floor(px + 0.5), fy = floor(py + 0.5)     (ts_integrate's)
//        not (0 <= fx < W and 0 <= fy < H): skip
//     3. a = alpha[k, fy, fx]; not (a >= alpha_min): skip
//     4. s = depth[k, fy, fx] / a - zv; not (s >= -depth_tol and s <= depth_tol): skip (something else is in front, or the vertex is off
//        the rendered surface)
//     5. nv.x = (N.x v[0] + N.y v[4]) + N.z v[8], nv.y with v[1], v[5], v[9], nv.z with v[2], v[6], v[10]
//     6. d = (nv.x xv + nv.y yv) + nv.z zv; unless two_sided: not (d < 0): skip (the vertex faces away)
//     7. nn = (nv.x nv.x + nv.y nv.y) + nv.z nv.z, pp = (xv xv + yv yv) + zv zv, wgt = (d d) / (nn pp): the squared cosine of the viewing
//        angle, no square root; not (wgt > 0): skip (a zero normal: 0 / 0 is NaN)
//     8. c[ch] = image[k, ch, fy, fx], ch = 0, 1, 2; any c[ch] - c[ch] != 0 (NaN, inf): skip
//     9. csum[ch] = csum[ch] + wgt c[ch], wsum = wsum + wgt
//   Every comparison is false on NaN, so a NaN anywhere skips the view.  The sums are state: K views in one call are K calls of one.
//   One thread per vertex, the view loop inside: the sums are read once and written once per call, the camera rows are uniform-address
//   loads (scalar registers).
//
// gm_mesh_color_spread, state (colour, has) per vertex, has_0 = seen (non-zero), colour_0 = the caller's colours where seen, +0 elsewhere.
// Step t = 0 .. iterations-1, a Jacobi step that reads only (colour_t, has_t), per vertex i:
//     seen: both carry over.  Otherwise sum = (0, 0, 0), n = 0; over j in adjacency order, f = adj_faces[j], and within the face its corners
//     q = 0, 1, 2, u = faces[f][q]: u != i and has_t[u]: sum = sum + colour_t[u] per channel, n++ (a neighbour across an interior edge
//     counts once per shared face)
//     n > 0: colour_{t+1}[i] = sum / (float)n per channel, has_{t+1}[i] = 1; otherwise both carry over
//   After the last step: colours = has ? colour : fallback, out_has = has, out_counts = {filled (has and not seen), unreached (not has)}.
//   A filled vertex is averaged again in every later step.  iterations is a REACH, not a convergence claim: after n steps exactly the
//   vertices within n edges of a seen one have a value; iterations == 0 returns the seen colours and the fallback elsewhere.
//
// One launch per step between two (colour, has) pairs - the caller's colours with out_has, and a second pair in the workspace -, the scheme of
// gm_tsdf_fill.hip: a step never reads what it writes, and no workgroup waits for another.  Both pairs start as (colour_0, has_0); a vertex a
// step does not update is seen or still without a value, and both pairs already hold what carries over (has only ever rises, so a vertex
// that got a value gets one in every later step).  The pair the first step reads is chosen by the parity of iterations: the last step writes
// the caller's.  The counts are per-workgroup integer sums in the workspace, added up by one workgroup: no atomics anywhere in this file.
// Vertex ids read from faces, face ids and offsets read from the CSR are forced into range: no fault, no meaning.
// Conventions of gm_tsdf.hip: caller workspace, stream-ordered, no device allocation, no host wait anywhere in this file.
#include "gm_common.h"
#include "gm_check.h"
#include "gm_wave.h"
#pragma clang fp contract(off)   // every product, sum and quotient rounds on its own, as the definition above says

namespace gm {

struct McMesh {
  int Vm, F;
  const int* __restrict__ faces;
  const int* __restrict__ off;
  const int* __restrict__ adj;
  __device__ __forceinline__ void range(int v, int& b, int& e) const {
    const int nnz = 3 * F;
    b = off[v]; e = off[v + 1];
    b = b < 0 ? 0 : (b > nnz ? nnz : b);
    e = e < b ? b : (e > nnz ? nnz : e);
  }
  __device__ __forceinline__ void face(int s, int id[3]) const {
    const size_t f = (size_t)clamp_index(adj[s], F);
    id[0] = clamp_index(faces[3 * f], Vm); id[1] = clamp_index(faces[3 * f + 1], Vm); id[2] = clamp_index(faces[3 * f + 2], Vm);
  }
};

__global__ __launch_bounds__(256) void mc_normals(McMesh m, const float* __restrict__ V, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m.Vm) return;
  int b = 0, e = 0;
  if (m.F > 0) m.range(i, b, e);
  float nx = 0.f, ny = 0.f, nz = 0.f;
  for (int s = b; s < e; s++) {
    int id[3];
    m.face(s, id);
    const float* pa = V + 3 * (size_t)id[0];
    const float* pb = V + 3 * (size_t)id[1];
    const float* pc = V + 3 * (size_t)id[2];
    const float ax = pa[0], ay = pa[1], az = pa[2];
    const float e1x = pb[0] - ax, e1y = pb[1] - ay, e1z = pb[2] - az;
    const float e2x = pc[0] - ax, e2y = pc[1] - ay, e2z = pc[2] - az;
    nx = nx + (e1y * e2z - e1z * e2y);
    ny = ny + (e1z * e2x - e1x * e2z);
    nz = nz + (e1x * e2y - e1y * e2x);
  }
  out[3 * (size_t)i] = nx; out[3 * (size_t)i + 1] = ny; out[3 * (size_t)i + 2] = nz;
}

__global__ __launch_bounds__(256) void mc_integrate(int K, int H, int W, const float* __restrict__ image, const float* __restrict__ depth,
                                                    const float* __restrict__ alpha, const float* __restrict__ views,
                                                    const float* __restrict__ tans, int Vm, const float* __restrict__ vertices,
                                                    const float* __restrict__ normals, float alpha_min, float depth_tol, int two_sided,
                                                    float* __restrict__ csum, float* __restrict__ wsum) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Vm) return;
  const float X = vertices[3 * (size_t)i], Y = vertices[3 * (size_t)i + 1], Z = vertices[3 * (size_t)i + 2];
  const float NX = normals[3 * (size_t)i], NY = normals[3 * (size_t)i + 1], NZ = normals[3 * (size_t)i + 2];
  const float fW = (float)W, fH = (float)H, neg_tol = -depth_tol;
  const size_t plane = (size_t)H * W;
  float c0 = csum[3 * (size_t)i], c1 = csum[3 * (size_t)i + 1], c2 = csum[3 * (size_t)i + 2], w = wsum[i];
  for (int k = 0; k < K; k++) {
    const float* v = views + 16 * (size_t)k;           // wave-uniform addresses: the rows live in scalar registers
    const float tx = tans[2 * (size_t)k], ty = tans[2 * (size_t)k + 1];
    const float xv = ((X * v[0] + Y * v[4]) + Z * v[8]) + v[12];
    const float yv = ((X * v[1] + Y * v[5]) + Z * v[9]) + v[13];
    const float zv = ((X * v[2] + Y * v[6]) + Z * v[10]) + v[14];
    if (!(zv > 0.f)) continue;
    const float px = ((xv / (zv * tx) + 1.0f) * fW - 1.0f) * 0.5f, py = ((yv / (zv * ty) + 1.0f) * fH - 1.0f) * 0.5f;
    const float fx = floorf(px + 0.5f), fy = floorf(py + 0.5f);
    if (!(fx >= 0.f && fx < fW && fy >= 0.f && fy < fH)) continue;
    const size_t at = (size_t)(int)fy * W + (size_t)(int)fx;
    const size_t pix = (size_t)k * plane + at;
    const float a = alpha[pix];
    if (!(a >= alpha_min)) continue;
    const float s = depth[pix] / a - zv;
    if (!(s >= neg_tol && s <= depth_tol)) continue;
    const float nvx = (NX * v[0] + NY * v[4]) + NZ * v[8];
    const float nvy = (NX * v[1] + NY * v[5]) + NZ * v[9];
    const float nvz = (NX * v[2] + NY * v[6]) + NZ * v[10];
    const float d = (nvx * xv + nvy * yv) + nvz * zv;
    if (!two_sided && !(d < 0.f)) continue;
    const float nn = (nvx * nvx + nvy * nvy) + nvz * nvz;
    const float pp = (xv * xv + yv * yv) + zv * zv;
    const float wgt = (d * d) / (nn * pp);
    if (!(wgt > 0.f)) continue;
    const float* img = image + 3 * (size_t)k * plane + at;
    const float r = img[0], g = img[plane], b = img[2 * plane];
    if (!(r - r == 0.f && g - g == 0.f && b - b == 0.f)) continue;
    c0 = c0 + wgt * r;
    c1 = c1 + wgt * g;
    c2 = c2 + wgt * b;
    w = w + wgt;
  }
  csum[3 * (size_t)i] = c0; csum[3 * (size_t)i + 1] = c1; csum[3 * (size_t)i + 2] = c2;
  wsum[i] = w;
}

// ---- spread ----
struct McWs {
  float* col;              // [Vm,3] the second colour array (the first is the caller's)
  uint8_t* has;            // [Vm] the second state array (the first is out_has)
  uint2* sums;             // [workgroups] (filled, unreached) of each workgroup of the last pass
  char* end;
  static McWs from(void* ws, size_t Vm) {
    char* p = reinterpret_cast<char*>(ws);
    McWs k;
    k.col = carve<float>(p, 3 * Vm);
    k.has = carve<uint8_t>(p, Vm);
    k.sums = carve<uint2>(p, (Vm + 255) / 256);
    k.end = p;
    return k;
  }
};

// (colour_0, has_0) into both pairs
__global__ __launch_bounds__(256) void mc_spread_init(int Vm, const uint8_t* __restrict__ seen, float* __restrict__ col0, float* __restrict__ col1,
                                                      uint8_t* __restrict__ has0, uint8_t* __restrict__ has1) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Vm) return;
  const bool sn = seen[i] != 0;
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    const float c = sn ? col0[3 * (size_t)i + ch] : 0.0f;
    col0[3 * (size_t)i + ch] = c; col1[3 * (size_t)i + ch] = c;
  }
  has0[i] = sn ? 1 : 0; has1[i] = sn ? 1 : 0;
}

__global__ __launch_bounds__(256) void mc_spread_step(McMesh m, const uint8_t* __restrict__ seen, const float* __restrict__ col_in,
                                                      const uint8_t* __restrict__ has_in, float* __restrict__ col_out,
                                                      uint8_t* __restrict__ has_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m.Vm) return;
  if (seen[i]) return;
  int b, e;
  m.range(i, b, e);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  int n = 0;
  for (int s = b; s < e; s++) {
    int id[3];
    m.face(s, id);
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const int u = id[q];
      if (u != i && has_in[u]) {
        s0 = s0 + col_in[3 * (size_t)u]; s1 = s1 + col_in[3 * (size_t)u + 1]; s2 = s2 + col_in[3 * (size_t)u + 2];
        n++;
      }
    }
  }
  if (n > 0) {
    const float fn = (float)n;
    col_out[3 * (size_t)i] = s0 / fn; col_out[3 * (size_t)i + 1] = s1 / fn; col_out[3 * (size_t)i + 2] = s2 / fn;
    has_out[i] = 1;
  }
}

// the fallback where nothing arrived, and the workgroup's share of the counts
__global__ __launch_bounds__(256) void mc_spread_finish(int Vm, const uint8_t* __restrict__ seen, const uint8_t* __restrict__ has, float f0, float f1,
                                                        float f2, float* __restrict__ col, uint2* __restrict__ sums) {
  __shared__ uint32_t lds[4][2];
  const int i = blockIdx.x * 256 + threadIdx.x;
  uint32_t filled = 0, unreached = 0;
  if (i < Vm) {
    if (has[i]) {
      filled = seen[i] ? 0u : 1u;
    } else {
      unreached = 1u;
      col[3 * (size_t)i] = f0; col[3 * (size_t)i + 1] = f1; col[3 * (size_t)i + 2] = f2;
    }
  }
  filled = wave_sum_u32(filled);
  unreached = wave_sum_u32(unreached);
  if ((threadIdx.x & 63) == 0) { lds[threadIdx.x >> 6][0] = filled; lds[threadIdx.x >> 6][1] = unreached; }
  __syncthreads();
  if (threadIdx.x == 0)
    sums[blockIdx.x] = make_uint2((lds[0][0] + lds[1][0]) + (lds[2][0] + lds[3][0]), (lds[0][1] + lds[1][1]) + (lds[2][1] + lds[3][1]));
}

// one workgroup adds the per-workgroup sums up (integers: any order gives the same counts)
__global__ __launch_bounds__(256) void mc_spread_counts(int blocks, const uint2* __restrict__ sums, int* __restrict__ counts) {
  __shared__ uint32_t lds[4][2];
  uint32_t filled = 0, unreached = 0;
  for (int j = threadIdx.x; j < blocks; j += 256) { const uint2 v = sums[j]; filled += v.x; unreached += v.y; }
  filled = wave_sum_u32(filled);
  unreached = wave_sum_u32(unreached);
  if ((threadIdx.x & 63) == 0) { lds[threadIdx.x >> 6][0] = filled; lds[threadIdx.x >> 6][1] = unreached; }
  __syncthreads();
  if (threadIdx.x == 0) {
    counts[0] = (int)((lds[0][0] + lds[1][0]) + (lds[2][0] + lds[3][0]));
    counts[1] = (int)((lds[0][1] + lds[1][1]) + (lds[2][1] + lds[3][1]));
  }
}

}  // namespace gm

// ---------------------------------------------------------------------------------------------
// the entry points (include/gmesh_hip.h): their refusals, then the launches
using namespace gm;

// the mesh rules the three calls share: sizes that 3 Vm and 3 F index with an int
static int check_color_mesh(const char* fn, int Vm, int F) {
  if (Vm < 0 || F < 0) { set_error("%s: negative size Vm=%d F=%d", fn, Vm, F); return GM_ERR_INVALID_ARG; }
  if (Vm > 0x7FFFFFFF / 3 || F > 0x7FFFFFFF / 3) { set_error("%s: Vm=%d F=%d: 3 Vm and 3 F must fit an int", fn, Vm, F); return GM_ERR_INVALID_ARG; }
  return GM_OK;
}

extern "C" {

int gm_mesh_vertex_normals(int Vm, int F, const float* vertices, const int* faces, const int* adj_offsets, const int* adj_faces, float* out_normals,
                           void* stream) {
  const char* fn = "gm_mesh_vertex_normals";
  if (int rc = check_color_mesh(fn, Vm, F)) return rc;
  if (Vm == 0) return GM_OK;
  if (!vertices || !out_normals || (F > 0 && (!faces || !adj_offsets || !adj_faces))) { set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG; }
  const ByteRange rg[5] = {{vertices, 12 * (size_t)Vm, "vertices", false}, {faces, 12 * (size_t)F, "faces", false},
                           {adj_offsets, 4 * ((size_t)Vm + 1), "adj_offsets", false}, {adj_faces, 12 * (size_t)F, "adj_faces", false},
                           {out_normals, 12 * (size_t)Vm, "out_normals", true}};
  if (int rc = check_ranges(fn, rg)) return rc;
  const McMesh m = {Vm, F, faces, adj_offsets, adj_faces};
  hipLaunchKernelGGL(mc_normals, dim3((unsigned)((Vm + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), m, vertices, out_normals);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_mesh_color_integrate(int K, int H, int W, const float* image, const float* depth, const float* alpha, const float* views, const float* tanfov,
                            int Vm, const float* vertices, const float* normals, float alpha_min, float depth_tol, int two_sided, float* csum,
                            float* wsum, void* stream) {
  const char* fn = "gm_mesh_color_integrate";
  if (K < 0 || H <= 0 || W <= 0 || H > (1 << 24) || W > (1 << 24)) { set_error("%s: invalid sizes K=%d H=%d W=%d", fn, K, H, W); return GM_ERR_INVALID_ARG; }
  if (int rc = check_color_mesh(fn, Vm, 0)) return rc;
  if (alpha_min != alpha_min || !(depth_tol >= 0.f)) { set_error("%s: alpha_min must not be NaN, depth_tol >= 0 and not NaN", fn); return GM_ERR_INVALID_ARG; }
  if (Vm == 0) return GM_OK;
  if (!vertices || !normals || !csum || !wsum) { set_error("%s: null pointer (vertices / normals / csum / wsum)", fn); return GM_ERR_INVALID_ARG; }
  if (K > 0 && (!image || !depth || !alpha || !views || !tanfov)) { set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG; }
  const size_t maps = 4 * (size_t)K * H * W;
  const ByteRange rg[9] = {{image, 3 * maps, "image", false}, {depth, maps, "depth", false}, {alpha, maps, "alpha", false},
                           {views, 64 * (size_t)K, "views", false}, {tanfov, 8 * (size_t)K, "tanfov", false}, {vertices, 12 * (size_t)Vm, "vertices", false},
                           {normals, 12 * (size_t)Vm, "normals", false}, {csum, 12 * (size_t)Vm, "csum", true}, {wsum, 4 * (size_t)Vm, "wsum", true}};
  if (int rc = check_ranges(fn, rg)) return rc;
  if (K == 0) return GM_OK;
  hipLaunchKernelGGL(mc_integrate, dim3((unsigned)((Vm + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), K, H, W, image, depth, alpha,
                     views, tanfov, Vm, vertices, normals, alpha_min, depth_tol, two_sided ? 1 : 0, csum, wsum);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

size_t gm_mesh_color_spread_workspace_bytes(int Vm) {
  const McWs k = McWs::from(nullptr, (size_t)(Vm > 0 ? Vm : 0));
  return (size_t)k.end + 256;    // (the caller's pointer may sit anywhere inside a 256-byte line)
}

int gm_mesh_color_spread(int Vm, int F, const int* faces, const int* adj_offsets, const int* adj_faces, const unsigned char* seen, int iterations,
                         const float* fallback, float* colors, unsigned char* out_has, int* out_counts, void* workspace, size_t workspace_bytes,
                         void* stream) {
  const char* fn = "gm_mesh_color_spread";
  if (int rc = check_color_mesh(fn, Vm, F)) return rc;
  if (iterations < 0) { set_error("%s: iterations = %d (negative)", fn, iterations); return GM_ERR_INVALID_ARG; }
  if (!fallback || !out_counts || !workspace || (Vm > 0 && (!seen || !colors || !out_has)) || (Vm > 0 && F > 0 && (!faces || !adj_offsets || !adj_faces))) {
    set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG;
  }
  const ByteRange rg[8] = {{faces, 12 * (size_t)F, "faces", false}, {adj_offsets, Vm > 0 ? 4 * ((size_t)Vm + 1) : 0, "adj_offsets", false},
                           {adj_faces, 12 * (size_t)F, "adj_faces", false}, {seen, (size_t)Vm, "seen", false}, {colors, 12 * (size_t)Vm, "colors", true},
                           {out_has, (size_t)Vm, "out_has", true}, {out_counts, 8, "out_counts", true}, {workspace, workspace_bytes, "workspace", true}};
  if (int rc = check_ranges(fn, rg)) return rc;
  const size_t need = gm_mesh_color_spread_workspace_bytes(Vm);
  if (workspace_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need); return GM_ERR_BUFFER; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 one(1), threads(256);
  if (Vm == 0) {
    hipLaunchKernelGGL(mc_spread_counts, one, threads, 0, s, 0, (const uint2*)nullptr, out_counts);
    GM_HIP(hipGetLastError());
    return GM_OK;
  }
  const McWs k = McWs::from(workspace, (size_t)Vm);
  const McMesh m = {Vm, F, faces, adj_offsets, adj_faces};
  const int nblocks = (Vm + 255) / 256;
  const dim3 blocks((unsigned)nblocks);
  float* col[2] = {colors, k.col};
  uint8_t* has[2] = {out_has, k.has};
  hipLaunchKernelGGL(mc_spread_init, blocks, threads, 0, s, Vm, seen, col[0], col[1], has[0], has[1]);
  if (F > 0) {
    int cur = iterations & 1;                    // the last step writes pair 0: the caller's
    for (int t = 0; t < iterations; t++, cur ^= 1)
      hipLaunchKernelGGL(mc_spread_step, blocks, threads, 0, s, m, seen, col[cur], has[cur], col[cur ^ 1], has[cur ^ 1]);
  }
  hipLaunchKernelGGL(mc_spread_finish, blocks, threads, 0, s, Vm, seen, has[0], fallback[0], fallback[1], fallback[2], col[0], k.sums);
  hipLaunchKernelGGL(mc_spread_counts, one, threads, 0, s, nblocks, k.sums, out_counts);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // extern "C"
