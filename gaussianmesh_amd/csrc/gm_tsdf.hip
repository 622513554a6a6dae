// gm_tsdf.hip -- from depth maps to a proxy mesh: gm_tsdf_integrate fuses the depth / opacity maps of K views into a truncated signed
// distance volume (Curless & Levoy 1996), gm_surface_nets pulls an indexed triangle mesh out of it (naive surface nets, Gibson 1998:
// one vertex per cell the surface crosses, one quad per grid edge it crosses).  The stage behind proxy_mesh.TsdfVolume / from_cloud.
//
// THE RESULT IS DEFINED BY ARITHMETIC (the contract gm_closest_face and gm_ray_mesh have): everything in float32, no contraction (file
// pragma), correctly rounded division, the order of operations as written here; tests/tsdf_ref.py restates both in numpy, bit for bit.
//
// gm_tsdf_integrate, per voxel (ix, iy, iz) and per view k = 0 .. K-1 in this order (v = the view's world_view_transform, stored
// transposed: v[4 r + c]; (tx, ty) its tan(FoV/2) pair; D, w the voxel's running value and weight):
//     p  = origin + ((float)i + 0.5f) * voxel                                   per axis: the voxel's CENTRE
//     xv = ((p.x v[0] + p.y v[4]) + p.z v[8]) + v[12], yv with v[1 + ..], zv with v[2 + ..]
//     not (zv > 0): skip the view
//     px = ((xv / (zv tx) + 1) W - 1) 0.5, py = ((yv / (zv ty) + 1) H - 1) 0.5      the rasterizer's rule (ndc2pix)
//     fx = floor(px + 0.5), fy = floor(py + 0.5); not (0 <= fx < W and 0 <= fy < H): skip
//     a = alpha[k, fy, fx]; not (a >= alpha_min): carve ? t = 1 (free space) : skip
//     else d = depth[k, fy, fx] / a, s = d - zv; not (s >= -trunc): skip (behind the surface: unobserved); q = s / trunc, t = q < 1 ? q : 1
//     w' = w + 1, D = (D w + t) / w', w = w'
//   Every comparison is false on NaN, so a NaN anywhere skips the view.  The volume is state: K views in one call are K calls of one.
//   One thread per voxel, x fastest, the view loop inside: D and w are read once and written once per call, the camera rows are
//   uniform-address loads (scalar registers), and the depth gathers of neighbouring voxels land on neighbouring pixels.
//
// gm_surface_nets, samples at the voxel centres, cell (cx, cy, cz) = the 8 samples (cx + dx, cy + dy, cz + dz), corner number dx + 2 dy + 4 dz:
//     active iff every corner has weight >= min_weight and the corners differ in `inside` (D < 0; an exact 0 and NaN are outside)
//     its vertex: over the 12 edges in the order x: (0,1) (2,3) (4,5) (6,7), y: (0,2) (1,3) (4,6) (5,7), z: (0,4) (1,5) (2,6) (3,7), for
//     every edge (a, b) whose ends differ in `inside`: t = D[a] / (D[a] - D[b]); sum += corner a's offset with t on the edge's own axis
//     (three running sums, starting at 0); m = sum / (float)count; position = origin + (((float)c + m) + 0.5f) * voxel per axis
//     vertex id = exclusive scan of the active flags over the cells in linear order (x fastest)
//   faces: per sample g = (ix, iy, iz) in linear order and axis a = x, y, z (u, v the next two axes cyclically), the grid edge g -> g + e_a
//     yields a quad iff its ends differ in `inside` and the four cells q0 = g - e_u - e_v, q1 = g - e_v, q2 = g, q3 = g - e_u exist and
//     are all active.  (q0, q1, q2, q3) winds around +a; inside(g): rows (q0, q1, q2), (q0, q2, q3), else (q0, q2, q1), (q0, q3, q2):
//     the normal points from negative to positive.  Rows 2 r, 2 r + 1 with r the exclusive scan of the quads over (g, a).
//   Rows at or beyond a capacity are not written (the rows below it are the full result's prefix); out_counts says what is needed.
//
// The scan is three plain passes - block sums (recursively, SN_BLOCK entries a block), scan of the sums, scatter - between kernel
// boundaries: deterministic, and no workgroup ever waits for another.
// Conventions of gm_closest_face: caller workspace, stream-ordered, no device allocation, no host wait anywhere in this file.
#include "gm_common.h"
#include "gm_check.h"
#include "gm_wave.h"
#pragma clang fp contract(off)   // every product and sum rounds on its own, as the definition above says

namespace gm {

#define SN_BLOCK 256     // entries per workgroup of every scan pass (tests/test_gpu_tsdf.py mirrors it)
#define SN_LEVELS 4

struct TsdfGrid { int nx, ny, nz; float ox, oy, oz, voxel; };

__global__ __launch_bounds__(256) void ts_integrate(int K, int H, int W, const float* __restrict__ depth, const float* __restrict__ alpha,
                                                    const float* __restrict__ views, const float* __restrict__ tans, TsdfGrid g, float trunc,
                                                    float alpha_min, int carve, float* __restrict__ tsdf, float* __restrict__ weight) {
  const size_t n = (size_t)g.nx * g.ny * g.nz;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int ix = (int)(i % g.nx), iy = (int)((i / g.nx) % g.ny), iz = (int)(i / ((size_t)g.nx * g.ny));
  const float X = g.ox + ((float)ix + 0.5f) * g.voxel, Y = g.oy + ((float)iy + 0.5f) * g.voxel, Z = g.oz + ((float)iz + 0.5f) * g.voxel;
  const float fW = (float)W, fH = (float)H, neg_trunc = -trunc;
  float D = tsdf[i], w = weight[i];
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
    const size_t pix = ((size_t)k * H + (size_t)(int)fy) * W + (size_t)(int)fx;
    const float a = alpha[pix];
    float t = 1.0f;
    if (!(a >= alpha_min)) {
      if (!carve) continue;
    } else {
      const float s = depth[pix] / a - zv;
      if (!(s >= neg_trunc)) continue;
      const float q = s / trunc;
      t = q < 1.0f ? q : 1.0f;
    }
    const float w1 = w + 1.0f;
    D = (D * w + t) / w1;
    w = w1;
  }
  tsdf[i] = D;
  weight[i] = w;
}

// ---- surface nets ----
struct SnWs {
  uint8_t* act;                  // [n] the cell whose lowest corner is sample g is active (0 where there is no such cell)
  uint8_t* flags;                // [n] bit 0: act, bits 1..3: the grid edge g -> g + e_x / e_y / e_z yields a quad
  int* vid;                      // [n] vertex id of that cell, -1 when it has none
  uint2* lvl[SN_LEVELS];         // (cells, quads) sums: lvl[0] per workgroup of samples, lvl[l + 1] per SN_BLOCK entries of lvl[l]
  size_t len[SN_LEVELS];
  int levels;
  char* end;
  static SnWs from(void* ws, size_t n) {
    char* p = reinterpret_cast<char*>(ws);
    SnWs k;
    k.act = carve<uint8_t>(p, n);
    k.flags = carve<uint8_t>(p, n);
    k.vid = carve<int>(p, n);
    size_t L = (n + SN_BLOCK - 1) / SN_BLOCK;
    k.levels = 0;
    for (;;) {
      k.lvl[k.levels] = carve<uint2>(p, L);
      k.len[k.levels] = L;
      k.levels++;
      if (L <= SN_BLOCK || k.levels == SN_LEVELS) break;    // (n <= 2^28: three levels at most)
      L = (L + SN_BLOCK - 1) / SN_BLOCK;
    }
    k.end = p;
    return k;
  }
};

static inline size_t sn_samples(int nx, int ny, int nz) { return (size_t)(nx > 2 ? nx : 2) * (size_t)(ny > 2 ? ny : 2) * (size_t)(nz > 2 ? nz : 2); }

// exclusive scan of one value per thread over the 256 threads of the workgroup (every thread calls it); total = the sum of all
__device__ __forceinline__ uint32_t sn_block_scan(uint32_t v, uint32_t* lds, uint32_t& total) {
  const uint32_t r = block_exclusive_scan<SN_BLOCK / 64>(v, lds, total);
  __syncthreads();               // the next call writes lds again
  return r;
}

struct SnDims {
  int n[3];
  __host__ __device__ size_t total() const { return (size_t)n[0] * n[1] * n[2]; }
  __device__ void split(size_t g, int i[3]) const { i[0] = (int)(g % n[0]); i[1] = (int)((g / n[0]) % n[1]); i[2] = (int)(g / ((size_t)n[0] * n[1])); }
  __device__ size_t stride(int a) const { return a == 0 ? 1 : (a == 1 ? (size_t)n[0] : (size_t)n[0] * n[1]); }
};

__global__ __launch_bounds__(256) void sn_cells(SnDims dm, const float* __restrict__ tsdf, const float* __restrict__ weight, float min_weight,
                                                uint8_t* __restrict__ act) {
  const size_t g = (size_t)blockIdx.x * SN_BLOCK + threadIdx.x;
  if (g >= dm.total()) return;
  int i[3];
  dm.split(g, i);
  uint8_t a = 0;
  if (i[0] + 1 < dm.n[0] && i[1] + 1 < dm.n[1] && i[2] + 1 < dm.n[2]) {
    bool ok = true;
    int neg = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const size_t j = g + (c & 1) + ((c >> 1) & 1) * dm.stride(1) + (c >> 2) * dm.stride(2);
      ok = ok && (weight[j] >= min_weight);
      neg += tsdf[j] < 0.f ? 1 : 0;
    }
    a = (ok && neg > 0 && neg < 8) ? 1 : 0;
  }
  act[g] = a;
}

__global__ __launch_bounds__(256) void sn_edges(SnDims dm, const float* __restrict__ tsdf, const uint8_t* __restrict__ act,
                                                uint8_t* __restrict__ flags, uint2* __restrict__ sums) {
  __shared__ uint32_t lds[4];
  const size_t g = (size_t)blockIdx.x * SN_BLOCK + threadIdx.x;
  uint32_t m = 0;
  if (g < dm.total()) {
    int i[3];
    dm.split(g, i);
    m = act[g];
    const bool in0 = tsdf[g] < 0.f;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const int u = (a + 1) % 3, v = (a + 2) % 3;
      if (i[a] + 1 < dm.n[a] && i[u] >= 1 && i[v] >= 1) {      // (a cell that would reach past the far side has act == 0)
        const size_t su = dm.stride(u), sv = dm.stride(v);
        const bool four = act[g - su - sv] && act[g - sv] && act[g] && act[g - su];
        if (four && in0 != (tsdf[g + dm.stride(a)] < 0.f)) m |= 2u << a;
      }
    }
    flags[g] = (uint8_t)m;
  }
  uint32_t cells, quads;
  sn_block_scan(m & 1u, lds, cells);
  sn_block_scan(__popc(m >> 1), lds, quads);
  if (threadIdx.x == 0) sums[blockIdx.x] = make_uint2(cells, quads);
}

__global__ __launch_bounds__(256) void sn_sums(const uint2* __restrict__ in, size_t len, uint2* __restrict__ out) {
  __shared__ uint32_t lds[4];
  const size_t j = (size_t)blockIdx.x * SN_BLOCK + threadIdx.x;
  const uint2 v = j < len ? in[j] : make_uint2(0u, 0u);
  uint32_t x, y;
  sn_block_scan(v.x, lds, x);
  sn_block_scan(v.y, lds, y);
  if (threadIdx.x == 0) out[blockIdx.x] = make_uint2(x, y);
}

// a[j] = exclusive scan inside the workgroup's SN_BLOCK entries + offsets[workgroup]; the top level (one workgroup, no offsets) also
// writes the totals: counts = {vertices, faces}
__global__ __launch_bounds__(256) void sn_scan_level(uint2* __restrict__ a, size_t len, const uint2* __restrict__ offsets, int* __restrict__ counts) {
  __shared__ uint32_t lds[4];
  const size_t j = (size_t)blockIdx.x * SN_BLOCK + threadIdx.x;
  const uint2 v = j < len ? a[j] : make_uint2(0u, 0u);
  uint32_t tx, ty;
  uint32_t x = sn_block_scan(v.x, lds, tx), y = sn_block_scan(v.y, lds, ty);
  if (offsets) { const uint2 o = offsets[blockIdx.x]; x += o.x; y += o.y; }
  if (j < len) a[j] = make_uint2(x, y);
  if (counts && threadIdx.x == 0) { counts[0] = (int)tx; counts[1] = (int)(2u * ty); }
}

__global__ __launch_bounds__(256) void sn_vertices(SnDims dm, const float* __restrict__ tsdf, const uint8_t* __restrict__ flags,
                                                   const uint2* __restrict__ sums, TsdfGrid gr, int max_vertices, int* __restrict__ vid,
                                                   float* __restrict__ out_vertices) {
  __shared__ uint32_t lds[4];
  const size_t g = (size_t)blockIdx.x * SN_BLOCK + threadIdx.x;
  const bool live = g < dm.total();
  const uint32_t a = live ? (flags[g] & 1u) : 0u;
  uint32_t total;
  const uint32_t r = sn_block_scan(a, lds, total) + sums[blockIdx.x].x;
  if (!live) return;
  vid[g] = a ? (int)r : -1;
  if (!a || r >= (uint32_t)max_vertices) return;
  int i[3];
  dm.split(g, i);
  float d[8];
#pragma unroll
  for (int c = 0; c < 8; c++) d[c] = tsdf[g + (c & 1) + ((c >> 1) & 1) * dm.stride(1) + (c >> 2) * dm.stride(2)];
  float s[3] = {0.f, 0.f, 0.f};
  int count = 0;
#pragma unroll
  for (int ax = 0; ax < 3; ax++) {
#pragma unroll
    for (int e = 0; e < 4; e++) {
      // the four edges along ax: corner a has offset 0 on ax and e's two bits on the other axes, in ascending corner order
      const int lo = (1 << ax) - 1;
      const int ca = (e & lo) | ((e & ~lo) << 1), cb = ca | (1 << ax);
      if ((d[ca] < 0.f) != (d[cb] < 0.f)) {
        const float t = d[ca] / (d[ca] - d[cb]);
#pragma unroll
        for (int k = 0; k < 3; k++) s[k] = s[k] + (k == ax ? t : (float)((ca >> k) & 1));
        count++;
      }
    }
  }
  const float fc = (float)count;
  const float org[3] = {gr.ox, gr.oy, gr.oz};
#pragma unroll
  for (int k = 0; k < 3; k++) out_vertices[3 * (size_t)r + k] = org[k] + (((float)i[k] + s[k] / fc) + 0.5f) * gr.voxel;
}

__global__ __launch_bounds__(256) void sn_faces(SnDims dm, const float* __restrict__ tsdf, const uint8_t* __restrict__ flags,
                                                const uint2* __restrict__ sums, const int* __restrict__ vid, int max_faces,
                                                int* __restrict__ out_faces) {
  __shared__ uint32_t lds[4];
  const size_t g = (size_t)blockIdx.x * SN_BLOCK + threadIdx.x;
  const bool live = g < dm.total();
  const uint32_t m = live ? (uint32_t)(flags[g] >> 1) : 0u;
  uint32_t total;
  uint32_t r = sn_block_scan(__popc(m), lds, total) + sums[blockIdx.x].y;
  if (!m) return;
  const bool in0 = tsdf[g] < 0.f;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (!(m & (1u << a))) continue;
    const size_t su = dm.stride((a + 1) % 3), sv = dm.stride((a + 2) % 3);
    const int q0 = vid[g - su - sv], q1 = vid[g - sv], q2 = vid[g], q3 = vid[g - su];
    const size_t row = 2 * (size_t)r;
    if (row < (size_t)max_faces) {
      int* f = out_faces + 3 * row;
      f[0] = q0; f[1] = in0 ? q1 : q2; f[2] = in0 ? q2 : q1;
    }
    if (row + 1 < (size_t)max_faces) {
      int* f = out_faces + 3 * (row + 1);
      f[0] = q0; f[1] = in0 ? q2 : q3; f[2] = in0 ? q3 : q2;
    }
    r++;
  }
}

}  // namespace gm

// ---------------------------------------------------------------------------------------------
// the entry points (include/gmesh_hip.h): their refusals, then the launches
using namespace gm;

extern "C" {

int gm_tsdf_integrate(int K, int H, int W, const float* depth, const float* alpha, const float* views, const float* tanfov, int nx, int ny, int nz,
                      const float* origin, float voxel, float trunc, float alpha_min, int carve, float* tsdf, float* weight, void* stream) {
  const char* fn = "gm_tsdf_integrate";
  if (K < 0 || H <= 0 || W <= 0 || H > (1 << 24) || W > (1 << 24)) { set_error("%s: invalid sizes K=%d H=%d W=%d", fn, K, H, W); return GM_ERR_INVALID_ARG; }
  if (int rc = check_tsdf_grid(fn, nx, ny, nz, 1, origin, voxel)) return rc;
  if (!(trunc > 0.f) || trunc > 3.4028234e38f || alpha_min != alpha_min) {
    set_error("%s: trunc must be positive and finite, alpha_min not NaN", fn); return GM_ERR_INVALID_ARG;
  }
  if (!tsdf || !weight) { set_error("%s: null pointer (tsdf / weight)", fn); return GM_ERR_INVALID_ARG; }
  // the volume against itself (also when there is nothing to integrate), then - once the maps are known to be there - against what is read
  const size_t n = (size_t)nx * ny * nz, maps = 4 * (size_t)K * H * W;
  const ByteRange rg[6] = {{tsdf, 4 * n, "tsdf", true}, {weight, 4 * n, "weight", true}, {depth, maps, "depth", false}, {alpha, maps, "alpha", false},
                           {views, 64 * (size_t)K, "views", false}, {tanfov, 8 * (size_t)K, "tanfov", false}};
  if (int rc = check_ranges(fn, rg, 2)) return rc;
  if (K == 0) return GM_OK;
  if (!depth || !alpha || !views || !tanfov) { set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG; }
  if (int rc = check_ranges(fn, rg)) return rc;
  const TsdfGrid g = {nx, ny, nz, origin[0], origin[1], origin[2], voxel};
  hipLaunchKernelGGL(ts_integrate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), K, H, W, depth, alpha, views,
                     tanfov, g, trunc, alpha_min, carve, tsdf, weight);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

size_t gm_surface_nets_workspace_bytes(int nx, int ny, int nz) {
  SnWs k = SnWs::from(nullptr, sn_samples(nx, ny, nz));
  return (size_t)k.end + 256;
}

int gm_surface_nets(int nx, int ny, int nz, const float* origin, float voxel, const float* tsdf, const float* weight, float min_weight,
                    int max_vertices, float* out_vertices, int max_faces, int* out_faces, int* out_counts, void* workspace, size_t workspace_bytes,
                    void* stream) {
  const char* fn = "gm_surface_nets";
  if (int rc = check_tsdf_grid(fn, nx, ny, nz, 2, origin, voxel)) return rc;
  if (min_weight != min_weight) { set_error("%s: min_weight is NaN", fn); return GM_ERR_INVALID_ARG; }
  if (max_vertices < 0 || max_faces < 0) { set_error("%s: negative capacity (%d vertices, %d faces)", fn, max_vertices, max_faces); return GM_ERR_INVALID_ARG; }
  if (!tsdf || !weight || !out_counts || !workspace || (max_vertices > 0 && !out_vertices) || (max_faces > 0 && !out_faces)) {
    set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG;
  }
  const SnDims dm = {{nx, ny, nz}};
  const size_t n = dm.total();
  const ByteRange rg[6] = {{tsdf, 4 * n, "tsdf", false}, {weight, 4 * n, "weight", false},               // (only read: they may be one buffer)
                           {out_vertices, 12 * (size_t)max_vertices, "out_vertices", true}, {out_faces, 12 * (size_t)max_faces, "out_faces", true},
                           {out_counts, 8, "out_counts", true}, {workspace, workspace_bytes, "workspace", true}};
  if (int rc = check_ranges(fn, rg)) return rc;
  const size_t need = gm_surface_nets_workspace_bytes(nx, ny, nz);
  if (workspace_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need); return GM_ERR_BUFFER; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SnWs k = SnWs::from(workspace, n);
  const TsdfGrid gr = {nx, ny, nz, origin[0], origin[1], origin[2], voxel};
  const dim3 blocks((unsigned)k.len[0]), threads(SN_BLOCK);
  hipLaunchKernelGGL(sn_cells, blocks, threads, 0, s, dm, tsdf, weight, min_weight, k.act);
  hipLaunchKernelGGL(sn_edges, blocks, threads, 0, s, dm, tsdf, k.act, k.flags, k.lvl[0]);
  for (int l = 0; l + 1 < k.levels; l++) hipLaunchKernelGGL(sn_sums, dim3((unsigned)k.len[l + 1]), threads, 0, s, k.lvl[l], k.len[l], k.lvl[l + 1]);
  const int top = k.levels - 1;
  hipLaunchKernelGGL(sn_scan_level, dim3(1), threads, 0, s, k.lvl[top], k.len[top], (const uint2*)nullptr, out_counts);
  for (int l = top - 1; l >= 0; l--)
    hipLaunchKernelGGL(sn_scan_level, dim3((unsigned)k.len[l + 1]), threads, 0, s, k.lvl[l], k.len[l], k.lvl[l + 1], (int*)nullptr);
  hipLaunchKernelGGL(sn_vertices, blocks, threads, 0, s, dm, tsdf, k.flags, k.lvl[0], gr, max_vertices, k.vid, out_vertices);
  hipLaunchKernelGGL(sn_faces, blocks, threads, 0, s, dm, tsdf, k.flags, k.lvl[0], k.vid, max_faces, out_faces);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // extern "C"
