// gm_deform.hip -- mesh-driven deformation of bound Gaussians and the edit tool's view-dependent colour.
//
// Replaces the Jittor tensor algebra of the reference (about ten separate elementwise/gather/matmul ops that
// materialise [N,3,3,3] gathers):
//   edittool/__init__.py:116-131  SingleObjectDeform.deform_gaussian
//   edittool/__init__.py:442-448  ObjectVisualTool.render_gaussian colour path (dir rotation + eval_sh + clamp)
//   edittool/general_utils.py:26-37 strip_symmetric (fused as the optional cov6 output)
// One thread per Gaussian; the per-vertex tables (dV, R, S: 84 B x Vm, ~0.6 MB for a 7.5k-vertex proxy mesh)
// stay L2-resident, the per-Gaussian streams (72 B in, 84-108 B out) are the HBM traffic.
#include "gm_common.h"
#include "gm_check.h"
#pragma clang fp contract(off)
#include "gm_sh.h"
#include "gm_stage.h"
#include "gm_pre_body.h"
#include <cstdlib>

namespace gm {

__global__ __launch_bounds__(256) void deform_kernel(int N, const int* __restrict__ tri, const float* __restrict__ w,
                                                     const float* __restrict__ dV, const float* __restrict__ Rv,
                                                     const float* __restrict__ Sv, const float* __restrict__ cov,
                                                     const float* __restrict__ pos, float* __restrict__ pos_out,
                                                     float* __restrict__ cov_out, float* __restrict__ rot_out,
                                                     float* __restrict__ cov6_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int t0 = tri[3 * (size_t)i], t1 = tri[3 * (size_t)i + 1], t2 = tri[3 * (size_t)i + 2];
  const float w0 = w[3 * (size_t)i], w1 = w[3 * (size_t)i + 1], w2 = w[3 * (size_t)i + 2];
  float d[3], Rb[9], Sb[9];
#pragma unroll
  for (int k = 0; k < 3; k++) d[k] = (w0 * dV[3 * (size_t)t0 + k] + w1 * dV[3 * (size_t)t1 + k]) + w2 * dV[3 * (size_t)t2 + k];
#pragma unroll
  for (int k = 0; k < 9; k++) {
    Rb[k] = (w0 * Rv[9 * (size_t)t0 + k] + w1 * Rv[9 * (size_t)t1 + k]) + w2 * Rv[9 * (size_t)t2 + k];
    Sb[k] = (w0 * Sv[9 * (size_t)t0 + k] + w1 * Sv[9 * (size_t)t1 + k]) + w2 * Sv[9 * (size_t)t2 + k];
  }
  float Rt[9], RS[9], A[9], C[9], O[9];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) Rt[3 * a + b] = Rb[3 * b + a];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) RS[3 * a + b] = (Rt[3 * a] * Sb[b] + Rt[3 * a + 1] * Sb[3 + b]) + Rt[3 * a + 2] * Sb[6 + b];
#pragma unroll
  for (int k = 0; k < 9; k++) C[k] = cov[9 * (size_t)i + k];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) A[3 * a + b] = (RS[3 * a] * C[b] + RS[3 * a + 1] * C[3 + b]) + RS[3 * a + 2] * C[6 + b];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) O[3 * a + b] = (A[3 * a] * RS[3 * b] + A[3 * a + 1] * RS[3 * b + 1]) + A[3 * a + 2] * RS[3 * b + 2];
#pragma unroll
  for (int k = 0; k < 9; k++) { cov_out[9 * (size_t)i + k] = O[k]; rot_out[9 * (size_t)i + k] = Rt[k]; }
#pragma unroll
  for (int k = 0; k < 3; k++) pos_out[3 * (size_t)i + k] = pos[3 * (size_t)i + k] + d[k];
  if (cov6_out) {
    float* o = cov6_out + 6 * (size_t)i;
    o[0] = O[0]; o[1] = O[1]; o[2] = O[2]; o[3] = O[4]; o[4] = O[5]; o[5] = O[8];
  }
}

__global__ __launch_bounds__(256) void sh_colors_kernel(int N, int deg, int M, const float* __restrict__ pos,
                                                        const float* __restrict__ campos, const float* __restrict__ rot,
                                                        const float* __restrict__ shs, float* __restrict__ rgb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  float dx = pos[3 * (size_t)i] - campos[0], dy = pos[3 * (size_t)i + 1] - campos[1], dz = pos[3 * (size_t)i + 2] - campos[2];
  const float len = sqrtf(dx * dx + dy * dy + dz * dz);
  dx = dx / len; dy = dy / len; dz = dz / len;
  float x = dx, y = dy, z = dz;
  if (rot) {   // dir_rot = rot^T dir
    const float* R = rot + 9 * (size_t)i;
    x = (R[0] * dx + R[3] * dy) + R[6] * dz;
    y = (R[1] * dx + R[4] * dy) + R[7] * dz;
    z = (R[2] * dx + R[5] * dy) + R[8] * dz;
  }
  float sh[48];
  load_sh(shs, i, M, (deg + 1) * (deg + 1), sh);
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    const float r = sh_channel(deg, [&](int k) { return sh[3 * k + ch]; }, x, y, z);
    rgb[3 * (size_t)i + ch] = fmaxf(r + 0.5f, 0.0f);
  }
}

// ---------------------------------------------------------------------------------------------
// The row body of the three fused kernels below (deform_shade_kernel, deform_shade_pre_batch_kernel, scene_shade_pre_batch_kernel).
// Their frames must come out bit for bit equal (tests/test_gpu_batch.py, test_gpu_scene_batch.py, test_gpu_parity.py; row by row, at every SH
// degree and block edge, and per element against float64: test_gpu_deform_rows.py), so every
// expression they share is written once, here, with its parenthesisation; arrays are plain pointers and stay in registers after inlining.
constexpr int DS_THREADS = 64;                     // one-wave workgroups of 64 Gaussians

// The block's SH rows -> LDS ([64][12] granules, the linear image of the rows).  A full block goes by LDS-DMA; the last, partial block by
// plain copies of each thread's own row.  The caller places this behind a sched_barrier(0) and waits (vmcnt(0) + __syncthreads) where it
// wants the rows: what it issues in between is in flight together with the DMA.
__device__ __forceinline__ void stage_sh_rows(float4* l_sh, const float* __restrict__ shs, size_t row0, int nrows, int t, size_t i) {
  if (nrows == DS_THREADS) {
    const char* gsh = reinterpret_cast<const char*>(shs + row0 * 48) + t * 16;
#pragma unroll
    for (int q = 0; q < 12; q++) dma16(gsh + q * 1024, reinterpret_cast<char*>(l_sh) + q * 1024);
  } else if (t < nrows) {
#pragma unroll
    for (int c = 0; c < 12; c++) l_sh[t * 12 + c] = reinterpret_cast<const float4*>(shs)[i * 12 + c];
  }
}

// The rest covariance of row i goes straight to registers (36 B per lane, the wave's 2304 B are contiguous): staging it as well
// would cost 2.25 KiB of LDS per wave, i.e. two resident waves per CU.  cov6 (wave-uniform): the row is its six distinct entries
// xx xy xz yy yz zz, 24 B per lane.
__device__ __forceinline__ void load_rest_cov(float* C, const float* __restrict__ cov, size_t i, bool live, bool cov6) {
  if (!live) {                                     // (decided once for the row, not per entry)
#pragma unroll
    for (int k = 0; k < 9; k++) C[k] = 0.f;
    return;
  }
  if (cov6) {
    float c6[6];
#pragma unroll
    for (int k = 0; k < 6; k++) c6[k] = cov[i * 6 + k];
    C[0] = c6[0]; C[1] = c6[1]; C[2] = c6[2]; C[3] = c6[1]; C[4] = c6[3]; C[5] = c6[4]; C[6] = c6[2]; C[7] = c6[4]; C[8] = c6[5];
  } else {
#pragma unroll
    for (int k = 0; k < 9; k++) C[k] = cov[i * 9 + k];
  }
}

// The three vertices of a Gaussian's face from the packed per-vertex table (pack_mesh_state_kernel: 6 float4 per vertex, 18 16-byte loads)
// and their barycentric blend: displacement d, rotation Rb, stretch Sb.
__device__ __forceinline__ void gather_blend(const float4* __restrict__ tab, int t0, int t1, int t2, float w0, float w1, float w2, float* d,
                                             float* Rb, float* Sb) {
  float va[24], vb[24], vc[24];
#pragma unroll
  for (int q = 0; q < 6; q++) {
    const float4 a = tab[6 * (size_t)t0 + q], b = tab[6 * (size_t)t1 + q], c = tab[6 * (size_t)t2 + q];
    va[4 * q] = a.x; va[4 * q + 1] = a.y; va[4 * q + 2] = a.z; va[4 * q + 3] = a.w;
    vb[4 * q] = b.x; vb[4 * q + 1] = b.y; vb[4 * q + 2] = b.z; vb[4 * q + 3] = b.w;
    vc[4 * q] = c.x; vc[4 * q + 1] = c.y; vc[4 * q + 2] = c.z; vc[4 * q + 3] = c.w;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) d[k] = (w0 * va[k] + w1 * vb[k]) + w2 * vc[k];
#pragma unroll
  for (int k = 0; k < 9; k++) {
    Rb[k] = (w0 * va[4 + k] + w1 * vb[4 + k]) + w2 * vc[4 + k];
    Sb[k] = (w0 * va[13 + k] + w1 * vb[13 + k]) + w2 * vc[13 + k];
  }
}

// Rt = Rb^T (the rotation the colour's view direction is turned by), O = (Rt Sb) C (Rt Sb)^T: deform_kernel's chain
__device__ __forceinline__ void deform_cov(const float* Rb, const float* Sb, const float* C, float* Rt, float* O) {
  float RS[9], A[9];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) Rt[3 * a + b] = Rb[3 * b + a];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) RS[3 * a + b] = (Rt[3 * a] * Sb[b] + Rt[3 * a + 1] * Sb[3 + b]) + Rt[3 * a + 2] * Sb[6 + b];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) A[3 * a + b] = (RS[3 * a] * C[b] + RS[3 * a + 1] * C[3 + b]) + RS[3 * a + 2] * C[6 + b];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) O[3 * a + b] = (A[3 * a] * RS[3 * b] + A[3 * a + 1] * RS[3 * b + 1]) + A[3 * a + 2] * RS[3 * b + 2];
}

// The edit tool's colour: SH of the view direction turned back into the rest frame (sh_colors_kernel with rot = Rt), from the
// thread's staged row
__device__ __forceinline__ void shade_rotated(int deg, const float* Rt, const float* npos, const float* __restrict__ campos, const float4* row,
                                              float* col) {
  float dx = npos[0] - campos[0], dy = npos[1] - campos[1], dz = npos[2] - campos[2];
  const float len = sqrtf(dx * dx + dy * dy + dz * dz);
  dx = dx / len; dy = dy / len; dz = dz / len;
  // dir_rot = rot^T dir with rot = Rt
  const float x = (Rt[0] * dx + Rt[3] * dy) + Rt[6] * dz;
  const float y = (Rt[1] * dx + Rt[4] * dy) + Rt[7] * dz;
  const float z = (Rt[2] * dx + Rt[5] * dy) + Rt[8] * dz;
  float sh[48];
#pragma unroll
  for (int c = 0; c < 12; c++) {
    const float4 v = row[c];
    sh[4 * c] = v.x; sh[4 * c + 1] = v.y; sh[4 * c + 2] = v.z; sh[4 * c + 3] = v.w;
  }
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    const float r = sh_channel(deg, [&](int k) { return sh[3 * k + ch]; }, x, y, z);
    col[ch] = fmaxf(r + 0.5f, 0.0f);
  }
}

// Where a fused pass leaves a row's preprocess results: the frame's geometry buffer and the caller's radii
struct PreSinks { float4* splat; int* radii_int; int* radii_out; uint32_t* tiles; uint4* bin; uint16_t* inst16; uint32_t* counters; uint32_t* slots; uint32_t* coarse; uint32_t* depth_key; };

static PreSinks pre_sinks(const GeomState& g, int* radii) {
  return PreSinks{g.splat, g.radii, radii, g.tiles_touched, g.bin, g.inst16, g.counters, g.slots, g.coarse, g.depth_key};
}

// Written once, where it is read: the radius goes to the caller's array (the internal copy exists for callers that pass none);
// the clamp flags and the per-Gaussian instance count are read by the backward pass and by the emission of a rectangle with
// 65535 instances or more only - a frame of this path has no backward, and the count rides in the emission record otherwise
// (9 of 349 bytes per Gaussian in a kernel that runs at the HBM's pace).  DIRECT: the record and the depth key go to the
// bucket's slab instead (direct_store).
template <bool DIRECT>
__device__ __forceinline__ void pre_write_row(const PreSinks& o, size_t i, int radius_i, uint32_t tiles, const uint4& dbin, uint32_t dkey,
                                              int tile_cull) {
  if (o.radii_out) o.radii_out[i] = radius_i; else o.radii_int[i] = radius_i;
  if (tiles >= GM_BIN_COUNT_SAT) o.tiles[i] = tiles;
  if (!DIRECT) {
    o.bin[i] = dbin;
    o.inst16[i] = (uint16_t)bin_count(dbin);       // what the ordering gathers per id; the record itself is read where it lies (duplicate_kernel)
    o.depth_key[i] = dkey;
  }
  if (i == 0) o.counters[GM_CNT_POLICY] = (uint32_t)tile_cull;
}

static PreCam pre_cam(int W, int H, int tile_cull, const float* view, const float* proj, float tanx, float tany) {
  PreCam c;
  c.W = W; c.H = H; c.gx = (W + GM_TILE - 1) / GM_TILE; c.gy = (H + GM_TILE - 1) / GM_TILE;
  c.tile_cull = tile_cull; c.view = view; c.proj = proj;
  c.tanx = tanx; c.tany = tany;
  c.fy = H / (2.0f * tany); c.fx = W / (2.0f * tanx);      // rasterizer_impl.cu:359-360
  return c;
}

// ---------------------------------------------------------------------------------------------
// Fused edit-loop kernel: deform + view-dependent colour in one pass (what ObjectVisualTool.render_gaussian needs per
// frame: means3D = x', colors_precomp, cov3D_precomp = strip_symmetric(Sigma'); edittool/__init__.py:421-472), and with PRE
// also the forward preprocess of the Gaussian it just produced.
// Reads 264 B and writes 48 B per Gaussian (+72 B if the caller also wants Sigma' and rot), against 72+108 (deform) +
// 240+12 (colour) for the two separate kernels.
// One-wave workgroups of 64 Gaussians.  The block's SH and covariance rows come into LDS by LDS-DMA
// (global_load_lds_dwordx4: no staging registers, no ds_write pass, and the loads are in flight while the wave gathers
// its vertices): per wave the dependent memory rounds are two (ids -> {rows DMA, vertex gathers}).  The LDS image is the
// linear image of the rows (a DMA instruction writes wave-uniform base + lane x 16 B); the 192-byte row stride makes the
// per-thread b128 reads bank-conflicted, which is immaterial next to the memory latency this kernel is bound by.
// Results leave through LDS as coalesced 16-byte stores.
// PACKED: dV points at the per-vertex table written by pack_mesh_state_kernel (6 float4 per vertex:
// {dV,0} {R0..3} {R4..7} {R8,S0,S1,S2} {S3..6} {S7,S8,0,0}); the three vertex gathers of a Gaussian are then 18 16-byte
// loads instead of 63 4-byte ones (Rv / Sv unused).
// PRE (edit-loop fast path): followed, in the same thread, by the forward preprocess of the
// Gaussian it just produced (gm_pre_body.h, the code preprocess_fwd_kernel runs on colors_precomp / cov3D_precomp
// inputs).  The deformed position / covariance / colour never travel through HBM (48 B written + 48 B read per
// Gaussian and one launch less per frame); pos_out / cov6_out / rgb_out are optional copies for callers that want them.
struct FusedPre {
  PreCam cam;
  const float* opac;
  PreSinks out;
  // DIRECT (gm_common.h, DepthSlab): the frame's snapshot of the stream's depth table and the bucket slabs the records are appended to
  const uint32_t* dmap; uint32_t* slab_cnt; uint2* slab_pairs; uint4* slab_recs; uint32_t slab_cap;
  int cov6;                     // the rest covariances come as [N][6] (a caller whose matrices are bit-symmetric: deform.pack_cov6)
};

// Direct depth placement: the wave's visible Gaussians are appended to their depth buckets' slabs.  One returning atomic per
// DISTINCT bucket of the wave (neighbours in memory are neighbours on the mesh: a wave usually spans two or three buckets), issued
// together; lanes whose bucket has not come up after GM_DIRECT_GROUPS rounds of the grouping loop (a cloud whose ids carry no
// locality) take a position on their own.  An entry beyond the slab's capacity is dropped - the counter still counts it and the
// frame is refused (direct_plan_kernel, gm_bucket.hip).
#ifndef GM_DIRECT_GROUPS
#define GM_DIRECT_GROUPS 6
#endif
struct DirectSlot { uint32_t bucket, base, rank; int leader; };
// first half, as soon as the depth key is known: bucket lookup, grouping, the returning atomics.  Nothing here waits for them - the
// emission count that follows (hundreds of instructions) runs while they are in flight.
__device__ __forceinline__ DirectSlot direct_reserve(const FusedPre& fp, uint32_t dkey) {
  const bool vis = dkey != 0xFFFFFFFFu;
  const int lane = threadIdx.x & 63;
  DirectSlot d;
  d.bucket = 0;
  if (vis) {
    const uint32_t e = fp.dmap[(dkey >> GM_COARSE_SHIFT) & (GM_COARSE_BINS - 1)];
    d.bucket = (e >> 16) + (((dkey & ((1u << GM_COARSE_SHIFT) - 1u)) * (e & 0xFFFFu)) >> GM_COARSE_SHIFT);
    d.bucket = min(d.bucket, (1u << GM_BUCKET_BITS) - 1u);   // (bins behind the table's last bucket: the last bucket - still monotone)
  }
  unsigned long long todo = __ballot(vis);
  uint32_t nsame = 1;
  d.rank = 0; d.leader = lane;
#pragma unroll 1
  for (int it = 0; it < GM_DIRECT_GROUPS && todo; it++) {
    const int l = __ffsll(todo) - 1;
    const uint32_t bl = (uint32_t)__builtin_amdgcn_readlane((int)d.bucket, l);
    const unsigned long long same = __ballot(vis && d.bucket == bl);
    if (vis && d.bucket == bl) { d.rank = lanes_below(same); d.leader = l; nsame = (uint32_t)__popcll(same); }
    todo &= ~same;
  }
  d.base = 0;
  if (vis && d.leader == lane) d.base = atomicAdd(fp.slab_cnt + (size_t)d.bucket * GM_SLAB_CNT_STRIDE, nsame);
  return d;
}
// second half: the leaders' positions reach their groups, the entry goes to its slab
__device__ __forceinline__ void direct_store(const FusedPre& fp, const DirectSlot& d, uint32_t id, uint32_t dkey, const uint4& bin) {
  const uint32_t pos = (uint32_t)__shfl((int)d.base, d.leader) + d.rank;
  if (dkey != 0xFFFFFFFFu && pos < fp.slab_cap) {
    const size_t at = (size_t)d.bucket * fp.slab_cap + pos;
    fp.slab_pairs[at] = make_uint2(dkey, id);
    fp.slab_recs[at] = bin;
  }
}

template <bool PACKED, bool PRE, bool DIRECT = false>
__global__ __launch_bounds__(64) void deform_shade_kernel(int N, int deg, const int* __restrict__ tri, const float* __restrict__ w,
                                                          const float* __restrict__ dV, const float* __restrict__ Rv,
                                                          const float* __restrict__ Sv, const float* __restrict__ cov,
                                                          const float* __restrict__ pos, const float* __restrict__ shs,
                                                          const float* __restrict__ campos, float* __restrict__ pos_out,
                                                          float* __restrict__ cov6_out, float* __restrict__ rgb_out,
                                                          float* __restrict__ cov_out, float* __restrict__ rot_out, const FusedPre fp) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float4* l_sh = reinterpret_cast<float4*>(lds);   // [64][12] granules: linear image of the block's SH rows (12 KiB)
  const size_t row0 = (size_t)blockIdx.x * DS_THREADS;
  const int nrows = min(DS_THREADS, N - (int)row0);
  const int t = threadIdx.x;
  const size_t i = row0 + t;
  const bool live = t < nrows;
  float O[9], Rt[9], npos[3], col[3];
  int t0 = 0, t1 = 0, t2 = 0; float w0 = 0.f, w1 = 0.f, w2 = 0.f, p0 = 0.f, p1 = 0.f, p2 = 0.f;
  if (live) {
    t0 = tri[3 * i]; t1 = tri[3 * i + 1]; t2 = tri[3 * i + 2];
    w0 = w[3 * i]; w1 = w[3 * i + 1]; w2 = w[3 * i + 2];
    p0 = pos[3 * i]; p1 = pos[3 * i + 1]; p2 = pos[3 * i + 2];
  }
  // ids are in (first use below waits for them); now start the row DMA, then the vertex gathers behind it
  __builtin_amdgcn_sched_barrier(0);
  stage_sh_rows(l_sh, shs, row0, nrows, t, i);
  float C[9];
  load_rest_cov(C, cov, i, live, PRE && fp.cov6);
  float d[3], Rb[9], Sb[9];
  if (PACKED) {
    gather_blend(reinterpret_cast<const float4*>(dV), t0, t1, t2, w0, w1, w2, d, Rb, Sb);
  } else {
#pragma unroll
    for (int k = 0; k < 3; k++) d[k] = (w0 * dV[3 * (size_t)t0 + k] + w1 * dV[3 * (size_t)t1 + k]) + w2 * dV[3 * (size_t)t2 + k];
#pragma unroll
    for (int k = 0; k < 9; k++) {
      Rb[k] = (w0 * Rv[9 * (size_t)t0 + k] + w1 * Rv[9 * (size_t)t1 + k]) + w2 * Rv[9 * (size_t)t2 + k];
      Sb[k] = (w0 * Sv[9 * (size_t)t0 + k] + w1 * Sv[9 * (size_t)t1 + k]) + w2 * Sv[9 * (size_t)t2 + k];
    }
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0): the DMA has landed
  __syncthreads();
  deform_cov(Rb, Sb, C, Rt, O);
  npos[0] = p0 + d[0]; npos[1] = p1 + d[1]; npos[2] = p2 + d[2];
  shade_rotated(deg, Rt, npos, campos, l_sh + t * 12, col);
  // ---- forward preprocess of the deformed Gaussian (colors_precomp / cov3D_precomp input mode)
  uint32_t tiles = 0, dkey = 0xFFFFFFFFu;
  uint4 dbin = make_uint4(0u, 0u, 0u, 0u);
  PreGeom pg;
  bool vis = false;
  if (PRE && live) {
    const V3 p = {npos[0], npos[1], npos[2]};
    const float c3[6] = {O[0], O[1], O[2], O[4], O[5], O[8]};
    vis = pre_project(fp.cam, p, c3, pg);
    if (vis) dkey = __float_as_uint(pg.depth);
  }
  DirectSlot slot;
  if (PRE && DIRECT) slot = direct_reserve(fp, dkey);          // (whole wave)
  if (PRE && live) {
    int radius_i = 0;
    if (vis) {
      const float opac = fp.opac[i];
      splat_store(fp.out.splat, i, pg.pix, pg.piy, pg.conx, pg.cony, pg.conz, opac, col[0], col[1], col[2], pg.depth);
      radius_i = (int)pg.radius;
      pre_emit(fp.cam, pg, opac, tiles, dbin);
    }
    pre_write_row<DIRECT>(fp.out, i, radius_i, tiles, dbin, dkey, fp.cam.tile_cull);
  }
  if (PRE && DIRECT) direct_store(fp, slot, (uint32_t)i, dkey, dbin);
  if (PRE) slot_accumulate(fp.out.slots, fp.out.coarse, tiles, dkey);
  if (!pos_out) return;                          // wave-uniform
  __syncthreads();                               // everyone is done reading the staged inputs: reuse LDS for the outputs
  float* o_pos = lds;                            // [256][3]
  float* o_rgb = lds + DS_THREADS * 3;           // [256][3]
  float* o_c6 = lds + DS_THREADS * 6;            // [256][6]  (stride 7 to stay conflict-free)
  float* o_cov = lds + DS_THREADS * 13;          // [256][9]
  float* o_rot = lds + DS_THREADS * 22;          // [256][9]
#pragma unroll
  for (int k = 0; k < 3; k++) { o_pos[t * 3 + k] = npos[k]; o_rgb[t * 3 + k] = col[k]; }
  o_c6[t * 7 + 0] = O[0]; o_c6[t * 7 + 1] = O[1]; o_c6[t * 7 + 2] = O[2]; o_c6[t * 7 + 3] = O[4]; o_c6[t * 7 + 4] = O[5]; o_c6[t * 7 + 5] = O[8];
  if (cov_out) {
#pragma unroll
    for (int k = 0; k < 9; k++) { o_cov[t * 9 + k] = O[k]; o_rot[t * 9 + k] = Rt[k]; }
  }
  __syncthreads();
  unstage_rows<3, 3, DS_THREADS>(pos_out, row0, nrows, o_pos);
  unstage_rows<3, 3, DS_THREADS>(rgb_out, row0, nrows, o_rgb);
  unstage_rows<6, 7, DS_THREADS>(cov6_out, row0, nrows, o_c6);
  if (cov_out) {
    unstage_rows<9, 9, DS_THREADS>(cov_out, row0, nrows, o_cov);
    unstage_rows<9, 9, DS_THREADS>(rot_out, row0, nrows, o_rot);
  }
}

// ---------------------------------------------------------------------------------------------
// K frames of one view stream from ONE pass over the static cloud (gm_forward_deformed_batch_async).  Of the 321 bytes per Gaussian the
// fused pass of a frame moves, 256 do not depend on the frame - face ids 12, weights 12, rest covariance 24 (36), rest position 12, SH row
// 192, opacity 4 - and a render loop with several frames in flight streamed them from HBM once per frame.  Here a wave loads them once
// (the SH rows stay in LDS, the rest in ~20 registers) and loops over the batch's frames: gather the frame's per-vertex table (L2
// resident: 0.7 MB per frame), deform, rotated-direction SH colour, project, emission record -> the frame's own geometry buffer.  Every
// expression is the one deform_shade_kernel<true, true> evaluates (the row body above, called in the same order), contraction off: each
// frame's geometry buffer comes out bit for bit as from the single-frame launch (tests/test_gpu_batch.py).
struct FusedFrame {
  PreCam cam;
  const float4* tab; const float* campos;
  PreSinks out;
};
struct FusedBatch { int frames, cov6; const float* opac; FusedFrame f[GM_BATCH_MAX]; };

__global__ __launch_bounds__(64) void deform_shade_pre_batch_kernel(int N, int deg, const int* __restrict__ tri, const float* __restrict__ w,
                                                                     const float* __restrict__ cov, const float* __restrict__ pos,
                                                                     const float* __restrict__ shs, const FusedBatch fb) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float4* l_sh = reinterpret_cast<float4*>(lds);   // [64][12] granules: linear image of the block's SH rows (12 KiB)
  const size_t row0 = (size_t)blockIdx.x * DS_THREADS;
  const int nrows = min(DS_THREADS, N - (int)row0);
  const int t = threadIdx.x;
  const size_t i = row0 + t;
  const bool live = t < nrows;
  int t0 = 0, t1 = 0, t2 = 0; float w0 = 0.f, w1 = 0.f, w2 = 0.f, p0 = 0.f, p1 = 0.f, p2 = 0.f, opac = 0.f;
  if (live) {
    t0 = tri[3 * i]; t1 = tri[3 * i + 1]; t2 = tri[3 * i + 2];
    w0 = w[3 * i]; w1 = w[3 * i + 1]; w2 = w[3 * i + 2];
    p0 = pos[3 * i]; p1 = pos[3 * i + 1]; p2 = pos[3 * i + 2];
    opac = fb.opac[i];
  }
  __builtin_amdgcn_sched_barrier(0);
  stage_sh_rows(l_sh, shs, row0, nrows, t, i);
  float C[9];
  load_rest_cov(C, cov, i, live, fb.cov6);
  __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0): the DMA has landed
  __syncthreads();
#pragma unroll 1
  for (int f = 0; f < fb.frames; f++) {
    const FusedFrame& F = fb.f[f];
    float d[3], Rb[9], Sb[9], O[9], Rt[9], npos[3], col[3];
    gather_blend(F.tab, t0, t1, t2, w0, w1, w2, d, Rb, Sb);
    deform_cov(Rb, Sb, C, Rt, O);
    npos[0] = p0 + d[0]; npos[1] = p1 + d[1]; npos[2] = p2 + d[2];
    shade_rotated(deg, Rt, npos, F.campos, l_sh + t * 12, col);
    uint32_t tiles = 0, dkey = 0xFFFFFFFFu;
    uint4 dbin = make_uint4(0u, 0u, 0u, 0u);
    PreGeom pg;
    bool vis = false;
    if (live) {
      const V3 p = {npos[0], npos[1], npos[2]};
      const float c3[6] = {O[0], O[1], O[2], O[4], O[5], O[8]};
      vis = pre_project(F.cam, p, c3, pg);
      if (vis) dkey = __float_as_uint(pg.depth);
      int radius_i = 0;
      if (vis) {
        splat_store(F.out.splat, i, pg.pix, pg.piy, pg.conx, pg.cony, pg.conz, opac, col[0], col[1], col[2], pg.depth);
        radius_i = (int)pg.radius;
        pre_emit(F.cam, pg, opac, tiles, dbin);
      }
      pre_write_row<false>(F.out, i, radius_i, tiles, dbin, dkey, F.cam.tile_cull);
    }
    slot_accumulate(F.out.slots, F.out.coarse, tiles, dkey);
  }
}

// one frame of a batched fused pass: camera constants and the frame's geometry buffer (shared by the object and the scene batch)
static FusedFrame fused_frame(const BatchFrameArgs& a, int W, int H, int tile_cull) {
  return FusedFrame{pre_cam(W, H, tile_cull, a.viewmatrix, a.projmatrix, a.tan_fovx, a.tan_fovy), reinterpret_cast<const float4*>(a.packed),
                    a.cam_pos, pre_sinks(a.g, a.radii)};
}

int launch_deform_shade_pre_batch(int frames, const BatchFrameArgs* fr, int P, int deg, int W, int H, int tile_cull, const int* tri, const float* w,
                                  const float* cov, const float* pos, const float* shs, const float* opacities, bool cov6, int debug, hipStream_t s) {
  if (P <= 0) return 0;
  if (frames < 1 || frames > GM_BATCH_MAX) { set_error("batched fused pass: 1..%d frames", GM_BATCH_MAX); return 1; }
  if (!aligned16(shs) || !aligned16(cov)) { set_error("gm_forward_deformed_batch: shs / cov must be 16-byte aligned"); return 1; }
  StageScope sc(ST_DEFORM, s);
  FusedBatch fb{};
  fb.frames = frames; fb.cov6 = cov6 ? 1 : 0; fb.opac = opacities;
  for (int k = 0; k < frames; k++) {
    if (!aligned16(fr[k].packed)) { set_error("gm_forward_deformed_batch: packed tables must be 16-byte aligned"); return 1; }
    fb.f[k] = fused_frame(fr[k], W, H, tile_cull);
  }
  hipLaunchKernelGGL(deform_shade_pre_batch_kernel, dim3((P + 63) / 64), dim3(64), sizeof(float) * 64 * 48, s, P, deg, tri, w, cov, pos, shs, fb);
  GM_LAUNCH_CHECK(debug, s);
  return 0;
}

// mesh state of one deformation frame, as broadcast to the ranks ([Vm][21] = V1 | R | S), minus the rest pose -> the
// gather table of deform_shade_kernel<.., true>
__global__ __launch_bounds__(256) void pack_mesh_state_kernel(int Vm, const float* __restrict__ state, const float* __restrict__ verts,
                                                               float4* __restrict__ packed) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= Vm) return;
  const float* s = state + 21 * (size_t)v;
  float4* o = packed + 6 * (size_t)v;
  o[0] = make_float4(s[0] - verts[3 * (size_t)v], s[1] - verts[3 * (size_t)v + 1], s[2] - verts[3 * (size_t)v + 2], 0.f);
  o[1] = make_float4(s[3], s[4], s[5], s[6]);
  o[2] = make_float4(s[7], s[8], s[9], s[10]);
  o[3] = make_float4(s[11], s[12], s[13], s[14]);
  o[4] = make_float4(s[15], s[16], s[17], s[18]);
  o[5] = make_float4(s[19], s[20], 0.f, 0.f);
}

int launch_deform_shade_pre(const RasterArgs& r, GeomState& g, int* radii, int deg, const int* tri, const float* w, const float* packed,
                            const float* cov, const float* pos, const float* shs, float* pos_out, float* cov6_out, float* rgb_out,
                            const DepthSlab* slab, bool cov6) {
  const int N = r.P;
  if (N <= 0) return 0;
  if (!aligned16(shs) || !aligned16(cov) || !aligned16(packed) ||
      (pos_out && (!aligned16(pos_out) || !aligned16(cov6_out) || !aligned16(rgb_out)))) {
    set_error("gm_forward_0_deformed: shs / cov / packed / outputs must be 16-byte aligned"); return 1;
  }
  StageScope sc(ST_DEFORM, r.stream);
  FusedPre fp;
  fp.cam = pre_cam(r.W, r.H, r.tile_cull, r.viewmatrix, r.projmatrix, r.tan_fovx, r.tan_fovy);
  fp.opac = r.opacities;
  fp.out = pre_sinks(g, radii);
  fp.cov6 = cov6 ? 1 : 0;
  fp.dmap = g.dmap; fp.slab_cnt = nullptr; fp.slab_pairs = nullptr; fp.slab_recs = nullptr; fp.slab_cap = 0;
  if (slab) { fp.slab_cnt = slab->cnt; fp.slab_pairs = slab->pairs; fp.slab_recs = slab->recs; fp.slab_cap = slab->cap; }
  // (measured: fewer resident workgroups per CU - 8 / 6 / 5 instead of 12, by padding this allocation - make the kernel 10 / 24 / 52 %
  // slower and the four-stream loop 6 / 13 / 21 %: it needs every wave it can get to keep enough bytes in flight)
  const size_t lds_bytes = sizeof(float) * 64 * 48;
  if (slab)
    hipLaunchKernelGGL((deform_shade_kernel<true, true, true>), dim3((N + 63) / 64), dim3(64), lds_bytes, r.stream, N, deg, tri, w, packed, nullptr,
                       nullptr, cov, pos, shs, r.cam_pos, pos_out, cov6_out, rgb_out, nullptr, nullptr, fp);
  else
    hipLaunchKernelGGL((deform_shade_kernel<true, true>), dim3((N + 63) / 64), dim3(64), lds_bytes, r.stream, N, deg, tri, w, packed, nullptr,
                       nullptr, cov, pos, shs, r.cam_pos, pos_out, cov6_out, rgb_out, nullptr, nullptr, fp);
  GM_LAUNCH_CHECK(r.debug, r.stream);
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Covariance -> (scale, quaternion): replaces SceneVisualTool.render_gaussian's per-frame
//   eigh(cov) on the device, det sign fixed on the HOST through numpy, sqrt(eigenvalues), matrix -> quaternion
// (edittool/__init__.py:204-207 and :23-38), i.e. a device->host->device round trip of 36 B per Gaussian per frame.
// One thread per Gaussian: cyclic Jacobi in double (3x3 symmetric, <= 8 sweeps), eigenvalues ascending like eigh,
// eigenvector matrix multiplied by sign(det) as the reference does, quaternion (w,x,y,z) by the branch-safe
// largest-component form (the reference's w = sqrt(1+trace)/2 divides by zero for trace <= -1), normalised.
// Eigenvector signs are not unique, so parity is on the reconstructed covariance R diag(s^2) R^T, not on (s, q).
// cov_to_scale_rot_row: the same for row i of cov -> rots[i], scales[3 i .. 3 i + 2] (gm_cov_to_scale_rot_body.inc, the kernel's own body);
// the scene batch's fused pass runs it on a deformed row's covariance in registers (i = 0 on local arrays).
__device__ __forceinline__ void cov_to_scale_rot_row(const float* cov, float4* rots, float* scales, int i) {
#include "gm_cov_to_scale_rot_body.inc"
}

__global__ __launch_bounds__(256) void cov_to_scale_rot_kernel(int N, const float* __restrict__ cov, float* __restrict__ scales,
                                                               float* __restrict__ rots) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
#include "gm_cov_to_scale_rot_body.inc"
}

// ---------------------------------------------------------------------------------------------
// K frames of a SCENE from ONE pass over its cloud (gm_forward_scene_batch_async): a free-standing background plus mesh-bound objects,
// the rows in the order SceneVisualTool.render_gaussian concatenates them (background, then each object).  One frame of that route is
// gm_cov_to_scale_rot of every row's covariance, then preprocess_fwd_kernel on (means, shs, scales, rotations): the colour from the
// rasterizer's own SH with the UNROTATED direction p - campos (edittool/__init__.py:196-223).  Here each row is, in each frame, one of:
//   static    a background row, or a row of an object at rest in this frame: its position and (s, q) = gm_cov_to_scale_rot of its covariance,
//             computed once per state by the caller (the Jacobi is deterministic: once equals every frame);
//   deformed  a row of an object the frame's gather table moves: the expressions of deform_kernel, in the order deform_shade_kernel evaluates
//             them, then the Jacobi of cov_to_scale_rot_kernel on the 3x3 result - skipped for a row behind the near plane, whose (s, q)
//             reach no output.
// Both kinds then run preprocess_fwd_kernel's computeCov3D, SH colour, projection and emission (gm_pre_body.h, scale modifier 1 as in
// render_gaussian): each frame's geometry buffer comes out as the single-frame route writes it, bit for bit (tests/test_gpu_scene_batch.py).
// As deform_shade_pre_batch_kernel: one 64-lane wave per workgroup, the block's SH rows in LDS by LDS-DMA, the static inputs in registers,
// a loop over the frames.  A wave may straddle the background / object boundary or two objects: the kind is chosen per lane.
struct SceneBatch {
  int frames, n_obj;
  uint32_t moving;                                 // objects some frame of the batch deforms (the OR of mask[])
  int rows[GM_SCENE_OBJECTS_MAX + 1];              // object j: rows [rows[j], rows[j + 1]); tri / w / cov are indexed by row - rows[0]
  uint32_t mask[GM_BATCH_MAX];                     // bit j of mask[f]: frame f deforms object j through f[f].tab
  const float* opac;
  FusedFrame f[GM_BATCH_MAX];
};

__global__ __launch_bounds__(64) void scene_shade_pre_batch_kernel(int N, int deg, const float* __restrict__ pos, const float* __restrict__ scales,
                                                                   const float* __restrict__ rots, const float* __restrict__ shs,
                                                                   const int* __restrict__ tri, const float* __restrict__ w,
                                                                   const float* __restrict__ cov, const SceneBatch sb) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float4* l_sh = reinterpret_cast<float4*>(lds);   // [64][12] granules: linear image of the block's SH rows (12 KiB)
  const size_t row0 = (size_t)blockIdx.x * DS_THREADS;
  const int nrows = min(DS_THREADS, N - (int)row0);
  const int t = threadIdx.x;
  const size_t i = row0 + t;
  const bool live = t < nrows;
  int obj = -1;                                    // the row's object; -1: static in every frame (background, or behind the last object)
  if (live && (int)i >= sb.rows[0] && (int)i < sb.rows[sb.n_obj]) {
    obj = 0;
    for (int j = 1; j < sb.n_obj; j++) obj = (int)i >= sb.rows[j] ? j : obj;      // (an empty object shares its start with the next)
  }
  const bool moving = obj >= 0 && ((sb.moving >> obj) & 1u);
  float p0 = 0.f, p1 = 0.f, p2 = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f, opac = 0.f;
  float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f);
  int t0 = 0, t1 = 0, t2 = 0; float w0 = 0.f, w1 = 0.f, w2 = 0.f;
  if (live) {
    p0 = pos[3 * i]; p1 = pos[3 * i + 1]; p2 = pos[3 * i + 2];
    s0 = scales[3 * i]; s1 = scales[3 * i + 1]; s2 = scales[3 * i + 2];
    q0 = reinterpret_cast<const float4*>(rots)[i];
    opac = sb.opac[i];
  }
  const size_t r = moving ? i - (size_t)sb.rows[0] : 0;
  if (moving) {
    t0 = tri[3 * r]; t1 = tri[3 * r + 1]; t2 = tri[3 * r + 2];
    w0 = w[3 * r]; w1 = w[3 * r + 1]; w2 = w[3 * r + 2];
  }
  __builtin_amdgcn_sched_barrier(0);
  stage_sh_rows(l_sh, shs, row0, nrows, t, i);
  float C[9];                                      // the rest covariance of a movable row
  load_rest_cov(C, cov, r, moving, false);
  __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0): the DMA has landed
  __syncthreads();
#pragma unroll 1
  for (int f = 0; f < sb.frames; f++) {
    const FusedFrame& F = sb.f[f];
    V3 p = {p0, p1, p2};
    float4 q = q0;
    float sc[3] = {s0, s1, s2};
    if (moving && ((sb.mask[f] >> obj) & 1u)) {
      float d[3], Rb[9], Sb[9], Rt[9], O[9];         // (Rt: the scene's colour takes the unrotated direction)
      gather_blend(F.tab, t0, t1, t2, w0, w1, w2, d, Rb, Sb);
      deform_cov(Rb, Sb, C, Rt, O);
      p = V3{p0 + d[0], p1 + d[1], p2 + d[2]};
      if (!(xform4x3(p, F.cam.view).z <= 0.2f)) cov_to_scale_rot_row(O, &q, sc, 0);     // (not culled by pre_project's near-plane test)
    }
    uint32_t tiles = 0, dkey = 0xFFFFFFFFu;
    uint4 dbin = make_uint4(0u, 0u, 0u, 0u);
    if (live) {
      float c3[6];
      cov3d_from_scale_rot(q, sc, c3);
      PreGeom pg;
      const bool vis = pre_project(F.cam, p, c3, pg);
      int radius_i = 0;
      if (vis) {
        float col[3];
        sh_color(deg, p, F.campos, l_sh + t * 12, col);
        dkey = __float_as_uint(pg.depth);
        splat_store(F.out.splat, i, pg.pix, pg.piy, pg.conx, pg.cony, pg.conz, opac, col[0], col[1], col[2], pg.depth);
        radius_i = (int)pg.radius;
        pre_emit(F.cam, pg, opac, tiles, dbin);
      }
      pre_write_row<false>(F.out, i, radius_i, tiles, dbin, dkey, F.cam.tile_cull);
    }
    slot_accumulate(F.out.slots, F.out.coarse, tiles, dkey);
  }
}

int launch_scene_shade_pre_batch(int frames, const BatchFrameArgs* fr, const uint32_t* deformed, int n_obj, const int* object_rows, int P, int deg,
                                 int W, int H, int tile_cull, const float* pos, const float* scales, const float* rots, const float* shs,
                                 const float* opacities, const int* tri, const float* w, const float* cov, int debug, hipStream_t s) {
  if (P <= 0) return 0;
  if (frames < 1 || frames > GM_BATCH_MAX || n_obj < 0 || n_obj > GM_SCENE_OBJECTS_MAX) {
    set_error("scene fused pass: 1..%d frames, 0..%d objects", GM_BATCH_MAX, GM_SCENE_OBJECTS_MAX); return 1;
  }
  if (!aligned16(shs) || !aligned16(rots)) { set_error("gm_forward_scene_batch: shs / rots must be 16-byte aligned"); return 1; }
  StageScope sc(ST_DEFORM, s);
  SceneBatch sb{};
  sb.frames = frames; sb.n_obj = n_obj; sb.opac = opacities;
  for (int j = 0; j <= n_obj; j++) sb.rows[j] = object_rows[j];
  for (int k = 0; k < frames; k++) {
    sb.mask[k] = deformed[k];
    sb.moving |= deformed[k];
    if (deformed[k] && !aligned16(fr[k].packed)) { set_error("gm_forward_scene_batch: packed tables must be 16-byte aligned"); return 1; }
    sb.f[k] = fused_frame(fr[k], W, H, tile_cull);
  }
  hipLaunchKernelGGL(scene_shade_pre_batch_kernel, dim3((P + 63) / 64), dim3(64), sizeof(float) * 64 * 48, s, P, deg, pos, scales, rots, shs, tri, w,
                     cov, sb);
  GM_LAUNCH_CHECK(debug, s);
  return 0;
}

}  // namespace gm

// ---------------------------------------------------------------------------------------------
// the entry points the rasteriser's orchestration (gm_api.hip) does not compose: their refusals, then the launches
using namespace gm;

extern "C" {

int gm_deform(int N, const int* tri, const float* w, const float* dV, const float* Rv, const float* Sv,
              const float* cov, const float* pos, float* pos_out, float* cov_out, float* rot_out, float* cov6_out,
              void* stream) {
  if (N < 0 || (N > 0 && (!tri || !w || !dV || !Rv || !Sv || !cov || !pos || !pos_out || !cov_out || !rot_out))) {
    set_error("gm_deform: bad args"); return GM_ERR_INVALID_ARG;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  StageScope sc(ST_DEFORM, s);
  if (N > 0)
    hipLaunchKernelGGL(deform_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, tri, w, dV, Rv, Sv, cov, pos, pos_out, cov_out,
                       rot_out, cov6_out);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_sh_colors(int N, int deg, int M, const float* pos, const float* campos, const float* rot, const float* shs,
                 float* rgb, void* stream) {
  if (N < 0 || deg < 0 || deg > 3 || M < (deg + 1) * (deg + 1) || (N > 0 && (!pos || !campos || !shs || !rgb))) {
    set_error("gm_sh_colors: bad args"); return GM_ERR_INVALID_ARG;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  StageScope sc(ST_SH_COLORS, s);
  if (N > 0) hipLaunchKernelGGL(sh_colors_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, deg, M, pos, campos, rot, shs, rgb);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_pack_mesh_state(int Vm, const float* state, const float* verts, float* packed, void* stream) {
  if (Vm < 0 || (Vm > 0 && (!state || !verts || !packed))) { set_error("gm_pack_mesh_state: bad args"); return GM_ERR_INVALID_ARG; }
  if (Vm == 0) return GM_OK;
  if (reinterpret_cast<uintptr_t>(packed) & 15) { set_error("gm_pack_mesh_state: packed must be 16-byte aligned"); return GM_ERR_INVALID_ARG; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  StageScope sc(ST_DEFORM, s);
  hipLaunchKernelGGL(pack_mesh_state_kernel, dim3((Vm + 255) / 256), dim3(256), 0, s, Vm, state, verts, reinterpret_cast<float4*>(packed));
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_deform_shade_packed(int N, int deg, int M, const int* tri, const float* w, const float* packed, const float* cov,
                           const float* pos, const float* shs, const float* campos, float* pos_out, float* cov6_out,
                           float* rgb_out, float* cov_out, float* rot_out, void* stream) {
  if (N < 0 || deg < 0 || deg > 3 || M < (deg + 1) * (deg + 1) ||
      (N > 0 && (!tri || !w || !packed || !cov || !pos || !shs || !campos || !pos_out || !cov6_out || !rgb_out)) ||
      ((cov_out == nullptr) != (rot_out == nullptr))) {
    set_error("gm_deform_shade_packed: bad args"); return GM_ERR_INVALID_ARG;
  }
  if (N == 0) return GM_OK;
  if (M != 16 || !aligned16(shs) || !aligned16(cov) || !aligned16(pos_out) || !aligned16(cov6_out) || !aligned16(rgb_out) ||
      !aligned16(packed) || (cov_out && (!aligned16(cov_out) || !aligned16(rot_out)))) {
    set_error("gm_deform_shade_packed: needs M == 16 and 16-byte aligned buffers"); return GM_ERR_INVALID_ARG;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  StageScope sc(ST_DEFORM, s);
  const size_t lds_bytes = sizeof(float) * 64 * 48;
  hipLaunchKernelGGL((deform_shade_kernel<true, false>), dim3((N + 63) / 64), dim3(64), lds_bytes, s, N, deg, tri, w, packed, nullptr, nullptr,
                     cov, pos, shs, campos, pos_out, cov6_out, rgb_out, cov_out, rot_out, FusedPre{});
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_deform_shade(int N, int deg, int M, const int* tri, const float* w, const float* dV, const float* Rv, const float* Sv,
                    const float* cov, const float* pos, const float* shs, const float* campos, float* pos_out, float* cov6_out,
                    float* rgb_out, float* cov_out, float* rot_out, void* stream) {
  if (N < 0 || deg < 0 || deg > 3 || M < (deg + 1) * (deg + 1) ||
      (N > 0 && (!tri || !w || !dV || !Rv || !Sv || !cov || !pos || !shs || !campos || !pos_out || !cov6_out || !rgb_out)) ||
      ((cov_out == nullptr) != (rot_out == nullptr))) {
    set_error("gm_deform_shade: bad args"); return GM_ERR_INVALID_ARG;
  }
  if (N == 0) return GM_OK;
  if (M != 16 || !aligned16(shs) || !aligned16(cov) || !aligned16(pos_out) || !aligned16(cov6_out) || !aligned16(rgb_out) ||
      (cov_out && (!aligned16(cov_out) || !aligned16(rot_out)))) {
    // general layout: run the two unfused kernels (needs the 72 B/Gaussian intermediates from the caller)
    if (!cov_out || !rot_out) { set_error("gm_deform_shade: M != 16 or unaligned buffers need cov_out/rot_out"); return GM_ERR_INVALID_ARG; }
    if (int rc = gm_deform(N, tri, w, dV, Rv, Sv, cov, pos, pos_out, cov_out, rot_out, cov6_out, stream)) return rc;
    return gm_sh_colors(N, deg, M, pos_out, campos, rot_out, shs, rgb_out, stream);
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  StageScope sc(ST_DEFORM, s);
  const size_t lds_bytes = sizeof(float) * 64 * 48;
  hipLaunchKernelGGL((deform_shade_kernel<false, false>), dim3((N + 63) / 64), dim3(64), lds_bytes, s, N, deg, tri, w, dV, Rv, Sv, cov, pos,
                     shs, campos, pos_out, cov6_out, rgb_out, cov_out, rot_out, FusedPre{});
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_cov_to_scale_rot(int N, const float* cov, float* scales, float* rots, void* stream) {
  if (N < 0 || (N > 0 && (!cov || !scales || !rots))) { set_error("gm_cov_to_scale_rot: bad args"); return GM_ERR_INVALID_ARG; }
  if (N > 0 && (reinterpret_cast<uintptr_t>(rots) & 15)) { set_error("gm_cov_to_scale_rot: rots must be 16-byte aligned"); return GM_ERR_INVALID_ARG; }
  if (N > 0)
    hipLaunchKernelGGL(cov_to_scale_rot_kernel, dim3((N + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), N, cov, scales, rots);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // extern "C"
