// gm_tsdf_fill.hip -- close the unobserved holes of a signed distance volume by volumetric diffusion (Davis, Marschner, Garr, Levoy
// 2002): the observed samples stay fixed, the distance diffuses from them into the samples no view saw, until inside and outside values
// meet and gm_surface_nets finds a zero crossing where the fused volume alone ends in a border.  The stage behind
// proxy_mesh.TsdfVolume.fill_holes / extract(fill_holes=); gm_tsdf.hip's volume is its input and is only read.
//
// THE RESULT IS DEFINED BY ARITHMETIC, as everything around gm_tsdf.hip is: float32, no contraction (file pragma), correctly rounded
// division, the order of operations as written here; tests/tsdf_fill_ref.py restates it in numpy, bit for bit.
//     src(g) = weight_in[g] >= min_weight (false on NaN); val_0 = src ? tsdf_in : +0, known_0 = src
//     iteration t = 0 .. N-1, a Jacobi step that reads only val_t / known_t: s = known_t(g) ? val_t(g) : 0, c = known_t(g) ? 1 : 0; over
//       the face neighbours in the order -x, +x, -y, +y, -z, +z: one inside the grid with known_t: s = s + val_t(nb), c++; one outside
//       the grid: with boundary_free s = s + 1 (free space), c++, otherwise nothing
//       not src(g) and c > 0: val_{t+1}(g) = s / (float)c, known_{t+1}(g) = 1; otherwise both carry over
//     tsdf_out = val_N, weight_out = src ? weight_in : (known_N ? fill_weight : 0), out_counts = {filled, still unknown}
//   A filled sample is averaged again in every later iteration (that is the diffusion; its own term damps the checkerboard mode);
//   after n iterations every sample within n six-connected steps of a known one has a value.
//
// One launch per iteration between two (value, state) pairs - tsdf_out with a state array of the workspace, and a second pair in the
// workspace -, so a step never reads what it writes and no workgroup waits for another.  Both pairs start as (val_0, known_0); a sample
// that is not updated in a step is a source or still unknown, and both pairs already hold what carries over.  The pair the first step
// reads is chosen by the parity of N: the last step writes tsdf_out.  A workgroup is a brick of 32 x 4 x 2 samples (x-rows of 128
// bytes); the first pass notes per brick whether it holds anything but sources, and a brick of sources - most of a carved volume -
// returns after reading that byte.  The neighbours come straight from global memory, all of a sample's loads issued together: a step is
// bound by the latency of its dependent rounds of loads, not by bytes (profiles/tsdf_fill_time.txt: 9.1 us a step at 128^3 with 3896
// of 8192 bricks open, 15.2 us with the loads one after the other), and a brick staged in LDS with its halo removes none of them.  The
// counts are integer atomics over per-workgroup sums: the same in every run.
// Conventions of gm_tsdf.hip: caller workspace, stream-ordered, no device allocation, no host wait anywhere in this file.
#include "gm_common.h"
#include "gm_check.h"
#include "gm_wave.h"
#pragma clang fp contract(off)   // every sum and quotient rounds on its own, as the definition above says

namespace gm {

#define TF_BX 32         // a brick: TF_BX x TF_BY x TF_BZ samples, one per thread of a 256-thread workgroup
#define TF_BY 4
#define TF_BZ 2
#define TF_KNOWN 1u      // state byte: the sample has a value
#define TF_SRC 2u        //             and it is an observed one (never written again)

struct TfGrid {
  int nx, ny, nz, bx, by, bz;
  static TfGrid of(int nx, int ny, int nz) {
    return {nx, ny, nz, (nx + TF_BX - 1) / TF_BX, (ny + TF_BY - 1) / TF_BY, (nz + TF_BZ - 1) / TF_BZ};
  }
  size_t samples() const { return (size_t)nx * ny * nz; }
  size_t bricks() const { return (size_t)bx * by * bz; }
  // this thread's sample of brick b; false: the brick reaches past the grid there
  __device__ bool locate(size_t b, int& ix, int& iy, int& iz) const {
    const int t = threadIdx.x;
    ix = (int)(b % bx) * TF_BX + (t & (TF_BX - 1));
    iy = (int)((b / bx) % by) * TF_BY + ((t / TF_BX) & (TF_BY - 1));
    iz = (int)(b / ((size_t)bx * by)) * TF_BZ + t / (TF_BX * TF_BY);
    return ix < nx && iy < ny && iz < nz;
  }
  __device__ size_t index(int ix, int iy, int iz) const { return ((size_t)iz * ny + iy) * nx + ix; }
};

struct TfWs {
  float* val;              // [n] the second value array (the first is tsdf_out)
  uint8_t* state[2];       // [n] each: TF_KNOWN | TF_SRC; state[0] goes with tsdf_out, state[1] with val
  uint8_t* open;           // [bricks] the brick holds a sample that is not a source
  char* end;
  static TfWs from(void* ws, const TfGrid& g) {
    char* p = reinterpret_cast<char*>(ws);
    TfWs k;
    k.val = carve<float>(p, g.samples());
    k.state[0] = carve<uint8_t>(p, g.samples());
    k.state[1] = carve<uint8_t>(p, g.samples());
    k.open = carve<uint8_t>(p, g.bricks());
    k.end = p;
    return k;
  }
};

// (val_0, known_0) into both pairs, the brick's byte, and the counters back to zero
__global__ __launch_bounds__(256) void tf_init(TfGrid g, const float* __restrict__ tsdf_in, const float* __restrict__ weight_in, float min_weight,
                                               float* __restrict__ val0, float* __restrict__ val1, uint8_t* __restrict__ state0,
                                               uint8_t* __restrict__ state1, uint8_t* __restrict__ open, int* __restrict__ counts) {
  int ix, iy, iz;
  int not_src = 0;
  if (g.locate(blockIdx.x, ix, iy, iz)) {
    const size_t i = g.index(ix, iy, iz);
    const bool src = weight_in[i] >= min_weight;
    const float v = src ? tsdf_in[i] : 0.0f;
    const uint8_t st = src ? (uint8_t)(TF_KNOWN | TF_SRC) : (uint8_t)0;
    val0[i] = v; val1[i] = v;
    state0[i] = st; state1[i] = st;
    not_src = src ? 0 : 1;
  }
  const int any = __syncthreads_or(not_src);
  if (threadIdx.x == 0) {
    open[blockIdx.x] = any ? 1 : 0;
    if (blockIdx.x == 0 && counts) { counts[0] = 0; counts[1] = 0; }
  }
}

__global__ __launch_bounds__(256) void tf_step(TfGrid g, int boundary_free, const uint8_t* __restrict__ open, const float* __restrict__ val_in,
                                               const uint8_t* __restrict__ state_in, float* __restrict__ val_out, uint8_t* __restrict__ state_out) {
  if (!open[blockIdx.x]) return;               // a wave-uniform byte: the whole workgroup leaves
  int ix, iy, iz;
  if (!g.locate(blockIdx.x, ix, iy, iz)) return;
  const size_t i = g.index(ix, iy, iz);
  const uint32_t st = state_in[i];
  if (st & TF_SRC) return;
  // All thirteen loads are issued before the first is used - a neighbour the grid does not have reads the sample itself and is not
  // used -, so a step waits for memory once, not once per neighbour; the sums below are pure arithmetic, in the definition's order.
  const size_t sy = (size_t)g.nx, sz = (size_t)g.nx * g.ny;
  const bool inside[6] = {ix > 0, ix + 1 < g.nx, iy > 0, iy + 1 < g.ny, iz > 0, iz + 1 < g.nz};
  const size_t at[6] = {i - 1, i + 1, i - sy, i + sy, i - sz, i + sz};
  uint32_t nst[6];
  float nval[6];
  const float own = val_in[i];
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const size_t j = inside[k] ? at[k] : i;
    nst[k] = state_in[j];
    nval[k] = val_in[j];
  }
  float s = 0.0f;
  int c = 0;
  if (st & TF_KNOWN) { s = own; c = 1; }
#pragma unroll
  for (int k = 0; k < 6; k++) {
    if (inside[k]) {
      if (nst[k] & TF_KNOWN) { s = s + nval[k]; c++; }
    } else if (boundary_free) { s = s + 1.0f; c++; }
  }
  if (c > 0) {
    val_out[i] = s / (float)c;
    state_out[i] = (uint8_t)TF_KNOWN;
  }
}

// weight_out and the counts from the final state (one thread per sample in linear order: the bricks do not matter here)
__global__ __launch_bounds__(256) void tf_finish(size_t n, const float* __restrict__ weight_in, const uint8_t* __restrict__ state, float fill_weight,
                                                 float* __restrict__ weight_out, int* __restrict__ counts) {
  __shared__ uint32_t sums[4][2];
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t filled = 0, unknown = 0;
  if (i < n) {
    const uint32_t st = state[i];
    weight_out[i] = (st & TF_SRC) ? weight_in[i] : ((st & TF_KNOWN) ? fill_weight : 0.0f);
    filled = st == TF_KNOWN ? 1u : 0u;
    unknown = st == 0u ? 1u : 0u;
  }
  if (!counts) return;
  filled = wave_sum_u32(filled);
  unknown = wave_sum_u32(unknown);
  if ((threadIdx.x & 63) == 0) { sums[threadIdx.x >> 6][0] = filled; sums[threadIdx.x >> 6][1] = unknown; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t f = (sums[0][0] + sums[1][0]) + (sums[2][0] + sums[3][0]), u = (sums[0][1] + sums[1][1]) + (sums[2][1] + sums[3][1]);
    if (f) atomicAdd(&counts[0], (int)f);
    if (u) atomicAdd(&counts[1], (int)u);
  }
}

}  // namespace gm

// ---------------------------------------------------------------------------------------------
// the entry points (include/gmesh_hip.h): their refusals, then the launches
using namespace gm;

extern "C" {

size_t gm_tsdf_fill_workspace_bytes(int nx, int ny, int nz) {
  const TfWs k = TfWs::from(nullptr, TfGrid::of(nx > 2 ? nx : 2, ny > 2 ? ny : 2, nz > 2 ? nz : 2));
  return (size_t)k.end + 256;    // (the caller's pointer may sit anywhere inside a 256-byte line)
}

int gm_tsdf_fill(int nx, int ny, int nz, const float* tsdf_in, const float* weight_in, float min_weight, int iterations, int boundary_free,
                 float fill_weight, float* tsdf_out, float* weight_out, int* out_counts, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "gm_tsdf_fill";
  static const float no_origin[3] = {0.f, 0.f, 0.f};                  // (the fill knows samples, not where they lie)
  if (int rc = check_tsdf_grid(fn, nx, ny, nz, 2, no_origin, 1.0f)) return rc;
  if (iterations < 0) { set_error("%s: iterations = %d (negative)", fn, iterations); return GM_ERR_INVALID_ARG; }
  if (min_weight != min_weight || fill_weight != fill_weight) { set_error("%s: min_weight or fill_weight is NaN", fn); return GM_ERR_INVALID_ARG; }
  if (!tsdf_in || !weight_in || !tsdf_out || !weight_out || !workspace) { set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG; }
  const TfGrid g = TfGrid::of(nx, ny, nz);
  const size_t n = g.samples();
  const ByteRange rg[6] = {{tsdf_in, 4 * n, "tsdf_in", false}, {weight_in, 4 * n, "weight_in", false},     // (only read: they may be one buffer)
                           {tsdf_out, 4 * n, "tsdf_out", true}, {weight_out, 4 * n, "weight_out", true}, {out_counts, 8, "out_counts", true},
                           {workspace, workspace_bytes, "workspace", true}};
  if (int rc = check_ranges(fn, rg)) return rc;
  const size_t need = gm_tsdf_fill_workspace_bytes(nx, ny, nz);
  if (workspace_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need); return GM_ERR_BUFFER; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const TfWs k = TfWs::from(workspace, g);
  const dim3 bricks((unsigned)g.bricks()), threads(256);
  float* val[2] = {tsdf_out, k.val};
  hipLaunchKernelGGL(tf_init, bricks, threads, 0, s, g, tsdf_in, weight_in, min_weight, val[0], val[1], k.state[0], k.state[1], k.open, out_counts);
  int cur = iterations & 1;                      // the last step writes pair 0: tsdf_out
  for (int t = 0; t < iterations; t++, cur ^= 1)
    hipLaunchKernelGGL(tf_step, bricks, threads, 0, s, g, boundary_free ? 1 : 0, k.open, val[cur], k.state[cur], val[cur ^ 1], k.state[cur ^ 1]);
  hipLaunchKernelGGL(tf_finish, dim3((unsigned)((n + 255) / 256)), threads, 0, s, n, weight_in, k.state[0], fill_weight, weight_out, out_counts);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // extern "C"
