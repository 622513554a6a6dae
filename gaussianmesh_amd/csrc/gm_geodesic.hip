// gm_geodesic.hip -- multi-source shortest-path distances along a proxy mesh (gm_mesh_geodesic): the stage behind
// mesh_region.SurfaceGraph.distances, which grows a picked vertex into a surface region ("everything within r of the click").
//
// THE RESULT IS DEFINED BY ARITHMETIC (the contract gm_closest_face and gm_ray_mesh have).  The input is a weighted graph as a
// symmetric CSR (mesh_region.surface_graph: the mesh's edges plus one unfolded edge across each interior edge), lengths >= 0 in
// float32.  For a source set S
//   d*[v] = min over paths s = p0, p1, .., pk = v, s in S, of the float32 sum taken left to right fl(..fl(fl(0 + l01) + l12).. + l(k-1)k),
//   d* = 0 at sources, +inf where no path arrives; out[v] = d*[v] if d*[v] <= max_distance, else +inf (the cutoff is inclusive).
// Three facts make d* independent of the schedule:
//   (1) fl(d + l) >= d for l >= 0: a path never gets shorter by going on;
//   (2) d <= d' implies fl(d + l) <= fl(d' + l): rounding is monotone;
//   (3) therefore ANY sequence of relaxations d[v] <- min(d[v], fl(d[u] + l_uv)), started from (0 at sources, +inf elsewhere) and run
//       until none lowers anything, ends at d*: every value ever stored is the sum of some path (so >= d*), and by induction along a
//       shortest path with (2) no fixed point lies above d*.  Jacobi, in place, any workgroup order: the same bits, which are also
//       what a float32 Dijkstra gives (tests/geodesic_ref.py).
// A candidate above max_distance is dropped; by (1) every prefix of a shortest path is no longer than the path, so dropping cannot
// change a kept value.  A NaN candidate never wins: the test is cand < d[v].
//
// Structure: gd_fill writes +inf and arms the sweep counters, gd_seed writes 0 at the sources (ids outside [0, Vm) are skipped); then
// `sweeps` launches of gd_sweep on a grid of ceil(Vm / 256) x B, one thread per row (b, v), PULL form: the thread reads its
// neighbours' distances and only it ever stores dist[b][v] - no float atomics.  The update is IN PLACE: a neighbour's value may be the
// one from before the launch or a lower one stored during it, by this workgroup or another; by (3) either is right, a stale one only
// costs sweeps.  Neighbour values are read by relaxed agent-scope loads (they pass the per-CU cache, so values stored earlier in the
// launch are usually seen) and stored likewise; nothing depends on that.  No workgroup waits for another and there is no loop on a
// flag: termination is decided across launch boundaries alone.  Sweep k adds the number of rows it lowered to counter k (one integer
// atomic per workgroup that lowered something) and returns at once when counter k - 1 is zero: a sweep that stored nothing read only
// values from before its launch, the true state, and found every row at its fixed point - `dist` is final.  gd_report copies the last
// counter to *unsettled.
// Tried and dropped (tools/geodesic_time.py): four relaxations of a row per launch instead of one - fewer
// launches, but every pass re-reads the row's neighbours: 0.57 against 0.79 ms at 7.5 k vertices x 8 sets, 392 against 245 ms at 480 k x 8.
//
// Conventions of gm_closest_face: caller workspace, stream-ordered, no device allocation, no host wait anywhere in this file.
#include "gm_common.h"
#include "gm_check.h"
#pragma clang fp contract(off)

namespace gm {

static inline int gd_div_up(int n, int d) { return n > 0 ? (n - 1) / d + 1 : 0; }

__device__ __forceinline__ float gd_load(const float* p) {
  return __uint_as_float(__hip_atomic_load(reinterpret_cast<const unsigned*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void gd_store(float* p, float x) {
  __hip_atomic_store(reinterpret_cast<unsigned*>(p), __float_as_uint(x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// counters[0] = 1 (what came before the first sweep is unknown), counters[1 .. sweeps] = 0; with fill, dist = +inf on a grid (x, B)
__global__ __launch_bounds__(256) void gd_fill(int Vm, float* __restrict__ dist, int fill, int sweeps, int* __restrict__ counters) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.y == 0 && i <= sweeps) counters[i] = i == 0 ? 1 : 0;
  if (fill && i < Vm) dist[(size_t)blockIdx.y * Vm + i] = INFINITY;
}

// grid (x, B): the threads of row b stride over set b's sources
__global__ __launch_bounds__(256) void gd_seed(int Vm, const int* __restrict__ source_offsets, const int* __restrict__ sources,
                                               float* __restrict__ dist) {
  const int b = blockIdx.y;
  const int end = source_offsets[b + 1];
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)source_offsets[b] + blockIdx.x * 256 + threadIdx.x; i < end; i += stride) {
    const int v = sources[i];
    if (v >= 0 && v < Vm) dist[(size_t)b * Vm + v] = 0.f;
  }
}

__global__ __launch_bounds__(256) void gd_sweep(int Vm, const int* __restrict__ row_offsets, const int* __restrict__ cols,
                                                const float* __restrict__ lengths, float max_distance, float* dist,
                                                const int* __restrict__ before, int* __restrict__ lowered) {
  if (*before == 0) return;                               // the sweep before this one lowered nothing: dist is final
  const int v = blockIdx.x * 256 + threadIdx.x;
  int low = 0;
  if (v < Vm) {
    float* row = dist + (size_t)blockIdx.y * Vm;
    const float dv = row[v];
    float best = dv;
    const int e1 = row_offsets[v + 1];
    for (int e = row_offsets[v]; e < e1; e++) {
      const int u = clamp_index(cols[e], Vm);
      const float cand = gd_load(row + u) + lengths[e];
      if (cand <= max_distance && cand < best) best = cand;
    }
    if (best < dv) { gd_store(row + v, best); low = 1; }
  }
  const int n = __syncthreads_count(low);
  if (threadIdx.x == 0 && n) atomicAdd(lowered, n);
}

__global__ void gd_report(const int* __restrict__ last, int* __restrict__ unsettled) { *unsettled = *last; }

}  // namespace gm

// ---------------------------------------------------------------------------------------------
// the entry points (include/gmesh_hip.h): their refusals, then the launches
using namespace gm;

extern "C" {

size_t gm_mesh_geodesic_workspace_bytes(int Vm, int B, int sweeps) {
  (void)Vm; (void)B;                                      // in place: the workspace holds the sweep counters alone
  return ((size_t)(sweeps > 0 ? sweeps : 0) + 1) * sizeof(int) + 256;
}

int gm_mesh_geodesic(int Vm, const int* row_offsets, const int* cols, const float* lengths, int B, const int* source_offsets, const int* sources,
                     float max_distance, int sweeps, int resume, float* dist, int* unsettled, void* workspace, size_t workspace_bytes, void* stream) {
  if (Vm < 0 || B < 0) { set_error("gm_mesh_geodesic: negative size Vm=%d B=%d", Vm, B); return GM_ERR_INVALID_ARG; }
  if (sweeps < 1) { set_error("gm_mesh_geodesic: sweeps must be >= 1; got %d", sweeps); return GM_ERR_INVALID_ARG; }
  if (!(max_distance >= 0.f)) { set_error("gm_mesh_geodesic: max_distance must be >= 0 and not NaN (+inf: no cutoff)"); return GM_ERR_INVALID_ARG; }
  if (Vm == 0) return GM_OK;
  if (B < 1 || B > 65535) { set_error("gm_mesh_geodesic: B must be 1 .. 65535 source sets; got %d", B); return GM_ERR_INVALID_ARG; }
  if (!row_offsets || !cols || !lengths || !source_offsets || !sources || !dist || !unsettled || !workspace) {
    set_error("gm_mesh_geodesic: null pointer"); return GM_ERR_INVALID_ARG;
  }
  const size_t need = gm_mesh_geodesic_workspace_bytes(Vm, B, sweeps);
  if (workspace_bytes < need) { set_error("gm_mesh_geodesic: workspace too small (%zu < %zu)", workspace_bytes, need); return GM_ERR_BUFFER; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int* counters = reinterpret_cast<int*>(workspace);
  const int row_blocks = gd_div_up(Vm, 256), arm_blocks = sweeps / 256 + 1;          // counters 0 .. sweeps
  hipLaunchKernelGGL(gd_fill, dim3(resume ? arm_blocks : (row_blocks > arm_blocks ? row_blocks : arm_blocks), resume ? 1 : B), dim3(256), 0, s, Vm,
                     dist, resume ? 0 : 1, sweeps, counters);
  if (!resume) hipLaunchKernelGGL(gd_seed, dim3(row_blocks, B), dim3(256), 0, s, Vm, source_offsets, sources, dist);
  for (int k = 1; k <= sweeps; k++)
    hipLaunchKernelGGL(gd_sweep, dim3(row_blocks, B), dim3(256), 0, s, Vm, row_offsets, cols, lengths, max_distance, dist, counters + k - 1,
                       counters + k);
  hipLaunchKernelGGL(gd_report, dim3(1), dim3(1), 0, s, counters + sweeps, unsettled);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // extern "C"
