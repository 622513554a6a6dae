// gm_render.hip -- per-tile alpha blending, forward and backward.
//
// Replaces (reference, RAST = gaussian_renderer/diff_gaussian_rasterizater/cuda_rasterizer):
//   RAST/forward.cu:261-374   renderCUDA (forward)
//   RAST/backward.cu:399-557  renderCUDA (backward)
//
// CDNA4 mapping: the reference gives each 16x16 tile to a 256-thread block that stages
// 256-entry batches in shared memory behind two block barriers and lets every pixel thread re-read the batch from LDS
// (and the colour from global memory).  Here a 16x16 tile is four independent wave64s, each owning one 8x8 pixel
// quadrant (one pixel per lane, lane = y * 8 + x) and launched as a one-wave workgroup:
//   * the wave walks the list of its PARENT tile (gm_common.h: emission policies); a two-stage front end (Gather, FwdLds /
//     BwdLds below) turns it into dense batches of up to 64 candidate records: a scan of the contiguous (key, id) stream picks
//     the entries whose key carries the tile's child bit, their records are gathered into registers two iterations ahead of
//     their use;
//   * while lane j holds candidate j it tests, once per batch and for all 64 in parallel, whether the entry can reach
//     alpha >= 1/255 anywhere inside the bounding box of the quadrant's still-live pixels (exact minimum of the conic's
//     quadratic form over the rectangle, with a rounding margin).  The cull is conservative: a culled entry would have been
//     skipped by every live pixel (alpha < 1/255), so results and n_contrib are unchanged;
//   * forward: the survivors' exponents come from the matrix core, 16 survivors x 64 pixels per three chained
//     v_mfma_f32_32x32x2_f32 (see render_fwd_kernel); the vector ALU keeps exp, the alpha decisions and the T / C recurrence;
//   * backward: a scalar suffix recurrence per pixel, then (weight, h) per pixel through an LDS slot matrix into a row-parallel
//     fold of the nine gradient sums and one atomic instruction per seven 36-byte records (see render_bwd_kernel);
//   * no s_barrier; "is every pixel done" is a ballot instead of __syncthreads_count.
// Discrete semantics are the reference's - skip alpha < 1/255, stop (without applying the entry) when T (1 - alpha) < 1e-4,
// n_contrib = 1-based list position of the last accepted entry - except that "skip power > 0" is "power := min(power, 0)"
// (see render_fwd_kernel: the two differ only where the reference's own rounding decides).
// FMA contraction is allowed here and exp() is v_exp_f32 on power * log2(e); see DESIGN.md for the tolerance argument.
#include "gm_common.h"
#include "gm_cull.h"
#include "gm_tile_order.h"
#include <cstdlib>

namespace gm {

#define LOG2E 1.4426950408889634f

__device__ __forceinline__ float bcast(float v, int j) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

// Workgroup -> 16-px tile, its parent tile (whose list it walks) and its bit in the instance keys' child mask.
// Consecutive workgroup ids go to consecutive XCDs (8 of them, each with its own L2), so the 2^s x 2^s children of
// a parent are given ids that are 8 apart: they run on the same XCD and share the parent's list and records in L2.
struct TileMap {
  int gx, gy, pgx, pgy, s;
  const uint32_t* order;        // list tiles by descending list length
  __device__ __forceinline__ bool locate(int b, int& tx, int& ty, int& parent, uint32_t& child_bit) const {
    const int nch = 1 << (2 * s);
    const int xcd = b & 7, j = b >> 3;
    const int slot = (j >> (2 * s)) * 8 + xcd, c = j & (nch - 1);
    if (slot >= pgx * pgy) return false;
    const int p = (int)order[slot];
    const int py = p / pgx, px = p - py * pgx;
    const int cy = c >> s, cx = c & ((1 << s) - 1);
    tx = (px << s) + cx; ty = (py << s) + cy;
    parent = p;
    child_bit = 1u << (GM_KEY_MASK_SHIFT + c);
    return tx < gx && ty < gy;
  }
  int blocks() const { return ((pgx * pgy + 7) / 8) * 8 << (2 * s); }
};

// Policy 2 (32-px parents): the key's mask has one bit per 8x8 QUADRANT of the parent, bit qy * 4 + qx; quadrant (wave & 1, wave >> 1)
// of tile (tx, ty) is quadrant (2 (tx & 1) + (wave & 1), 2 (ty & 1) + (wave >> 1)) of its parent.
__device__ __forceinline__ uint32_t quadrant_bit(int tx, int ty, int wave) {
  return 1u << (GM_KEY_MASK_SHIFT + (2 * (ty & 1) + (wave >> 1)) * 4 + 2 * (tx & 1) + (wave & 1));
}

// Dispatch order of the blend kernels (gm_tile_order.h) as a launch of its own: only when the tile pass did not produce it.
__global__ __launch_bounds__(1024) void tile_order_kernel(const uint2* __restrict__ ranges, int tiles, uint32_t* __restrict__ order,
                                                          uint32_t* __restrict__ hint, uint32_t* __restrict__ epoch,
                                                          uint32_t* __restrict__ scratch) {
  __shared__ uint32_t cnt[256];
  __shared__ uint32_t wsum[16];
  tile_order_block<1024>(ranges, tiles, order, cnt, wsum, hint, epoch, scratch);
}

// Dispatch order of the BACKWARD blend.  What a quadrant's wave has to walk is known exactly after the forward: the list
// up to the deepest contributor of its pixels (n_contrib); list length says little (a 12 k-entry list that saturates after
// 200 entries is cheap, a 1.5 k-entry silhouette list walked to the end is not).  One workgroup per list tile takes the maximum
// of n_contrib over the tile's area, one workgroup sorts the tiles by it.
__global__ __launch_bounds__(256) void tile_work_kernel(const uint32_t* __restrict__ n_contrib, int W, int H, int pgx, int shift,
                                                        uint32_t* __restrict__ work) {
  __shared__ uint32_t part[4];
  const int p = blockIdx.x, py = p / pgx, px = p - py * pgx;
  const int side = GM_TILE << shift;                          // 16, 32 or 64 pixels
  const int x0 = px * side, y0 = py * side;
  uint32_t m = 0;
  for (int i = threadIdx.x; i < side * side; i += 256) {
    const int x = x0 + (i & (side - 1)), y = y0 + (i >> (4 + shift));
    if (x < W && y < H) m = max(m, n_contrib[(size_t)y * W + x]);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) work[p] = max(max(part[0], part[1]), max(part[2], part[3]));
}
__global__ __launch_bounds__(1024) void tile_order_work_kernel(const uint32_t* __restrict__ work, int tiles, uint32_t* __restrict__ order) {
  __shared__ uint32_t cnt[256];
  __shared__ uint32_t wsum[16];
  tile_order_by<1024>([&](int t) { return work[t]; }, tiles, order, cnt, wsum);
}

int launch_tile_order(ImageState& img, int tiles, uint32_t* work_hint, int debug, hipStream_t s) {
  StageScope sc(ST_RANGES, s);
  hipLaunchKernelGGL(tile_order_kernel, dim3(1), dim3(1024), 0, s, img.ranges, tiles, img.tile_order, work_hint, img.epoch, img.tile_work);   // tile_work: scratch here, the backward fills it anew
  GM_LAUNCH_CHECK(debug, s);
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Front end shared by both blend kernels: from the parent tile's list to dense batches of candidate records.
//   stage A (key scan): every iteration the wave looks at up to RQ_K chunks of 64 consecutive (key, id) pairs (loaded the
//            iteration before, 512 contiguous bytes per chunk) and appends the entries whose key carries this tile's child
//            bit, in list order, to a wave-private ring of (id, list position) in LDS - one ballot + mbcnt per chunk;
//   stage B (gather): up to 64 candidates are popped (lane j <- candidate j) and their 36-byte splat records loaded into
//            registers; three register sets rotate (being issued / in flight / being consumed), so the batch issued in
//            iteration i is consumed in iteration i + 2 and the dependent chain list position -> id -> record never stalls
//            a wave that finds few entries of its own.
// Each iteration issues exactly RQ_K pair loads followed by 3 record loads (clamped addresses when there is nothing to
// fetch), so `s_waitcnt vmcnt(3)` at the top of an iteration means "everything except the gather issued last iteration
// has landed"; left to itself the compiler puts vmcnt(0) in the middle of the iteration.  A batch holds up to 64 REAL
// candidates instead of the ~16 of 64 list entries that concern a 16-px tile of a 32-px parent: the per-batch work
// (culling, staging) is paid a quarter as often and nothing is fetched for entries of the other children.
// (Measured and dropped: the same front end with the records landing in a three-slot LDS ring by LDS-DMA instead of
// registers - 10 KiB of LDS per wave, 3-4 workgroups per CU instead of 6: render 0.19-0.22 ms against 0.18 before.)
#define RQ_K 4                   // key chunks scanned per iteration
#define RQ_QA 128                // candidate ring entries per wave (power of two)

struct Gather {                  // lane j: record of candidate j
  float4 a;                      // x, y, conic.x, conic.y
  float4 b;                      // conic.z, opacity, r, g
  float c;                       // b
  uint32_t id, pos;              // Gaussian id, list position
};
// exponent of one staged entry at one pixel, e = power * log2(e), on the packed-f32 pipe (v_pk_add / v_pk_mul operate on a
// register PAIR in one issue slot): d = (x, y) - pix, q = (a', c') * d, q.x += b' d.y, e = q.x d.x + q.y d.y.
// Staged record: RA = (x, y, a', c'), RB = (b', opacity, r, g) with a' = -log2e/2 conic.x, b' = -log2e conic.y, c' = -log2e/2 conic.z.
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float staged_exponent(const float4& RA, float bq, v2f pix, v2f& d) {
  const v2f xy = {RA.x, RA.y}, ac = {RA.z, RA.w};
  d = xy - pix;
  v2f q = ac * d;
  q.x = __builtin_fmaf(bq, d.y, q.x);
  const v2f r = q * d;
  return r.x + r.y;
}

__device__ __forceinline__ Gather issue_gather(const float4* __restrict__ splat, uint2 cand) {
  Gather g;
  g.a = splat_row(splat, (size_t)cand.x, 0); g.b = splat_row(splat, (size_t)cand.x, 1); g.c = splat_blue(splat, (size_t)cand.x);
  g.id = cand.x; g.pos = cand.y;
  return g;
}

// ---------------------------------------------------------------------------------------------
// Forward blend, round 3: the exponent of every (survivor, pixel) pair comes from the MATRIX core.
//
// With c = (cx, cy) the pixel's offset from the centre of its 8x4 half of the quadrant and (u, v) the splat centre's offset
// from the same point, the exponent e = log2(e) * power is a quadratic polynomial in c whose six coefficients depend on the
// survivor only:   e = a' cx^2 + b' cx cy + c' cy^2 + (-2a'u - b'v) cx + (-b'u - 2c'v) cy + (a'u^2 + b'uv + c'v^2).
// For 16 survivors and the 64 pixels of the wave that is D[32 x 32] = A[32 x 6] B[6 x 32]: row (half h, survivor s) of A holds
// survivor s's coefficients about the centre of half h, column j of B the six monomials of pixel j of a half - three chained
// v_mfma_f32_32x32x2_f32.  Row 8 (s / 4) + 4 h + s % 4 lands in register s of the lanes of half h (tools/mfma_probe/probe32.hip),
// i.e. lane = pixel ends up with the exponents of the 16 survivors in 16 registers, which is exactly what the per-pixel
// recurrence wants.  The coefficients are computed once per candidate, lane-parallel, when the batch is staged, and fetched
// as three 4-byte LDS reads per lane and group; what is still broadcast per survivor is (r, g, b, opacity).
// Per survivor the vector ALU keeps exp, the opacity product, the two alpha decisions and the T / C recurrence: ~13
// instructions instead of ~20, and the LDS return traffic drops from 40 to ~17 bytes per lane.  192 matrix cycles per 16
// survivors ride beside ~800 vector cycles.
// Arithmetic: the polynomial is evaluated about a point at most 3.5 / 1.5 pixels away from every pixel, so its terms are at most
// a few tens for the narrowest splat the 0.3-px^2 low-pass filter allows; the matrix core sums the six products to within 2 ulp
// of the largest (probe32: 1.2e-7 of the sum of magnitudes): |e - e_exact| <~ 1e-5, alpha to ~1e-5 relative (the pixel-relative
// form of round 2: ~5e-7).  Because e now carries an absolute error, the reference's "skip when power > 0" (a guard against
// rounding at the splat's own centre, where power = -0 +- 1e-7) becomes e := min(e, 0): skipping would drop a splat at its
// brightest pixel whenever the polynomial came out at +1e-6.  The backward kernel clamps likewise.
typedef float v16f __attribute__((ext_vector_type(16)));

// The A-operand table of the exponent polynomial (image-only frames; a training step's two halves take the SAME alpha >= 1/255 decision
// for every (entry, pixel) - backward.cu repeats forward.cu's expression for exactly that reason - by both using staged_exponent: EXACT
// below.  The other way round, the backward on this polynomial, was built in round 4 and measured 26 % slower: NOTEBOOK.md section 2,
// tools/experiments/render_bwd_matrix_exponent_round4.hip.txt).  ct[4 * 6 * 32]: [group of 16 survivors][monomial][MFMA row]; row of (half h,
// survivor sg of the group) = 8 (sg / 4) + 4 h + sg % 4.  e' = log2(e) power + log2(opacity): the opacity rides in the constant
// coefficient, so that 2^e' IS opacity * G and the per-survivor opacity product (and its broadcast) is gone from both kernels.
// Contraction is off and every product is spelled out: every build of the kernel must produce bit-identical coefficients, whatever the
// compiler would fuse in one of them.  (ucx, vcy): centre of half 0 of the wave's quadrant; half 1 lies four rows below.
#define GM_POLY_PAD -1.0e30f      // constant coefficient of a row that holds no survivor: 2^e' = 0, the entry is skipped by every pixel
__device__ __forceinline__ void stage_poly(float* __restrict__ ct, int slot, float x, float y, float conx, float cony, float conz, float opacity,
                                           float ucx, float vcy, float kshift = 0.0f) {
#pragma clang fp contract(off)
  const int g = slot >> 4, sg = slot & 15;
  const float a = (-0.5f * LOG2E) * conx, b = (-LOG2E) * cony, c = (-0.5f * LOG2E) * conz;
  const float u = x - ucx, v0 = y - vcy, v1 = v0 - 4.0f;
  // log2(opacity) (v_log_f32); a conic that is not positive (an overflowing or rounded-away determinant in the preprocess) has
  // power > 0 wherever the reference evaluates it and is skipped there (forward.cu:336): the row is padded out
  const float au = a * u, bu = b * u, lo = (conx > 0.f && conz > 0.f) ? __builtin_amdgcn_logf(opacity) + kshift : GM_POLY_PAD;
  float* row = &ct[192 * g + 8 * (sg >> 2) + (sg & 3)];                           // row of (half 0, survivor sg); half 1: + 4
  row[0] = a; row[4] = a; row[32] = b; row[36] = b; row[64] = c; row[68] = c;
  row[96] = -2.0f * au - b * v0;  row[100] = -2.0f * au - b * v1;
  row[128] = -bu - 2.0f * c * v0; row[132] = -bu - 2.0f * c * v1;
  row[160] = (u * (au + b * v0) + c * v0 * v0) + lo; row[164] = (u * (au + b * v1) + c * v1 * v1) + lo;
}
__device__ __forceinline__ void pad_poly(float* __restrict__ ct, int slot) {       // slot < 64
  float* row = &ct[192 * (slot >> 4) + 8 * ((slot & 15) >> 2) + (slot & 3)];
  row[160] = GM_POLY_PAD; row[164] = GM_POLY_PAD;
}
// the three chained steps; B0 / B1 / B2: the lane's monomials (cx^2 | cx cy), (cy^2 | cx), (cy | 1) for k = lane / 32
__device__ __forceinline__ v16f poly_exponents(const float* __restrict__ ct, int j, int lane, float B0, float B1, float B2) {
  const float* ctg = &ct[12 * j + lane];                                          // 192 (j / 16) + lane
  const float A0 = ctg[0], A1 = ctg[64], A2 = ctg[128];
  v16f E = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  E = __builtin_amdgcn_mfma_f32_32x32x2f32(A0, B0, E, 0, 0, 0);
  E = __builtin_amdgcn_mfma_f32_32x32x2f32(A1, B1, E, 0, 0, 0);
  E = __builtin_amdgcn_mfma_f32_32x32x2f32(A2, B2, E, 0, 0, 0);
  return E;
}
// The matrix-core forward folds min(0.99, .) into the exponent: 2^(e' - log2 0.99) with v_exp's clamp bit IS alpha / 0.99; the factor
// 0.99 rides in the staged colours and in T - 0.99 w' (10 instead of 11 vector instructions per survivor).  The EXACT build keeps `min`.
// Alternates that were compile-time switches until round 6 (three register sets, unfolded clamp, 256-thread workgroups) and their
// numbers: tools/experiments/render_blend_compile_time_alternates_round5.hip.txt.
#define GM_FWD_SUB 4              // survivors whose alpha evaluations interleave in the forward recurrence
struct RenderFrames {            // the frames of a batched forward blend (gridDim.z): buffer distances + where each frame's status words go
  int frames;
  FrameOfs go, bo, io, co;
  int* status[GM_BATCH_MAX];
};
struct FwdLds {                  // per wave: 5.1 KiB
  uint2 qa[RQ_QA];               // candidate ring: (Gaussian id, list position)
  float ct[4 * 6 * 32];          // [group of 16 survivors][monomial][MFMA row]: lane l of MFMA step m reads ct[192 g + 64 m + l]
  float4 sb[68];                 // (r, g, b, opacity) per survivor (+ 4 entries of padding with opacity 0 behind the last)
};

// STATE = false: image-only frame (GM_FWD_IMAGE_ONLY) - final_T / n_contrib, which only a backward pass reads, are neither
// tracked nor written.  TRACE: per-wave start / end / list length / iterations / candidates / survivors (tools/wave_trace.py).
// EXACT (GM_FWD_EXACT_EXPONENT: the forward of a training step; gm_debug_forward_exact_exponent forces it for every frame): the exponents of a group come from the
// pixel-relative form of round 2 / of the backward kernel (staged_exponent: |e - e_exact| ~ 5e-7) instead of the matrix core's
// polynomial (~1e-5).  Everything else - lists, cull, decisions, recurrence - is the same code, so the two builds may differ only
// where an entry's alpha or a pixel's T sits within the polynomial's error of a threshold (tests/test_gpu_parity.py).
// AUX (gm_forward_1_aux; a batch: render_fwd_aux_batch_kernel): the blend also writes the per-pixel maps out_alpha = 1 - T_final (the float T of the colour
// output) and out_depth = sum alpha_i T_i z_i over the accepted entries, z_i = the view-space depth the preprocess left in depth_key
// (not normalised, no background term; either map may be NULL).  The survivors' z is gathered from depth_key when a batch is staged -
// 4 bytes per survivor, the 36-byte record stays as it is.  A frame whose depth_key is stale (aux_latch[GM_CNT_DEPTH_STALE], set by a
// direct-placement first half) is refused: background, alpha = depth = 0, status word 3 = 3.  The AUX = false instantiations are the
// render_fwd_kernel<STATE, TRACE, EXACT> below: every AUX term is compiled out of them.
// The body is TEXT (gm_render_fwd_body.inc) included into both kernels, not a __device__ function they call: called through a function,
// the plain kernels came out with other instructions (sign extensions, a reordered copy) - the AUX variant was to leave them exactly as they
// were.  For the same reason the AUX accumulator and its reads are under `#if GM_BLEND_AUX`: a name the lambdas of the body merely mention
// is captured, and a capture changes the register allocation of the plain kernels.
template <bool STATE, bool TRACE, bool EXACT = false>
__global__ __launch_bounds__(64) void render_fwd_kernel(const uint2* __restrict__ ranges, const uint2* __restrict__ pairs,
                                                        const float4* __restrict__ splat, int W, int H, TileMap tm,
                                                        const float* __restrict__ bg, float* __restrict__ out_color,
                                                        float* __restrict__ final_T, uint32_t* __restrict__ n_contrib,
                                                        unsigned long long* __restrict__ trace,
                                                        const uint32_t* __restrict__ counters, int* __restrict__ status_host,
                                                        uint32_t* __restrict__ hint, const uint32_t* __restrict__ epoch, const RenderFrames rf) {
  constexpr bool AUX = false;
  const uint32_t* const depth_key = nullptr;
  uint32_t* const aux_latch = nullptr;
#define GM_BLEND_AUX 0
#include "gm_render_fwd_body.inc"
#undef GM_BLEND_AUX
}
template <bool STATE, bool EXACT>
__global__ __launch_bounds__(64) void render_fwd_aux_kernel(const uint2* __restrict__ ranges, const uint2* __restrict__ pairs,
                                                            const float4* __restrict__ splat, int W, int H, TileMap tm,
                                                            const float* __restrict__ bg, float* __restrict__ out_color,
                                                            float* __restrict__ final_T, uint32_t* __restrict__ n_contrib,
                                                            const uint32_t* __restrict__ counters, int* __restrict__ status_host,
                                                            uint32_t* __restrict__ hint, const uint32_t* __restrict__ epoch, const RenderFrames rf,
                                                            const uint32_t* __restrict__ depth_key, float* __restrict__ out_depth,
                                                            float* __restrict__ out_alpha, uint32_t* __restrict__ aux_latch) {
  constexpr bool AUX = true, TRACE = false;
  unsigned long long* const trace = nullptr;
#define GM_BLEND_AUX 1
#include "gm_render_fwd_body.inc"
#undef GM_BLEND_AUX
}
// The AUX blend of a batch (gm_forward_deformed_batch_aux_async): render_fwd_aux_kernel whose frame blockIdx.z also reads depth_key and
// the latch of its own geometry buffer (rf.go) and writes its maps at its own distances (dofs, aofs: not part of RenderFrames, which the
// plain kernels take).  A kernel of its own rather than a template parameter: the single-frame AUX kernels keep their names, argument
// lists and instructions.
template <bool STATE, bool EXACT>
__global__ __launch_bounds__(64) void render_fwd_aux_batch_kernel(const uint2* __restrict__ ranges, const uint2* __restrict__ pairs,
                                                                  const float4* __restrict__ splat, int W, int H, TileMap tm,
                                                                  const float* __restrict__ bg, float* __restrict__ out_color,
                                                                  float* __restrict__ final_T, uint32_t* __restrict__ n_contrib,
                                                                  const uint32_t* __restrict__ counters, int* __restrict__ status_host,
                                                                  uint32_t* __restrict__ hint, const uint32_t* __restrict__ epoch, const RenderFrames rf,
                                                                  const uint32_t* __restrict__ depth_key, float* __restrict__ out_depth,
                                                                  float* __restrict__ out_alpha, uint32_t* __restrict__ aux_latch,
                                                                  const FrameOfs dofs, const FrameOfs aofs) {
  constexpr bool AUX = true, TRACE = false;
  unsigned long long* const trace = nullptr;
  depth_key = frame_ptr(depth_key, rf.go); aux_latch = frame_ptr(aux_latch, rf.go);
  out_depth = frame_ptr(out_depth, dofs); out_alpha = frame_ptr(out_alpha, aofs);
#define GM_BLEND_AUX 1
#include "gm_render_fwd_body.inc"
#undef GM_BLEND_AUX
}

static unsigned long long* g_render_trace = nullptr;      // debugging aid (tools/wave_trace.py), never set by the package
extern "C" void gm_debug_render_trace(void* buffer) { g_render_trace = reinterpret_cast<unsigned long long*>(buffer); }
static float* g_bwd_front_T = nullptr;                   // verification aid (tests only): see render_bwd_kernel
extern "C" void gm_debug_backward_front_T(void* plane) { g_bwd_front_T = reinterpret_cast<float*>(plane); }
static bool g_fwd_exact = false;                          // verification aid (tests only): the EXACT build of the forward blend for EVERY frame
extern "C" void gm_debug_forward_exact_exponent(int on) { g_fwd_exact = on != 0; }

int launch_render_fwd(const GeomState& g, const uint2* pairs, ImageState& img, int W, int H, int mode,
                      const float* background, float* out_color, int* status_host, bool image_only, uint32_t* work_hint, int debug,
                      hipStream_t s, bool exact_exponent, const BatchOfs* bt, float* out_depth, float* out_alpha, bool aux,
                      uint32_t* aux_latch) {
  StageScope sc(ST_RENDER, s);
  const TileGrid tg(W, H, mode);
  const TileMap tm{tg.gx, tg.gy, tg.pgx, tg.pgy, tg.s, img.tile_order};
  RenderFrames rf{};
  rf.frames = 1;
  if (bt) {
    rf.frames = bt->frames; rf.go = bt->geom; rf.bo = bt->binning; rf.io = bt->image; rf.co = bt->color;
    for (int f = 0; f < GM_BATCH_MAX; f++) rf.status[f] = bt->status[f];
  }
  if (rf.frames > 1 && tg.ptiles <= 0) { set_error("batched blend: empty tile grid"); return 1; }
  if (tg.ptiles > 0) {
    const dim3 grid(tm.blocks() * 4, 1, (uint32_t)rf.frames), block(64);     // one wave (8x8 quadrant) per workgroup
    const bool exact = g_fwd_exact || exact_exponent;
    if (aux && bt) {
#define GM_AUX_ARGS grid, block, 0, s, img.ranges, pairs, g.splat, W, H, tm, background, out_color, img.final_T, img.n_contrib, g.counters, status_host, \
                    work_hint, img.epoch, rf, g.depth_key, out_depth, out_alpha, aux_latch, bt->depth, bt->alpha
      if (exact) hipLaunchKernelGGL((render_fwd_aux_batch_kernel<true, true>), GM_AUX_ARGS);
      else if (image_only) hipLaunchKernelGGL((render_fwd_aux_batch_kernel<false, false>), GM_AUX_ARGS);
      else hipLaunchKernelGGL((render_fwd_aux_batch_kernel<true, false>), GM_AUX_ARGS);
#undef GM_AUX_ARGS
    } else if (aux) {
#define GM_AUX_ARGS grid, block, 0, s, img.ranges, pairs, g.splat, W, H, tm, background, out_color, img.final_T, img.n_contrib, g.counters, status_host, \
                    work_hint, img.epoch, rf, g.depth_key, out_depth, out_alpha, aux_latch
      if (exact) hipLaunchKernelGGL((render_fwd_aux_kernel<true, true>), GM_AUX_ARGS);   // (as below: the EXACT build keeps the state)
      else if (image_only) hipLaunchKernelGGL((render_fwd_aux_kernel<false, false>), GM_AUX_ARGS);
      else hipLaunchKernelGGL((render_fwd_aux_kernel<true, false>), GM_AUX_ARGS);
#undef GM_AUX_ARGS
    } else if (g_fwd_exact || exact_exponent)
      hipLaunchKernelGGL((render_fwd_kernel<true, false, true>), grid, block, 0, s, img.ranges, pairs, g.splat, W, H, tm,
                         background, out_color, img.final_T, img.n_contrib, nullptr, g.counters, status_host, work_hint, img.epoch, rf);
    else if (g_render_trace)
      hipLaunchKernelGGL((render_fwd_kernel<true, true>), grid, block, 0, s, img.ranges, pairs, g.splat, W, H, tm,
                         background, out_color, img.final_T, img.n_contrib, g_render_trace, g.counters, status_host, work_hint, img.epoch, rf);
    else if (image_only)
      hipLaunchKernelGGL((render_fwd_kernel<false, false>), grid, block, 0, s, img.ranges, pairs, g.splat, W, H, tm,
                         background, out_color, img.final_T, img.n_contrib, nullptr, g.counters, status_host, work_hint, img.epoch, rf);
    else
      hipLaunchKernelGGL((render_fwd_kernel<true, false>), grid, block, 0, s, img.ranges, pairs, g.splat, W, H, tm,
                         background, out_color, img.final_T, img.n_contrib, nullptr, g.counters, status_host, work_hint, img.epoch, rf);
  } else if (status_host) {
    GM_HIP(hipMemcpyAsync(status_host, g.counters, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  GM_LAUNCH_CHECK(debug, s);
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Backward blend.
#define GM_ACC_STRIDE 12   // floats per Gaussian in grad_acc: dcolor rgb (0-2), moments of h: 1, dx, dy, dx^2, dx dy, dy^2 (3-8)


// Backward blend, two phases per wave (round 3).  The exponent of an entry is evaluated per pixel in the pixel-relative form
// (staged_exponent, |e - e_exact| ~ 5e-7) and the opacity multiplied in afterwards; the forward's come from the matrix core (~1e-5), so
// the two halves can disagree on an entry whose alpha lies within 1e-5 of 1/255 (weight <= 0.4 %).  Round 4 built
// the backward on the matrix core with the forward's polynomial - identical decisions, every gradient test green - and it was 26 % slower:
// tools/experiments/render_bwd_matrix_exponent_round4.hip.txt.
//
// Phase 1, lane = pixel: the walk of backward.cu:441-556 with everything that is not the per-pixel recurrence taken out.
// Going back to front, with T_i the transmittance in front of entry i, w_i = alpha_i T_i and cd_i = c_i . dL/dpixel,
//   dL/dalpha_i = T_i cd_i - (A_i + T_final bg . dL/dpixel) / (1 - alpha_i),   A_{i-1} = A_i + w_i cd_i
// (the reference carries the three-channel `accum_rec` = A / T and the last colour / alpha for the same quantity: one
// scalar recurrence instead of three vector ones).  An entry a lane does not take gets alpha = 0, which makes every update
// the identity - no execution-mask juggling.  All an entry leaves behind per pixel are the two factors every gradient sum is
// a multiple of: w (dL/dcolour) and h = G dL/dG.  They go to a row of an LDS matrix M[slot][pixel]; the entry's centre and
// id are kept per slot.  Entries no pixel of the wave takes use no slot.
// Phase 2, lane = (pixel row r, slot es), once per SEVEN used slots: each lane folds the eight pixels of its row into the nine
// sums of its slot's Gaussian - dL/dcolour rgb and the six moments (1, dx, dy, dx^2, dx dy, dy^2) of h, dy being constant
// along a row - six vector instructions per pixel, no cross-lane traffic; the eight row partials of a slot meet through LDS
// (written [row][slot * 9 + value], read back by lane = slot * 9 + value: both conflict-free), and ONE atomic instruction
// with 63 active lanes commits seven 36-byte records (one L2 transaction per record, as before).
// Per entry: ~28 + ~9 vector instructions instead of ~44 + 28 for the per-entry cross-lane reduction of round 2
// (v_permlane32/16_swap + DPP butterfly), which is gone.
struct StagedB {                 // one survivor of the staged batch (one LDS address per entry in the walk)
  float4 a;                      // x, y, conic.x', conic.z'   (conic pre-multiplied for the exp2 argument)
  float4 b;                      // conic.y', opacity, r, g
  float4 c;                      // b, list position (bits), Gaussian id (bits), -
};
struct SlotB { float2 xy; uint32_t id, pad; };   // splat centre and id of a phase-2 slot
struct BwdLds {                  // per wave: 7.7 KiB
  uint2 qa[RQ_QA];               // candidate ring of the front end: (Gaussian id, list position)
  StagedB st[64];                // staged batch
  union {
    float2 M[7][65];             // (w, h) per slot and pixel; row stride 65 keeps phase 2's row reads conflict-free
    float part[8][72];           // phase 2: row partials [row][slot * 9 + value] (columns 63.. belong to the idle lanes)
    struct { float2 rg[64]; float bl[64]; } dpt;   // kernel start only: dL/dpixel of every pixel
  };
  SlotB slot[8];
};

//
// AUX (gm_backward_aux): the depth and alpha maps are two more colour channels with background 0 - colour z_i (depth_key) and 1.
// Their gradients (dL_ddepth / dL_dalpha [H, W], either may be NULL) enter cd_i = c_i . dL/dpixel + z_i dL/ddepth + dL/dalpha, and so
// dL/dalpha_i and the A recurrence; dL/dz_i = sum over pixels of w dL/ddepth is folded in phase 2 and committed to grad_acc[12 i + 9]
// (a word the colour backward leaves at zero).  The AUX = false instantiation is render_bwd_kernel below; the body is included text, as
// render_fwd_kernel's (gm_render_bwd_body.inc).
__global__ __launch_bounds__(64) void render_bwd_kernel(const uint2* __restrict__ ranges,
                                                               const uint2* __restrict__ pairs,
                                                               const float4* __restrict__ splat, int W, int H, TileMap tm,
                                                               const float* __restrict__ bg, const float* __restrict__ final_T,
                                                               const uint32_t* __restrict__ n_contrib,
                                                               const float* __restrict__ dL_dpix, float* __restrict__ grad_acc,
                                                               const uint32_t* __restrict__ counters, int mode, float* __restrict__ front_T) {
  constexpr bool AUX = false;
  const uint32_t* const depth_key = nullptr;
  const float* const dL_ddepth = nullptr;
  const float* const dL_dalpha = nullptr;
#include "gm_render_bwd_body.inc"
}
__global__ __launch_bounds__(64) void render_bwd_aux_kernel(const uint2* __restrict__ ranges, const uint2* __restrict__ pairs,
                                                            const float4* __restrict__ splat, int W, int H, TileMap tm,
                                                            const float* __restrict__ bg, const float* __restrict__ final_T,
                                                            const uint32_t* __restrict__ n_contrib,
                                                            const float* __restrict__ dL_dpix, float* __restrict__ grad_acc,
                                                            const uint32_t* __restrict__ counters, int mode, float* __restrict__ front_T,
                                                            const uint32_t* __restrict__ depth_key, const float* __restrict__ dL_ddepth,
                                                            const float* __restrict__ dL_dalpha) {
  constexpr bool AUX = true;
#include "gm_render_bwd_body.inc"
}


int launch_render_bwd(const GeomState& g, const uint2* pairs, ImageState& img, int W, int H, int mode,
                      const float* background, const float* dL_dpix, int debug, hipStream_t s, bool aux, const float* dL_ddepth,
                      const float* dL_dalpha) {
  StageScope sc(ST_RENDER_BWD, s);
  const TileGrid tg(W, H, mode);
  const TileMap tm{tg.gx, tg.gy, tg.pgx, tg.pgy, tg.s, img.tile_order_bwd};
  if (tg.ptiles > 0) {
    hipLaunchKernelGGL(tile_work_kernel, dim3(tg.ptiles), dim3(256), 0, s, img.n_contrib, W, H, tg.pgx, tg.s, img.tile_work);
    hipLaunchKernelGGL(tile_order_work_kernel, dim3(1), dim3(1024), 0, s, img.tile_work, tg.ptiles, img.tile_order_bwd);
  }
  if (tg.ptiles > 0 && aux)
    hipLaunchKernelGGL(render_bwd_aux_kernel, dim3(tm.blocks() * 4), dim3(64), 0, s, img.ranges, pairs, g.splat, W, H, tm,
                       background, img.final_T, img.n_contrib, dL_dpix, g.grad_acc, g.counters, mode, g_bwd_front_T, g.depth_key, dL_ddepth, dL_dalpha);
  else if (tg.ptiles > 0)
    hipLaunchKernelGGL(render_bwd_kernel, dim3(tm.blocks() * 4), dim3(64), 0, s, img.ranges, pairs, g.splat, W, H, tm,
                       background, img.final_T, img.n_contrib, dL_dpix, g.grad_acc, g.counters, mode, g_bwd_front_T);
  GM_LAUNCH_CHECK(debug, s);
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Per-Gaussian blend weights (gm_blend_weights): the forward's walk, scattering per Gaussian instead of writing per pixel.
//
// The weight of an (entry, pixel) pair, w = alpha T - the float the colour blend multiplies the entry's colour by - exists only inside the
// blend kernels.  This one repeats the walk of the EXACT forward (same front end, same cull, staged_exponent, the same decisions and the same
// T recurrence, instruction for instruction: T (1 - alpha) is ONE fused multiply-add there, -alpha T + T, and is spelled as one here) and keeps,
// per Gaussian and summed over the pixels of the frame,
//   sums[i][0] += u,  sums[i][1] += u k,  peak[i] = max(peak[i], bits(w)),   u = rint(w 2^24) (w <= 0.99: exact in a u32), k = the pixel's mask byte.
// Integers, so that the result does not depend on the order in which waves, policies or views arrive.
// Phase 1, lane = pixel, 16 survivors at a time: w of every (survivor, pixel) pair goes to an LDS matrix M[survivor][pixel].
// Phase 2, lane = (survivor es = lane / 4, quarter qd = lane % 4): each lane folds 16 pixels of its survivor (row stride 65: the 64 lanes read 64
// different banks), two cross-lane steps join the quarters, and the totals of the batch's up to 64 survivors wait in LDS until the batch is done:
// then lane j commits survivor j - one 64-bit atomic add per non-zero sum and one atomic max, issued from as many lanes of one instruction as the
// batch has survivors with a weight (the backward blend's shape).  u k <= 0.99 * 2^24 * 255 < 2^32, a wave's sum of u < 2^30.
struct WgtLds {                  // per wave: 8.2 KiB
  uint2 qa[RQ_QA];               // candidate ring of the front end
  float4 ra[68];                 // staged batch: (x, y, a', c'), b', opacity, Gaussian id (+ 4 entries of padding with opacity 0 behind the last)
  float bq[68];
  float op[68];
  uint32_t id[64];
  float M[16][65];               // w per (survivor of the group, pixel)
  uint32_t kk[64];               // mask byte per pixel (kernel start)
  uint32_t rt[64], rp[64];       // per survivor of the batch: sum of u, largest bits(w)
  unsigned long long ri[64];     //                            sum of u k
};
__global__ __launch_bounds__(64) void blend_weights_kernel(const uint2* __restrict__ ranges, const uint2* __restrict__ pairs,
                                                           const float4* __restrict__ splat, int W, int H, TileMap tm,
                                                           const uint32_t* __restrict__ counters, int mode, const uint8_t* __restrict__ mask,
                                                           unsigned long long* __restrict__ sums, uint32_t* __restrict__ peak) {
  const int lane = threadIdx.x & 63;
  const int wave = (int)((blockIdx.x >> 3) & 3);
  const int tile_block = (int)(((blockIdx.x >> 5) << 3) | (blockIdx.x & 7));
  if ((int)counters[GM_CNT_POLICY] != mode || counters[GM_CNT_REFUSED] != 0u) return;   // refused, or lists of another policy: add nothing
  int tx, ty, parent;
  uint32_t child_bit;
  if (!tm.locate(tile_block, tx, ty, parent, child_bit)) return;
  if (tm.s == 1) child_bit = quadrant_bit(tx, ty, wave);
  const uint2 range = ranges[parent];
  const int n = (int)(range.y - range.x);
  if (n <= 0) return;
  const uint2* list = pairs + range.x;

  const int px = tx * GM_TILE + (wave & 1) * 8 + (lane & 7);
  const int py = ty * GM_TILE + (wave >> 1) * 8 + (lane >> 3);
  const bool inside = px < W && py < H;
  float T = inside ? 1.0f : -1.0f;               // T < 0: stopped (or outside the frame), as in the forward
  const float rx0 = (float)(tx * GM_TILE + (wave & 1) * 8), ry0 = (float)(ty * GM_TILE + (wave >> 1) * 8);
  const v2f pixf = {(float)px, (float)py};
  __shared__ WgtLds L;
  L.kk[lane] = inside ? (mask ? (uint32_t)mask[(size_t)W * py + px] : 255u) : 0u;   // (a pixel outside the frame has no weight: its byte is never read)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int es = lane >> 2, qd = lane & 3;       // phase 2 role
#pragma unroll
  for (int i = 0; i < 16; i++) L.M[i][lane] = 0.f;                // phase 2 also converts the rows behind a group's last survivor: M only ever holds weights
  uint32_t kq[16];
#pragma unroll
  for (int i = 0; i < 16; i++) kq[i] = L.kk[16 * qd + i];

  const int nlast = n - 1;
  int kpos = 0;
  uint32_t qa_head = 0, qa_cnt = 0;
  uint2 kv[RQ_K];
  auto scan = [&]() {                            // the forward's front end (gm_render_fwd_body.inc)
    bool go = true;
#pragma unroll
    for (int k = 0; k < RQ_K; k++) {
      go = go && kpos < n && qa_cnt + 64u <= (uint32_t)RQ_QA;
      if (go) {
        const int p = kpos + lane;
        const bool mine = p < n && (kv[k].x & child_bit) != 0u;
        const unsigned long long bal = __ballot(mine);
        if (mine) L.qa[(qa_head + qa_cnt + lanes_below(bal)) & (RQ_QA - 1)] = make_uint2(kv[k].y, (uint32_t)p);
        qa_cnt += (uint32_t)__popcll(bal);
        kpos += 64;
      }
    }
  };
  auto load_keys = [&]() {
#pragma unroll
    for (int k = 0; k < RQ_K; k++) kv[k] = list[min(kpos + k * 64 + lane, nlast)];
  };
  auto pop = [&](int& count) {
    count = (int)min(qa_cnt, 64u);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint2 cand = lane < count ? L.qa[(qa_head + (uint32_t)lane) & (RQ_QA - 1)] : make_uint2(0u, 0u);
    qa_head += (uint32_t)count; qa_cnt -= (uint32_t)count;
    return issue_gather(splat, cand);
  };
  load_keys();
  scan();
  load_keys();
  auto step = [&](Gather& cur, int& n0, Gather& nxt, int& n2) -> bool {
    const unsigned long long live = __ballot(T > 0.0f);
    if (live == 0ull) return false;
    if (n0 == 0 && qa_cnt == 0u && kpos >= n) return false;
    uint32_t cols = (uint32_t)live | (uint32_t)(live >> 32);
    cols |= cols >> 16; cols |= cols >> 8; cols &= 0xFFu;
    const float cx0 = rx0 + (float)(__ffs((int)cols) - 1), cx1 = rx0 + (float)(31 - __clz((int)cols));
    const float cy0 = ry0 + (float)((__ffsll(live) - 1) >> 3), cy1 = ry0 + (float)((63 - __clzll((long long)live)) >> 3);
    __builtin_amdgcn_s_waitcnt(0x0F70);                                  // vmcnt(0)
    scan();
    load_keys();
    nxt = pop(n2);
    if (n0 > 0) {
      const bool keep = lane < n0 && may_touch(cur.a.x, cur.a.y, cur.a.z, cur.a.w, cur.b.x, cur.b.y, cx0, cx1, cy0, cy1);
      const unsigned long long kb = __ballot(keep);
      const int ns = __popcll(kb);
      if (keep) {
        const int slot = (int)lanes_below(kb);
        L.ra[slot] = make_float4(cur.a.x, cur.a.y, (-0.5f * LOG2E) * cur.a.z, (-0.5f * LOG2E) * cur.b.x);
        L.bq[slot] = (-LOG2E) * cur.a.w;
        L.op[slot] = cur.b.y;
        L.id[slot] = cur.id;
      }
      if (lane < 4) {                                                    // survivors are taken four at a time: alpha = 0 behind the last
        L.ra[ns + lane] = make_float4(0.f, 0.f, 0.f, 0.f); L.bq[ns + lane] = 0.f; L.op[ns + lane] = 0.f;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      int processed = 0;                                                 // survivors of the batch whose totals are in rt / ri / rp
      bool alive = true;
      for (int j = 0; j < ns && alive; j += 16) {
        int gdone = 0;                                                   // survivors of this group that phase 1 walked
#pragma unroll
        for (int q = 0; q < 4; q++) {
          if (j + 4 * q >= ns || !alive) break;
          float al[4];
#pragma unroll
          for (int t = 0; t < 4; t++) {
            const int sl = j + 4 * q + t;
            v2f dd;
            const float e = staged_exponent(L.ra[sl], L.bq[sl], pixf, dd);
            const float oG = L.op[sl] * __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(e), 0.0f, 1.0f);
            al[t] = (oG >= 1.0f / 255.0f) ? fminf(0.99f, oG) : 0.0f;
          }
#pragma unroll
          for (int t = 0; t < 4; t++) {
            const float wa = al[t] * T, tt = __builtin_fmaf(-al[t], T, T);   // the forward's two instructions (see above)
            const bool stop = tt < 0.0001f;
            L.M[4 * q + t][lane] = stop ? 0.0f : wa;
            T = stop ? -__builtin_fabsf(T) : tt;
          }
          gdone = min(4 * q + 4, ns - j);
          alive = __any(T > 0.0f);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        uint32_t tot = 0u, pk = 0u;
        unsigned long long ins = 0ull;
        const float* mr = &L.M[es][16 * qd];
#pragma unroll
        for (int i = 0; i < 16; i++) {
          const float w = mr[i];
          const uint32_t u = (uint32_t)__builtin_rintf(w * 16777216.0f);
          tot += u;
          ins += (unsigned long long)u * kq[i];
          pk = max(pk, __float_as_uint(w));
        }
#pragma unroll
        for (int d = 1; d <= 2; d <<= 1) {
          tot += (uint32_t)__shfl_xor((int)tot, d);
          pk = max(pk, (uint32_t)__shfl_xor((int)pk, d));
          const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)ins, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(ins >> 32), d);
          ins += ((unsigned long long)hi << 32) | lo;
        }
        if (qd == 0 && es < gdone) { L.rt[j + es] = tot; L.rp[j + es] = pk; L.ri[j + es] = ins; }
        processed = j + gdone;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");          // M has been read before the next group writes it
        __builtin_amdgcn_wave_barrier();
      }
      if (lane < processed) {
        const uint32_t tot = L.rt[lane];
        if (tot != 0u) {                                                 // (an accepted pair has w >= 1e-4 / 255: u >= 6)
          const size_t gid = (size_t)L.id[lane];
          const unsigned long long ins = L.ri[lane];
          atomicAdd(sums + 2 * gid, (unsigned long long)tot);
          if (ins != 0ull) atomicAdd(sums + 2 * gid + 1, ins);
          if (peak) atomicMax(peak + gid, L.rp[lane]);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");            // the batch's rows have been read before the next is staged
      __builtin_amdgcn_wave_barrier();
    }
    return true;
  };
  int n0, n1 = 0;
  Gather g0 = pop(n0), g1 = g0;
  for (;;) {
    if (!step(g0, n0, g1, n1)) break;
    if (!step(g1, n1, g0, n0)) break;
  }
}

int launch_blend_weights(const GeomState& g, const uint2* pairs, ImageState& img, int W, int H, int mode, const uint8_t* mask,
                         unsigned long long* sums, uint32_t* peak, int debug, hipStream_t s) {
  const TileGrid tg(W, H, mode);
  const TileMap tm{tg.gx, tg.gy, tg.pgx, tg.pgy, tg.s, img.tile_order};
  if (tg.ptiles > 0)
    hipLaunchKernelGGL(blend_weights_kernel, dim3(tm.blocks() * 4), dim3(64), 0, s, img.ranges, pairs, g.splat, W, H, tm, g.counters, mode, mask,
                       sums, peak);
  GM_LAUNCH_CHECK(debug, s);
  return 0;
}

}  // namespace gm
