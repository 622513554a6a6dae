// gm_api.hip -- the rasteriser's extern "C" entry points (include/gmesh_hip.h) and their host orchestration; the error string, stage
// profiling and the scratch accessors.  Every other operator's entry point stands beside its kernels, at the end of its file.
//
// Orchestration replaces CudaRasterizer::Rasterizer::{forward_0, forward_1, backward, markVisible}
// (cuda_rasterizer/rasterizer_impl.cu:338-413, 416-511, 515-609, 141-153).
#include "gm_common.h"
#include "gm_check.h"
#include <cmath>
#include <cstdlib>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

namespace gm {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
int hip_fail(hipError_t e, const char* what, const char* file, int line) {
  set_error("HIP error %d (%s) at %s:%d in %s", (int)e, hipGetErrorString(e), file, line, what);
  return GM_ERR_HIP;
}

// ---- per-stage profiling -------------------------------------------------------------------
static const char* kStageNames[ST_COUNT] = {"preprocess", "depth_sort", "scan", "duplicate", "tile_sort", "ranges",
                                            "render", "render_bwd", "preprocess_bwd", "deform", "sh_colors", "loss", "loss_bwd", "mesh_rs"};
struct EvPair { hipEvent_t a, b; int st; };
static std::mutex g_prof_mu;
static bool g_prof_on = false;
static std::vector<EvPair> g_pending;
static double g_ms[ST_COUNT];
static int64_t g_n[ST_COUNT];

StageScope::StageScope(Stage st_, hipStream_t s_) : st(st_), s(s_), rec(nullptr) {
  if (!g_prof_on) return;
  EvPair* p = new EvPair;
  p->st = st;
  if (hipEventCreate(&p->a) != hipSuccess || hipEventCreate(&p->b) != hipSuccess) { delete p; return; }
  (void)hipEventRecord(p->a, s);
  rec = p;
}
StageScope::~StageScope() {
  if (!rec) return;
  EvPair* p = reinterpret_cast<EvPair*>(rec);
  (void)hipEventRecord(p->b, s);
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_pending.push_back(*p);
  delete p;
}
static void drain_profile() {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (auto& p : g_pending) {
    float ms = 0.f;
    if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      g_ms[p.st] += ms;
      g_n[p.st] += 1;
    }
    (void)hipEventDestroy(p.a);
    (void)hipEventDestroy(p.b);
  }
  g_pending.clear();
}

#define GM_LIST_TILES_MAX 65536     // list tiles of a single frame: two 8-bit tile passes
// What every entry point that takes a frame refuses about it: a policy outside 0..3, the sizes, a tile grid the emission record cannot
// hold (a tile rectangle has 12 bits per field - gm_common.h, bin_pack - a wider or taller grid would spill into the count), and more
// list tiles under the policy than the tile sort takes: max_list_tiles = 65536, or 1 << GM_BUCKET_BITS for a batch (the one-pass sort).
// who: the messages' prefix ("" for none)
static int check_frame(const char* who, int policy, int P, int W, int H, int max_list_tiles) {
  const char* sep = *who ? ": " : "";
  if (policy < 0 || policy > 3) { set_error("%s%semission policy %d out of range 0..3", who, sep, policy); return GM_ERR_INVALID_ARG; }
  if (P < 0 || W <= 0 || H <= 0) { set_error("%s%sinvalid sizes P=%d W=%d H=%d", who, sep, P, W, H); return GM_ERR_INVALID_ARG; }
  const TileGrid tg(W, H, policy);
  if (tg.gx > 4095 || tg.gy > 4095) {
    set_error("%s%s%dx%d is a grid of %d x %d 16-px tiles; the limit is 4095 x 4095 tiles (65520 pixels a side)", who, sep, W, H, tg.gx, tg.gy);
    return GM_ERR_INVALID_ARG;
  }
  if (tg.ptiles > max_list_tiles) {
    set_error("%s%s%dx%d has %d list tiles under emission policy %d; the limit is %d (policies 2 and 3 have fewer)", who, sep, W, H, tg.ptiles, policy,
              max_list_tiles);
    return GM_ERR_INVALID_ARG;
  }
  return GM_OK;
}

// need_opacities: the forward reads them, the backward does not
static int check_raster_args(const RasterArgs& a, bool need_opacities) {
  if (int rc = check_frame("", a.tile_cull, a.P, a.W, a.H, GM_LIST_TILES_MAX)) return rc;
  if (a.P == 0) return 0;                       // empty cloud: every per-Gaussian pointer may be null
  if ((a.shs == nullptr) == (a.colors_precomp == nullptr)) {
    set_error("provide exactly one of shs / colors_precomp"); return GM_ERR_INVALID_ARG;
  }
  const bool sr = a.scales != nullptr && a.rotations != nullptr;
  if ((a.scales != nullptr) != (a.rotations != nullptr) || sr == (a.cov3D_precomp != nullptr)) {
    set_error("provide exactly one of (scales, rotations) / cov3D_precomp"); return GM_ERR_INVALID_ARG;
  }
  if (a.shs && (a.D < 0 || a.D > 3 || a.M < (a.D + 1) * (a.D + 1))) {
    set_error("SH degree %d needs M >= %d coefficients (got %d); degree must be 0..3", a.D, (a.D + 1) * (a.D + 1), a.M);
    return GM_ERR_INVALID_ARG;
  }
  if (!a.means3D || (need_opacities && !a.opacities) || !a.viewmatrix || !a.projmatrix || !a.cam_pos) {
    set_error("null required input"); return GM_ERR_INVALID_ARG;
  }
  return 0;
}

}  // namespace gm

using namespace gm;

extern "C" {

int gm_abi_version(void) { return GM_ABI_VERSION; }
const char* gm_last_error(void) { return g_err; }

size_t gm_geom_bytes(int P) {
  GeomState g = GeomState::from(nullptr, (size_t)(P > 0 ? P : 1));
  return (size_t)g.end + 256;
}
size_t gm_image_bytes(int W, int H) {
  ImageState s = ImageState::from(nullptr, W > 0 ? W : 1, H > 0 ? H : 1);
  return (size_t)s.end + 256;
}
size_t gm_work_hint_bytes(int W, int H) {          // frame counter + one word per list tile (at most one per 16-px tile)
  const size_t T = (size_t)((W > 0 ? W : 1) + GM_TILE - 1) / GM_TILE * (size_t)(((H > 0 ? H : 1) + GM_TILE - 1) / GM_TILE);
  return 4 * (T + 1);
}
size_t gm_binning_bytes(int64_t R) {
  BinningState b = BinningState::from(nullptr, (size_t)(R > 0 ? R : 1));
  return (size_t)b.end + 256;
}

// Measurement aid (tools/stage_marginal.sh): GM_DEBUG_STOP_AFTER = deform | depth | dup | tile in the environment makes every forward
// stop launching after that stage - the frames are garbage, the loop's rate tells what the remaining stages cost the pipeline.
static int debug_stop_after() {
  static const int v = [] {
    const char* e = getenv("GM_DEBUG_STOP_AFTER");
    if (!e) return 0;
    return !strcmp(e, "deform") ? 1 : !strcmp(e, "depth") ? 2 : !strcmp(e, "dup") ? 3 : !strcmp(e, "tile") ? 4 : 0;
  }();
  return v;
}

// first half of a forward after the per-Gaussian kernel: order the visible Gaussians, hand the instance count to the host
static int order_and_count(GeomState& g, int P, int debug, hipStream_t st, int* num_rendered_host, void* count_event) {
  if (debug_stop_after() == 1) return GM_OK;
  return launch_depth_order(g, P, debug, st, num_rendered_host, reinterpret_cast<hipEvent_t>(count_event));
}

int gm_forward_0_async(int emission_policy, void* geom_buffer, int P, int D, int M, const float* background, int width, int height,
                       const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                       const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                       const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                       float tan_fovy, int prefiltered, int* radii, int debug, void* stream, int* num_rendered_host,
                       void* count_event) {
  const RasterArgs a{P, D, M, width, height, background, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, viewmatrix, projmatrix,
                     cam_pos, scale_modifier, tan_fovx, tan_fovy, prefiltered, debug, emission_policy, reinterpret_cast<hipStream_t>(stream)};
  if (int rc = check_raster_args(a, true)) return rc;
  if (P == 0) { if (num_rendered_host) *num_rendered_host = 0; return GM_OK; }
  if (!geom_buffer) { set_error("geom_buffer is null"); return GM_ERR_INVALID_ARG; }
  GeomState g = GeomState::from(geom_buffer, (size_t)P);
  if (int rc = launch_arm_counters(g, a.stream)) return rc;
  if (int rc = launch_preprocess(a, g, radii)) return rc;
  return order_and_count(g, P, debug, a.stream, num_rendered_host, count_event);
}

size_t gm_depth_plan_bytes(void) { return sizeof(uint32_t) * GM_PLAN_WORDS; }
size_t gm_depth_slab_bytes(int P) {
  DepthSlab d = DepthSlab::from(nullptr, (size_t)(P > 0 ? P : 1));
  return (size_t)d.end + 256;
}

int gm_forward_0_deformed_async(int emission_policy, void* geom_buffer, int P, int deg, int M, int width, int height, const int* tri,
                                const float* w, const float* packed, const float* cov, const float* pos, const float* shs,
                                const float* opacities, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                                float tan_fovx, float tan_fovy, float* pos_out, float* cov6_out, float* rgb_out, int* radii, int debug,
                                void* stream, int* num_rendered_host, void* count_event) {
  return gm_forward_0_deformed_stream_async(emission_policy, geom_buffer, P, deg, M, width, height, tri, w, packed, cov, pos, shs, opacities,
                                            viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, pos_out, cov6_out, rgb_out, radii, debug, stream,
                                            num_rendered_host, count_event, nullptr, nullptr, 0);
}

int gm_forward_0_deformed_stream_async(int emission_policy, void* geom_buffer, int P, int deg, int M, int width, int height, const int* tri,
                                       const float* w, const float* packed, const float* cov, const float* pos, const float* shs,
                                       const float* opacities, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                                       float tan_fovx, float tan_fovy, float* pos_out, float* cov6_out, float* rgb_out, int* radii,
                                       int debug, void* stream, int* num_rendered_host, void* count_event, void* depth_slab,
                                       unsigned int* depth_plan, int flags) {
  if (int rc = check_frame("", emission_policy, P, width, height, GM_LIST_TILES_MAX)) return rc;
  if (flags & ~(GM_STREAM_DIRECT | GM_STREAM_COV6)) { set_error("gm_forward_0_deformed_stream: unknown flags 0x%x", flags); return GM_ERR_INVALID_ARG; }
  const int direct = flags & GM_STREAM_DIRECT;
  const bool cov6 = (flags & GM_STREAM_COV6) != 0;
  if (direct && (!depth_slab || !depth_plan)) { set_error("gm_forward_0_deformed_stream: direct placement needs depth_slab and depth_plan"); return GM_ERR_INVALID_ARG; }
  if (P == 0) { if (num_rendered_host) *num_rendered_host = 0; return GM_OK; }
  if (deg < 0 || deg > 3 || M != 16) { set_error("gm_forward_0_deformed: needs SH rows of M == 16 coefficients, degree 0..3"); return GM_ERR_INVALID_ARG; }
  if (!geom_buffer || !tri || !w || !packed || !cov || !pos || !shs || !opacities || !viewmatrix || !projmatrix || !cam_pos) {
    set_error("gm_forward_0_deformed: null required input"); return GM_ERR_INVALID_ARG;
  }
  const int nout = (pos_out != nullptr) + (cov6_out != nullptr) + (rgb_out != nullptr);
  if (nout != 0 && nout != 3) { set_error("gm_forward_0_deformed: pass pos_out, cov6_out and rgb_out together or none"); return GM_ERR_INVALID_ARG; }
  RasterArgs a{};
  a.P = P; a.D = deg; a.M = M; a.W = width; a.H = height; a.opacities = opacities; a.viewmatrix = viewmatrix; a.projmatrix = projmatrix;
  a.cam_pos = cam_pos; a.scale_modifier = 1.0f; a.tan_fovx = tan_fovx; a.tan_fovy = tan_fovy; a.debug = debug; a.tile_cull = emission_policy;
  a.stream = reinterpret_cast<hipStream_t>(stream);
  GeomState g = GeomState::from(geom_buffer, (size_t)P);
  if (direct) {
    DepthSlab d = DepthSlab::from(depth_slab, (size_t)P);
    if (int rc = launch_arm_direct(g, d, depth_plan, a.stream)) return rc;
    GM_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(g.counters + GM_CNT_DEPTH_STALE), 1, 1, a.stream));   // no depth_key: gm_forward_1_aux refuses the frame
    if (int rc = launch_deform_shade_pre(a, g, radii, deg, tri, w, packed, cov, pos, shs, pos_out, cov6_out, rgb_out, &d, cov6)) return rc;
    if (debug_stop_after() == 1) return GM_OK;
    return launch_depth_order_direct(g, d, depth_plan, P, debug, a.stream, num_rendered_host, reinterpret_cast<hipEvent_t>(count_event));
  }
  if (int rc = launch_arm_counters(g, a.stream)) return rc;
  if (int rc = launch_deform_shade_pre(a, g, radii, deg, tri, w, packed, cov, pos, shs, pos_out, cov6_out, rgb_out, nullptr, cov6)) return rc;
  if (int rc = order_and_count(g, P, debug, a.stream, num_rendered_host, count_event)) return rc;
  if (depth_plan && debug_stop_after() != 1) return launch_publish_depth_plan(g, depth_plan, a.stream);
  return GM_OK;
}

static int forward_1_impl(int emission_policy, void* geom_buffer, void* binning_buffer, void* image_buffer, int P, int num_rendered,
                          int64_t binning_capacity, const float* background, int width, int height, float* out_color, int debug, void* stream,
                          int* status_host, int flags, unsigned int* work_hint, bool aux, float* out_depth, float* out_alpha) {
  if (int rc = check_frame("", emission_policy, P, width, height, GM_LIST_TILES_MAX)) return rc;
  if (flags & ~(GM_FWD_IMAGE_ONLY | GM_FWD_EXACT_EXPONENT)) { set_error("unknown flags 0x%x", flags); return GM_ERR_INVALID_ARG; }
  if ((flags & GM_FWD_IMAGE_ONLY) && (flags & GM_FWD_EXACT_EXPONENT)) {
    set_error("GM_FWD_EXACT_EXPONENT is for a forward a backward pass follows: not together with GM_FWD_IMAGE_ONLY"); return GM_ERR_INVALID_ARG;
  }
  if (!image_buffer || !out_color || !background) { set_error("null image_buffer / out_color / background"); return GM_ERR_INVALID_ARG; }
  const bool device_count = num_rendered < 0;          // sync-free: the count stays on the device, bounded by the capacity
  const int64_t cap = device_count ? binning_capacity : (int64_t)num_rendered;
  if (cap < 0) { set_error("negative binning capacity"); return GM_ERR_INVALID_ARG; }
  if (P > 0 && (!geom_buffer || (cap > 0 && !binning_buffer))) { set_error("null scratch buffer"); return GM_ERR_INVALID_ARG; }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int mode = emission_policy;
  ImageState img = ImageState::from(image_buffer, width, height);
  const int tiles = TileGrid(width, height, mode).ptiles;
  GeomState g = GeomState::from(geom_buffer, (size_t)(P > 0 ? P : 1));
  BinningState b = BinningState::from(binning_buffer, (size_t)cap);
  const int slot = tile_sort_final_slot(tiles);
  bool order_done = false;
  if (const int stop = debug_stop_after()) {
    if (stop <= 2) return GM_OK;
    if (stop == 3) return launch_duplicate(g, b, P, width, height, mode, (size_t)cap, debug, st);
  }
  if (P > 0 && cap > 0) {
    if (int rc = launch_duplicate(g, b, P, width, height, mode, (size_t)cap, debug, st)) return rc;
    if (int rc = launch_tile_sort(g, b, img, (size_t)cap, device_count ? g.counters + GM_CNT_RENDERED : nullptr, tiles, &order_done, work_hint, debug, st)) return rc;
    if (slot == 0)
      if (int rc = launch_tile_ranges(g, b, slot, img, (int)cap, device_count ? g.counters + GM_CNT_RENDERED : nullptr, tiles, debug, st)) return rc;
  } else {
    GM_HIP(hipMemsetAsync(img.ranges, 0, sizeof(uint2) * (size_t)tiles, st));
  }
  if (!order_done)
    if (int rc = launch_tile_order(img, tiles, work_hint, debug, st)) return rc;
  if (status_host && P == 0) {                       // no geometry state to report from
    status_host[0] = 0; status_host[1] = 0; status_host[2] = mode; status_host[3] = 0;
    status_host = nullptr;
  }
  if (debug_stop_after() == 4) return GM_OK;
  return launch_render_fwd(g, b.pairs[slot], img, width, height, mode, background, out_color, status_host, (flags & GM_FWD_IMAGE_ONLY) != 0,
                           work_hint, debug, st, (flags & GM_FWD_EXACT_EXPONENT) != 0, nullptr, out_depth, out_alpha, aux,
                           P > 0 ? g.counters : nullptr);
}

int gm_forward_1_geom(int emission_policy, void* geom_buffer, void* binning_buffer, void* image_buffer, int P, int num_rendered,
                      int64_t binning_capacity, const float* background, int width, int height, float* out_color, int debug, void* stream,
                      int* status_host, int flags, unsigned int* work_hint) {
  return forward_1_impl(emission_policy, geom_buffer, binning_buffer, image_buffer, P, num_rendered, binning_capacity, background, width, height,
                        out_color, debug, stream, status_host, flags, work_hint, false, nullptr, nullptr);
}

int gm_forward_1_aux(int emission_policy, void* geom_buffer, void* binning_buffer, void* image_buffer, int P, int num_rendered,
                     int64_t binning_capacity, const float* background, int width, int height, float* out_color, int debug, void* stream,
                     int* status_host, int flags, unsigned int* work_hint, float* out_depth, float* out_alpha) {
  if (width > 0 && height > 0) {                     // the maps against the image and each other: ahead of every other refusal
    const size_t HW = 4 * (size_t)width * height;
    const ByteRange rg[3] = {{out_depth, HW, "out_depth", true}, {out_alpha, HW, "out_alpha", true}, {out_color, 3 * HW, "out_color", false}};
    if (int rc = check_ranges("gm_forward_1_aux", rg)) return rc;
  }
  return forward_1_impl(emission_policy, geom_buffer, binning_buffer, image_buffer, P, num_rendered, binning_capacity, background, width, height,
                        out_color, debug, stream, status_host, flags, work_hint, true, out_depth, out_alpha);
}

// The scene batch (gm_forward_scene_batch_async): its row layout, per-frame deformation masks and static (scale, rotation) rows
struct SceneRows {
  int n_objects;
  const int* object_rows;
  const unsigned int* deformed;
  const float *scales, *rots;
};

// The buffers of a batch as a table for check_ranges.  The checker prints a range's name as it is, so each is spelled out with its frame
// ("frame 2's out_color buffer").
struct FrameRanges {
  ByteRange rg[6 * GM_BATCH_MAX];
  char name[6 * GM_BATCH_MAX][40];
  int n = 0;
  void add(const void* p, size_t bytes, int k, const char* what, bool apart) {
    snprintf(name[n], sizeof name[n], "frame %d's %s", k, what);
    rg[n] = {p, bytes, name[n], apart};
    n++;
  }
};

// gm_forward_scene_batch_async's own refusals: the row layout, the masks, and buffers of the batch that overlap as ranges
static int check_scene_batch(const char* who, const SceneRows& sc, int K, const gm_batch_frame* frames, int P, int width, int height,
                             int64_t binning_capacity, const int* tri, const float* w, const float* cov) {
  const int n = sc.n_objects;
  if (n < 0 || n > GM_SCENE_OBJECTS_MAX) { set_error("%s: n_objects = %d, not in 0..GM_SCENE_OBJECTS_MAX (%d)", who, n, GM_SCENE_OBJECTS_MAX); return GM_ERR_INVALID_ARG; }
  for (int j = 0; j <= n; j++) {
    const int r = sc.object_rows[j];
    if (r < 0 || r > P || (j > 0 && r < sc.object_rows[j - 1])) {
      set_error("%s: object_rows must ascend within [0, P = %d]: object_rows[%d] = %d", who, P, j, r); return GM_ERR_INVALID_ARG;
    }
  }
  for (int k = 0; k < K; k++) {
    const unsigned int m = sc.deformed[k];
    if (n < 32 && (m >> n)) { set_error("%s: frame %d: deformed mask 0x%x has a bit at or above n_objects = %d", who, k, m, n); return GM_ERR_INVALID_ARG; }
    if (m && !frames[k].packed) { set_error("%s: frame %d deforms objects (mask 0x%x) but packed is NULL", who, k, m); return GM_ERR_INVALID_ARG; }
    if (m && (!tri || !w || !cov)) { set_error("%s: frame %d deforms objects: tri / w / cov are required", who, k); return GM_ERR_INVALID_ARG; }
  }
  // every buffer a frame writes, as a byte range: no two may share memory (within a frame or between frames)
  FrameRanges r;
  for (int k = 0; k < K; k++) {
    const gm_batch_frame& f = frames[k];
    r.add(f.geom_buffer, gm_geom_bytes(P), k, "geometry buffer", true);
    r.add(f.binning_buffer, gm_binning_bytes(binning_capacity), k, "binning buffer", true);
    r.add(f.image_buffer, gm_image_bytes(width, height), k, "image buffer", true);
    r.add(f.out_color, 12 * (size_t)width * height, k, "out_color buffer", true);
    if (f.radii) r.add(f.radii, 4 * (size_t)P, k, "radii buffer", true);
    if (f.status_host) r.add(f.status_host, 16, k, "status_host buffer", true);
  }
  return check_ranges(who, r.rg, r.n);
}

// The batch entry points (gm_forward_deformed_batch_async; with aux, gm_forward_deformed_batch_aux_async; with scene,
// gm_forward_scene_batch_async): validation, then the launch chain.
static int forward_batch_impl(const char* who, int emission_policy, int K, const gm_batch_frame* frames, int P, int deg, int M, int width, int height,
                              const int* tri, const float* w, const float* cov, const float* pos, const float* shs, const float* opacities,
                              const float* background, int64_t binning_capacity, int flags, unsigned int* work_hint, int debug, void* stream,
                              bool aux, float* const* out_depth, float* const* out_alpha, const SceneRows* scene = nullptr) {
  if (int rc = check_frame(who, emission_policy, P, width, height, 1 << GM_BUCKET_BITS)) return rc;   // (a batch needs the one-pass tile sort)
  if (K < 1 || K > GM_BATCH_MAX || !frames) { set_error("%s: 1..%d frames", who, GM_BATCH_MAX); return GM_ERR_INVALID_ARG; }
  if (flags & ~(scene ? GM_BATCH_IMAGE_ONLY : (GM_BATCH_IMAGE_ONLY | GM_BATCH_COV6))) { set_error("%s: unknown flags 0x%x", who, flags); return GM_ERR_INVALID_ARG; }
  if (P == 0) { set_error("%s: invalid sizes P=%d W=%d H=%d (an empty cloud goes through the single-frame calls)", who, P, width, height); return GM_ERR_INVALID_ARG; }
  if (deg < 0 || deg > 3 || M != 16) { set_error("%s: needs SH rows of M == 16 coefficients, degree 0..3", who); return GM_ERR_INVALID_ARG; }
  if (scene ? (!pos || !scene->scales || !scene->rots || !shs || !opacities || !background || !scene->object_rows || !scene->deformed)
            : (!tri || !w || !cov || !pos || !shs || !opacities || !background)) {
    set_error("%s: null required input", who); return GM_ERR_INVALID_ARG;
  }
  if (binning_capacity <= 0) { set_error("%s: binning_capacity must be positive (sync-free second half)", who); return GM_ERR_INVALID_ARG; }
  const TileGrid tg(width, height, emission_policy);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  BatchFrameArgs fr[GM_BATCH_MAX];
  BatchOfs B{};
  B.frames = K;
  for (int k = 0; k < K; k++) {
    const gm_batch_frame& f = frames[k];
    if ((!scene && !f.packed) || !f.viewmatrix || !f.projmatrix || !f.cam_pos || !f.geom_buffer || !f.binning_buffer || !f.image_buffer || !f.out_color) {
      set_error("%s: frame %d has a null pointer", who, k); return GM_ERR_INVALID_ARG;
    }
    if ((reinterpret_cast<uintptr_t>(f.geom_buffer) | reinterpret_cast<uintptr_t>(f.binning_buffer) | reinterpret_cast<uintptr_t>(f.image_buffer)) & 255) {
      set_error("%s: frame %d: scratch buffers must be 256-byte aligned", who, k); return GM_ERR_INVALID_ARG;
    }
    for (int j = 0; j < k; j++)
      if (frames[j].geom_buffer == f.geom_buffer || frames[j].binning_buffer == f.binning_buffer || frames[j].image_buffer == f.image_buffer || frames[j].out_color == f.out_color) {
        set_error("%s: frames %d and %d share a buffer", who, j, k); return GM_ERR_INVALID_ARG;
      }
    fr[k].packed = f.packed; fr[k].viewmatrix = f.viewmatrix; fr[k].projmatrix = f.projmatrix; fr[k].cam_pos = f.cam_pos;
    fr[k].tan_fovx = f.tan_fovx; fr[k].tan_fovy = f.tan_fovy; fr[k].radii = f.radii;
    fr[k].g = GeomState::from(f.geom_buffer, (size_t)P);
    B.geom.d[k] = (long long)(reinterpret_cast<intptr_t>(f.geom_buffer) - reinterpret_cast<intptr_t>(frames[0].geom_buffer));
    B.binning.d[k] = (long long)(reinterpret_cast<intptr_t>(f.binning_buffer) - reinterpret_cast<intptr_t>(frames[0].binning_buffer));
    B.image.d[k] = (long long)(reinterpret_cast<intptr_t>(f.image_buffer) - reinterpret_cast<intptr_t>(frames[0].image_buffer));
    B.color.d[k] = (long long)(reinterpret_cast<intptr_t>(f.out_color) - reinterpret_cast<intptr_t>(frames[0].out_color));
    B.status[k] = f.status_host;
  }
  if (scene)
    if (int rc = check_scene_batch(who, *scene, K, frames, P, width, height, binning_capacity, tri, w, cov)) return rc;
  if (aux) {                          // the maps: each array NULL or K non-null pointers; no map range shares memory with a colour image or another map
    const size_t HW = 4 * (size_t)width * height;
    FrameRanges r;
    for (int k = 0; k < K; k++) {
      if ((out_depth && !out_depth[k]) || (out_alpha && !out_alpha[k])) { set_error("%s: frame %d: null map pointer in a non-null array", who, k); return GM_ERR_INVALID_ARG; }
      r.add(frames[k].out_color, 3 * HW, k, "colour image", false);
    }
    for (int m = 0; m < 2; m++) {
      float* const* maps = m ? out_alpha : out_depth;
      for (int k = 0; maps && k < K; k++) {
        if (reinterpret_cast<uintptr_t>(maps[k]) & 3) { set_error("%s: frame %d: unaligned map pointer", who, k); return GM_ERR_INVALID_ARG; }
        r.add(maps[k], HW, k, m ? "alpha map" : "depth map", true);
        (m ? B.alpha : B.depth).d[k] = (long long)(reinterpret_cast<intptr_t>(maps[k]) - reinterpret_cast<intptr_t>(maps[0]));
      }
    }
    if (int rc = check_ranges(who, r.rg, r.n)) return rc;
  }
  GeomState g = fr[0].g;
  ImageState img = ImageState::from(frames[0].image_buffer, width, height);
  BinningState b = BinningState::from(frames[0].binning_buffer, (size_t)binning_capacity);
  if (int rc = launch_arm_counters(g, st, &B)) return rc;
  if (scene) {
    if (int rc = launch_scene_shade_pre_batch(K, fr, scene->deformed, scene->n_objects, scene->object_rows, P, deg, width, height, emission_policy, pos,
                                              scene->scales, scene->rots, shs, opacities, tri, w, cov, debug, st)) return rc;
  } else if (int rc = launch_deform_shade_pre_batch(K, fr, P, deg, width, height, emission_policy, tri, w, cov, pos, shs, opacities, (flags & GM_BATCH_COV6) != 0, debug, st)) {
    return rc;
  }
  if (int rc = launch_depth_order(g, P, debug, st, nullptr, nullptr, &B)) return rc;
  if (int rc = launch_duplicate(g, b, P, width, height, emission_policy, (size_t)binning_capacity, debug, st, &B)) return rc;
  bool order_done = false;
  if (int rc = launch_tile_sort(g, b, img, (size_t)binning_capacity, g.counters + GM_CNT_RENDERED, tg.ptiles, &order_done, work_hint, debug, st, &B)) return rc;
  if (!order_done) { set_error("%s: internal: the tile pass did not produce the dispatch order", who); return GM_ERR_INVALID_ARG; }
  return launch_render_fwd(g, b.pairs[tile_sort_final_slot(tg.ptiles)], img, width, height, emission_policy, background, frames[0].out_color, frames[0].status_host,
                           (flags & GM_BATCH_IMAGE_ONLY) != 0, work_hint, debug, st, false, &B,
                           aux && out_depth ? out_depth[0] : nullptr, aux && out_alpha ? out_alpha[0] : nullptr, aux, aux ? g.counters : nullptr);
}

int gm_forward_deformed_batch_async(int emission_policy, int K, const gm_batch_frame* frames, int P, int deg, int M, int width, int height,
                                    const int* tri, const float* w, const float* cov, const float* pos, const float* shs, const float* opacities,
                                    const float* background, int64_t binning_capacity, int flags, unsigned int* work_hint, int debug, void* stream) {
  return forward_batch_impl("gm_forward_deformed_batch", emission_policy, K, frames, P, deg, M, width, height, tri, w, cov, pos, shs, opacities,
                            background, binning_capacity, flags, work_hint, debug, stream, false, nullptr, nullptr);
}

int gm_forward_deformed_batch_aux_async(int emission_policy, int K, const gm_batch_frame* frames, int P, int deg, int M, int width, int height,
                                        const int* tri, const float* w, const float* cov, const float* pos, const float* shs, const float* opacities,
                                        const float* background, int64_t binning_capacity, int flags, unsigned int* work_hint, int debug, void* stream,
                                        float* const* out_depth, float* const* out_alpha) {
  return forward_batch_impl("gm_forward_deformed_batch_aux", emission_policy, K, frames, P, deg, M, width, height, tri, w, cov, pos, shs, opacities,
                            background, binning_capacity, flags, work_hint, debug, stream, true, out_depth, out_alpha);
}

int gm_forward_scene_batch_async(int emission_policy, int K, const gm_batch_frame* frames, int P, int deg, int M, int width, int height,
                                 int n_objects, const int* object_rows, const unsigned int* deformed, const float* pos, const float* scales,
                                 const float* rots, const float* shs, const float* opacities, const int* tri, const float* w, const float* cov,
                                 const float* background, int64_t binning_capacity, int flags, unsigned int* work_hint, int debug, void* stream) {
  const SceneRows scene{n_objects, object_rows, deformed, scales, rots};
  return forward_batch_impl("gm_forward_scene_batch", emission_policy, K, frames, P, deg, M, width, height, tri, w, cov, pos, shs, opacities,
                            background, binning_capacity, flags, work_hint, debug, stream, false, nullptr, nullptr, &scene);
}

int gm_forward_status_async(void* geom_buffer, int P, int* status_host, void* stream) {
  if (!status_host) { set_error("status_host is null"); return GM_ERR_INVALID_ARG; }
  if (P <= 0) { status_host[0] = 0; status_host[1] = 0; status_host[2] = 0; status_host[3] = 0; return GM_OK; }
  if (!geom_buffer) { set_error("geom_buffer is null"); return GM_ERR_INVALID_ARG; }
  GeomState g = GeomState::from(geom_buffer, (size_t)P);
  GM_HIP(hipMemcpyAsync(status_host, g.counters, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, reinterpret_cast<hipStream_t>(stream)));
  return GM_OK;
}

int gm_forward_0(void* geom_buffer, int P, int D, int M, const float* background, int width, int height,
                 const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                 const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                 const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                 float tan_fovy, int prefiltered, int* radii, int debug, void* stream, int* num_rendered) {
  if (!num_rendered) { set_error("num_rendered is null"); return GM_ERR_INVALID_ARG; }
  *num_rendered = 0;
  if (int rc = gm_forward_0_async(GM_POLICY_DEFAULT, geom_buffer, P, D, M, background, width, height, means3D, shs, colors_precomp, opacities,
                                  scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy,
                                  prefiltered, radii, debug, stream, nullptr, nullptr)) return rc;
  if (P == 0) return GM_OK;
  GeomState g = GeomState::from(geom_buffer, (size_t)P);
  uint32_t rw[2] = {0u, 0u};                 // {num_rendered, prefilter violation}
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  GM_HIP(hipMemcpyAsync(rw, g.counters + GM_CNT_RENDERED, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  GM_HIP(hipStreamSynchronize(st));         // the one host sync of a forward (reference: rasterizer_impl.cu:411)
  const uint32_t r = rw[0];
  if (rw[1]) { set_error("Point is filtered although prefiltered is set. This shouldn't happen!"); return GM_ERR_INVALID_ARG; }   // auxiliary.h:157
  if (r > 0x7FFFFFFFu) { set_error("num_rendered overflows int32 (%u)", r); return GM_ERR_INVALID_ARG; }
  *num_rendered = (int)r;
  return GM_OK;
}

int gm_forward_1(void* geom_buffer, void* binning_buffer, void* image_buffer, int P, int D, int M, int num_rendered,
                 const float* background, int width, int height, const float* means3D, const float* shs,
                 const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                 const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                 const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered, float* out_color, int* radii,
                 int debug, void* stream) {
  const RasterArgs a{P, D, M, width, height, background, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, viewmatrix, projmatrix,
                     cam_pos, scale_modifier, tan_fovx, tan_fovy, prefiltered, debug, GM_POLICY_DEFAULT, reinterpret_cast<hipStream_t>(stream)};
  if (int rc = check_raster_args(a, true)) return rc;
  (void)radii;
  if (num_rendered < 0) { set_error("negative num_rendered"); return GM_ERR_INVALID_ARG; }
  return gm_forward_1_geom(GM_POLICY_DEFAULT, geom_buffer, binning_buffer, image_buffer, P, num_rendered, 0, background, width, height, out_color,
                           debug, stream, nullptr, 0, nullptr);
}

static int backward_impl(int emission_policy, int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
                         const float* shs, const float* colors_precomp, const float* scales, float scale_modifier,
                         const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                         const float* campos, float tan_fovx, float tan_fovy, const int* radii, void* geom_buffer,
                         void* binning_buffer, void* image_buffer, const float* dL_dpix, float* dL_dmean2D, float* dL_dconic,
                         float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                         float* dL_dscale, float* dL_drot, int debug, void* stream, const ShAdamArgs* sh_adam,
                         const float* dL_ddepth = nullptr, const float* dL_dalpha = nullptr, float* dL_dz = nullptr) {
  const RasterArgs a{P, D, M, width, height, background, means3D, shs, colors_precomp, /*opacities*/ nullptr, scales, rotations, cov3D_precomp, viewmatrix,
                     projmatrix, campos, scale_modifier, tan_fovx, tan_fovy, /*prefiltered*/ 0, debug, emission_policy, reinterpret_cast<hipStream_t>(stream)};
  if (int rc = check_raster_args(a, false)) return rc;
  if (P == 0) return GM_OK;
  // intermediates a caller may decline: dL/dconic always, dL/dcolour when the colours come from SH rows, dL/dcov3D when the covariances
  // come from scale / rotation
  if (!geom_buffer || !image_buffer || !dL_dpix || !dL_dmean2D || !dL_dopacity || (!shs && !dL_dcolor) ||
      !dL_dmean3D || (!scales && !dL_dcov3D) || (shs && !dL_dsh && !sh_adam) || (scales && (!dL_dscale || !dL_drot))) {
    set_error("gm_backward: null buffer"); return GM_ERR_INVALID_ARG;
  }
  GeomState g = GeomState::from(geom_buffer, (size_t)P);
  ImageState img = ImageState::from(image_buffer, width, height);
  BinningState b = BinningState::from(binning_buffer, (size_t)(R > 0 ? R : 0));
  const int slot = tile_sort_final_slot(TileGrid(width, height, a.tile_cull).ptiles);
  GM_HIP(hipMemsetAsync(g.grad_acc, 0, sizeof(float) * 12 * (size_t)P, a.stream));   // the only zero-fill of a backward
  if (R > 0) {
    if (!binning_buffer) { set_error("gm_backward: null binning buffer"); return GM_ERR_INVALID_ARG; }
    if (int rc = launch_render_bwd(g, b.pairs[slot], img, width, height, a.tile_cull, background, dL_dpix, debug, a.stream,
                                   dL_ddepth || dL_dalpha, dL_ddepth, dL_dalpha)) return rc;
  }
  if (int rc = launch_preprocess_bwd(a, g, radii, dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh,
                                     dL_dscale, dL_drot, sh_adam)) return rc;
  if (dL_ddepth || dL_dz) return launch_depth_grad(P, g, viewmatrix, dL_dmean3D, dL_dz, a.stream);
  return GM_OK;
}

int gm_backward_aux(int emission_policy, int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
                    const float* shs, const float* colors_precomp, const float* scales, float scale_modifier,
                    const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                    const float* campos, float tan_fovx, float tan_fovy, const int* radii, void* geom_buffer,
                    void* binning_buffer, void* image_buffer, const float* dL_dpix, float* dL_dmean2D, float* dL_dconic,
                    float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                    float* dL_dscale, float* dL_drot, const float* dL_ddepth, const float* dL_dalpha, float* dL_dz, int debug, void* stream) {
  if (P > 0) {                                       // dL_dz against the gradient outputs written around it: ahead of every other refusal
    const size_t n = 4 * (size_t)P;
    const ByteRange rg[4] = {{dL_dz, n, "dL_dz", true}, {dL_dmean3D, 3 * n, "dL_dmean3D", false}, {dL_dmean2D, 3 * n, "dL_dmean2D", false},
                             {dL_dopacity, n, "dL_dopacity", false}};
    if (int rc = check_ranges("gm_backward_aux", rg)) return rc;
  }
  return backward_impl(emission_policy, P, D, M, R, background, width, height, means3D, shs, colors_precomp, scales, scale_modifier, rotations, cov3D_precomp,
                       viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii, geom_buffer, binning_buffer, image_buffer, dL_dpix, dL_dmean2D, dL_dconic,
                       dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, debug, stream, nullptr, dL_ddepth, dL_dalpha, dL_dz);
}

int gm_backward_p(int emission_policy, int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
                  const float* shs, const float* colors_precomp, const float* scales, float scale_modifier,
                  const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                  const float* campos, float tan_fovx, float tan_fovy, const int* radii, void* geom_buffer,
                  void* binning_buffer, void* image_buffer, const float* dL_dpix, float* dL_dmean2D, float* dL_dconic,
                  float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                  float* dL_dscale, float* dL_drot, int debug, void* stream) {
  return backward_impl(emission_policy, P, D, M, R, background, width, height, means3D, shs, colors_precomp, scales, scale_modifier, rotations, cov3D_precomp,
                       viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii, geom_buffer, binning_buffer, image_buffer, dL_dpix, dL_dmean2D, dL_dconic,
                       dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, debug, stream, nullptr);
}

int gm_backward_sh_step(int emission_policy, int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
                        float* shs, const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                        const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                        void* geom_buffer, void* binning_buffer, void* image_buffer, const float* dL_dpix, float* dL_dmean2D, float* dL_dopacity,
                        float* dL_dmean3D, float* dL_dcov3D, float* dL_dscale, float* dL_drot, int rows, float* exp_avg, float* exp_avg_sq,
                        float lr_dc, float lr_rest, double beta1, double beta2, double eps, int step, int debug, void* stream) {
  if (!shs || M != 16 || D < 0 || D > 3) { set_error("gm_backward_sh_step: needs the [P,16,3] SH operand"); return GM_ERR_INVALID_ARG; }
  if (rows < 0 || rows > P || !exp_avg || !exp_avg_sq || step < 1) { set_error("gm_backward_sh_step: bad optimizer state (rows %d of %d, step %d)", rows, P, step); return GM_ERR_INVALID_ARG; }
  ShAdamArgs ad;
  ad.p = shs; ad.m = exp_avg; ad.v = exp_avg_sq; ad.rows = rows;
  ad.b1 = (float)beta1; ad.b2 = (float)beta2; ad.c1 = (float)(1.0 - beta1); ad.c2 = (float)(1.0 - beta2); ad.eps = (float)eps;
  const double corr = sqrt(1.0 - pow(beta2, (double)step)) / (1.0 - pow(beta1, (double)step));      // as gm_adam_step_active
  ad.step_lo = (float)(lr_dc * corr); ad.step_hi = (float)(lr_rest * corr);
  return backward_impl(emission_policy, P, D, M, R, background, width, height, means3D, shs, nullptr, scales, scale_modifier, rotations, cov3D_precomp,
                       viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii, geom_buffer, binning_buffer, image_buffer, dL_dpix, dL_dmean2D, nullptr,
                       dL_dopacity, nullptr, dL_dmean3D, dL_dcov3D, nullptr, dL_dscale, dL_drot, debug, stream, &ad);
}

int gm_backward(int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
                const float* shs, const float* colors_precomp, const float* scales, float scale_modifier,
                const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                const float* campos, float tan_fovx, float tan_fovy, const int* radii, void* geom_buffer,
                void* binning_buffer, void* image_buffer, const float* dL_dpix, float* dL_dmean2D, float* dL_dconic,
                float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                float* dL_dscale, float* dL_drot, int debug, void* stream) {
  return gm_backward_p(GM_POLICY_DEFAULT, P, D, M, R, background, width, height, means3D, shs, colors_precomp, scales, scale_modifier, rotations,
                       cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii, geom_buffer, binning_buffer, image_buffer,
                       dL_dpix, dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, debug, stream);
}

int gm_splat_floats(void) { return GM_SPLAT_STRIDE; }
void* gm_geom_field(void* geom_buffer, int P, const char* name) {
  GeomState g = GeomState::from(geom_buffer, (size_t)(P > 0 ? P : 1));
  if (!strcmp(name, "splat")) return g.splat;
  if (!strcmp(name, "depth_key")) return g.depth_key;
  if (!strcmp(name, "radii")) return g.radii;
  if (!strcmp(name, "tiles_touched")) return g.tiles_touched;
  if (!strcmp(name, "bin")) return g.bin;
  if (!strcmp(name, "inst16")) return g.inst16;
  if (!strcmp(name, "bin_sorted")) return g.bin_sorted;
  if (!strcmp(name, "grad_acc")) return g.grad_acc;
  if (!strcmp(name, "cov3D")) return g.cov3D;
  if (!strcmp(name, "clamped")) return g.clamped;
  if (!strcmp(name, "order")) return g.order;
  if (!strcmp(name, "bucket_start")) return g.bucket_start;
  if (!strcmp(name, "counters")) return g.counters;
  if (!strcmp(name, "bmap")) return g.bmap;
  if (!strcmp(name, "dmap")) return g.dmap;
  return nullptr;
}
void* gm_image_field(void* image_buffer, int W, int H, const char* name) {
  ImageState s = ImageState::from(image_buffer, W, H);
  if (!strcmp(name, "final_T")) return s.final_T;
  if (!strcmp(name, "n_contrib")) return s.n_contrib;
  if (!strcmp(name, "ranges")) return s.ranges;
  if (!strcmp(name, "tile_order")) return s.tile_order;
  return nullptr;
}
void* gm_binning_field(void* binning_buffer, int64_t R, int W, int H, int emission_policy, const char* name) {
  BinningState b = BinningState::from(binning_buffer, (size_t)(R > 0 ? R : 0));
  const int slot = tile_sort_final_slot(TileGrid(W, H, emission_policy < 0 ? 0 : (emission_policy > 3 ? 3 : emission_policy)).ptiles);
  if (!strcmp(name, "pairs")) return b.pairs[slot];
  return nullptr;
}

int gm_blend_weights(int emission_policy, void* geom_buffer, void* binning_buffer, void* image_buffer, int P, int64_t binning_capacity,
                     int width, int height, const uint8_t* mask, unsigned long long* sums, unsigned int* peak, int debug, void* stream) {
  if (int rc = check_frame("gm_blend_weights", emission_policy, P, width, height, GM_LIST_TILES_MAX)) return rc;
  if (binning_capacity < 0) { set_error("gm_blend_weights: negative binning capacity"); return GM_ERR_INVALID_ARG; }
  if (P == 0) return GM_OK;
  if (!geom_buffer || !binning_buffer || !image_buffer || !sums) {
    set_error("gm_blend_weights: null geom_buffer / binning_buffer / image_buffer / sums"); return GM_ERR_INVALID_ARG;
  }
  const ByteRange rg[6] = {{geom_buffer, gm_geom_bytes(P), "geom_buffer", false}, {binning_buffer, gm_binning_bytes(binning_capacity), "binning_buffer", false},
                           {image_buffer, gm_image_bytes(width, height), "image_buffer", false}, {mask, (size_t)width * height, "mask", false},
                           {sums, 16 * (size_t)P, "sums", true}, {peak, 4 * (size_t)P, "peak", true}};
  if (int rc = check_ranges("gm_blend_weights", rg)) return rc;
  if (binning_capacity == 0) return GM_OK;                       // a frame without instances: every list is empty
  GeomState g = GeomState::from(geom_buffer, (size_t)P);
  ImageState img = ImageState::from(image_buffer, width, height);
  BinningState b = BinningState::from(binning_buffer, (size_t)binning_capacity);
  return launch_blend_weights(g, b.pairs[tile_sort_final_slot(TileGrid(width, height, emission_policy).ptiles)], img, width, height, emission_policy, mask,
                              sums, peak, debug, reinterpret_cast<hipStream_t>(stream));
}

int64_t gm_ssim_partials(int planes, int H, int W) {
  if (planes < 0 || H < 0 || W < 0) return 0;
  return (int64_t)planes * ((H + 31) / 32) * ((W + 31) / 32);
}

void gm_profile_enable(int on) { g_prof_on = on != 0; }
void gm_profile_reset(void) {
  drain_profile();
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (int i = 0; i < ST_COUNT; i++) { g_ms[i] = 0; g_n[i] = 0; }
}
int gm_profile_read(const char* stage, double* total_ms, int64_t* launches) {
  drain_profile();
  for (int i = 0; i < ST_COUNT; i++)
    if (!strcmp(stage, kStageNames[i])) {
      if (total_ms) *total_ms = g_ms[i];
      if (launches) *launches = g_n[i];
      return GM_OK;
    }
  set_error("unknown stage '%s'", stage);
  return GM_ERR_INVALID_ARG;
}

}  // extern "C"
