// gm_loss.hip -- photometric loss of the training loop: L1 and SSIM (11x11 Gaussian window, sigma 1.5, zero padding)
// with the SSIM gradient, as two single-halo tile kernels.
//
// Replaces (reference): utils/loss_utils.py:17-18 (l1_loss), :23-81 (gaussian / create_window / ssim / _ssim: five
// depthwise 11x11 convolutions per call + elementwise passes, then Jittor autograd through them), as used by
// train_mesh_gaussian.py:92-94:  loss = (1 - l) * L1 + l * (1 - ssim(image, gt)).
//
// The 11x11 window is the outer product of a normalised 1-D Gaussian (loss_utils.py:23-32), so the convolutions are
// done separably (11 + 11 taps) on a 32x32 pixel tile with a 5-pixel halo staged in LDS.
//   forward : x = image, y = gt.  mu1, mu2, E[xx], E[yy], E[xy] -> ssim map S; per-workgroup partial sums of S and of
//             |x - y|; optionally the three partial derivatives dS/dmu1, dS/dE[xx], dS/dE[xy] per pixel.
//   backward: dL/dx = conv(g dS/dmu1) + 2 x conv(g dS/dE[xx]) + y conv(g dS/dE[xy]) + g_l1 sign(x - y)
//             (the window is symmetric, so the adjoint of the correlation is the same correlation).
// HBM traffic per pixel-channel: forward 8 B in + 12 B out, backward 20 B in + 4 B out.
// ssim_fwd_u8_kernel / ssim_bwd_u8_kernel: the same two bodies (gm_ssim_fwd_body.inc / gm_ssim_bwd_body.inc) with the target read as the
// 8-bit planes of a dataset and composited over a background on load: 2 B (rgb + one mask plane) instead of 4 B of target per
// pixel-channel, and no composite pass in front of the loss.
#include "gm_common.h"
#include "gm_check.h"

namespace gm {

#define LS_TILE 32
#define LS_HALO 5
#define LS_SPAN (LS_TILE + 2 * LS_HALO)     // 42
#define LS_THREADS 256

struct LossWindow { float w[11]; };
typedef float lv2f __attribute__((ext_vector_type(2)));

static LossWindow make_window() {
  // loss_utils.py:23-25: exp(-(x - 5)^2 / (2 sigma^2)) in Python doubles -> float32 array -> divided by its float32 sum
  LossWindow lw;
  float g[11], sum = 0.f;
  for (int i = 0; i < 11; i++) { g[i] = (float)exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); sum += g[i]; }
  for (int i = 0; i < 11; i++) lw.w[i] = g[i] / sum;
  return lw;
}

__device__ __forceinline__ float block_sum(float v, float* red /*[4]*/) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// The target image y of the two kernel bodies (gm_ssim_fwd_body.inc, gm_ssim_bwd_body.inc): the staging loop of the forward and the per-pixel
// read of the backward get it through LS_TARGET.  The float kernels read a float [planes,H,W] image.  The u8 kernels read the 8-bit planes
// a dataset file holds and composite them on load, as the reference's training loop composites its target every iteration
// (train_mesh_gaussian.py:89-91: gt * mask + bg * (1 - mask) on images that PILtoJittor divided by 255): g = rgb/255, m = mask/255,
// y = g*m + bg[c]*(1 - m), each operation rounded to float32 on its own and in this order, so that y has the bits the tensor expression
// gives; without a mask y = g.
template <bool HAS_MASK>
struct U8Target {
  const unsigned char* __restrict__ rgb;     // [3,H,W]
  const unsigned char* __restrict__ mask;    // [Cm,H,W] (HAS_MASK)
  size_t mask_stride;                        // elements between the mask planes of two channels (0: one shared plane)
  float bgc;                                 // background[channel]
  __device__ __forceinline__ float load(size_t p, size_t off, int z) const {
#pragma clang fp contract(off)
    // u / 255.0f is a true (correctly rounded) division: multiplying by 1/255.0f differs from it for 126 of the 256 values.
    // Bytes are fetched one per lane (global_load_ubyte): a row segment of the 42-wide halo tile starts at any byte address, and
    // consecutive lanes read consecutive bytes of it.
    float y = (float)rgb[p] / 255.0f;
    if (HAS_MASK) {
      const float m = (float)mask[(size_t)z * mask_stride + off] / 255.0f;
      const float t1 = y * m;
      const float t2 = 1.0f - m;
      const float t3 = bgc * t2;
      y = t1 + t3;
    }
    // The value leaves as an opaque register, as a loaded float is: which products of the body the compiler fuses or packs must not
    // depend on how the target was made (the float kernels leave that to the compiler, and bit-identity with them is the contract).
    asm volatile("" : "+v"(y));
    return y;
  }
};
#define LS_U8_BEGIN const U8Target<HAS_MASK> tgt{rgb, mask, mask_stride, HAS_MASK ? bg[blockIdx.z] : 0.f};
#define LS_U8(p) tgt.load(p, (p) - plane, blockIdx.z)

__global__ __launch_bounds__(LS_THREADS) void ssim_fwd_kernel(const float* __restrict__ img1, const float* __restrict__ img2,
                                                              int H, int W, LossWindow win, float* __restrict__ d_mu1,
                                                              float* __restrict__ d_e11, float* __restrict__ d_e12,
                                                              float* __restrict__ partial) {
#define LS_TARGET_BEGIN
#define LS_TARGET(p) img2[p]
#include "gm_ssim_fwd_body.inc"
#undef LS_TARGET_BEGIN
#undef LS_TARGET
}

template <bool HAS_MASK>
__global__ __launch_bounds__(LS_THREADS) void ssim_fwd_u8_kernel(const float* __restrict__ img1, const unsigned char* __restrict__ rgb,
                                                                 const unsigned char* __restrict__ mask, size_t mask_stride,
                                                                 const float* __restrict__ bg, int H, int W, LossWindow win,
                                                                 float* __restrict__ d_mu1, float* __restrict__ d_e11,
                                                                 float* __restrict__ d_e12, float* __restrict__ partial) {
#define LS_TARGET_BEGIN LS_U8_BEGIN
#define LS_TARGET(p) LS_U8(p)
#include "gm_ssim_fwd_body.inc"
#undef LS_TARGET_BEGIN
#undef LS_TARGET
}

__global__ __launch_bounds__(LS_THREADS) void ssim_bwd_kernel(const float* __restrict__ img1, const float* __restrict__ img2,
                                                              const float* __restrict__ d_mu1, const float* __restrict__ d_e11,
                                                              const float* __restrict__ d_e12, int H, int W, LossWindow win,
                                                              const float* __restrict__ g_ssim /*[planes]*/,
                                                              const float* __restrict__ g_l1 /*[1] or null*/,
                                                              float* __restrict__ dL_dimg1) {
#define LS_TARGET_BEGIN
#define LS_TARGET_PIXEL(p, j) img2[p]
#include "gm_ssim_bwd_body.inc"
#undef LS_TARGET_BEGIN
#undef LS_TARGET_PIXEL
}

template <bool HAS_MASK>
__global__ __launch_bounds__(LS_THREADS) void ssim_bwd_u8_kernel(const float* __restrict__ img1, const unsigned char* __restrict__ rgb,
                                                                 const unsigned char* __restrict__ mask, size_t mask_stride,
                                                                 const float* __restrict__ bg, const float* __restrict__ d_mu1,
                                                                 const float* __restrict__ d_e11, const float* __restrict__ d_e12, int H,
                                                                 int W, LossWindow win, const float* __restrict__ g_ssim,
                                                                 const float* __restrict__ g_l1, float* __restrict__ dL_dimg1) {
  // the thread's four target pixels are made before the vertical taps and enter the final sum as plain registers
#define LS_TARGET_BEGIN                                                                          \
  LS_U8_BEGIN                                                                                    \
  float yv[4];                                                                                   \
  _Pragma("unroll") for (int j = 0; j < 4; j++) {                                                \
    const int gx = ox + (tid & 31), gy = oy + (tid >> 5) * 4 + j;                                \
    const size_t p = plane + (size_t)(gy < H ? gy : 0) * W + (gx < W ? gx : 0);                  \
    yv[j] = LS_U8(p);                                                                            \
  }
#define LS_TARGET_PIXEL(p, j) yv[j]
#include "gm_ssim_bwd_body.inc"
#undef LS_TARGET_BEGIN
#undef LS_TARGET_PIXEL
}

// value = offset + c_ssim * sum partial[.][0] + c_l1 * sum partial[.][1], summed in double by one workgroup: the fused loss's scalar
// without the four small launches (reduce, dot, add, cast) the tensor library spends on it
__global__ __launch_bounds__(1024) void loss_combine_kernel(const float* __restrict__ partial, long long n, double c_ssim, double c_l1,
                                                            double offset, float* __restrict__ out) {
  __shared__ double red[2][16];
  double a = 0.0, b = 0.0;
  for (long long i = threadIdx.x; i < n; i += 1024) { a += (double)partial[2 * i]; b += (double)partial[2 * i + 1]; }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { a += __shfl_xor(a, d); b += __shfl_xor(b, d); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sa = 0.0, sb = 0.0;
#pragma unroll
    for (int w = 0; w < 16; w++) { sa += red[0][w]; sb += red[1][w]; }
    out[0] = (float)(offset + c_ssim * sa + c_l1 * sb);
  }
}

}  // namespace gm

// ---------------------------------------------------------------------------------------------
// the entry points (include/gmesh_hip.h): their refusals, then the launches
using namespace gm;

// what the two calls with an 8-bit target refuse about it
static int check_u8_target(const char* who, const unsigned char* rgb, const unsigned char* mask, int64_t mask_plane_stride, const float* background,
                           int planes, int H, int W) {
  if (planes != 3) { set_error("%s: an 8-bit target has 3 planes", who); return GM_ERR_INVALID_ARG; }
  if (!rgb) { set_error("%s: null rgb", who); return GM_ERR_INVALID_ARG; }
  if (mask && !background) { set_error("%s: a mask needs the background colour (device float[3])", who); return GM_ERR_INVALID_ARG; }
  if (mask && mask_plane_stride != 0 && mask_plane_stride < (int64_t)H * W) {
    set_error("%s: mask_plane_stride is 0 (one shared plane) or at least H*W", who); return GM_ERR_INVALID_ARG;
  }
  return GM_OK;
}

extern "C" {

int gm_loss_combine(const float* partial, int64_t n_partials, double c_ssim, double c_l1, double offset, float* out, void* stream) {
  if (n_partials < 0) { set_error("gm_loss_combine: negative count"); return GM_ERR_INVALID_ARG; }
  if (!out || (n_partials > 0 && !partial)) { set_error("gm_loss_combine: null partial / out"); return GM_ERR_INVALID_ARG; }
  hipLaunchKernelGGL(loss_combine_kernel, dim3(1), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), partial, (long long)n_partials, c_ssim, c_l1,
                     offset, out);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_ssim_fwd(const float* img1, const float* img2, int planes, int H, int W, float* dS_dmu1, float* dS_dE11, float* dS_dE12,
                float* partial, void* stream) {
  if (planes < 0 || H < 0 || W < 0) { set_error("gm_ssim_fwd: negative size"); return GM_ERR_INVALID_ARG; }
  if (planes == 0 || H == 0 || W == 0) return GM_OK;
  if (!img1 || !img2 || !partial) { set_error("gm_ssim_fwd: null image or partial buffer"); return GM_ERR_INVALID_ARG; }
  const int nmaps = (dS_dmu1 != nullptr) + (dS_dE11 != nullptr) + (dS_dE12 != nullptr);
  if (nmaps != 0 && nmaps != 3) { set_error("gm_ssim_fwd: pass all three derivative maps or none"); return GM_ERR_INVALID_ARG; }
  if (planes > 65535) { set_error("gm_ssim_fwd: at most 65535 image planes per call"); return GM_ERR_INVALID_ARG; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  StageScope sc(ST_LOSS, s);
  const dim3 grid((W + LS_TILE - 1) / LS_TILE, (H + LS_TILE - 1) / LS_TILE, planes);
  const LossWindow win = make_window();
  hipLaunchKernelGGL(ssim_fwd_kernel, grid, dim3(LS_THREADS), 0, s, img1, img2, H, W, win, dS_dmu1, dS_dE11, dS_dE12, partial);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_ssim_bwd(const float* img1, const float* img2, const float* dS_dmu1, const float* dS_dE11, const float* dS_dE12, int planes,
                int H, int W, const float* g_ssim, const float* g_l1, float* dL_dimg1, void* stream) {
  if (planes < 0 || H < 0 || W < 0) { set_error("gm_ssim_bwd: negative size"); return GM_ERR_INVALID_ARG; }
  if (planes == 0 || H == 0 || W == 0) return GM_OK;
  if (!img1 || !img2 || !dS_dmu1 || !dS_dE11 || !dS_dE12 || !g_ssim || !dL_dimg1) { set_error("gm_ssim_bwd: null argument"); return GM_ERR_INVALID_ARG; }
  if (planes > 65535) { set_error("gm_ssim_bwd: at most 65535 image planes per call"); return GM_ERR_INVALID_ARG; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  StageScope sc(ST_LOSS_BWD, s);
  const dim3 grid((W + LS_TILE - 1) / LS_TILE, (H + LS_TILE - 1) / LS_TILE, planes);
  hipLaunchKernelGGL(ssim_bwd_kernel, grid, dim3(LS_THREADS), 0, s, img1, img2, dS_dmu1, dS_dE11, dS_dE12, H, W, make_window(), g_ssim, g_l1,
                     dL_dimg1);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

// the same two kernels' bodies with an 8-bit target composited on load (three planes; U8Target)
int gm_ssim_fwd_u8(const float* img1, const uint8_t* rgb, const uint8_t* mask, int64_t mask_plane_stride, const float* background,
                   int planes, int H, int W, float* dS_dmu1, float* dS_dE11, float* dS_dE12, float* partial, void* stream) {
  if (planes < 0 || H < 0 || W < 0) { set_error("gm_ssim_fwd_u8: negative size"); return GM_ERR_INVALID_ARG; }
  if (planes == 0 || H == 0 || W == 0) return GM_OK;
  if (!img1 || !partial) { set_error("gm_ssim_fwd_u8: null image or partial buffer"); return GM_ERR_INVALID_ARG; }
  const int nmaps = (dS_dmu1 != nullptr) + (dS_dE11 != nullptr) + (dS_dE12 != nullptr);
  if (nmaps != 0 && nmaps != 3) { set_error("gm_ssim_fwd_u8: pass all three derivative maps or none"); return GM_ERR_INVALID_ARG; }
  if (int rc = check_u8_target("gm_ssim_fwd_u8", rgb, mask, mask_plane_stride, background, planes, H, W)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  StageScope sc(ST_LOSS, s);
  const dim3 grid((W + LS_TILE - 1) / LS_TILE, (H + LS_TILE - 1) / LS_TILE, 3);
  const LossWindow win = make_window();
  const size_t mask_stride = (size_t)mask_plane_stride;
#define LS_FWD_U8(MASK)                                                                                                                \
  hipLaunchKernelGGL(ssim_fwd_u8_kernel<MASK>, grid, dim3(LS_THREADS), 0, s, img1, rgb, mask, mask_stride, background, H, W, win, dS_dmu1, \
                     dS_dE11, dS_dE12, partial)
  if (mask) LS_FWD_U8(true); else LS_FWD_U8(false);
#undef LS_FWD_U8
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_ssim_bwd_u8(const float* img1, const uint8_t* rgb, const uint8_t* mask, int64_t mask_plane_stride, const float* background,
                   const float* dS_dmu1, const float* dS_dE11, const float* dS_dE12, int planes, int H, int W, const float* g_ssim,
                   const float* g_l1, float* dL_dimg1, void* stream) {
  if (planes < 0 || H < 0 || W < 0) { set_error("gm_ssim_bwd_u8: negative size"); return GM_ERR_INVALID_ARG; }
  if (planes == 0 || H == 0 || W == 0) return GM_OK;
  if (!img1 || !dS_dmu1 || !dS_dE11 || !dS_dE12 || !g_ssim || !dL_dimg1) { set_error("gm_ssim_bwd_u8: null argument"); return GM_ERR_INVALID_ARG; }
  if (int rc = check_u8_target("gm_ssim_bwd_u8", rgb, mask, mask_plane_stride, background, planes, H, W)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  StageScope sc(ST_LOSS_BWD, s);
  const dim3 grid((W + LS_TILE - 1) / LS_TILE, (H + LS_TILE - 1) / LS_TILE, 3);
  const size_t mask_stride = (size_t)mask_plane_stride;
  if (mask)
    hipLaunchKernelGGL(ssim_bwd_u8_kernel<true>, grid, dim3(LS_THREADS), 0, s, img1, rgb, mask, mask_stride, background, dS_dmu1, dS_dE11, dS_dE12, H, W,
                       make_window(), g_ssim, g_l1, dL_dimg1);
  else
    hipLaunchKernelGGL(ssim_bwd_u8_kernel<false>, grid, dim3(LS_THREADS), 0, s, img1, rgb, mask, mask_stride, background, dS_dmu1, dS_dE11, dS_dE12, H, W,
                       make_window(), g_ssim, g_l1, dL_dimg1);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // extern "C"
