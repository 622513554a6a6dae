// gm_train.hip -- the per-Gaussian host-framework work around the rasterizer in one training iteration, fused:
//
//   mesh_activate_fwd / _bwd : MeshBasedGaussianModel's parameter -> rasterizer-input map and its adjoint
//       get_xyz      = softmax(bc) . (v1,v2,v3) + alpha r (sigmoid(d) - 0.5) n      scene/mesh_based_gaussian_model.py:138-152
//       get_scaling  = exp(_scaling)            get_rotation = normalize(_rotation)                   :122-128, 33-43
//       get_opacity  = sigmoid(_opacity)                                                              :172-174
//     In the reference these are ~15 Jittor elementwise ops forward and ~25 in the autograd pass, each a pass over P;
//     here one kernel each way (60 B in, 44 B out per Gaussian forward).
//   plain_activate_fwd / _bwd : the same for the plain 3DGS model (scene/gaussian_model.py), xyz being a parameter itself.
//   adam_kernel : jittor.nn.Adam's update for all parameter groups of the model in ONE launch (table of tensors,
//     per-group learning rate; the SH tensor [P,16,3] takes two rates - coefficient 0 is the reference's "f_dc" group,
//     the rest "f_rest" - so no concatenation / split of the 192-byte SH rows is needed per iteration):
//       m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= lr sqrt(1-b2^t)/(1-b1^t) m / (sqrt(v) + eps)
//     (scene/mesh_based_gaussian_model.py:242-263 training_setup; jittor/optim.py Adam.step).
//     `active` (gm_adam_step_active): while the model's active SH degree D is below 3 (train_mesh_gaussian.py:70-71: one degree per
//     1000 iterations, starting at 0) the coefficients >= (D+1)^2 of every row have never had a non-zero gradient: g = m = v = 0,
//     and the rule above leaves p, m and v exactly as they are.  The kernel then does not touch them at all - at D = 0 that is
//     45 of the 60 parameters of a Gaussian, 28 bytes each.
#include "gm_common.h"
#include "gm_check.h"
#include <cmath>

namespace gm {

struct ActArgs {                 // mesh-bound parameter -> rasterizer-input map
  int N;
  float alpha;
  const float *bc, *dist, *scaling, *rotation, *opacity, *v1, *v2, *v3, *normal, *r;
};
struct AdamTensor {
  float* p; const float* g; float* m; float* v;
  unsigned long long n;
  float step_lo, step_hi;      // lr * sqrt(1-b2^t)/(1-b1^t) for elements with (index % period) < split / the others
  unsigned period, split;      // period == 0: one rate (step_lo) for the whole tensor
  unsigned active;             // 0: every element; else only elements with (index % period) < active (rounded up to a 16-byte granule) are touched
};
struct AdamTable { AdamTensor t[8]; int count; float b1, b2, eps, omb1, omb2; };   // omb = (float)(1 - beta), formed in double

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + __expf(-x)); }

// __expf(x) for the softmax's x = b - max b <= 0.  The exponential instruction behind __expf returns 0 where the result would be subnormal
// (x < -87.34), and w_i = 0 then zeroes w_i v_i and d_bc_i = w_i (dw_i - dot), which are up to ~10 w_i and may well be normal numbers.
// Below -87 the exponential is taken 44 higher - x + 44 is exact there - and scaled back by e^-44, a product that rounds to the
// subnormal it should be; above, the bits are __expf's as before.
__device__ __forceinline__ float softmax_exp(float x) { return x < -87.0f ? __expf(x + 44.0f) * 7.78113225e-20f : __expf(x); }

// sqrt(|AB x AC|) of the bound face: the reference's circumradius() (utils/loss_utils.py:86-101)
__device__ __forceinline__ float face_radius(const ActArgs& a, size_t i3) {
  const float ax = a.v2[i3] - a.v1[i3], ay = a.v2[i3 + 1] - a.v1[i3 + 1], az = a.v2[i3 + 2] - a.v1[i3 + 2];
  const float bx = a.v3[i3] - a.v1[i3], by = a.v3[i3 + 1] - a.v1[i3 + 1], bz = a.v3[i3 + 2] - a.v1[i3 + 2];
  const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  return sqrtf(sqrtf(cx * cx + cy * cy + cz * cz));
}

// mr_partial (may be null): per-workgroup sums of the mesh-restrict term max(0, max_c scales - mr_weight * face_radius)
// (utils/loss_utils.py:103-108); the host side adds the partials.
__global__ __launch_bounds__(256) void mesh_activate_fwd_kernel(const ActArgs a, float* __restrict__ xyz, float* __restrict__ scales,
                                                                 float4* __restrict__ rots, float* __restrict__ opac,
                                                                 float mr_weight, float* __restrict__ mr_partial) {
  __shared__ float red[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  float term = 0.f;
  if (i < a.N) {
  const size_t i3 = 3 * (size_t)i;
  const float b0 = a.bc[i3], b1 = a.bc[i3 + 1], b2 = a.bc[i3 + 2];
  const float mx = fmaxf(b0, fmaxf(b1, b2));
  const float e0 = softmax_exp(b0 - mx), e1 = softmax_exp(b1 - mx), e2 = softmax_exp(b2 - mx);
  const float inv = 1.0f / (e0 + e1 + e2);
  const float w0 = e0 * inv, w1 = e1 * inv, w2 = e2 * inv;
  const float k = a.alpha * a.r[i] * (sigmoidf(a.dist[i]) - 0.5f);
#pragma unroll
  for (int c = 0; c < 3; c++)
    xyz[i3 + c] = (w0 * a.v1[i3 + c] + w1 * a.v2[i3 + c] + w2 * a.v3[i3 + c]) + k * a.normal[i3 + c];
  float smax = -3.4e38f;
#pragma unroll
  for (int c = 0; c < 3; c++) { const float sc = __expf(a.scaling[i3 + c]); scales[i3 + c] = sc; smax = fmaxf(smax, sc); }
  const float4 q = reinterpret_cast<const float4*>(a.rotation)[i];
  const float qlen = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  const float qn = 1.0f / (qlen < 1e-12f ? 1e-12f : qlen);   // F.normalize eps; not fmaxf: a NaN |q| stays NaN, as torch's clamp_min keeps it (Jittor's maximum on a NaN: not checked)
  rots[i] = make_float4(q.x * qn, q.y * qn, q.z * qn, q.w * qn);
  opac[i] = sigmoidf(a.opacity[i]);
  if (mr_partial) term = fmaxf(smax - mr_weight * face_radius(a, i3), 0.f);
  }
  if (mr_partial) {                              // wave-uniform
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) term += __shfl_xor(term, d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = term;
    __syncthreads();
    if (threadIdx.x == 0) mr_partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

__global__ __launch_bounds__(256) void mesh_activate_bwd_kernel(const ActArgs a, const float* __restrict__ d_xyz,
                                                                 const float* __restrict__ d_scales, const float4* __restrict__ d_rots,
                                                                 const float* __restrict__ d_opac, float* __restrict__ d_bc,
                                                                 float* __restrict__ d_dist, float* __restrict__ d_scaling,
                                                                 float4* __restrict__ d_rotation, float* __restrict__ d_opacity,
                                                                 float mr_weight, const float* __restrict__ d_mr /*[1] or null*/) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  const size_t i3 = 3 * (size_t)i;
  const float gx = d_xyz ? d_xyz[i3] : 0.f, gy = d_xyz ? d_xyz[i3 + 1] : 0.f, gz = d_xyz ? d_xyz[i3 + 2] : 0.f;
  {  // softmax-barycentric position and normal offset
    const float b0 = a.bc[i3], b1 = a.bc[i3 + 1], b2 = a.bc[i3 + 2];
    const float mx = fmaxf(b0, fmaxf(b1, b2));
    const float e0 = softmax_exp(b0 - mx), e1 = softmax_exp(b1 - mx), e2 = softmax_exp(b2 - mx);
    const float inv = 1.0f / (e0 + e1 + e2);
    const float w0 = e0 * inv, w1 = e1 * inv, w2 = e2 * inv;
    const float dw0 = gx * a.v1[i3] + gy * a.v1[i3 + 1] + gz * a.v1[i3 + 2];
    const float dw1 = gx * a.v2[i3] + gy * a.v2[i3 + 1] + gz * a.v2[i3 + 2];
    const float dw2 = gx * a.v3[i3] + gy * a.v3[i3 + 1] + gz * a.v3[i3 + 2];
    const float dot = w0 * dw0 + w1 * dw1 + w2 * dw2;
    d_bc[i3] = w0 * (dw0 - dot); d_bc[i3 + 1] = w1 * (dw1 - dot); d_bc[i3 + 2] = w2 * (dw2 - dot);
    const float sd = sigmoidf(a.dist[i]);
    const float gn = gx * a.normal[i3] + gy * a.normal[i3 + 1] + gz * a.normal[i3 + 2];
    d_dist[i] = gn * a.alpha * a.r[i] * sd * (1.0f - sd);
  }
  {
    float sc[3], ds[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { sc[c] = __expf(a.scaling[i3 + c]); ds[c] = d_scales ? d_scales[i3 + c] : 0.f; }
    if (d_mr) {                                  // d/dscales of max(0, max_c scales - w R): one-hot on the first largest axis
      const int am = (sc[0] >= sc[1] && sc[0] >= sc[2]) ? 0 : (sc[1] >= sc[2] ? 1 : 2);
      if (sc[am] - mr_weight * face_radius(a, i3) > 0.f) ds[am] += d_mr[0];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) d_scaling[i3 + c] = ds[c] * sc[c];
  }
  {
    const float4 q = reinterpret_cast<const float4*>(a.rotation)[i];
    const float len = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    const float qn = 1.0f / (len < 1e-12f ? 1e-12f : len);   // (a NaN |q| stays NaN, as in the forward)
    const float4 g = d_rots ? d_rots[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (len > 1e-12f) {                          // d(q/|q|) = (g - y (y.g)) / |q|
      const float4 y = make_float4(q.x * qn, q.y * qn, q.z * qn, q.w * qn);
      const float yd = y.x * g.x + y.y * g.y + y.z * g.z + y.w * g.w;
      d_rotation[i] = make_float4((g.x - y.x * yd) * qn, (g.y - y.y * yd) * qn, (g.z - y.z * yd) * qn, (g.w - y.w * yd) * qn);
    } else {                                     // the clamp is active: q / eps, as jt.normalize's x / maximum(|x|, eps) differentiates
      d_rotation[i] = make_float4(g.x * qn, g.y * qn, g.z * qn, g.w * qn);
    }
  }
  {
    const float o = sigmoidf(a.opacity[i]);
    d_opacity[i] = d_opac ? d_opac[i] * o * (1.0f - o) : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------
// plain_activate_fwd / _bwd : GaussianModel's raw parameters -> rasterizer inputs and the adjoint (scene/gaussian_model.py:26-43,
// 96-117): xyz copied, scales = exp(_scaling), rots = _rotation / max(|_rotation|, 1e-12), opac = sigmoid(_opacity).  The outputs
// (forward) and the incoming gradients (backward) are rows [row0, row0 + N) of buffers that may hold more rows (the joint
// [background; object] buffers of renderer.bg_render).  expf, not __expf, and the forward in torch's own formulas (sigmoid =
// 1 / (1 + exp(-x)), q / max(|q|, eps) by division) and the opacity adjoint as torch / Jittor form it, g (1 - s) s in float32: 0 where
// s rounds to 1 (x > ~17).  A more accurate e / (1 + e)^2 there would hand Adam ~1e-13 gradients that it turns into full-rate steps
// the reference never takes.
__global__ __launch_bounds__(256) void plain_activate_fwd_kernel(int N, const float* __restrict__ xyz_in, const float* __restrict__ scaling,
                                                                  const float4* __restrict__ rotation, const float* __restrict__ opacity,
                                                                  float* __restrict__ xyz, float* __restrict__ scales,
                                                                  float4* __restrict__ rots, float* __restrict__ opac) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const size_t i3 = 3 * (size_t)i;
#pragma unroll
  for (int c = 0; c < 3; c++) { xyz[i3 + c] = xyz_in[i3 + c]; scales[i3 + c] = expf(scaling[i3 + c]); }
  const float4 q = rotation[i];
  const float len = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  const float n = len < 1e-12f ? 1e-12f : len;   // F.normalize eps; not fmaxf: a NaN |q| stays NaN, as torch's clamp_min keeps it
  rots[i] = make_float4(q.x / n, q.y / n, q.z / n, q.w / n);
  opac[i] = 1.0f / (1.0f + expf(-opacity[i]));
}

__global__ __launch_bounds__(256) void plain_activate_bwd_kernel(int N, const float* __restrict__ scaling, const float4* __restrict__ rotation,
                                                                  const float* __restrict__ opacity, const float* __restrict__ g_xyz,
                                                                  const float* __restrict__ g_scales, const float4* __restrict__ g_rots,
                                                                  const float* __restrict__ g_opac, float* __restrict__ d_xyz,
                                                                  float* __restrict__ d_scaling, float4* __restrict__ d_rotation,
                                                                  float* __restrict__ d_opacity) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const size_t i3 = 3 * (size_t)i;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    d_xyz[i3 + c] = g_xyz ? g_xyz[i3 + c] : 0.f;
    d_scaling[i3 + c] = g_scales ? g_scales[i3 + c] * expf(scaling[i3 + c]) : 0.f;
  }
  const float4 q = rotation[i];
  const float4 g = g_rots ? g_rots[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  const float len = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  const float qn = 1.0f / (len < 1e-12f ? 1e-12f : len);   // (a NaN |q| stays NaN, as in the forward)
  if (len > 1e-12f) {                            // d(q/|q|) = (g - y (y.g)) / |q|
    const float4 y = make_float4(q.x * qn, q.y * qn, q.z * qn, q.w * qn);
    const float yd = y.x * g.x + y.y * g.y + y.z * g.z + y.w * g.w;
    d_rotation[i] = make_float4((g.x - y.x * yd) * qn, (g.y - y.y * yd) * qn, (g.z - y.z * yd) * qn, (g.w - y.w * yd) * qn);
  } else {                                       // the clamp is active: q / eps
    d_rotation[i] = make_float4(g.x * qn, g.y * qn, g.z * qn, g.w * qn);
  }
  const float o = 1.0f / (1.0f + expf(-opacity[i]));
  d_opacity[i] = g_opac ? (g_opac[i] * (1.0f - o)) * o : 0.f;
}

// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adam_kernel(const AdamTable tab) {
  const AdamTensor t = tab.t[blockIdx.y];
  const float b1 = tab.b1, b2 = tab.b2, eps = tab.eps, c1 = tab.omb1, c2 = tab.omb2;
  const unsigned long long n4 = t.n >> 2;
  if (t.active) {
    // only the first ga granules of every period: thread <-> (period index, live granule)
    const unsigned gp = t.period >> 2, ga = (t.active + 3u) >> 2;
    const unsigned long long rows = n4 / gp, live = rows * ga;
    for (unsigned long long w = (unsigned long long)blockIdx.x * 256 + threadIdx.x; w < live; w += (unsigned long long)gridDim.x * 256) {
      const unsigned long long row = w / ga;
      const unsigned k = (unsigned)(w - row * ga);
      const unsigned long long q = row * gp + k;
      const float4 g = reinterpret_cast<const float4*>(t.g)[q];
      float4 p = reinterpret_cast<float4*>(t.p)[q], m = reinterpret_cast<float4*>(t.m)[q], v = reinterpret_cast<float4*>(t.v)[q];
      float* pp = &p.x; float* mm = &m.x; float* vv = &v.x; const float* gg = &g.x;
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const float st = (4u * k + c >= t.split) ? t.step_hi : t.step_lo;
        adam_update(pp[c], mm[c], vv[c], gg[c], b1, b2, c1, c2, eps, st);
      }
      reinterpret_cast<float4*>(t.p)[q] = p; reinterpret_cast<float4*>(t.m)[q] = m; reinterpret_cast<float4*>(t.v)[q] = v;
    }
    return;                                        // (API: n is a multiple of the period when `active` is given)
  }
  for (unsigned long long q = (unsigned long long)blockIdx.x * 256 + threadIdx.x; q < n4; q += (unsigned long long)gridDim.x * 256) {
    const float4 g = reinterpret_cast<const float4*>(t.g)[q];
    float4 p = reinterpret_cast<float4*>(t.p)[q], m = reinterpret_cast<float4*>(t.m)[q], v = reinterpret_cast<float4*>(t.v)[q];
    float* pp = &p.x; float* mm = &m.x; float* vv = &v.x; const float* gg = &g.x;
    const unsigned in_period = t.period ? (unsigned)(q % (t.period >> 2)) * 4u : 0u;     // period is a multiple of 4 (checked by the API)
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const float st = (t.period && in_period + c >= t.split) ? t.step_hi : t.step_lo;
      adam_update(pp[c], mm[c], vv[c], gg[c], b1, b2, c1, c2, eps, st);
    }
    reinterpret_cast<float4*>(t.p)[q] = p; reinterpret_cast<float4*>(t.m)[q] = m; reinterpret_cast<float4*>(t.v)[q] = v;
  }
  // tail (n not a multiple of 4): first workgroup
  if (blockIdx.x == 0 && threadIdx.x < (t.n & 3)) {
    const unsigned long long e = (n4 << 2) + threadIdx.x;
    const float st = (t.period && (unsigned)(e % t.period) >= t.split) ? t.step_hi : t.step_lo;
    const float g = t.g[e];
    float m = t.m[e], v = t.v[e], pe = t.p[e];
    adam_update(pe, m, v, g, b1, b2, c1, c2, eps, st);
    t.m[e] = m; t.v[e] = v; t.p[e] = pe;
  }
}

// ---------------------------------------------------------------------------------------------
// Densification statistics of one training iteration (train_mesh_gaussian.py:119-126) in one pass:
//   max_radii2D[vis] = max(max_radii2D[vis], radii[vis])                                            (:123)
//   bc_gradient_accum[vis] += |viewspace_grad[vis, :2]| ;  denom[vis] += 1       (mesh_based_gaussian_model.py:587-589)
// with vis = radii > 0 (render()'s visibility_filter); the reference spends three masked gather / scatter ops on each.
__global__ __launch_bounds__(256) void densify_stats_kernel(int N, const int* __restrict__ radii, const float* __restrict__ grad2d,
                                                            float* __restrict__ max_radii2D, float* __restrict__ grad_accum,
                                                            float* __restrict__ denom) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int r = radii[i];
  if (r <= 0) return;
  max_radii2D[i] = fmaxf(max_radii2D[i], (float)r);
  const float gx = grad2d[3 * (size_t)i], gy = grad2d[3 * (size_t)i + 1];
  grad_accum[i] += sqrtf(gx * gx + gy * gy);
  denom[i] += 1.0f;
}

}  // namespace gm

// ---------------------------------------------------------------------------------------------
// the entry points (include/gmesh_hip.h): their refusals, then the launches
using namespace gm;

// the operands the mesh-bound activation and its adjoint share
static int fill_act(ActArgs& a, int N, float alpha, const float* bc, const float* dist, const float* scaling, const float* rotation,
                    const float* opacity, const float* v1, const float* v2, const float* v3, const float* normal, const float* r) {
  if (N < 0) { set_error("gm_mesh_activate: negative N"); return GM_ERR_INVALID_ARG; }
  if (N > 0 && (!bc || !dist || !scaling || !rotation || !opacity || !v1 || !v2 || !v3 || !normal || !r)) {
    set_error("gm_mesh_activate: null input"); return GM_ERR_INVALID_ARG;
  }
  if (N > 0 && (reinterpret_cast<uintptr_t>(rotation) & 15)) { set_error("gm_mesh_activate: rotation must be 16-byte aligned"); return GM_ERR_INVALID_ARG; }
  a.N = N; a.alpha = alpha; a.bc = bc; a.dist = dist; a.scaling = scaling; a.rotation = rotation; a.opacity = opacity;
  a.v1 = v1; a.v2 = v2; a.v3 = v3; a.normal = normal; a.r = r;
  return GM_OK;
}

extern "C" {

int gm_mesh_activate_fwd(int N, float alpha, const float* bc, const float* dist, const float* scaling, const float* rotation,
                         const float* opacity, const float* v1, const float* v2, const float* v3, const float* normal, const float* r,
                         float* xyz, float* scales, float* rots, float* opac, float mr_weight, float* mr_partial, void* stream) {
  ActArgs a;
  if (int rc = fill_act(a, N, alpha, bc, dist, scaling, rotation, opacity, v1, v2, v3, normal, r)) return rc;
  if (N == 0) return GM_OK;
  if (!xyz || !scales || !rots || !opac || (reinterpret_cast<uintptr_t>(rots) & 15)) {
    set_error("gm_mesh_activate_fwd: null output or unaligned rots"); return GM_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(mesh_activate_fwd_kernel, dim3((N + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a, xyz, scales,
                     reinterpret_cast<float4*>(rots), opac, mr_weight, mr_partial);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_mesh_activate_bwd(int N, float alpha, const float* bc, const float* dist, const float* scaling, const float* rotation,
                         const float* opacity, const float* v1, const float* v2, const float* v3, const float* normal, const float* r,
                         const float* d_xyz, const float* d_scales, const float* d_rots, const float* d_opac, float* d_bc, float* d_dist,
                         float* d_scaling, float* d_rotation, float* d_opacity, float mr_weight, const float* d_mr, void* stream) {
  ActArgs a;
  if (int rc = fill_act(a, N, alpha, bc, dist, scaling, rotation, opacity, v1, v2, v3, normal, r)) return rc;
  if (N == 0) return GM_OK;
  if (!d_bc || !d_dist || !d_scaling || !d_rotation || !d_opacity || (reinterpret_cast<uintptr_t>(d_rotation) & 15) ||
      (d_rots && (reinterpret_cast<uintptr_t>(d_rots) & 15))) {
    set_error("gm_mesh_activate_bwd: null output or unaligned rotation gradient"); return GM_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(mesh_activate_bwd_kernel, dim3((N + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a, d_xyz, d_scales,
                     reinterpret_cast<const float4*>(d_rots), d_opac, d_bc, d_dist, d_scaling, reinterpret_cast<float4*>(d_rotation), d_opacity,
                     mr_weight, d_mr);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_plain_activate_fwd(int N, const float* xyz, const float* scaling, const float* rotation, const float* opacity, float* out_xyz,
                          float* out_scales, float* out_rots, float* out_opac, int row0, int capacity, void* stream) {
  if (N < 0 || row0 < 0 || capacity < 0 || (long long)row0 + N > capacity) {
    set_error("gm_plain_activate_fwd: rows [%d, %d + %d) do not fit a capacity of %d", row0, row0, N, capacity); return GM_ERR_INVALID_ARG;
  }
  if (N == 0) return GM_OK;
  if (!xyz || !scaling || !rotation || !opacity || !out_xyz || !out_scales || !out_rots || !out_opac) {
    set_error("gm_plain_activate_fwd: null pointer"); return GM_ERR_INVALID_ARG;
  }
  if ((reinterpret_cast<uintptr_t>(rotation) | reinterpret_cast<uintptr_t>(out_rots)) & 15) {
    set_error("gm_plain_activate_fwd: rotation / out_rots must be 16-byte aligned"); return GM_ERR_INVALID_ARG;
  }
  const size_t r = (size_t)row0;
  hipLaunchKernelGGL(plain_activate_fwd_kernel, dim3((N + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), N, xyz, scaling,
                     reinterpret_cast<const float4*>(rotation), opacity, out_xyz + 3 * r, out_scales + 3 * r, reinterpret_cast<float4*>(out_rots + 4 * r),
                     out_opac + r);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_plain_activate_bwd(int N, const float* scaling, const float* rotation, const float* opacity, const float* g_xyz, const float* g_scales,
                          const float* g_rots, const float* g_opac, int row0, int capacity, float* d_xyz, float* d_scaling, float* d_rotation,
                          float* d_opacity, void* stream) {
  if (N < 0 || row0 < 0 || capacity < 0 || (long long)row0 + N > capacity) {
    set_error("gm_plain_activate_bwd: rows [%d, %d + %d) do not fit a capacity of %d", row0, row0, N, capacity); return GM_ERR_INVALID_ARG;
  }
  if (N == 0) return GM_OK;
  if (!scaling || !rotation || !opacity || !d_xyz || !d_scaling || !d_rotation || !d_opacity) {
    set_error("gm_plain_activate_bwd: null pointer"); return GM_ERR_INVALID_ARG;
  }
  if ((reinterpret_cast<uintptr_t>(rotation) | reinterpret_cast<uintptr_t>(d_rotation) | reinterpret_cast<uintptr_t>(g_rots)) & 15) {
    set_error("gm_plain_activate_bwd: rotation / g_rots / d_rotation must be 16-byte aligned"); return GM_ERR_INVALID_ARG;
  }
  const size_t r = (size_t)row0;
  hipLaunchKernelGGL(plain_activate_bwd_kernel, dim3((N + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), N, scaling,
                     reinterpret_cast<const float4*>(rotation), opacity, g_xyz ? g_xyz + 3 * r : nullptr, g_scales ? g_scales + 3 * r : nullptr,
                     reinterpret_cast<const float4*>(g_rots ? g_rots + 4 * r : nullptr), g_opac ? g_opac + r : nullptr, d_xyz, d_scaling,
                     reinterpret_cast<float4*>(d_rotation), d_opacity);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_adam_step(int count, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                 const uint64_t* sizes, const float* lr, const float* lr_rest, const uint32_t* period, const uint32_t* split,
                 double beta1, double beta2, double eps, int step, void* stream) {
  return gm_adam_step_active(count, params, grads, exp_avg, exp_avg_sq, sizes, lr, lr_rest, period, split, nullptr, beta1, beta2, eps, step, stream);
}

int gm_adam_step_active(int count, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                        const uint64_t* sizes, const float* lr, const float* lr_rest, const uint32_t* period, const uint32_t* split,
                        const uint32_t* active, double beta1, double beta2, double eps, int step, void* stream) {
  if (count < 0 || count > 8 || step < 1) { set_error("gm_adam_step: 0..8 tensors per call, step >= 1"); return GM_ERR_INVALID_ARG; }
  if (count > 0 && (!params || !grads || !exp_avg || !exp_avg_sq || !sizes || !lr)) { set_error("gm_adam_step: null table"); return GM_ERR_INVALID_ARG; }
  AdamTable tab;
  tab.count = 0; tab.b1 = (float)beta1; tab.b2 = (float)beta2; tab.eps = (float)eps;
  tab.omb1 = (float)(1.0 - beta1); tab.omb2 = (float)(1.0 - beta2);
  const double corr = sqrt(1.0 - pow(beta2, (double)step)) / (1.0 - pow(beta1, (double)step));
  unsigned long long mx = 0;                  // the longest tensor: it sizes the grid
  for (int i = 0; i < count; i++) {
    if (sizes[i] == 0) continue;
    if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i]) { set_error("gm_adam_step: null tensor %d", i); return GM_ERR_INVALID_ARG; }
    if ((reinterpret_cast<uintptr_t>(params[i]) | reinterpret_cast<uintptr_t>(grads[i]) | reinterpret_cast<uintptr_t>(exp_avg[i]) |
         reinterpret_cast<uintptr_t>(exp_avg_sq[i])) & 15) { set_error("gm_adam_step: tensor %d is not 16-byte aligned", i); return GM_ERR_INVALID_ARG; }
    AdamTensor& t = tab.t[tab.count++];
    t.p = params[i]; t.g = grads[i]; t.m = exp_avg[i]; t.v = exp_avg_sq[i]; t.n = sizes[i];
    t.step_lo = (float)(lr[i] * corr);
    t.period = period ? period[i] : 0u; t.split = split ? split[i] : 0u;
    if (t.period & 3u) { set_error("gm_adam_step: period must be a multiple of 4"); return GM_ERR_INVALID_ARG; }
    t.active = (active && active[i] && t.period && active[i] < t.period) ? active[i] : 0u;
    if (t.active && (t.n % t.period) != 0) { set_error("gm_adam_step_active: tensor %d is not a whole number of periods", i); return GM_ERR_INVALID_ARG; }
    t.step_hi = (float)((lr_rest && t.period) ? lr_rest[i] * corr : lr[i] * corr);
    mx = t.n > mx ? t.n : mx;
  }
  if (tab.count == 0) return GM_OK;
  unsigned long long nb = (mx / 4 + 255) / 256;
  if (nb < 1) nb = 1;
  if (nb > 16384) nb = 16384;
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)nb, (unsigned)tab.count), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), tab);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_densify_stats(int N, const int* radii, const float* viewspace_grad, float* max_radii2D, float* grad_accum, float* denom, void* stream) {
  if (N < 0 || (N > 0 && (!radii || !viewspace_grad || !max_radii2D || !grad_accum || !denom))) {
    set_error("gm_densify_stats: bad args"); return GM_ERR_INVALID_ARG;
  }
  if (N == 0) return GM_OK;
  hipLaunchKernelGGL(densify_stats_kernel, dim3((N + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), N, radii, viewspace_grad,
                     max_radii2D, grad_accum, denom);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // extern "C"
