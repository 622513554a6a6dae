// Body of ssim_bwd_kernel / ssim_bwd_u8_kernel (gm_loss.hip), included in place: LS_TARGET_BEGIN as in gm_ssim_fwd_body.inc (run once, before the vertical taps),
// LS_TARGET_PIXEL(p, j): the target at the thread's j-th output pixel (element p).
  // (dS/dmu1, dS/dE[xx]) travel as a pair, dS/dE[xy] alone: packed-f32 sums as in ssim_fwd_kernel
  __shared__ float2 sm01[LS_SPAN][LS_SPAN + 1];
  __shared__ float sm2[LS_SPAN][LS_SPAN + 1];
  __shared__ float2 hb01[LS_SPAN][LS_TILE + 1];
  __shared__ float hb2[LS_SPAN][LS_TILE + 1];
  const int tid = threadIdx.x;
  const int ox = blockIdx.x * LS_TILE, oy = blockIdx.y * LS_TILE;
  const size_t plane = (size_t)blockIdx.z * H * W;
  for (int i = tid; i < LS_SPAN * LS_SPAN; i += LS_THREADS) {
    const int r = i / LS_SPAN, c = i - r * LS_SPAN;
    const int gx = ox + c - LS_HALO, gy = oy + r - LS_HALO;
    const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;          // no ssim-map pixel outside the image
    const size_t p = plane + (size_t)(in ? gy : 0) * W + (in ? gx : 0);
    sm01[r][c] = make_float2(in ? d_mu1[p] : 0.f, in ? d_e11[p] : 0.f);
    sm2[r][c] = in ? d_e12[p] : 0.f;
  }
  __syncthreads();
  for (int i = tid; i < LS_SPAN * (LS_TILE / 4); i += LS_THREADS) {      // see ssim_fwd_kernel
    const int r = i % LS_SPAN, c0 = (i / LS_SPAN) * 4;
    lv2f v01[14];
    float v2[14];
#pragma unroll
    for (int k = 0; k < 14; k++) { const float2 u = sm01[r][c0 + k]; v01[k] = lv2f{u.x, u.y}; v2[k] = sm2[r][c0 + k]; }
#pragma unroll
    for (int o = 0; o < 4; o++) {
      lv2f a01 = {0.f, 0.f};
      float a2 = 0.f;
#pragma unroll
      for (int k = 0; k < 11; k++) {
        const float w = win.w[k];
        const lv2f ww = {w, w};
        a01 = ww * v01[o + k] + a01; a2 += w * v2[o + k];
      }
      hb01[r][c0 + o] = make_float2(a01.x, a01.y); hb2[r][c0 + o] = a2;
    }
  }
  __syncthreads();
  LS_TARGET_BEGIN
  const float gs = g_ssim[blockIdx.z];
  const float gl = g_l1 ? g_l1[0] : 0.f;
  const int c = tid & 31;
  float vq[3][4];
  {
    lv2f c01[14];
    float c2[14];
#pragma unroll
    for (int k = 0; k < 14; k++) { const float2 u = hb01[(tid >> 5) * 4 + k][c]; c01[k] = lv2f{u.x, u.y}; c2[k] = hb2[(tid >> 5) * 4 + k][c]; }
#pragma unroll
    for (int o = 0; o < 4; o++) {
      lv2f a01 = {0.f, 0.f};
      float a2 = 0.f;
#pragma unroll
      for (int k = 0; k < 11; k++) {
        const float w = win.w[k];
        const lv2f ww = {w, w};
        a01 = ww * c01[o + k] + a01; a2 += w * c2[o + k];
      }
      vq[0][o] = a01.x; vq[1][o] = a01.y; vq[2][o] = a2;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int r = (tid >> 5) * 4 + j;
    const float A = vq[0][j], B = vq[1][j], Cc = vq[2][j];
    const int gx = ox + c, gy = oy + r;
    if (gx < W && gy < H) {
      const size_t p = plane + (size_t)gy * W + gx;
      const float x = img1[p], y = LS_TARGET_PIXEL(p, j), d = x - y;
      const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
      dL_dimg1[p] = gs * (A + 2.f * x * B + y * Cc) + gl * sgn;
    }
  }
