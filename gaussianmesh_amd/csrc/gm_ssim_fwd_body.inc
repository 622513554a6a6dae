// Body of ssim_fwd_kernel / ssim_fwd_u8_kernel (gm_loss.hip), included in place: the including kernel defines LS_TARGET_BEGIN (statements run
// once per workgroup before the first target read; may be empty) and LS_TARGET(p) (the target value at element p = plane + row * W + col;
// `plane` is in scope).  An inlined function template is optimised on its own first and changed the float kernels' machine code; a
// fragment leaves it as it was (tools/kernel_disasm.sh).
  // Quantities travel in PAIRS - (x, y), (xx, yy), then xy alone - so that the 11-tap sums run on the packed-f32 pipe (v_pk_fma_f32:
  // two of them per issue slot): three instructions per tap and output instead of five, and one 8-byte LDS access per pair.  Every sum
  // keeps its own order of additions: results are bit-identical to the one-quantity-at-a-time form.
  // LDS: the staged inputs and the horizontal sums share their memory (27.1 KiB per workgroup, five workgroups per CU instead of the
  // three that 41 KiB allowed): the horizontal pass keeps its results in registers until every thread has read its inputs.
  struct Horiz { float2 hb01[LS_SPAN][LS_TILE + 1], hb23[LS_SPAN][LS_TILE + 1]; float hb4[LS_SPAN][LS_TILE + 1]; };
  __shared__ __attribute__((aligned(16))) char lds_raw[sizeof(Horiz)];
  static_assert(sizeof(float2) * LS_SPAN * (LS_SPAN + 1) <= sizeof(Horiz), "the staged inputs fit the horizontal sums' memory");
  float2 (*sxy)[LS_SPAN + 1] = reinterpret_cast<float2 (*)[LS_SPAN + 1]>(lds_raw);          // staged (image, target) with the halo
  Horiz& hz = *reinterpret_cast<Horiz*>(lds_raw);                  // horizontal sums of (x, y), (xx, yy) and xy
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int ox = blockIdx.x * LS_TILE, oy = blockIdx.y * LS_TILE;
  const size_t plane = (size_t)blockIdx.z * H * W;
  LS_TARGET_BEGIN
  for (int i = tid; i < LS_SPAN * LS_SPAN; i += LS_THREADS) {
    const int r = i / LS_SPAN, c = i - r * LS_SPAN;
    const int gx = ox + c - LS_HALO, gy = oy + r - LS_HALO;
    const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;          // zero padding (conv2d padding = 5)
    const size_t p = plane + (size_t)(in ? gy : 0) * W + (in ? gx : 0);
    sxy[r][c] = make_float2(in ? img1[p] : 0.f, in ? LS_TARGET(p) : 0.f);
  }
  __syncthreads();
  // horizontal taps: one work item = 4 adjacent output columns of one row (14 staged values feed 4 x 11 taps);
  // consecutive lanes take consecutive rows (row stride 43 pairs: conflict-free)
  constexpr int HITEMS = LS_SPAN * (LS_TILE / 4), HPASS = (HITEMS + LS_THREADS - 1) / LS_THREADS;     // 336 items, 2 passes
  lv2f h01[HPASS][4], h23[HPASS][4];
  float h4[HPASS][4];
#pragma unroll
  for (int ps = 0; ps < HPASS; ps++) {
    const int i = tid + ps * LS_THREADS;
    if (i < HITEMS) {
      const int r = i % LS_SPAN, c0 = (i / LS_SPAN) * 4;
      lv2f p0[14], p1[14];
      float xy[14];
#pragma unroll
      for (int k = 0; k < 14; k++) {
        const float2 v = sxy[r][c0 + k];
        p0[k] = lv2f{v.x, v.y};
        p1[k] = p0[k] * p0[k];
        xy[k] = v.x * v.y;
      }
#pragma unroll
      for (int o = 0; o < 4; o++) {
        lv2f a01 = {0.f, 0.f}, a23 = {0.f, 0.f};
        float a4 = 0.f;
#pragma unroll
        for (int k = 0; k < 11; k++) {
          const float w = win.w[k];
          const lv2f ww = {w, w};
          a01 = ww * p0[o + k] + a01; a23 = ww * p1[o + k] + a23; a4 += w * xy[o + k];
        }
        h01[ps][o] = a01; h23[ps][o] = a23; h4[ps][o] = a4;
      }
    }
  }
  // the thread's own four pixels (L1 term) before the staged inputs are overwritten
  float2 own[4];
#pragma unroll
  for (int j = 0; j < 4; j++) own[j] = sxy[(tid >> 5) * 4 + j + LS_HALO][(tid & 31) + LS_HALO];
  __syncthreads();
#pragma unroll
  for (int ps = 0; ps < HPASS; ps++) {
    const int i = tid + ps * LS_THREADS;
    if (i < HITEMS) {
      const int r = i % LS_SPAN, c0 = (i / LS_SPAN) * 4;
#pragma unroll
      for (int o = 0; o < 4; o++) {
        hz.hb01[r][c0 + o] = make_float2(h01[ps][o].x, h01[ps][o].y); hz.hb23[r][c0 + o] = make_float2(h23[ps][o].x, h23[ps][o].y);
        hz.hb4[r][c0 + o] = h4[ps][o];
      }
    }
  }
  __syncthreads();
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
  // With or without the maps the same instructions make S: the maps are a uniform branch of ONE kernel.  As two template instantiations
  // the compiler fused different products into the sums of S in each, and where E[xx] - mu^2 cancels (flat regions) the partial sums
  // of a call without the maps differed by several ulps from those of a call with them.
  const bool write_maps = d_mu1 != nullptr;
  const int c = tid & 31;
  float s_sum = 0.f, l1_sum = 0.f;
  // vertical taps: a thread owns 4 adjacent rows of one column (14 values per quantity feed 4 x 11 taps)
  float vq[5][4];
  {
    lv2f c01[14], c23[14];
    float c4[14];
#pragma unroll
    for (int k = 0; k < 14; k++) {
      const float2 u = hz.hb01[(tid >> 5) * 4 + k][c], v = hz.hb23[(tid >> 5) * 4 + k][c];
      c01[k] = lv2f{u.x, u.y}; c23[k] = lv2f{v.x, v.y}; c4[k] = hz.hb4[(tid >> 5) * 4 + k][c];
    }
#pragma unroll
    for (int o = 0; o < 4; o++) {
      lv2f a01 = {0.f, 0.f}, a23 = {0.f, 0.f};
      float a4 = 0.f;
#pragma unroll
      for (int k = 0; k < 11; k++) {
        const float w = win.w[k];
        const lv2f ww = {w, w};
        a01 = ww * c01[o + k] + a01; a23 = ww * c23[o + k] + a23; a4 += w * c4[o + k];
      }
      vq[0][o] = a01.x; vq[1][o] = a01.y; vq[2][o] = a23.x; vq[3][o] = a23.y; vq[4][o] = a4;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int r = (tid >> 5) * 4 + j;
    const float mu1 = vq[0][j], mu2 = vq[1][j], e11 = vq[2][j], e22 = vq[3][j], e12 = vq[4][j];
    const int gx = ox + c, gy = oy + r;
    if (gx < W && gy < H) {
      const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
      const float s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu12;
      const float A1 = 2.f * mu12 + C1, A2 = 2.f * s12 + C2, B1 = mu1_sq + mu2_sq + C1, B2 = s1 + s2 + C2;
      const float inv_b1 = 1.0f / B1, inv_b2 = 1.0f / B2;
      const float S = (A1 * A2) * (inv_b1 * inv_b2);
      s_sum += S;
      l1_sum += fabsf(own[j].x - own[j].y);
      if (write_maps) {
        const size_t p = plane + (size_t)gy * W + gx;
        // S as a function of (mu1, E[xx], E[xy]) with sigma1^2 = E[xx] - mu1^2, sigma12 = E[xy] - mu1 mu2
        const float dS_ds1 = -S * inv_b2;                       // = dS/dE[xx]
        const float dS_ds12 = 2.f * A1 * (inv_b1 * inv_b2);     // = dS/dE[xy]
        d_mu1[p] = 2.f * mu2 * A2 * (inv_b1 * inv_b2) - 2.f * mu1 * S * inv_b1 - 2.f * mu1 * dS_ds1 - mu2 * dS_ds12;
        d_e11[p] = dS_ds1;
        d_e12[p] = dS_ds12;
      }
    }
  }
  const float ts = block_sum(s_sum, red);
  const float tl = block_sum(l1_sum, red);
  if (tid == 0) {
    const size_t b = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partial[2 * b] = ts;
    partial[2 * b + 1] = tl;
  }
