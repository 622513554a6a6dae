// gm_cov3d_body.inc -- computeCov3D, forward.cu:118-152, as statements included where they run: in preprocess_fwd_kernel
// (gm_preprocess.hip) and in cov3d_from_scale_rot (gm_pre_body.h, the scene batch's fused pass).  Included in place rather than
// called, so that preprocess_fwd_kernel's machine code is what it was when the block was written out in it (an inlined call is
// optimised on its own first and comes out differently).  Contraction off in the including scope.
//   in:  q (float4: r, x, y, z), GM_COV3D_SCALE(k) (scale k times the scale modifier, evaluated after the rotation is built)
//   out: c3[6], the entries xx xy xz yy yz zz of (S R)^T (S R)
      float Rg[9], Mc[9];
      quat_cols(q.x, q.y, q.z, q.w, Rg);
      const float s[3] = {GM_COV3D_SCALE(0), GM_COV3D_SCALE(1), GM_COV3D_SCALE(2)};
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
        for (int k = 0; k < 3; k++) Mc[3 * c + k] = s[k] * Rg[3 * c + k];
#define SIG(u, w) (Mc[3 * u + 0] * Mc[3 * w + 0] + Mc[3 * u + 1] * Mc[3 * w + 1] + Mc[3 * u + 2] * Mc[3 * w + 2])
      c3[0] = SIG(0, 0); c3[1] = SIG(0, 1); c3[2] = SIG(0, 2); c3[3] = SIG(1, 1); c3[4] = SIG(1, 2); c3[5] = SIG(2, 2);
#undef SIG
