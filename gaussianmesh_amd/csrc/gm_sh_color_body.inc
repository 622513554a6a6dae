// gm_sh_color_body.inc -- computeColorFromSH, forward.cu:20-71, as statements included where they run: in preprocess_fwd_kernel
// (gm_preprocess.hip) and in sh_color (gm_pre_body.h, the scene batch's fused pass).  Included in place for the reason given in
// gm_cov3d_body.inc.  The UNROTATED direction (p - campos) / |p - campos|; contraction off in the including scope.
//   in:  p (V3), GM_SH_CAMPOS (float[3]), GM_SH_DEG (degree), GM_SH_LOAD(sh) (statements that fill sh[48] with the row's coefficients)
//   out: col[3] = max(SH(dir) + 0.5, 0), clampbits |= bit ch for each clamped channel ch (clampbits declared and zeroed by the includer)
      float dx = p.x - GM_SH_CAMPOS[0], dy = p.y - GM_SH_CAMPOS[1], dz = p.z - GM_SH_CAMPOS[2];
      const float len = sqrtf(dx * dx + dy * dy + dz * dz);
      dx = dx / len; dy = dy / len; dz = dz / len;
      float sh[48];
      GM_SH_LOAD(sh)
#pragma unroll
      for (int ch = 0; ch < 3; ch++) {
        float r = sh_channel(GM_SH_DEG, [&](int i) { return sh[3 * i + ch]; }, dx, dy, dz);
        r += 0.5f;
        if (r < 0) clampbits |= (uint8_t)(1u << ch);
        col[ch] = fmaxf(r, 0.0f);
      }
