// gm_render_fwd_body.inc -- body of render_fwd_kernel / render_fwd_aux_kernel (gm_render.hip), included once into each kernel.
  const unsigned long long t_start = TRACE ? wall_clock64() : 0ull;
  // frame blockIdx.z of a batch (gm_common.h FrameOfs; a single frame: zero distances, its status words through status_host)
  ranges = frame_ptr(ranges, rf.io); pairs = frame_ptr(pairs, rf.bo); splat = frame_ptr(splat, rf.go); tm.order = frame_ptr(tm.order, rf.io);
  out_color = frame_ptr(out_color, rf.co); counters = frame_ptr(counters, rf.go); epoch = frame_ptr(epoch, rf.io);
  if (STATE) { final_T = frame_ptr(final_T, rf.io); n_contrib = frame_ptr(n_contrib, rf.io); }
  if (rf.frames > 1) status_host = rf.status[blockIdx.z];
  int tr_iters = 0, tr_cand = 0;
  // One 8x8 pixel quadrant = one wave = one workgroup (placed and retired on its own); ids 8 apart share an XCD:
  // id = ((tile slot j) * 4 + quadrant) * 8 + xcd.
  const int lane = threadIdx.x & 63;
  const int wave = (int)((blockIdx.x >> 3) & 3);
  const int tile_block = (int)(((blockIdx.x >> 5) << 3) | (blockIdx.x & 7));
  const bool stale = AUX && aux_latch && aux_latch[GM_CNT_DEPTH_STALE] != 0u;          // AUX: no valid depth_key in this frame - refuse it
  if (AUX && stale && blockIdx.x == 0 && threadIdx.x == 0 && counters[GM_CNT_REFUSED] == 0u) aux_latch[GM_CNT_REFUSED] = 3u;
  if (status_host && blockIdx.x == 0 && threadIdx.x < 4) {               // the frame's status words {num_rendered, -, policy, refused}
    int word = (int)counters[threadIdx.x];
    if (AUX && stale && threadIdx.x == GM_CNT_REFUSED && word == 0) word = 3;
    __hip_atomic_store(status_host + threadIdx.x, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // straight into
  }
  int tx, ty, parent;                                                    // the caller's page-locked words: no copy launch behind the frame
  uint32_t child_bit;
  if (!tm.locate(tile_block, tx, ty, parent, child_bit)) return;
  if (tm.s == 1) child_bit = quadrant_bit(tx, ty, wave);                 // policy 2: the keys carry one bit per 8x8 quadrant of the parent
  const uint2 range = ranges[parent];
  const int n = (AUX && stale) ? 0 : (int)(range.y - range.x);
  const uint2* list = pairs + range.x;           // (key, Gaussian id) per list entry

  const int px = tx * GM_TILE + (wave & 1) * 8 + (lane & 7);
  const int py = ty * GM_TILE + (wave >> 1) * 8 + (lane >> 3);
  const bool inside = px < W && py < H;
  // T > 0: transmittance of a live pixel.  T < 0: the pixel has stopped (reference `done`) and |T| is its final transmittance - a
  // stopped pixel then takes nothing with no extra state: T (1 - alpha) < 0 < 1e-4 is the stop test itself.
  float T = inside ? 1.0f : -1.0f, Cb = 0.f;
#if GM_BLEND_AUX
  float Dz = 0.f;                                                             // sum alpha T z (see render_fwd_aux_kernel for the #if)
#endif
  v2f Crg = {0.f, 0.f};
  uint32_t last = 0;
  int work = 0;                                                               // entries this wave evaluated (wave-uniform): the work hint
  if (n > 0) {
    const float rx0 = (float)(tx * GM_TILE + (wave & 1) * 8), ry0 = (float)(ty * GM_TILE + (wave >> 1) * 8);
    __shared__ FwdLds L;
    __shared__ float4 x_ra[EXACT ? 68 : 1];                                     // EXACT: (x, y, a', c') and b' per survivor
    __shared__ float x_bq[EXACT ? 68 : 1];
    __shared__ uint32_t x_sp[EXACT ? 68 : 1];                                   //        list position + 1 (its place in the colour record holds the opacity)
    __shared__ float x_z[AUX ? 68 : 1];                                         // AUX: (0.99 unless EXACT) z per survivor
    const v2f pixf = {(float)px, (float)py};
    // B operand of the three MFMA steps: monomials (cx^2, cx cy) / (cy^2, cx) / (cy, 1) of this lane's pixel column; k = lane / 32
    const float ccx = (float)(lane & 7) - 3.5f, ccy = (float)((lane >> 3) & 3) - 1.5f;
    const bool khi = lane >= 32;
    const float B0 = khi ? ccx * ccy : ccx * ccx, B1 = khi ? ccx : ccy * ccy, B2 = khi ? 1.0f : ccy;
    const float ucx = rx0 + 3.5f, vcy = ry0 + 1.5f;                            // centre of half 0 (half 1: + 4 rows)
    // rows of a group that hold no survivor are multiplied all the same: they must be finite (their opacity is 0), so the table
    // starts out as zeros and afterwards only ever holds coefficients of real entries
#pragma unroll
    for (int i = 0; i < 12; i++) L.ct[64 * i + lane] = 0.f;
    const int nlast = n - 1;
    int kpos = 0;                                  // next list position to scan
    uint32_t qa_head = 0, qa_cnt = 0;              // candidate ring (wave-uniform)
    uint2 kv[RQ_K];
    auto scan = [&]() {                            // stage A: the chunks in kv, in order, while the ring has room
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
    auto pop = [&](int& count) {                   // stage B: up to 64 candidates, lane j <- candidate j, record loads issued
      count = (int)min(qa_cnt, 64u);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const uint2 cand = lane < count ? L.qa[(qa_head + (uint32_t)lane) & (RQ_QA - 1)] : make_uint2(0u, 0u);
      qa_head += (uint32_t)count; qa_cnt -= (uint32_t)count;
      return issue_gather(splat, cand);
    };
    load_keys();
    scan();                                        // (waits for the first keys)
    load_keys();
    auto step = [&](Gather& cur, int& n0, Gather& nxt, int& n2) -> bool {      // register sets rotate by call site
      if (TRACE) { tr_iters++; tr_cand += n0; }
      const unsigned long long live = __ballot(T > 0.0f);
      if (live == 0ull) return false;
      if (n0 == 0 && qa_cnt == 0u && kpos >= n) return false;
      // cull against the bounding box of the pixels that are still live (lane = y * 8 + x; scalar bit arithmetic)
      uint32_t cols = (uint32_t)live | (uint32_t)(live >> 32);
      cols |= cols >> 16; cols |= cols >> 8; cols &= 0xFFu;
      const float cx0 = rx0 + (float)(__ffs((int)cols) - 1), cx1 = rx0 + (float)(31 - __clz((int)cols));
      const float cy0 = ry0 + (float)((__ffsll(live) - 1) >> 3), cy1 = ry0 + (float)((63 - __clzll((long long)live)) >> 3);
      __builtin_amdgcn_s_waitcnt(0x0F70);                                  // vmcnt(0): the keys and the gather issued last iteration
      scan();
      load_keys();
      nxt = pop(n2);
      if (n0 > 0) {
        const bool keep = lane < n0 && may_touch(cur.a.x, cur.a.y, cur.a.z, cur.a.w, cur.b.x, cur.b.y, cx0, cx1, cy0, cy1);
        const unsigned long long kb = __ballot(keep);
        const int ns = __popcll(kb);
        work += ns;
        // stage the survivors, compacted (slot = rank among the survivors, list order): polynomial coefficients about the two
        // half centres into the MFMA's A layout, colour + opacity, list position
        if (keep) {
          const int slot = (int)lanes_below(kb);
          constexpr bool FOLD = !EXACT;
          if (!EXACT) stage_poly(L.ct, slot, cur.a.x, cur.a.y, cur.a.z, cur.a.w, cur.b.x, cur.b.y, ucx, vcy, FOLD ? 0.0144995696951f : 0.0f);   // -log2(0.99)
          // (r, g, b, w): w = the opacity in the EXACT build, otherwise (the opacity lives in the polynomial) the 1-based list position
          // the backward state wants - one broadcast read per survivor for colour AND n_contrib
          const float cs = FOLD ? 0.99f : 1.0f;
          L.sb[slot] = make_float4(cs * cur.b.z, cs * cur.b.w, cs * cur.c, EXACT ? cur.b.y : (STATE ? __uint_as_float(cur.pos + 1u) : 0.f));
          if (EXACT) {
            x_ra[slot] = make_float4(cur.a.x, cur.a.y, (-0.5f * LOG2E) * cur.a.z, (-0.5f * LOG2E) * cur.b.x);
            x_bq[slot] = (-LOG2E) * cur.a.w;
          }
          if (STATE && EXACT) x_sp[slot] = cur.pos + 1u;   // 1-based list position: n_contrib
          if (AUX) x_z[slot] = cs * __uint_as_float(depth_key[cur.id]);
        }
        // survivors are taken four at a time: the up to three slots behind the last must come out as alpha = 0
        if (!EXACT && lane < 4 && ns + lane < 64) pad_poly(L.ct, ns + lane);
        if (lane < 4) L.sb[ns + lane] = make_float4(0.f, 0.f, 0.f, 0.f);     // (their colours are multiplied by that 0: they must be finite)
        if (AUX && lane < 4) x_z[ns + lane] = 0.f;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // groups of 16 survivors.  (Measured and dropped: issuing the NEXT group's three MFMA steps before the current group's
        // exponents are consumed - two accumulator sets, 142 VGPRs, three waves per SIMD instead of four: 4430 vs 4700 frames/s.)
        auto exponents = [&](const int j) -> v16f {
          if (EXACT) {                                                    // slots behind the last survivor: opacity 0, any exponent will do
            v16f E;
#pragma unroll
            for (int t = 0; t < 16; t++) {
              const int sl = min(j + t, 67);
              v2f dd;
              E[t] = staged_exponent(x_ra[sl], x_bq[sl], pixf, dd);
            }
            return E;
          }
          return poly_exponents(L.ct, j, lane, B0, B1, B2);
        };
        auto blend16 = [&](const v16f& E, const int j) -> bool {          // false: every pixel of the wave has stopped
          constexpr int SUB = GM_FWD_SUB;                                  // survivors per sub-block: their alpha evaluations interleave
#pragma unroll
          for (int q = 0; q < 16 / SUB; q++) {
            if (q > 0 && j + SUB * q >= ns) break;
            float4 S[SUB];
#pragma unroll
            for (int t = 0; t < SUB; t++) S[t] = L.sb[j + SUB * q + t];
            uint32_t SP[SUB];
            if (STATE) {
#pragma unroll
              for (int t = 0; t < SUB; t++) SP[t] = EXACT ? x_sp[j + SUB * q + t] : __float_as_uint(S[t].w);
            }
#if GM_BLEND_AUX
            float Z[SUB];
#pragma unroll
            for (int t = 0; t < SUB; t++) Z[t] = x_z[j + SUB * q + t];
#endif
            float al[SUB]; bool ok[SUB];
#pragma unroll
            for (int t = 0; t < SUB; t++) {
              // opacity * G = 2^e' in one instruction (the opacity is part of the polynomial); EXACT: min(2^e, 1) * opacity, the exponent
              // clamped at 0 by v_exp_f32's clamp bit (see above)
              if (!EXACT) {
                // al[t] = alpha / 0.99: 2^(e' - log2 0.99), clamped to 1 by v_exp's clamp bit (= min(0.99, .) of alpha), 0 where alpha < 1/255
                const float oGp = __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(E[SUB * q + t]), 0.0f, 1.0f);
                ok[t] = oGp >= (1.0f / 255.0f) / 0.99f;
                al[t] = ok[t] ? oGp : 0.0f;
                continue;
              }
              const float oG = S[t].w * __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(E[SUB * q + t]), 0.0f, 1.0f);
              ok[t] = oG >= 1.0f / 255.0f;
              al[t] = ok[t] ? fminf(0.99f, oG) : 0.0f;                                        // skip alpha < 1/255; alpha = min(0.99, .)
            }
#pragma unroll
            for (int t = 0; t < SUB; t++) {          // in list order
              // weight alpha T; T (1 - alpha) as T - alpha T.  Folded form: wa = (alpha / 0.99) T weighs colours staged as 0.99 c
              const float wa = al[t] * T, tt = !EXACT ? __builtin_fmaf(-0.99f, wa, T) : T - wa;
              const bool stop = tt < 0.0001f;                                               // (tt == T >= 1e-4 when alpha == 0; tt < 0 once stopped)
              const float w = stop ? 0.0f : wa;
              T = stop ? -__builtin_fabsf(T) : tt;                                          // stop WITHOUT applying the entry
              const v2f rg = {S[t].x, S[t].y}, ww = {w, w};
              Crg = rg * ww + Crg; Cb += S[t].z * w;
#if GM_BLEND_AUX
              Dz = __builtin_fmaf(Z[t], w, Dz);
#endif
              // accepted <=> alpha >= 1/255 and not stopping (a stopped pixel's T < 0 stops again): the two compares' masks combined on the
              // scalar unit select the list position - one vector instruction where `w > 0 ? .. : ..` took two
              if (STATE) last = (ok[t] && !stop) ? SP[t] : last;
            }
            if (!__any(T > 0.0f)) return false;
          }
          return true;
        };
        for (int j = 0; j < ns; j += 16) {
          const v16f E = exponents(j);
          if (!blend16(E, j)) break;
        }
      }
      return true;
    };
    // TWO register sets (round 4): the batch issued in iteration i is consumed in iteration i + 1 (an iteration is 0.3 - 2 us, an L2
    // hit 0.2 - 0.4 us) and every load issued before an iteration has landed at its top (vmcnt(0)).  Nine registers fewer than with a
    // third set in flight: the image-only kernel needs 95 VGPRs instead of 111 - FIVE waves per SIMD instead of four - and the
    // pipelined loop gains 3.2 % (4820 -> 4980 frames/s, A/B in one call, profiles/r04_ab_sets.txt; the training forward, 104 VGPRs,
    // stays at four waves and gains 3 % from the shorter iteration).  Round 2 chose three sets for a lone wave's latency; what the
    // loop is short of is resident waves.
    int n0, n1 = 0;
    Gather g0 = pop(n0), g1 = g0;
    for (;;) {
      if (!step(g0, n0, g1, n1)) break;
      if (!step(g1, n1, g0, n0)) break;
    }
  }
  if (hint && work > 0 && lane == 0)                                     // (gm_tile_order.h: the next frames' dispatch order)
    atomicMax(&hint[1 + parent], (epoch[0] << 20) | min((uint32_t)work, GM_HINT_WORK_MASK));
  if (inside) {
    const size_t HW = (size_t)H * W, pid = (size_t)W * py + px;
    T = __builtin_fabsf(T);
    if (STATE) { final_T[pid] = T; n_contrib[pid] = last; }
    out_color[pid] = Crg.x + T * bg[0];
    out_color[HW + pid] = Crg.y + T * bg[1];
    out_color[2 * HW + pid] = Cb + T * bg[2];
#if GM_BLEND_AUX
    if (out_alpha) out_alpha[pid] = 1.0f - T;
    if (out_depth) out_depth[pid] = Dz;
#endif
  }
  if (TRACE && lane == 0) {
    unsigned long long* t = trace + 8 * ((size_t)tile_block * 4 + wave);
    t[0] = t_start; t[1] = wall_clock64(); t[2] = (unsigned long long)n;
    t[3] = (unsigned long long)tr_iters | ((unsigned long long)tr_cand << 16) | ((unsigned long long)work << 40);
    t[4] = 0; t[5] = 0;
  }
