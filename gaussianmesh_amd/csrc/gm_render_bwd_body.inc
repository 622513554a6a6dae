// gm_render_bwd_body.inc -- body of render_bwd_kernel / render_bwd_aux_kernel (gm_render.hip), included once into each kernel.
  const int lane = threadIdx.x & 63;
  const int wave = (int)((blockIdx.x >> 3) & 3);
  const int tile_block = (int)(((blockIdx.x >> 5) << 3) | (blockIdx.x & 7));
  int tx, ty, parent;
  uint32_t child_bit;
  if ((int)counters[GM_CNT_POLICY] != mode || counters[GM_CNT_REFUSED] != 0u) return;   // lists were built under another emission policy: contribute nothing
  if (!tm.locate(tile_block, tx, ty, parent, child_bit)) return;
  if (tm.s == 1) child_bit = quadrant_bit(tx, ty, wave);
  const uint2 range = ranges[parent];
  const int n = (int)(range.y - range.x);
  if (n == 0) return;
  const uint2* list = pairs + range.x;           // (key, Gaussian id) per list entry
  const size_t HW = (size_t)H * W;

  const int px = tx * GM_TILE + (wave & 1) * 8 + (lane & 7);
  const int py = ty * GM_TILE + (wave >> 1) * 8 + (lane >> 3);
  const bool inside = px < W && py < H;
  const size_t pid = inside ? (size_t)W * py + px : 0;
  const float T_final = inside ? final_T[pid] : 0.f;
  float T = T_final;
  const v2f pix = {(float)px, (float)py};
  const int last = inside ? (int)n_contrib[pid] : 0;
  const float dpr = inside ? dL_dpix[pid] : 0.f, dpg = inside ? dL_dpix[HW + pid] : 0.f, dpb = inside ? dL_dpix[2 * HW + pid] : 0.f;
  float A = T_final * (bg[0] * dpr + bg[1] * dpg + bg[2] * dpb);      // A_i + T_final bg . dL/dpixel (see above)
  const float dpd = (AUX && inside && dL_ddepth) ? dL_ddepth[pid] : 0.f, dpa = (AUX && inside && dL_dalpha) ? dL_dalpha[pid] : 0.f;
  // entries at list positions >= max over the wave of n_contrib are never used: start there
  int max_last = last;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) max_last = max(max_last, __shfl_xor(max_last, d));
  const int start = __builtin_amdgcn_readfirstlane(max_last);   // number of list entries this wave has to visit (positions start-1 .. 0);
                                                                // readfirstlane: the compiler cannot see that the butterfly left a uniform value,
                                                                // and everything the walk's loops carry would otherwise live in vector registers
  if (start == 0) return;

  const float rx0 = (float)(tx * GM_TILE + (wave & 1) * 8), ry0 = (float)(ty * GM_TILE + (wave >> 1) * 8);
  __shared__ BwdLds B;
  BwdLds& L = B;
  // phase 2 geometry of this lane: slot es (7: idle), pixel row r; dL/dpixel of the row's eight pixels stays in registers
  const int es = lane & 7, r = lane >> 3, esc = min(es, 6);
  float2 dq[8];
  float dqb[8], dqd[8];
  __shared__ float x_dd[AUX ? 64 : 1];                               // AUX: dL/ddepth per pixel (kernel start); phase 2: row partials of dL/dz
  B.dpt.rg[lane] = make_float2(dpr, dpg); B.dpt.bl[lane] = dpb;
  if (AUX) x_dd[lane] = dpd;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < 8; i++) {
    dq[i] = B.dpt.rg[r * 8 + i];
    dqb[i] = B.dpt.bl[r * 8 + i];
    if (AUX) dqd[i] = x_dd[r * 8 + i];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const float rowy = ry0 + (float)r;
  const int cl = min(lane, 62), ce = cl / 9, ck = cl - 9 * ce;      // commit role of this lane: value ck of slot ce
  int m = 0;                                                          // slots in use (wave-uniform)
  float2* mrow = &B.M[0][lane];
  SlotB* mslot = &B.slot[0];

  auto phase2 = [&](const int cnt) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const float2 c = B.slot[esc].xy;
    const float x0 = c.x - rx0, dy = c.y - rowy;
    v2f s01 = {0.f, 0.f};
    float s2 = 0.f, s3 = 0.f, s4 = 0.f, s6 = 0.f, sz = 0.f;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const float2 v = B.M[esc][r * 8 + i];                       // (w, h) of pixel i of this lane's row
      const float dx = x0 - (float)i, hx = v.y * dx;
      const v2f ww = {v.x, v.x}, drg = {dq[i].x, dq[i].y};
      s3 += v.y; s4 += hx;
      s6 = __builtin_fmaf(hx, dx, s6);
      s01 = ww * drg + s01;
      s2 = __builtin_fmaf(v.x, dqb[i], s2);
      if (AUX) sz = __builtin_fmaf(v.x, dqd[i], sz);
    }
    const v2f s34 = {s3, s4};
    const float s5 = dy * s34.x, s7 = dy * s34.y, s8 = dy * s5;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");        // every lane has read M before `part` (same storage) is written
    __builtin_amdgcn_wave_barrier();
    float* prow = &B.part[r][es * 9];
    prow[0] = s01.x; prow[1] = s01.y; prow[2] = s2; prow[3] = s34.x; prow[4] = s34.y; prow[5] = s5; prow[6] = s6; prow[7] = s7; prow[8] = s8;
    if (AUX) x_dd[r * 8 + es] = sz;                                 // (x_dd: [row][slot] from here on)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    float tot = 0.f;
#pragma unroll
    for (int q = 0; q < 8; q++) tot += B.part[q][cl];
    const uint32_t gid = B.slot[ce].id;
    if (lane < 63 && ce < cnt) atomicAdd(grad_acc + (size_t)gid * GM_ACC_STRIDE + ck, tot);
    if (AUX && lane < cnt) {                                         // dL/dz of slot `lane`: one more atomic instruction, cnt lanes
      float tz = 0.f;
#pragma unroll
      for (int q = 0; q < 8; q++) tz += x_dd[q * 8 + lane];
      atomicAdd(grad_acc + (size_t)B.slot[lane].id * GM_ACC_STRIDE + 9, tz);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");        // `part` has been read before phase 1 writes M again
    __builtin_amdgcn_wave_barrier();
  };

  // Same front end as render_fwd_kernel, walking the list back to front: chunk lane j <-> position start-1-kpos-j
  // (positions below 0 re-read entry 0 and are not "mine"); candidates enter the ring in descending list position.
  int kpos = 0;                                  // entries scanned so far (from the back)
  uint32_t qa_head = 0, qa_cnt = 0;
  uint2 kv[RQ_K];
  auto scan = [&]() {
    bool go = true;
#pragma unroll
    for (int k = 0; k < RQ_K; k++) {
      go = go && kpos < start && qa_cnt + 64u <= (uint32_t)RQ_QA;
      if (go) {
        const int p = start - 1 - kpos - lane;
        const bool mine = p >= 0 && (kv[k].x & child_bit) != 0u;
        const unsigned long long bal = __ballot(mine);
        if (mine) L.qa[(qa_head + qa_cnt + lanes_below(bal)) & (RQ_QA - 1)] = make_uint2(kv[k].y, (uint32_t)p);
        qa_cnt += (uint32_t)__popcll(bal);
        kpos += 64;
      }
    }
  };
  auto load_keys = [&]() {
#pragma unroll
    for (int k = 0; k < RQ_K; k++) kv[k] = list[max(start - 1 - kpos - k * 64 - lane, 0)];
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
  auto step = [&](Gather& cur, int& n0, const int n1, Gather& nxt, int& n2) -> bool {      // see render_fwd_kernel
    if (n0 == 0 && n1 == 0 && qa_cnt == 0u && kpos >= start) return false;
    __builtin_amdgcn_s_waitcnt(0x0F73);                                  // vmcnt(3): all but the gather issued last iteration (three register sets)
    scan();
    load_keys();
    nxt = pop(n2);
    if (n0 > 0) {
      // A pixel takes part in this batch only if its last contributor lies above the batch's lowest position: cull against
      // the bounding box of those pixels (at the deep end of the walk only the few pixels that reached far into the list
      // are still in play).  Lane = y * 8 + x.
      const int pos_lo = __builtin_amdgcn_readlane((int)cur.pos, n0 - 1);
      const unsigned long long live = __ballot(last > pos_lo);
      float cx0 = rx0, cx1 = rx0 + 7.0f, cy0 = ry0, cy1 = ry0 + 7.0f;
      if (live != 0ull) {
        uint32_t cols = (uint32_t)live | (uint32_t)(live >> 32);
        cols |= cols >> 16; cols |= cols >> 8; cols &= 0xFFu;
        cx0 = rx0 + (float)(__ffs((int)cols) - 1);
        cx1 = rx0 + (float)(31 - __clz((int)cols));
        cy0 = ry0 + (float)((__ffsll(live) - 1) >> 3);
        cy1 = ry0 + (float)((63 - __clzll((long long)live)) >> 3);
      }
      const bool keep = live != 0ull && lane < n0 && may_touch(cur.a.x, cur.a.y, cur.a.z, cur.a.w, cur.b.x, cur.b.y, cx0, cx1, cy0, cy1);
      // compacted, conic pre-multiplied for the exp2 argument, as in render_fwd_kernel
      const unsigned long long kb = __ballot(keep);
      const int ns = __popcll(kb);
      if (keep) {
        const int sl = (int)lanes_below(kb);
        StagedB& o = B.st[sl];
        o.a = make_float4(cur.a.x, cur.a.y, (-0.5f * LOG2E) * cur.a.z, (-0.5f * LOG2E) * cur.b.x);
        o.b = make_float4((-LOG2E) * cur.a.w, cur.b.y, cur.b.z, cur.b.w);
        o.c = make_float4(cur.c, __uint_as_float(cur.pos), __uint_as_float(cur.id),           // 0-based list position == reference `contributor`
                          AUX ? __uint_as_float(depth_key[cur.id]) : 0.f);                  // AUX: z
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      // One staged entry of the walk (records in registers).  Returns nothing; an entry no lane takes costs the exponent and the vote.
      auto entry = [&](const float4& RA, const float4& RB, const float4& RC) {
        v2f dd;
        const float e = staged_exponent(RA, RB.x, pix, dd);             // power * log2(e), pixel-relative form (the forward kernel's polynomial
                                                                         // agrees to ~1e-5; its decisions can differ on an entry in a few 10^5)
        const float G = __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(e), 0.0f, 1.0f);   // exponent clamped at 0, as in the forward kernel
        const float oG = RB.y * G;                                       // opacity * G (the unclamped alpha)
        const int pos = (int)__float_as_uint(RC.y);
        const bool valid = (pos < last) && (oG >= 1.0f / 255.0f);        // (alpha = min(0.99, oG) >= 1/255  <=>  oG >= 1/255)
        if (!__any(valid)) return;
        const float oGe = valid ? oG : 0.0f;                             // a lane that skips the entry: alpha 0, every update the identity
        const float al = __builtin_amdgcn_fmed3f(oGe, 0.0f, 0.99f);      // alpha = min(0.99, opacity G)
        const float inv = __builtin_amdgcn_rcpf(1.f - al);               // 1 / (1 - alpha)
        float cd = __builtin_fmaf(RC.x, dpb, __builtin_fmaf(RB.w, dpg, RB.z * dpr));
        if (AUX) cd += __builtin_fmaf(RC.w, dpd, dpa);                  // the depth (colour z) and alpha (colour 1) channels
        T = T * inv;                                                     // transmittance in front of the entry
        const float wv = al * T;
        const float dL_dalpha = T * cd - A * inv;
        A = __builtin_fmaf(wv, cd, A);
        *mrow = make_float2(wv, oGe * dL_dalpha);                        // M[m][lane]: w ; h = G dL/dG with dL/dG = opacity dL/dalpha
        mslot->xy = make_float2(RA.x, RA.y);                             // slot[m] (uniform address, uniform value)
        mslot->id = __float_as_uint(RC.z);
        mrow += 65; mslot += 1;                                          // the two LDS addresses advance as vector registers of their own:
        m += 1;                                                          // the slot count itself then lives in a scalar register
        if (m == 7) { phase2(7); m = 0; mrow = &B.M[0][lane]; mslot = &B.slot[0]; }
      };
      // Software pipeline of the staged records, round 5: TWO register sets by call site (the loop body is the entry twice).  Entry
      // j + 2's three LDS reads are issued when entry j is done with its set and land while entry j + 1 is walked.  With ONE rotating set
      // (round 4) the compiler copies four values per entry out of the registers the prefetch is about to
      // overwrite (opacity, b', list position, the next LDS address): 4 of the ~28 vector instructions of an entry in a kernel that keeps
      // its SIMDs' vector ALUs 78 % busy (profiles/r05_blend_sq_pmc.txt).
      // (ns == 0 - nothing survived the cull - reads slot 0 and walks nothing)
      const int j1 = max(min(1, ns - 1), 0);
      float4 RA0 = B.st[0].a, RB0 = B.st[0].b, RC0 = B.st[0].c;
      float4 RA1 = B.st[j1].a, RB1 = B.st[j1].b, RC1 = B.st[j1].c;
      for (int j = 0; j < ns; j += 2) {
        entry(RA0, RB0, RC0);
        { const int jn = min(j + 2, ns - 1); RA0 = B.st[jn].a; RB0 = B.st[jn].b; RC0 = B.st[jn].c; }
        if (j + 1 >= ns) break;
        entry(RA1, RB1, RC1);
        { const int jn = min(j + 3, ns - 1); RA1 = B.st[jn].a; RB1 = B.st[jn].b; RC1 = B.st[jn].c; }
      }
    }
    return true;
  };
  int n0, n1, n2 = 0;
  Gather g0 = pop(n0), g1 = pop(n1), g2 = g1;
  for (;;) {
    if (!step(g0, n0, n1, g2, n2)) break;
    if (!step(g1, n1, n2, g0, n0)) break;
    if (!step(g2, n2, n0, g1, n1)) break;
  }
  if (m > 0) phase2(m);
  // verification aid (gm_debug_backward_front_T; null on the product path): the transmittance the walk arrives at in FRONT of a pixel's
  // first entry.  It is final_T divided by (1 - alpha) of every entry the backward took for the pixel: 1 up to rounding when those
  // are the entries the forward blended, off by a factor (1 - alpha) >= 0.4 % for every entry the two halves disagree about.
  if (front_T && inside) front_T[pid] = T;
