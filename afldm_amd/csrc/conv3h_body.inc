// conv3h_body.inc - the tile body of the halo-patch 3x3 convolution, included TEXTUALLY (design notes: conv3h.hip):
//   * by k_conv3h (conv3h.hip) with H3_BX / H3_NBX / H3_BZ = blockIdx.x / gridDim.x / blockIdx.z;
//   * by the merged launches (actconv.hip) as the LAST phase of a workgroup that ran other work before it.
// In scope at the point of inclusion: template parameters T, BM, W_, BN, WGM, WGN, NPROD, TPS, SUB; `ConvP p`;
// `char* smem` (the workgroup's dynamic LDS, LDS_TOTAL bytes, 16-byte aligned).  The early `return`s end the workgroup.
// H3_PRODUCER_EXIT: what an LDS-DMA producer wave does when its K loop is over (`return;` - or, when the workgroup lives on
// after the tile, the epilogue's barriers before it).
// H3_PATCH_AUX: cache-policy bits of the patch LDS-DMA (0; 16 = sc1 when other workgroups wrote the pixels during THIS launch).
// (Textual inclusion keeps k_conv3h's token stream - and so its register allocation - what it was before the split.)
  typedef Mma<T> MM;
  typedef typename MM::Chunk Chunk;
  constexpr int NWC = WGM * WGN, MF = kH3MF, STAGES = kH3Stages;
  constexpr int EPC = MM::EPC, KSTEP = 8 * EPC, ESZ = (int)sizeof(T);
  constexpr int WMS = BM / WGM, WNS = BN / WGN, TM = WMS / MF, TN = WNS / MF;
  constexpr int ROWS = BM / W_, SEG = ROWS < W_ ? ROWS : W_, NSEG = ROWS / SEG;      // planes are square: H == W_
  constexpr int PW = W_ + 2, PR = NSEG * (SEG + 2), NPQ = PR * PW, NPI = (NPQ + 7) / 8;
  constexpr int PATCH = NPI * 1024;
  constexpr int SPC = 9 / TPS;                                   // K steps per channel block
  constexpr int WIT = BN / 8;                                    // weight instructions per tap
  constexpr int WI = TPS * WIT, WPW = WI / NPROD, PPW = (NPI + NPROD - 1) / NPROD;
  constexpr int WPS = WPW / TPS;                                 // weight instructions per wave of a folded-shortcut step: ONE tap's worth
  constexpr int W_TAP = BN * 128, W_STAGE = TPS * W_TAP;
  constexpr int LDS_TOTAL = 2 * PATCH + STAGES * W_STAGE;
  constexpr unsigned OOB = 0x80000000u;
  static_assert(TPS == 1 || TPS == 3, "taps per step");
  static_assert(BM % W_ == 0 && ROWS % SEG == 0 && WI % NPROD == 0 && WMS % MF == 0 && WNS % MF == 0, "tile shape");
  static_assert((STAGES - 2) * WPW + PPW < 64, "vmcnt is a 6-bit counter");
  static_assert(STAGES == 3 && (TPS == 1 || WIT % NPROD == 0), "three-slot ring; three taps per step: a wave's first WPS instructions are the stage's first tap slot");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave_all = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool is_producer = wave_all >= NWC;
  const int li = lane & 15, lg = lane >> 4;             // fragment row / lane group of the consumers

  // Tile order.  Default: each XCD (private L2) takes a contiguous run of tiles, n fastest - it reads 1/8 of the
  // pixels and ALL the weights.  p.xcd_gn > 0: the 8 XCDs form a (8 / gn) x gn grid over (m tiles, n tiles), so an
  // XCD reads gn / 8 of the weights and 1 / (8 / gn) of the pixels - the 4x4 level's 10-21 MB of weights were
  // fetched 8 times otherwise (launch_h3 picks gn from the byte counts).  Same time in the step (those fetches hit
  // the MALL), a third less fabric traffic for the family.
  int tile_m, tile_n;
  if (p.xcd_gn > 0) {
    const int xcd = H3_BX & 7, j = H3_BX >> 3;
    const int gn = p.xcd_gn, tn_per = p.tiles_n / gn, tm_per = (H3_NBX / p.tiles_n) / (8 / gn);
    const int xm = xcd / gn, xn = xcd - xm * gn;
    const int lm = j / tn_per, ln = j - lm * tn_per;
    tile_m = xm * tm_per + lm;
    tile_n = xn * tn_per + ln;
  } else {
    const int tile = xcd_remap(H3_BX, H3_NBX);
    tile_m = tile / p.tiles_n;
    tile_n = tile - tile_m * p.tiles_n;
  }
  static_assert(!SUB || (NSEG == 1 && TPS == 1), "sub-tiled planes: one segment per tile");
  const int n0 = tile_n * BN;
  const int Ct = p.C1, HW = SUB ? p.H * p.W : W_ * W_;
  const int ncb = Ct / KSTEP;
  const int ks = H3_BZ;
  const int cb_lo = (ncb * ks) / p.splitk, cb_hi = (ncb * (ks + 1)) / p.splitk;   // this slice's channel blocks
  // folded 1x1 shortcut (h3_has_shortcut, conv3h_tile.hpp): its nsc channel blocks follow the 3x3 ones as blocks cb_hi .. cb_end - 1 of ONE K
  // step each - the centre tap of a patch whose halo is left zero (never read: no bytes fetched for it).  Three taps per step:
  // such a step fills the stage's first tap slot only; split-K slice ks takes the shortcut blocks [sc_lo, sc_lo + nsc) behind
  // its own 3x3 blocks (the shares may differ by one; the slabs then carry conv + shortcut partial sums).
  constexpr bool HAS_SC = h3_has_shortcut(BN, TPS, SUB);
  const int nsc_all = (HAS_SC && p.sc_x1) ? (p.sc_C1 + p.sc_C2) / KSTEP : 0;
  const int sc_lo = TPS == 3 ? (nsc_all * ks) / p.splitk : 0;
  const int nsc = TPS == 3 ? (nsc_all * (ks + 1)) / p.splitk - sc_lo : nsc_all;
  const int cb_end = cb_hi + nsc;
  const int Gm = (cb_hi - cb_lo) * SPC, G = Gm + nsc;
  int m0, b_tile, oh0, ow0 = 0, sp_tile;                         // first pixel, sample, tile origin, tile index inside the sample
  if constexpr (SUB) {
    const int tw = p.W / W_, tps = (p.H / ROWS) * tw;
    b_tile = tile_m / tps;
    sp_tile = tile_m - b_tile * tps;
    const int ty = sp_tile / tw;
    oh0 = ty * ROWS;
    ow0 = (sp_tile - ty * tw) * W_;
    m0 = b_tile * HW + oh0 * p.W + ow0;
  } else {
    m0 = tile_m * BM;
    b_tile = m0 / HW;
    oh0 = NSEG == 1 ? (m0 - b_tile * HW) / W_ : 0;               // first image row of the (single) segment
    sp_tile = (m0 - b_tile * HW) / BM;
  }
  // global pixel (row of x / y / residual) of tile pixel tp
  auto gpix = [&](int tp) -> int {
    if constexpr (SUB) return m0 + (tp / W_) * p.W + (tp % W_);
    else return m0 + tp;
  };

  if (is_producer) {
    const int wave = wave_all - NWC;
    __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x1, 0, (int)((long long)p.M * Ct * ESZ), 0x00020000);
    __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (int)((long long)p.Cout * 9 * Ct * ESZ), 0x00020000);
    // patch: instruction j covers patch pixels 8 j .. 8 j + 7, lane l = (pixel l >> 3, position l & 7).  Waves whose
    // share is one short re-issue the last instruction (same source, same destination): uniform vmcnt counts.
    unsigned poff[PPW], woff[WPW];
    int pj[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      int j = wave + NPROD * i;
      if (j > NPI - 1) j = NPI - 1;
      pj[i] = j;
      const int q = 8 * j + (lane >> 3);
      const int c = h_chunk_at(lane & 7, h_sw_patch<W_>(q));
      const int pr = q / PW, pc = q - pr * PW;
      const int sg = pr / (SEG + 2), jj = pr - sg * (SEG + 2);            // segment (one sample's rows) and row inside it
      const int ih = oh0 + jj - 1;
      bool ok;
      int pixel;
      if constexpr (SUB) {
        const int iw = ow0 + pc - 1;
        ok = q < NPQ && iw >= 0 && iw < p.W && ih >= 0 && ih < p.H;
        pixel = b_tile * HW + ih * p.W + iw;
      } else {
        ok = q < NPQ && pc >= 1 && pc <= W_ && ih >= 0 && ih < W_;
        pixel = m0 + (sg * SEG + jj - 1) * W_ + (pc - 1);
      }
      if (p.x_c8) {
        const int bb = pixel / HW, pp = pixel - bb * HW;         // chunk c of channel block cb: plane (bb, 8 cb + c), pixel pp
        poff[i] = ok ? (((unsigned)(bb * (Ct / EPC) + c) * (unsigned)HW + (unsigned)pp) * (unsigned)EPC) * ESZ : OOB;
      } else {
        poff[i] = ok ? ((unsigned)pixel * (unsigned)Ct + (unsigned)(c * EPC)) * ESZ : OOB;
      }
    }
#pragma unroll
    for (int i = 0; i < WPW; ++i) {
      const int j = wave + NPROD * i;                            // instruction inside the stage: (tap in step, row group)
      const int tis = j / WIT, r = 8 * (j - tis * WIT) + (lane >> 3);
      const int c = h_chunk_at(lane & 7, h_sw_rows(r));
      woff[i] = (((unsigned)(n0 + r) * 9u + (unsigned)tis) * (unsigned)Ct + (unsigned)(c * EPC)) * ESZ;
    }
    const int Csc = p.sc_C1 + p.sc_C2;
    __amdgpu_buffer_rsrc_t rws = __builtin_amdgcn_make_buffer_rsrc((void*)p.sc_w, 0, (int)((long long)p.Cout * Csc * ESZ), 0x00020000);
    // cursor of the next weight step to issue
    int is_g = 0, is_st = 0, is_cb = cb_lo, is_slot = 0;
    auto issue_weights = [&]() {
      char* sbase = smem + 2 * PATCH + is_slot * W_STAGE;
      if (HAS_SC && is_g >= Gm && is_g < G) {
        // shortcut step: the 1x1 weight rows [n0, n0 + BN) x channel block sc_lo + is_g - Gm, laid out as one tap of the 3x3
        // stream (three taps per step: instructions j < WIT of the stage, i.e. a wave's first WPS - the other two slots stay as they are)
        const unsigned so = (unsigned)((sc_lo + is_g - Gm) * KSTEP * ESZ);
#pragma unroll
        for (int i = 0; i < WPS; ++i) {
          const int r = 8 * (wave + NPROD * i) + (lane >> 3);
          const unsigned wo = ((unsigned)(n0 + r) * (unsigned)Csc + (unsigned)(h_chunk_at(lane & 7, h_sw_rows(r)) * EPC)) * ESZ;
          lds_ptr_t dst = (lds_ptr_t)(sbase + (wave + NPROD * i) * 1024);
          if (p.w_nt) __builtin_amdgcn_raw_ptr_buffer_load_lds(rws, dst, 16, (int)wo, (int)so, 0, 2);
          else __builtin_amdgcn_raw_ptr_buffer_load_lds(rws, dst, 16, (int)wo, (int)so, 0, 0);
        }
      } else {
        const unsigned so = is_g < Gm ? (unsigned)((is_st * TPS * Ct + is_cb * KSTEP) * ESZ) : OOB;
#pragma unroll
        for (int i = 0; i < WPW; ++i) {
          lds_ptr_t dst = (lds_ptr_t)(sbase + (wave + NPROD * i) * 1024);
          if (p.w_nt) __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, dst, 16, (int)woff[i], (int)so, 0, 2);
          else __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, dst, 16, (int)woff[i], (int)so, 0, 0);
        }
      }
      ++is_g;
      if (++is_st == SPC) {
        is_st = 0;
        ++is_cb;
      }
      is_slot = is_slot + 1 == STAGES ? 0 : is_slot + 1;
    };
    auto issue_patch = [&](int cb) {
      char* sbase = smem + ((cb - cb_lo) & 1) * PATCH;
      if (HAS_SC && cb >= cb_hi) {
        // shortcut block j: channels [j KSTEP, (j + 1) KSTEP) of the virtual concat sc_x1 | sc_x2 (NHWC); only the tile's own
        // pixels are fetched (the centre tap never reads the halo), addresses recomputed here - nine times a tile - rather
        // than kept in registers
        const int c0 = (sc_lo + cb - cb_hi) * KSTEP;
        const bool in1 = c0 < p.sc_C1;
        const int Cs = in1 ? p.sc_C1 : p.sc_C2;
        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(in1 ? p.sc_x1 : p.sc_x2), 0,
                                                                     (int)((long long)p.M * Cs * ESZ), 0x00020000);
        const unsigned so = (unsigned)((in1 ? c0 : c0 - p.sc_C1) * ESZ);
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
          const int q = 8 * pj[i] + (lane >> 3);
          const int c = h_chunk_at(lane & 7, h_sw_patch<W_>(q));
          const int pr = q / PW, pc = q - pr * PW;
          const int sg = pr / (SEG + 2), jj = pr - sg * (SEG + 2);
          const bool in = q < NPQ && pc >= 1 && pc <= W_ && jj >= 1 && jj <= SEG;
          const int pixel = m0 + (sg * SEG + jj - 1) * W_ + (pc - 1);
          const unsigned off = in ? ((unsigned)pixel * (unsigned)Cs + (unsigned)(c * EPC)) * ESZ : OOB;
          lds_ptr_t dst = (lds_ptr_t)(sbase + pj[i] * 1024);
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, dst, 16, (int)off, (int)so, 0, 0);
        }
        return;
      }
      const unsigned so = p.x_c8 ? (unsigned)cb * (unsigned)(KSTEP * ESZ) * (unsigned)HW : (unsigned)(cb * KSTEP * ESZ);
#pragma unroll
      for (int i = 0; i < PPW; ++i) {
        lds_ptr_t dst = (lds_ptr_t)(sbase + pj[i] * 1024);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, dst, 16, (int)poff[i], (int)so, 0, H3_PATCH_AUX);
      }
    };
    issue_patch(cb_lo);
#pragma unroll
    for (int s = 0; s < STAGES - 1; ++s) issue_weights();
    int st = 0, cb = cb_lo, since = STAGES;                      // K steps since the last patch issue (in the loop)
    bool fresh = false;                                          // this step's patch was issued one step ago (shortcut blocks)
    for (int g = 0; g < G; ++g) {
      // in flight behind the weights of step g: the weights of steps g+1 .. g+STAGES-2, and - for the STAGES-1 steps
      // after a patch issue - that patch (issued behind step g+STAGES-1's weights of its iteration).  A shortcut block is
      // one step long, so the next one's patch goes out IN FRONT of that step's weights and only those may stay in flight.
      if constexpr (TPS == 1) {
        if (fresh) wait_vmcnt<WPW>();
        else if (since <= STAGES - 1) wait_vmcnt<(STAGES - 2) * WPW + PPW>();
        else wait_vmcnt<(STAGES - 2) * WPW>();
      } else {
        // three-slot stages (STAGES == 3): behind step g's weights lie step g + 1's - WPS instructions when that is a shortcut
        // step, else WPW (the zero-fill tail included) - and a patch issued one or two steps ago in front of a 3x3 block;
        // a shortcut block's patch (fresh) lies in FRONT of step g + 1's weights and is waited for
        const bool sc_next = HAS_SC && g + 1 >= Gm && g + 1 < G;
        const bool patch_behind = !fresh && since <= STAGES - 1;
        if (sc_next) {
          if (patch_behind) wait_vmcnt<WPS + PPW>();
          else wait_vmcnt<WPS>();
        } else {
          if (patch_behind) wait_vmcnt<WPW + PPW>();
          else wait_vmcnt<WPW>();
        }
      }
      __builtin_amdgcn_s_barrier();
      ++since;
      fresh = false;
      if (!(p.dbg & 1)) {
        if (HAS_SC && cb >= cb_hi) {
          if (cb + 1 < cb_end) {
            issue_patch(cb + 1);
            fresh = true;
            since = STAGES;
          }
          issue_weights();
        } else {
          issue_weights();
          if (st == 0 && cb + 1 < cb_end) {
            issue_patch(cb + 1);
            since = 1;
          }
        }
      }
      if ((HAS_SC && cb >= cb_hi) || ++st == SPC) {
        st = 0;
        ++cb;
      }
    }
    wait_vmcnt<0>();   // drain the zero-fill tail before the workgroup's LDS can be re-assigned
    H3_PRODUCER_EXIT
  }

  // ------------------------------------------------------------------------------------------- consumers
  const int cw = wave_all, wm = cw / WGN, wn = cw - wm * WGN;
  constexpr int NKK = 2;                                         // fragment K steps inside a 128-byte row
  int qb[TM];                                                    // patch pixel of (tile pixel, tap (0, 0))
#pragma unroll
  for (int t = 0; t < TM; ++t) {
    const int pix = wm * WMS + t * MF + li;
    const int r = pix / W_, c = pix - r * W_;
    const int sg = r / SEG, rr = r - sg * SEG;
    qb[t] = (sg * (SEG + 2) + rr) * PW + c;
  }
  // fragment address of (row q, K step kk) = (q * 128 + (h_pos(chunk(0, lg), q) << 4)) ^ (kk << 5)
  auto frag_off = [&](int q) { return q * 128 + (h_pos(lg, h_sw_patch<W_>(q)) << 4); };                      // patch rows
  const int a_off0 = (wn * WNS + li) * 128 + (h_pos(lg, h_sw_rows(wn * WNS + li)) << 4);                    // + t * MF * 128 for weight tile t ((row >> 1) & 7 depends on li only)

  // The residual enters through the ACCUMULATORS (fragment layout), a few tiles per K step during the first NRS
  // steps: requested at the top of step s, added at the top of step s + 1 - its latency runs under MFMA work instead
  // of in the epilogue (one dependent global load per copied row was most of the fixed cost of a residual
  // convolution) or in front of the first step.  residual + sum of products, fp32.
  // (split-K: the slabs carry plain partial sums, the reduction kernel adds the epilogue terms)
  auto cout_of = [&](int tn) { return n0 + wn * WNS + tn * MF + 4 * lg; };      // a lane's accumulator: 4 consecutive couts of one pixel
  f32x4 acc[TN][TM];
#pragma unroll
  for (int a = 0; a < TN; ++a)
#pragma unroll
    for (int b = 0; b < TM; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int NRT = TN * TM;                                   // residual quads per lane
  constexpr int NRS = TPS == 1 ? 8 : 3;                          // steps they are spread over (G >= 9 / 3)
  constexpr int RCH = (NRT + NRS - 1) / NRS;
  typedef __attribute__((ext_vector_type(4))) T Quad;
  Quad rv[RCH];
  const bool use_res = p.residual && p.splitk == 1 && !(p.dbg & 16);
  // (fp32 on the 8 + 4 wave tiles: 16-byte residual quads do not fit next to 96 accumulators at 3 waves per SIMD -
  //  there the accumulators simply start from the residual, loaded in front of the first step)
  constexpr bool RSPREAD = !(sizeof(T) == 4 && NWC >= 8);
  if (!RSPREAD && use_res) {
    const T* res = (const T*)p.residual;
#pragma unroll
    for (int a = 0; a < TN; ++a)
#pragma unroll
      for (int b = 0; b < TM; ++b) {
        float r0, r1, r2, r3;
        load4<T>(res + (size_t)gpix(wm * WMS + b * MF + li) * p.res_ld + cout_of(a), r0, r1, r2, r3);
        acc[a][b] = f32x4{r0, r1, r2, r3};
      }
  }
  auto res_issue = [&](int chunk) {
    const T* res = (const T*)p.residual;
#pragma unroll
    for (int k = 0; k < RCH; ++k) {
      const int idx = chunk * RCH + k;
      if (idx < NRT) {
        const int a = idx / TM, b = idx % TM;
        rv[k] = *reinterpret_cast<const Quad*>(res + (size_t)gpix(wm * WMS + b * MF + li) * p.res_ld + cout_of(a));
      }
    }
  };
  auto res_add = [&](int chunk) {
#pragma unroll
    for (int k = 0; k < RCH; ++k) {
      const int idx = chunk * RCH + k;
      if (idx < NRT) {
        const int a = idx / TM, b = idx % TM;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[a][b][e] += to_f32(rv[k][e]);
      }
    }
  };

  // TPS == 3 (the small tiles): the fragment offsets of all nine taps are computed ONCE (9 x TM registers) and the
  // step loop is unrolled over the three filter rows; computed per step (as the TPS == 1 tiles do) they were ~85 VALU
  // instructions in front of every step's first LDS read.
  int btab[TPS == 3 ? 9 : 1][TM];
  if constexpr (TPS == 3) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int t = 0; t < TM; ++t) btab[tap][t] = frag_off(qb[t] + (tap / 3) * PW + (tap - (tap / 3) * 3));
  }
  {
    int slot = 0, st = 0, pbuf = 0;
    auto step_end = [&]() {
      slot = slot + 1 == STAGES ? 0 : slot + 1;
      if (++st == SPC) {
        st = 0;
        pbuf ^= 1;
      }
    };
    // plain form of a K step (fragments of one phase, then its MFMAs; the compiler's own schedule): used for the
    // first NRS steps of a residual convolution, where the residual chunks need the registers the hand-ordered
    // pipeline below spends on fragments in flight
    auto k_step_plain = [&](auto ST) {                 // ST: the step's index inside its channel block when static (TPS == 3), else -1
      constexpr int sst = decltype(ST)::value;
      if (!(p.dbg & 2)) {
        const char* sP = smem + pbuf * PATCH;
        const char* sW = smem + 2 * PATCH + slot * W_STAGE;
#pragma unroll
        for (int ti = 0; ti < TPS; ++ti) {
          const int tap = st * TPS + ti;
          const int tapoff = (tap / 3) * PW + (tap - (tap / 3) * 3);
          int bo[TM];
#pragma unroll
          for (int t = 0; t < TM; ++t) {
            if constexpr (sst >= 0) bo[t] = btab[sst * TPS + ti][t];
            else bo[t] = frag_off(qb[t] + tapoff);
          }
#pragma unroll
          for (int kk = 0; kk < NKK; ++kk) {
            Chunk a[TN], b[TM];
#pragma unroll
            for (int t = 0; t < TN; ++t) a[t] = ld16<Chunk>(sW + ti * W_TAP + ((a_off0 + t * MF * 128) ^ (kk << 5)));
#pragma unroll
            for (int t = 0; t < TM; ++t) b[t] = ld16<Chunk>(sP + (bo[t] ^ (kk << 5)));
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
#pragma unroll
              for (int tm = 0; tm < TM; ++tm) MM::mma(acc[tn][tm], a[tn], b[tm]);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
      step_end();
    };
    auto k_step = [&](auto ST) {                        // ST = -2 (TPS == 3): a folded-shortcut step - the centre tap against the stage's first slot
      constexpr int sst = decltype(ST)::value;
      constexpr int NT = sst == -2 ? 1 : TPS;              // taps of this step
      if (!(p.dbg & 2)) {
        const char* sP = smem + pbuf * PATCH;
        const char* sW = smem + 2 * PATCH + slot * W_STAGE;
        int boff[NT][TM];
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) {
          const int tap = st * TPS + ti;                         // TPS == 3: kh = st, kw = ti
          const int tapoff = (tap / 3) * PW + (tap - (tap / 3) * 3);
#pragma unroll
          for (int t = 0; t < TM; ++t) {
            if constexpr (sst >= 0) boff[ti][t] = btab[sst * TPS + ti][t];
            else if constexpr (sst == -2) boff[ti][t] = btab[TPS == 3 ? 4 : 0][t];
            else boff[ti][t] = frag_off(qb[t] + tapoff);
          }
        }
        // hand-ordered fragment pipeline over the step's TPS x NKK phases of TN MFMA groups (one weight fragment x TM
        // pixel fragments each): weight fragment i + AD is requested when group i starts, the pixel fragments of the
        // next phase in the middle of the current one.  (Left alone the compiler rotates two weight buffers with a
        // distance of ONE group: every group then waits out an LDS round trip.)
        constexpr int NPH = NT * NKK, NG = NPH * TN, AD = 3;
        Chunk af[NG], bf[NPH][TM];
        auto lda = [&](int i) {
          const int ph = i / TN, ti = ph / NKK, kk = ph - ti * NKK;
#ifdef AFLDM_H3_NOLOAD                                                // (timing decomposition build: MFMAs without fragment reads)
          return Chunk{};
#endif
          return ld16<Chunk>(sW + ti * W_TAP + ((a_off0 + (i - ph * TN) * MF * 128) ^ (kk << 5)));
        };
        auto ldb = [&](int ph, int t) {
          const int ti = ph / NKK, kk = ph - ti * NKK;
#ifdef AFLDM_H3_NOLOAD
          return Chunk{};
#endif
          return ld16<Chunk>(sP + (boff[ti][t] ^ (kk << 5)));
        };
#pragma unroll
        for (int t = 0; t < TM; ++t) bf[0][t] = ldb(0, t);
#pragma unroll
        for (int i = 0; i < AD; ++i) af[i] = lda(i);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NG; ++i) {
          if (i + AD < NG) af[i + AD] = lda(i + AD);
          if (i % TN == TN / 2 && i / TN + 1 < NPH) {
#pragma unroll
            for (int t = 0; t < TM; ++t) bf[i / TN + 1][t] = ldb(i / TN + 1, t);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int tm = 0; tm < TM; ++tm) {
#ifdef AFLDM_H3_NOMMA                                                 // (timing decomposition build: fragment reads without MFMAs)
            asm volatile("" ::"v"(af[i]), "v"(bf[i / TN][tm]));
            continue;
#endif
            MM::mma(acc[i % TN][tm], af[i], bf[i / TN][tm]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      step_end();
    };
    typedef std::integral_constant<int, -1> RT;
    int g = 0;
    if (RSPREAD && use_res) {     // (wave-uniform) the first NRS steps, peeled: static accumulator indices for the residual chunks
      auto peeled = [&](auto C) {
        constexpr int c = decltype(C)::value;
        __builtin_amdgcn_s_barrier();
        if (c > 0) res_add(c - 1);
        res_issue(c);
        if constexpr (TPS == 3) k_step_plain(C);      // NRS == SPC == 3: step c of the first channel block
        else k_step_plain(RT{});
      };
      static_assert(TPS == 1 || NRS == SPC, "peeled steps = one channel block");
      peeled(std::integral_constant<int, 0>{});
      peeled(std::integral_constant<int, 1>{});
      peeled(std::integral_constant<int, 2>{});
      if constexpr (NRS > 3) {
        peeled(std::integral_constant<int, 3>{});
        peeled(std::integral_constant<int, 4>{});
        peeled(std::integral_constant<int, 5>{});
        peeled(std::integral_constant<int, 6>{});
        peeled(std::integral_constant<int, 7>{});
      }
      static_assert(NRS == 3 || NRS == 8, "peeled steps");
      res_add(NRS - 1);
      g = NRS;
    }
    if constexpr (TPS == 3) {
      for (; g < Gm; g += 3) {                           // Gm - g is a multiple of SPC = 3
        __builtin_amdgcn_s_barrier();
        k_step(std::integral_constant<int, 0>{});
        __builtin_amdgcn_s_barrier();
        k_step(std::integral_constant<int, 1>{});
        __builtin_amdgcn_s_barrier();
        k_step(std::integral_constant<int, 2>{});
      }
      if constexpr (HAS_SC) {
        for (; g < G; ++g) {                             // folded shortcut: one centre-tap step per channel block
          __builtin_amdgcn_s_barrier();
          k_step(std::integral_constant<int, -2>{});
          st = 0;
          pbuf ^= 1;
        }
      }
    } else {
      for (; g < Gm; ++g) {
        __builtin_amdgcn_s_barrier();
        k_step(RT{});
      }
      for (; HAS_SC && g < G; ++g) {                     // folded shortcut: one centre-tap step per channel block
        __builtin_amdgcn_s_barrier();
        st = 4;
        k_step(RT{});
        st = 0;
        pbuf ^= 1;
      }
    }
  }

  // ------------------------------------------------------------------------------------------- epilogue
  if (p.dbg & 8) return;       // (timing decomposition only)
  if constexpr (ESZ == 2) {
    if (p.splitk == 1) {
      // bf16, whole K in this workgroup: (residual + sum) + (bias + temb) is rounded in the accumulator layout and the
      // tile is staged in bf16 - ONE pass for all BM rows (half the LDS bytes of an fp32 tile, two barriers fewer),
      // then leaves as whole rows, 16 bytes per lane; per-channel GroupNorm partial sums of the stored values
      // accumulated by the thread that owns the column (fixed order, no atomics).
      // A tile of several whole samples (NSEG > 1: the 4x4 planes) carries one (bias + temb) vector and one statistics
      // record per sample.
      constexpr int NTC = NWC * 64, EO = 8, CPR = BN / EO, RPI = NTC / CPR, OROW = BN + 8;
      constexpr int SB_BYTES = ((NSEG * BN * 4 + 1023) / 1024) * 1024, HWT = BM / NSEG;      // rows of one sample segment
      static_assert(SB_BYTES + BM * OROW * 2 <= LDS_TOTAL && RPI * BN * 8 <= LDS_TOTAL, "staging tile");
      float* sB = reinterpret_cast<float*>(smem);        // [NSEG][BN] bias + time embedding per sample of this tile
      T* sO = reinterpret_cast<T*>(smem + SB_BYTES);     // [BM][OROW]
      const T* temb = (const T*)p.temb;
      const int etid = cw * 64 + lane;
      __syncthreads();                                    // pipeline buffers idle
      for (int c = etid; c < NSEG * BN; c += NTC) {
        const int sgi = c / BN, cc = c - sgi * BN;
        float v = p.bias ? p.bias[n0 + cc] : 0.f;
        if (temb) v += to_f32(temb[(size_t)(b_tile + sgi) * p.temb_stride + (n0 + cc) % p.temb_mod]);
        sB[c] = v;
      }
      __syncthreads();
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) {
        const int cl = cout_of(tn) - n0;
#pragma unroll
        for (int t = 0; t < TM; ++t) {
          const int row = wm * WMS + t * MF + li;
          const f32x4 b4 = *reinterpret_cast<const f32x4*>(sB + (NSEG == 1 ? 0 : row / HWT) * BN + cl);
          Quad o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = from_f32<T>(acc[tn][t][e] + b4[e]);
          *reinterpret_cast<Quad*>(sO + row * OROW + cl) = o;
        }
      }
      __syncthreads();
      if constexpr (NSEG > 1) {
        // row lanes are dealt per sample segment: a thread's rows (and its partial sums) belong to ONE sample
        constexpr int RPS = RPI / NSEG;                   // row lanes per segment
        static_assert(RPS >= 1, "row lanes");
        const int ch = etid % CPR, trs = etid / CPR;
        const int sgi = trs / RPS, lr = trs - sgi * RPS;
        const bool active = trs < RPS * NSEG;
        const int n = n0 + ch * EO;
        float ss1[EO], ss2[EO];
#pragma unroll
        for (int e = 0; e < EO; ++e) ss1[e] = ss2[e] = 0.f;
        if (active) {
          for (int r = lr; r < HWT; r += RPS) {
            const int row = sgi * HWT + r;
            const Chunk o = ld16<Chunk>(sO + row * OROW + ch * EO);
            if (!(p.dbg & 4)) st16_out<Chunk>((T*)p.y + (size_t)(m0 + row) * p.y_ld + n, o);
            if (p.stats_out) {
#pragma unroll
              for (int e = 0; e < EO; ++e) {
                const float vr = to_f32(o[e]);
                ss1[e] += vr;
                ss2[e] = fmaf(vr, vr, ss2[e]);
              }
            }
          }
        }
        if (p.stats_out) {
          float* sR = reinterpret_cast<float*>(smem);     // [NSEG * RPS][BN][2]
          __syncthreads();
          if (active) {
#pragma unroll
            for (int e = 0; e < EO; ++e) *reinterpret_cast<f32x2*>(sR + ((trs * BN) + ch * EO + e) * 2) = f32x2{ss1[e], ss2[e]};
          }
          __syncthreads();
          for (int c = etid; c < NSEG * BN; c += NTC) {
            const int sg2 = c / BN, cc = c - sg2 * BN;
            float a1 = 0.f, a2 = 0.f;
            for (int r = 0; r < RPS; ++r) {
              const f32x2 v = *reinterpret_cast<const f32x2*>(sR + (((sg2 * RPS + r) * BN) + cc) * 2);
              a1 += v[0];
              a2 += v[1];
            }
            *reinterpret_cast<f32x2*>(p.stats_out + (((size_t)(b_tile + sg2) * p.stats_S) * p.Cout + n0 + cc) * 2) = f32x2{a1, a2};   // S = 1
          }
        }
        return;
      }
      const bool active = etid < RPI * CPR;
      const int ch = etid % CPR, tr = etid / CPR;
      const int n = n0 + ch * EO;
      float ss1[EO], ss2[EO];
#pragma unroll
      for (int e = 0; e < EO; ++e) ss1[e] = ss2[e] = 0.f;
      if (active) {
#pragma unroll 4
        for (int row = tr; row < BM; row += RPI) {
          const Chunk o = ld16<Chunk>(sO + row * OROW + ch * EO);
          T* ydst = p.y_c8 ? (T*)p.y + (((size_t)b_tile * (p.Cout / EO) + n / EO) * HW + (gpix(row) - b_tile * HW)) * EO
                           : (T*)p.y + (size_t)gpix(row) * p.y_ld + n;
          if (!(p.dbg & 4)) st16_out<Chunk>(ydst, o);      // write-through (build.py: AFLDM_WT)
          if (p.stats_out) {
#pragma unroll
            for (int e = 0; e < EO; ++e) {
              const float vr = to_f32(o[e]);
              ss1[e] += vr;
              ss2[e] = fmaf(vr, vr, ss2[e]);
            }
          }
        }
      }
      if (p.stats_out) {
        // (with a GroupNorm to apply behind the statistics the scratch sits BEHIND the staged tile, which is read once more)
        constexpr int SR_NORM = ((SB_BYTES + BM * OROW * 2 + 15) / 16) * 16;
        // scratch behind the staged tile: sR [RPI][BN][2] + sCol [BN][2] + sG [BN / ncpg][2] (<= BN pairs: one channel per group)
        constexpr bool CAN_NORM = BM == W_ * W_ && SR_NORM + RPI * BN * 8 + BN * 8 + BN * 8 <= LDS_TOTAL;      // the tile is a whole sample
        // the host promises this epilogue for the one-sample 8x8 tiles of 96 couts (norm_fusable in conv.hip: variant 51, bf16)
        static_assert(!(BM == 64 && W_ == 8 && BN == 96 && sizeof(T) == 2) || CAN_NORM, "y_norm epilogue: LDS budget no longer holds for the tiles norm_fusable() accepts");
        const bool do_norm = CAN_NORM && p.y_norm != nullptr;
        float* sR = reinterpret_cast<float*>(smem + (do_norm ? SR_NORM : 0));       // [RPI][BN][2]
        __syncthreads();
        if (active) {
#pragma unroll
          for (int e = 0; e < EO; ++e) *reinterpret_cast<f32x2*>(sR + ((tr * BN) + ch * EO + e) * 2) = f32x2{ss1[e], ss2[e]};
        }
        __syncthreads();
        float* sCol = sR + RPI * BN * 2;                    // [BN][2] column sums (GroupNorm only)
        for (int c = etid; c < BN; c += NTC) {
          float a1 = 0.f, a2 = 0.f;
          for (int r = 0; r < RPI; ++r) {
            const f32x2 v = *reinterpret_cast<const f32x2*>(sR + ((r * BN) + c) * 2);
            a1 += v[0];
            a2 += v[1];
          }
          *reinterpret_cast<f32x2*>(p.stats_out + (((size_t)b_tile * p.stats_S + sp_tile) * p.Cout + n0 + c) * 2) = f32x2{a1, a2};
          if (do_norm) *reinterpret_cast<f32x2*>(sCol + 2 * c) = f32x2{a1, a2};
        }
        if constexpr (CAN_NORM) {
          if (do_norm) {
            // the NEXT GroupNorm from this tile's own sums: the tile is one whole sample and its couts are whole groups, so
            // (mean, rstd) need nobody else (fp64 finish, as every consumer of the partial sums does); the staged rows are
            // normalised and leave a second time - what a stand-alone afldm_gn_apply launch would have re-read from memory
            float* sG = sCol + 2 * BN;                      // [BN / ncpg][2] (mean, rstd)
            __syncthreads();
            const int ng = BN / p.ncpg;
            for (int g = etid; g < ng; g += NTC) {
              double s1 = 0.0, s2 = 0.0;
              for (int k = 0; k < p.ncpg; ++k) {
                s1 += (double)sCol[2 * (g * p.ncpg + k)];
                s2 += (double)sCol[2 * (g * p.ncpg + k) + 1];
              }
              float mean, rstd;
              gn_mean_rstd(s1, s2, (double)BM * p.ncpg, p.neps, mean, rstd);
              sG[2 * g] = mean;
              sG[2 * g + 1] = rstd;
            }
            __syncthreads();
            if (active) {
              float sc[EO], sh[EO];
#pragma unroll
              for (int e = 0; e < EO; ++e) {
                const int c = ch * EO + e, g = c / p.ncpg;
                sc[e] = sG[2 * g + 1] * p.ngamma[n + e];
                sh[e] = p.nbeta[n + e] - sG[2 * g] * sc[e];
              }
#pragma unroll 4
              for (int row = tr; row < BM; row += RPI) {
                const Chunk o = ld16<Chunk>(sO + row * OROW + ch * EO);
                Chunk y;
#pragma unroll
                for (int e = 0; e < EO; ++e) y[e] = from_f32<T>(to_f32(o[e]) * sc[e] + sh[e]);
                st16_out<Chunk>((T*)p.y_norm + (size_t)gpix(row) * p.Cout + n, y);
              }
            }
          }
        }
      }
      return;
    }
  }
  {
    constexpr int SROW = BN + 8;                       // fp32 row stride: conflict-free 16-byte writes
    constexpr int PROWS = BM < 128 ? BM : 128;         // rows staged per pass
    constexpr int PASSES = BM / PROWS;
    constexpr int WPP = WGM / PASSES;                  // consumer wave rows (wm) per pass
    static_assert(PROWS * SROW * 4 <= LDS_TOTAL && WGM % PASSES == 0 && WPP * WMS == PROWS, "staging tile");
    constexpr int NTC = NWC * 64;
    constexpr int EO = 16 / ESZ;                       // output elements per 16-byte store
    constexpr int CPR = BN / EO;                       // 16-byte chunks per row
    constexpr int RPI = NTC / CPR;                     // rows the workgroup covers per sweep
    static_assert(RPI * BN * 2 * 4 <= LDS_TOTAL, "statistics scratch");
    float* sC = reinterpret_cast<float*>(smem);
    const T* temb = (const T*)p.temb;
    const int etid = cw * 64 + lane;
    const bool active = etid < RPI * CPR;
    const int ch = etid % CPR, tr = etid / CPR;
    const int n = n0 + ch * EO;
    // bias + time embedding of the thread's column (one sample per tile): added as ONE vector, acc + (bias + temb)
    float bvec[EO], ss1[EO], ss2[EO];
#pragma unroll
    for (int e = 0; e < EO; ++e) bvec[e] = ss1[e] = ss2[e] = 0.f;
    if (active && p.splitk == 1) {
      if (p.bias) {
#pragma unroll
        for (int q = 0; q < EO / 4; ++q) {
          const f32x4 bv = *reinterpret_cast<const f32x4*>(p.bias + n + 4 * q);
          bvec[4 * q] = bv[0]; bvec[4 * q + 1] = bv[1]; bvec[4 * q + 2] = bv[2]; bvec[4 * q + 3] = bv[3];
        }
      }
      if (temb) {
        const Chunk tv = ld16<Chunk>(temb + (size_t)b_tile * p.temb_stride + n % p.temb_mod);
#pragma unroll
        for (int e = 0; e < EO; ++e) bvec[e] += to_f32(tv[e]);
      }
    }
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
      __syncthreads();   // pipeline buffers idle (first pass) / previous pass copied out
      if (wm / WPP == ps) {
        const int wml = wm - ps * WPP;
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
          for (int t = 0; t < TM; ++t) {
            const int row = wml * WMS + t * MF + li;
            *reinterpret_cast<f32x4*>(sC + row * SROW + (cout_of(tn) - n0)) = acc[tn][t];
            __builtin_amdgcn_sched_barrier(0);
          }
      }
      __syncthreads();
      if (p.splitk > 1) {
        // split-K slab: fp32 rows, 16 bytes per lane
        constexpr int QPR = BN / 4;
#pragma unroll 1
        for (int i = etid; i < PROWS * QPR; i += NTC) {
          const int row = i / QPR, q = i - row * QPR;
          const f32x4 a = *reinterpret_cast<const f32x4*>(sC + row * SROW + 4 * q);
          *reinterpret_cast<f32x4*>(p.ws + ((size_t)ks * p.M + gpix(ps * PROWS + row)) * p.Cout + n0 + 4 * q) = a;
        }
        continue;
      }
      if (active) {
#pragma unroll 2
        for (int row = tr; row < PROWS; row += RPI) {
          const int m = gpix(ps * PROWS + row);
          float v[EO];
#pragma unroll
          for (int q = 0; q < EO / 4; ++q) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(sC + row * SROW + ch * EO + 4 * q);
            v[4 * q] = a[0]; v[4 * q + 1] = a[1]; v[4 * q + 2] = a[2]; v[4 * q + 3] = a[3];
          }
          Chunk o;
#pragma unroll
          for (int e = 0; e < EO; ++e) o[e] = from_f32<T>(v[e] + bvec[e]);       // (residual + sum) + (bias + temb)
          if (!(p.dbg & 4)) st16_out<Chunk>((T*)p.y + (size_t)m * p.y_ld + n, o);
          if (p.stats_out) {
#pragma unroll
            for (int e = 0; e < EO; ++e) {
              const float vr = to_f32(o[e]);      // statistics of what the consumer will read
              ss1[e] += vr;
              ss2[e] = fmaf(vr, vr, ss2[e]);
            }
          }
        }
      }
    }
    if (p.stats_out && p.splitk == 1) {
      // per-channel sums of this tile's BM rows (one split of one sample): the RPI row-interleaved partials of a
      // column are added in a fixed order through LDS
      float* sR = sC;   // [RPI][BN][2]
      __syncthreads();
      if (active) {
#pragma unroll
        for (int e = 0; e < EO; ++e) *reinterpret_cast<f32x2*>(sR + ((tr * BN) + ch * EO + e) * 2) = f32x2{ss1[e], ss2[e]};
      }
      __syncthreads();
      for (int c = etid; c < BN; c += NTC) {
        float a1 = 0.f, a2 = 0.f;
        for (int r = 0; r < RPI; ++r) {
          const f32x2 v = *reinterpret_cast<const f32x2*>(sR + ((r * BN) + c) * 2);
          a1 += v[0];
          a2 += v[1];
        }
        *reinterpret_cast<f32x2*>(p.stats_out + (((size_t)b_tile * p.stats_S + sp_tile) * p.Cout + n0 + c) * 2) = f32x2{a1, a2};
      }
    }
  }
