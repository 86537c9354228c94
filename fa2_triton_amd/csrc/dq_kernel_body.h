// dq_kernel_body.h -- the body of the general dQ kernel, included inside dq_kernel (bwd_kernel.h,
// LOCAL = false) and dq_local_kernel (local_kernel.h, LOCAL = true).  In scope at the point of
// inclusion: BF16, DT, CAUSAL, BIASK, DROPOUT, ALIGNED, DQF32, LOCAL and the kernel argument `p`
// (fa2_bwd_args).  See fwd_kernel_body.h for why this is included text.
  using E = Elem<BF16>;
  static_assert(!LOCAL || (!CAUSAL && BIASK == 0 && !DROPOUT), "the window comes without causal / bias / dropout");
  constexpr bool BIAS = BIASK != 0, BIASL = BIASK >= 16;
  constexpr int NW = DqCfg<DT>::NW;
  constexpr int NT = NW * 64;
  constexpr int BM = NW * 32, BN = 64;
  constexpr int KS = DT / 16;
  constexpr int NDT = DT / 32;
  constexpr int TILE = BN * DT * 2;
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE + (BIASL ? NW * kBiasTile : 0)];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r32 = lane & 31, hh = lane >> 5;
  char* const bw = smem + 4 * TILE + w * kBiasTile;  // this wave's bias tile (BIASL)
  // work items head-major per XCD (xcd_item), heaviest first; under a causal mask a workgroup runs
  // a mirrored pair of row blocks of one head (nmb-1-j, then j: equal causal work per workgroup)
  const int nmb = (p.seqlen_q + BM - 1) / BM;
  constexpr bool PAIR = CAUSAL;
  const int per_bh = PAIR ? (nmb + 1) / 2 : nmb;
  const int item = xcd_item(blockIdx.x, gridDim.x);
  const int bh = item / per_bh;
  const int mbi = item - bh * per_bh;
  const int nrep = PAIR && nmb - 1 - mbi != mbi ? 2 : 1;
  for (int rep = 0; rep < nrep; ++rep) {
  if (rep > 0) __syncthreads();  // every wave is past the first item's LDS epilogue
  const int mb = PAIR ? (rep == 0 ? nmb - 1 - mbi : mbi) : (CAUSAL ? (nmb - 1 - mbi) : mbi);
  const int b = bh / p.heads_q, hq = bh - b * p.heads_q;
  const int hkv = hq / (p.heads_q / p.heads_kv);
  int Lq = p.seqlen_q, Lk = p.seqlen_k;
  if (p.cu_seqlens) Lq = Lk = p.cu_seqlens[b + 1] - p.cu_seqlens[b];
  const int D = p.head_dim;
  const int diag = Lk - Lq;
  const int m0 = mb * BM;
  const int mw0 = m0 + 32 * w;
  const int qi = mw0 + r32;
  const float scale = p.softmax_scale, scale2 = scale * kLog2e;

  const uint16_t* kg = (const uint16_t*)p.k + b * p.k_stride[0] + hkv * p.k_stride[2];
  const uint16_t* vg = (const uint16_t*)p.v + b * p.v_stride[0] + hkv * p.v_stride[2];
  const int wleft = LOCAL ? window_bound(p.window_left) : 0, wright = LOCAL ? window_bound(p.window_right) : 0;
  int n_end = 0;
  if (m0 < Lq) {
    n_end = Lk;
    if (CAUSAL) n_end = min(Lk, m0 + BM + diag);
    if constexpr (LOCAL) n_end = min(Lk, m0 + BM + diag + wright);
    n_end = max(n_end, 0);
  }
  // LOCAL: the first tile is the one holding the lowest key the block's first row sees
  int n_begin = 0;
  if constexpr (LOCAL) n_begin = min(max(0, m0 + diag - wleft) & ~(BN - 1), n_end);
  const int ntiles = LOCAL ? (n_end - n_begin + BN - 1) / BN : (n_end + BN - 1) / BN;
  auto kt = [&](int buf) { return smem + buf * 2 * TILE; };
  auto vt = [&](int buf) { return smem + TILE + buf * 2 * TILE; };
  // buffer-resource LDS-DMA, rows past Lk zero-filled; K and V row strides are equal on the
  // aligned path (api.hip), so one set of lane offsets serves both
  BufStager<DT, BN, NT> kst;
  int mrows = 0;
  if (ALIGNED) {
    kst.init(tid, p.k_stride[1], D);
    mrows = BufStager<DT, BN, NT>::max_rows(p.k_stride[1]);
  }
  auto stage_kv = [&](int buf, int n) {
    if constexpr (ALIGNED) {
      kst.issue(kt(buf), kg, p.k_stride[1], n, Lk, mrows);
      kst.issue(vt(buf), vg, p.v_stride[1], n, Lk, mrows);
    } else {
      stage_tile<DT, BN, NT, false>(kt(buf), kg, p.k_stride[1], n, Lk, D, tid);
      stage_tile<DT, BN, NT, false>(vt(buf), vg, p.v_stride[1], n, Lk, D, tid);
    }
  };
  // this wave's bias tiles (BIASL): [32 rows from mw0][64 keys], rows past seqlen_q read as zeros
  using BiasStager = BufStager<64, 32, 64>;
  BiasStager bst;
  const uint16_t* bg = nullptr;
  int brows = 0;
  if constexpr (BIASL) {
    int ln = lane;  // opaque: the offsets are not hoisted out of the item loop (spilled across it)
    asm volatile("" : "+v"(ln));
    bst.init(ln, p.bias_stride[2], 64);
    brows = BiasStager::max_rows(p.bias_stride[2]);
    bg = (const uint16_t*)p.bias + b * p.bias_stride[0] + hq * p.bias_stride[1];
  }
  auto bias_issue = [&](int n) {
    if constexpr (BIASL) {
      const i32x4 r = bias_tile_rsrc(bg + n, p.bias_stride[2], mw0, p.seqlen_q, brows, p.seqlen_k - n, 64);
#pragma unroll
      for (int it = 0; it < BiasStager::kIters; ++it) bst.piece(bw, r, it);
    }
  };
  // bias of the current tile landed; `later` (the next K/V tile's pieces) may stay in flight
  constexpr int kKV = 2 * BufStager<DT, BN, NT>::kIters;
  auto bias_wait = [&](bool later) {
    if constexpr (BIASL) {
      if (later) {
        if constexpr (kKV == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else if constexpr (kKV == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else vm_wait_all();
      } else {
        vm_wait_all();
      }
    }
  };
  auto bias_frag = [&](int h, int g) -> u32x2 {
    if constexpr (BIASL) return bias_tile_frag(bw, r32, hh, h, g);
    else return u32x2{0u, 0u};
  };
  if (ntiles > 0) stage_kv(0, n_begin);

  const bool qvalid = qi < Lq;
  u32x4 qf[KS], of[KS];
  {
    const uint16_t* qrow = (const uint16_t*)p.q + b * p.q_stride[0] + hq * p.q_stride[2] + (int64_t)(qvalid ? qi : 0) * p.q_stride[1];
    const uint16_t* orow = (const uint16_t*)p.dout + b * p.do_stride[0] + hq * p.do_stride[2] + (int64_t)(qvalid ? qi : 0) * p.do_stride[1];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      qf[ks] = load_row_frag<ALIGNED>(qrow, 16 * ks + 8 * hh, D, qvalid);
      of[ks] = load_row_frag<ALIGNED>(orow, 16 * ks + 8 * hh, D, qvalid);
    }
  }
  const int64_t srow = (int64_t)bh * p.lse_row_stride;
  const float lse_i = qvalid ? p.lse[srow + qi] : 0.f;
  // delta_i = rowsum(O * dO) of this lane's row (/root/reference/src/backward/compute_delta.py:
  // 17-73), computed here from the dO fragments already in registers and published to the
  // workspace for dkdv_kernel, which runs after this kernel (rows [Lq, grid rows) get 0)
  float del_i;
  if constexpr (LOCAL) {
    // The same sum formed the way the dP chains form theirs: the diagonal of O dO^T by MFMA (A = the
    // wave's O rows, B = its dO rows, the k-steps in the chains' order from a zero accumulator).
    // A row that sees one key alone has O equal to that key's V row bitwise, so dP - delta is then
    // exactly 0 -- dS, dQ and dK with it -- instead of the last-bit residue of one sum taken in
    // two orders.  C[q'][q] sits in lane (q & 31, h) at register (i & 3) + 8 (i >> 2) + 4 h = q':
    // the diagonal is register (q & 3) + 4 (q >> 3) of the lane with h = (q >> 2) & 1.
    const uint16_t* orow = (const uint16_t*)p.o + b * p.o_stride[0] + hq * p.o_stride[2] + (int64_t)(qvalid ? qi : 0) * p.o_stride[1];
    f32x16 dd = zero16();
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) dd = E::mfma(load_row_frag<ALIGNED>(orow, 16 * ks + 8 * hh, D, qvalid), of[ks], dd);
    const int idx = (r32 & 3) + 4 * (r32 >> 3);
    float mine = dd[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) mine = idx == i ? dd[i] : mine;
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(mine), __float_as_uint(mine), false, false);
    del_i = qvalid ? __uint_as_float(((r32 >> 2) & 1) ? r[1] : r[0]) : 0.f;
    if (hh == 0 && qi < p.lse_row_stride) p.delta[srow + qi] = -del_i;  // negated (delta_kernel)
  } else {
    const uint16_t* orow = (const uint16_t*)p.o + b * p.o_stride[0] + hq * p.o_stride[2] + (int64_t)(qvalid ? qi : 0) * p.o_stride[1];
    float part = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const u32x4 ov = load_row_frag<ALIGNED>(orow, 16 * ks + 8 * hh, D, qvalid);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        part = fmaf(E::to_f32((uint16_t)(ov[j] & 0xFFFF)), E::to_f32((uint16_t)(of[ks][j] & 0xFFFF)), part);
        part = fmaf(E::to_f32((uint16_t)(ov[j] >> 16)), E::to_f32((uint16_t)(of[ks][j] >> 16)), part);
      }
    }
    del_i = qvalid ? half_sum(part) : 0.f;
    if (hh == 0 && qi < p.lse_row_stride) p.delta[srow + qi] = -del_i;  // negated (delta_kernel)
  }

  f32x16 acc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) acc[dt] = zero16();

  __builtin_amdgcn_s_waitcnt(0);  // prologue: Q fragments (compiler-tracked) + first tiles
  __syncthreads();

  // key kj visible to this lane's row iff kj < lim_lane (0 for padded rows)
  int lim_lane = !qvalid ? 0 : (CAUSAL ? min(Lk, qi + diag + 1) : Lk);
  int lo_lane = 0;  // LOCAL: ... and kj >= lo_lane
  if constexpr (LOCAL) {
    lim_lane = !qvalid ? 0 : min(Lk, qi + diag + wright + 1);
    lo_lane = qi + diag - wleft;
  }
  const float sc = BIAS ? 1.f : scale2;
  const float nlse = -lse_i;
  // dropout: Philox offset of (b, hq, qi, key 0), as the forward (fwd_kernel.h)
  uint64_t drop_row = 0;
  float inv_keep = 1.f;
  if (DROPOUT) {
    const uint64_t cu0 = p.cu_seqlens ? (uint64_t)p.cu_seqlens[b] : 0;
    drop_row = (uint64_t)Lk * (cu0 + (uint64_t)Lq * ((uint64_t)hq + (uint64_t)p.heads_q * (p.cu_seqlens ? 0 : b))) +
               (uint64_t)qi * (uint64_t)Lk;
    inv_keep = 1.f / (1.f - p.dropout_p);
  }

  // dropout keep words of this lane's row for the two 32-key halves of a tile (the forward's saved
  // mask, tiled layout of fa2_amd.h), loaded one tile ahead: the loop's vm_wait_all retires them
  uint32_t mwc[2] = {0u, 0u}, mwn[2] = {0u, 0u};
  auto load_mw = [&](int n0, uint32_t* out) {
    if constexpr (DROPOUT) {
      if (p.dropout_mask) {
        const int nrb = (p.seqlen_q + 31) >> 5, ncw = (p.seqlen_k + 31) >> 5;
        const int64_t rowbase = ((int64_t)(b * p.heads_q + hq) * nrb + (qi >> 5)) * ncw;
#pragma unroll
        for (int t = 0; t < 2; ++t)
          out[t] = (qvalid && n0 + 32 * t < p.seqlen_k) ? p.dropout_mask[(rowbase + ((n0 >> 5) + t)) * 32 + (qi & 31)] : 0u;
      }
    }
  };
  // one 64-key tile: S^T and dP^T for both 32-key halves first, then the softmax-gradient
  // VALU of each half beside the other half's MFMAs, then dQ^T += K^T dS^T.
  auto tile = [&](auto mask_c, const char* K, const char* V, int n0, bool later) {
    constexpr bool MASK = decltype(mask_c)::value;
    const int rel = lim_lane - n0 - 4 * hh;
    bias_wait(later);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (MASK && !(n0 + 32 * t < Lk && (!CAUSAL || n0 + 32 * t <= mw0 + 31 + diag))) continue;
      // LOCAL: a 32-key half above or below every row of the wave
      if constexpr (LOCAL && MASK) {
        if (n0 + 32 * t > mw0 + 31 + diag + wright || n0 + 32 * t + 31 < mw0 + diag - wleft) continue;
      }
      f32x16 s = zero16(), dp = zero16();
      {
        constexpr int L = kDqLead < KS ? kDqLead : KS;
        u32x4 fk[KS], fv[KS];
        auto rd = [&](int ks) {
          fk[ks] = lds_row_frag<DT, BN>(K, 32 * t, r32, ks, hh);
          fv[ks] = lds_row_frag<DT, BN>(V, 32 * t, r32, ks, hh);
        };
#pragma unroll
        for (int j = 0; j < L; ++j) rd(j);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          if (ks + L < KS) rd(ks + L);
          s = E::mfma(fk[ks], qf[ks], s);
          dp = E::mfma(fv[ks], of[ks], dp);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      u32x4 dsp[2];
#pragma unroll
      for (int sp = 0; sp < 2; ++sp) {
        float dsv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int i = 8 * sp + j;
          const int o = 32 * t + (i & 3) + 8 * (i >> 2);
          float x = s[i];
          if constexpr (BIASL) {
            x = fmaf(x, scale2, kLog2e * bias_elem<BIASK>(bias_frag(t, i >> 2), i & 3));
          } else if constexpr (BIAS) {
            const int kj = n0 + o + 4 * hh;
            const int kc = kj < Lk ? kj : Lk - 1;
            const int qc = qvalid ? qi : 0;
            x = fmaf(x, scale2, kLog2e * load_bias(p.bias, b * p.bias_stride[0] + hq * p.bias_stride[1] +
                                                             (int64_t)qc * p.bias_stride[2] + kc, p.bias_dtype));
          }
          float pr = __builtin_amdgcn_exp2f(fmaf(x, sc, nlse));
          if (MASK) pr = o < rel ? pr : 0.f;
          if constexpr (LOCAL && MASK) pr = o >= lo_lane - n0 - 4 * hh ? pr : 0.f;
          if (DROPOUT) {  // dS = P (dP~ M / (1 - p) - delta), the forward's keep mask M
            // the forward's keep mask M (fully unrolled here: the rolled dropout_keep16 measured
            // 8 % slower in this kernel, which does not spill either way)
            bool keep;
            if (p.dropout_mask) {  // the forward's saved bits (loaded a tile ahead)
              keep = (mwc[t] >> ((i & 3) + 8 * (i >> 2) + 4 * hh)) & 1u;
            } else {
              const uint64_t kjj = (uint64_t)(n0 + o + 4 * hh);
              keep = philox_uniform(p.dropout_seed, drop_row + kjj) > p.dropout_p;
            }
            dsv[j] = pr * (dp[i] * (keep ? inv_keep : 0.f) - del_i);
          } else {
            dsv[j] = pr * (dp[i] - del_i);  // softmax_scale is applied to dQ once, at the end
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) dsp[sp][j] = E::pack2(dsv[2 * j], dsv[2 * j + 1]);
      }
      __builtin_amdgcn_sched_barrier(0);
      {
        constexpr int N = 2 * NDT, L = 2 * kDqLead < N ? 2 * kDqLead : N;
        u32x4 fr[N];
        auto rd = [&](int m) { return lds_tr_frag<DT, BN>(K, 32 * t + 16 * (m / NDT), 32 * (m % NDT), lane); };
#pragma unroll
        for (int j = 0; j < L; ++j) fr[j] = rd(j);
#pragma unroll
        for (int m = 0; m < N; ++m) {
          if (m + L < N) fr[m + L] = rd(m + L);
          acc[m % NDT] = E::mfma(fr[m], dsp[m / NDT], acc[m % NDT]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  };

  // Interior tiles (no mask, no bias, no dropout): the two 32-key halves are software
  // pipelined inside the tile so that every softmax-gradient VALU op sits beside an MFMA of
  // the same wave:
  //   [S, dP of half 0] [S, dP of half 1 | dS of half 0] [dQ of half 0 | dS 0-7 of half 1]
  //   [dQ of half 1 | dS 8-15 of half 1 beside its first steps]
  auto tile_pipe = [&](const char* K, const char* V, bool later) {
    constexpr int L = kDqPipeLead;  // two score pairs live: one step of fragments in flight
    f32x16 s[2], dp[2];
    u32x4 dsp[2][2];
    u32x2 bz[2];  // bias of the current 4-key group (BIASL), read one element group ahead
    // dS of element e (0..15) of half t -> packed pair in dsp[t]
    float dsv_lo = 0.f;
    auto ds_elem = [&](int t, int e) {
      float x = s[t][e], u = sc;
      if constexpr (BIASL) {
        if ((e & 3) == 0) bz[t] = bias_frag(t, e >> 2);
        x = fmaf(x, p.softmax_scale, bias_elem<BIASK>(bz[t], e & 3));
        u = kLog2e;
      }
      const float pr = __builtin_amdgcn_exp2f(fmaf(x, u, nlse));
      const float d = pr * (dp[t][e] - del_i);
      if (e & 1) dsp[t][e >> 3][(e & 7) >> 1] = E::pack2(dsv_lo, d);
      else dsv_lo = d;
    };
    // S and dP of half t: 2 KS fenced steps; step k of the S/dP chains, VALU hook per step
    auto sdp = [&](int t, auto hook) {
      u32x4 fk[KS], fv[KS];
      auto rd = [&](int ks) {
        fk[ks] = lds_row_frag<DT, BN>(K, 32 * t, r32, ks, hh);
        fv[ks] = lds_row_frag<DT, BN>(V, 32 * t, r32, ks, hh);
      };
#pragma unroll
      for (int j = 0; j < L; ++j) rd(j);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        if (ks + L < KS) rd(ks + L);
        s[t] = E::mfma(fk[ks], qf[ks], ks == 0 ? zero16() : s[t]);
        hook(2 * ks);
        __builtin_amdgcn_sched_barrier(0);
        dp[t] = E::mfma(fv[ks], of[ks], ks == 0 ? zero16() : dp[t]);
        hook(2 * ks + 1);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    // dQ^T += K^T dS^T of half t: 2 NDT fenced steps with a VALU hook per step
    auto dq_half = [&](int t, auto hook) {
      constexpr int N = 2 * NDT, LL = 2 * L < N ? 2 * L : N;
      u32x4 fr[N];
      auto rd = [&](int m) { return lds_tr_frag<DT, BN>(K, 32 * t + 16 * (m / NDT), 32 * (m % NDT), lane); };
#pragma unroll
      for (int j = 0; j < LL; ++j) fr[j] = rd(j);
#pragma unroll
      for (int m = 0; m < N; ++m) {
        if (m + LL < N) fr[m + LL] = rd(m + LL);
        acc[m % NDT] = E::mfma(fr[m], dsp[t][m / NDT], acc[m % NDT]);
        hook(m);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    constexpr int SDP_STEPS = 2 * KS, DQ_STEPS = 2 * NDT;
    sdp(0, [](int) {});
    bias_wait(later);
    sdp(1, [&](int st) {  // 16 dS elements of half 0 over the S/dP steps of half 1
#pragma unroll
      for (int e = st * 16 / SDP_STEPS; e < (st + 1) * 16 / SDP_STEPS; ++e) ds_elem(0, e);
    });
    // dS of half 1: elements 0-7 (packed fragment dsp[1][0]) beside the dQ steps of half 0,
    // elements 8-15 (dsp[1][1], first read at step DQ_STEPS / 2 of dq_half(1)) beside the dQ
    // steps of half 1 that read dsp[1][0].  (All 16 over half 0's dQ steps: 1.8 % slower causal,
    // profiles/r02_ab_dq_spread.txt.)
    dq_half(0, [&](int st) {
#pragma unroll
      for (int e = st * 8 / DQ_STEPS; e < (st + 1) * 8 / DQ_STEPS; ++e) ds_elem(1, e);
    });
    dq_half(1, [&](int st) {
      constexpr int H = DQ_STEPS / 2;
      if (st < H) {
#pragma unroll
        for (int e = 8 + st * 8 / H; e < 8 + (st + 1) * 8 / H; ++e) ds_elem(1, e);
      }
    });
  };

  load_mw(0, mwc);
  for (int it = 0; it < ntiles; ++it) {
    const int cur = it & 1;
    const int n0 = LOCAL ? n_begin + it * BN : it * BN;
    // wave-uniform tile class; LOCAL: the wave's rows see keys [mw0 + diag - left, mw0 + 31 + diag + right]
    bool dead = CAUSAL && (n0 > mw0 + 31 + diag);
    if constexpr (LOCAL) dead = n0 > mw0 + 31 + diag + wright || n0 + BN - 1 < mw0 + diag - wleft;
    // (the bias tile first: its counted wait leaves the next K/V tile in flight)
    if (!dead) bias_issue(n0);
    const bool later = it + 1 < ntiles;
    if (DROPOUT && later) load_mw(n0 + BN, mwn);
    if (later) stage_kv(cur ^ 1, n0 + BN);
    bool need_mask = (n0 + BN > Lk) || (mw0 + 31 >= Lq) || (CAUSAL && n0 + BN - 1 > mw0 + diag);
    if constexpr (LOCAL) need_mask = need_mask || n0 + BN - 1 > mw0 + diag + wright || n0 < mw0 + 31 + diag - wleft;
    if (!dead) {
      if (need_mask)
        tile(std::true_type{}, kt(cur), vt(cur), n0, later);
      else if constexpr ((!BIAS || BIASL) && !DROPOUT)
        tile_pipe(kt(cur), vt(cur), later);
      else
        tile(std::false_type{}, kt(cur), vt(cur), n0, later);
    }
    vm_wait_all();
    __syncthreads();
    if constexpr (DROPOUT) {
      mwc[0] = mwn[0];
      mwc[1] = mwn[1];
    }
  }

  if constexpr (ALIGNED && !DQF32) {
    // the last tile's barrier is behind every wave: the K/V buffers hold the staging images
    uint16_t* q0 = (uint16_t*)p.dq + b * p.dq_stride[0] + hq * p.dq_stride[2] + (int64_t)mw0 * p.dq_stride[1];
    store_rows_lds<BF16, DT>(smem + w * 32 * DT * 2, acc, scale, qvalid, q0, p.dq_stride[1],
                             min(32, p.seqlen_q - mw0), D, lane);
  } else if (qi < p.seqlen_q) {
    const bool ok = qvalid;
    char* base = (char*)p.dq;
    const int esz = DQF32 ? 4 : 2;
    char* row = base + (int64_t)esz * (b * p.dq_stride[0] + hq * p.dq_stride[2] + (int64_t)qi * p.dq_stride[1]);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d0 = 32 * dt + 8 * g4 + 4 * hh;
        float a[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = ok ? acc[dt][4 * g4 + j] * scale : 0.f;
        if (DQF32) {
          float* r = (float*)row;
          if (ALIGNED) {
            if (d0 < D) *(f32x4*)(r + d0) = f32x4{a[0], a[1], a[2], a[3]};
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (d0 + j < D) r[d0 + j] = a[j];
          }
        } else {
          uint16_t* r = (uint16_t*)row;
          if (ALIGNED) {
            if (d0 < D) *(u32x2*)(r + d0) = u32x2{E::pack2(a[0], a[1]), E::pack2(a[2], a[3])};
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (d0 + j < D) r[d0 + j] = E::from_f32(a[j]);
          }
        }
      }
    }
  }
  }
