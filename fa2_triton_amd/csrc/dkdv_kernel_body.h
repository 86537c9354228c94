// dkdv_kernel_body.h -- the body of the general dK/dV kernel, included inside dkdv_kernel
// (bwd_kernel.h, LOCAL = false) and dkdv_local_kernel (local_kernel.h, LOCAL = true).  In scope at
// the point of inclusion: BF16, DT, CAUSAL, BIASK, DROPOUT, ALIGNED, LOCAL, the kernel argument `p`
// (fa2_bwd_args) and `nsplit`.  See fwd_kernel_body.h for why this is included text.
  using E = Elem<BF16>;
  static_assert(!LOCAL || (!CAUSAL && BIASK == 0 && !DROPOUT), "the window comes without causal / bias / dropout");
  constexpr bool BIAS = BIASK != 0, BIASL = BIASK >= 16;
  constexpr int kBiasKTile = 32 * 32 * 2;  // one wave's [32 rows][32 keys] bias tile
  constexpr int NT = 256;
  constexpr int BNK = 128;          // keys per workgroup
  constexpr int BMQ = 32;           // query rows per tile
  constexpr int KS = DT / 16;
  constexpr int NDT = DT / 32;
  constexpr int VT = BNK * DT * 2;  // V tile bytes
  constexpr int QT = BMQ * DT * 2;  // Q (or dO) tile bytes
  constexpr int ST = 2 * BMQ * 4;   // LSE2 + delta rows of a tile
  __shared__ __attribute__((aligned(16))) char smem[VT + 4 * QT + 2 * ST + (BIASL ? 4 * kBiasKTile : 0)];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wu = __builtin_amdgcn_readfirstlane(w);  // the same, in an SGPR: scalar branches
  const int r32 = lane & 31, hh = lane >> 5;
  const int nkb = (p.seqlen_k + BNK - 1) / BNK;
  const int item = xcd_item(blockIdx.x, gridDim.x);  // head-major, see xcd_item
  const int grp = item / nkb;                        // (batch, kv-head, q-head split)
  const int n0 = (item - grp * nkb) * BNK;           // causal: low keys see the most rows
  const int bkv = grp / nsplit, split = grp - bkv * nsplit;
  const int b = bkv / p.heads_kv, hkv = bkv - b * p.heads_kv;
  const int G = p.heads_q / p.heads_kv / nsplit;     // q-heads of this workgroup
  const int h0 = (hkv * nsplit + split) * G;         // its first q-head
  int Lq = p.seqlen_q, Lk = p.seqlen_k;
  if (p.cu_seqlens) Lq = Lk = p.cu_seqlens[b + 1] - p.cu_seqlens[b];
  const int D = p.head_dim;
  const int diag = Lk - Lq;
  const int kw0 = n0 + 32 * w;   // first key of this wave
  const int kj = kw0 + r32;      // this lane's key
  const bool kval = kj < Lk;
  const float scale = p.softmax_scale, scale2 = scale * kLog2e;
  const float sc = BIAS ? 1.f : scale2;
  // dropout: flat Philox offset of (b, hq, row, key) exactly as the forward (fwd_kernel.h)
  const int cu0 = p.cu_seqlens ? p.cu_seqlens[b] : 0;
  auto drop_base = [&](int hq_) -> uint64_t {
    return (uint64_t)Lk * ((uint64_t)cu0 + (uint64_t)Lq * ((uint64_t)hq_ + (uint64_t)p.heads_q * (p.cu_seqlens ? 0 : b)));
  };
  const float inv_keep = DROPOUT ? 1.f / (1.f - p.dropout_p) : 1.f;

  char* Vs = smem;
  auto qt = [&](int buf) { return smem + VT + buf * 2 * QT; };
  auto ot = [&](int buf) { return smem + VT + QT + buf * 2 * QT; };
  auto st = [&](int buf) { return smem + VT + 4 * QT + buf * ST; };

  // query tiles: causal -> the first row that sees key n0 is n0 - diag
  const int wleft = LOCAL ? window_bound(p.window_left) : 0, wright = LOCAL ? window_bound(p.window_right) : 0;
  int m_begin = 0;
  if (CAUSAL) m_begin = max(0, n0 - diag) & ~(BMQ - 1);
  if constexpr (LOCAL) m_begin = max(0, n0 - diag - wright) & ~(BMQ - 1);
  int n_mt = (n0 < Lk && m_begin < Lq) ? (Lq - m_begin + BMQ - 1) / BMQ : 0;
  if constexpr (LOCAL) {
    // one past the last row that sees the block's last key
    const int m_end = min(Lq, n0 + BNK - diag + wleft);
    n_mt = (n0 < Lk && m_begin < m_end) ? (m_end - m_begin + BMQ - 1) / BMQ : 0;
  }
  // Query tiles are swept from the last one down: every workgroup of a (batch, kv-head) then
  // reads the same Q / dO tile at the same step -- one HBM read, the other key blocks hit L2 --
  // where an ascending sweep from each block's own first visible tile spreads the reads of one
  // tile over the whole pass (dkdv HBM reads halved).
  const int m_last = m_begin + (n_mt - 1) * BMQ;
  auto tile_row = [&](int t) { return m_last - t * BMQ; };
  const int total = n_mt * G;  // (q-head, tile) steps

  // buffer-resource LDS-DMA (rows past Lq read as zeros; masked out of every product)
  BufStager<DT, BMQ, NT> qst, ost;
  int qrows = 0, orows = 0;
  if (ALIGNED) {
    qst.init(tid, p.q_stride[1], D);
    ost.init(tid, p.do_stride[1], D);
    qrows = BufStager<DT, BMQ, NT>::max_rows(p.q_stride[1]);
    orows = BufStager<DT, BMQ, NT>::max_rows(p.do_stride[1]);
  }
  int st_g = 0, st_mt = 0;  // (q-head in group, query tile) of the next step to stage
  auto stage = [&](int buf) {
    const int hq = h0 + st_g;
    const int m = tile_row(st_mt);
    if (++st_mt == n_mt) {
      st_mt = 0;
      ++st_g;
    }
    const uint16_t* qg = (const uint16_t*)p.q + b * p.q_stride[0] + hq * p.q_stride[2];
    const uint16_t* og = (const uint16_t*)p.dout + b * p.do_stride[0] + hq * p.do_stride[2];
    if constexpr (ALIGNED) {
      qst.issue(qt(buf), qg, p.q_stride[1], m, Lq, qrows);
      ost.issue(ot(buf), og, p.do_stride[1], m, Lq, orows);
    } else {
      stage_tile<DT, BMQ, NT, false>(qt(buf), qg, p.q_stride[1], m, Lq, D, tid);
      stage_tile<DT, BMQ, NT, false>(ot(buf), og, p.do_stride[1], m, Lq, D, tid);
    }
    if (wu < 2) {  // LSE2 rows (wave 0) then delta rows (wave 1): 32 dwords each, lanes 0..31
      // wave-uniform row bases in SGPR descriptors (no per-lane 64-bit address at the register
      // limit)
      const int64_t row0 = (int64_t)(b * p.heads_q + hq) * p.lse_row_stride + m;
      const uint32_t lds = __builtin_amdgcn_readfirstlane(lds_addr(st(buf))) + wu * BMQ * 4;
      int t = threadIdx.x;
      asm volatile("" : "+v"(t));
      blds4_lo32((uint32_t)(t & 31) * 4u, make_rsrc((wu == 0 ? p.lse : p.delta) + row0, BMQ * 4), lds);
    }
  };
  // The same staging for the descending sweep with every address carried from step to step in
  // SGPRs: the byte address of the next tile's first Q / dO row and the index of its first
  // LSE2 / delta row move by one tile per step and jump to the next q-head's last tile when the
  // head changes, so a step's staging is a few scalar adds and the descriptor words.  (Recomputed
  // per step from the head and row indices, the 64-bit address arithmetic of `stage` put ~130
  // scalar instructions in front of every step; a timing ablation without it ran 4-7 % faster.)
  const int64_t q_rb = p.q_stride[1] * 2, o_rb = p.do_stride[1] * 2;  // row bytes
  uint64_t nq = 0, no = 0;  // next tile's first-row byte addresses
  int64_t nl = 0;           // next tile's first LSE2 / delta element
  int nm = m_last;          // next tile's first row
  if constexpr (ALIGNED) {
    nq = uniform64((int64_t)(uintptr_t)p.q + 2 * (b * p.q_stride[0] + h0 * p.q_stride[2]) + (int64_t)m_last * q_rb);
    no = uniform64((int64_t)(uintptr_t)p.dout + 2 * (b * p.do_stride[0] + h0 * p.do_stride[2]) + (int64_t)m_last * o_rb);
    nl = uniform64((int64_t)(b * p.heads_q + h0) * p.lse_row_stride + m_last);
  }
  const int64_t q_wrap = (int64_t)(n_mt - 1) * BMQ * q_rb + 2 * p.q_stride[2];
  const int64_t o_wrap = (int64_t)(n_mt - 1) * BMQ * o_rb + 2 * p.do_stride[2];
  const int64_t l_wrap = (int64_t)(n_mt - 1) * BMQ + p.lse_row_stride;
  auto stage_desc = [&](int buf) {
    const int rows = Lq - nm;  // >= 1: rows past Lq read as zeros (descriptor range)
    const i32x4 rq = make_rsrc((const void*)(uintptr_t)nq, (uint32_t)min(rows, qrows) * (uint32_t)q_rb);
    const i32x4 ro = make_rsrc((const void*)(uintptr_t)no, (uint32_t)min(rows, orows) * (uint32_t)o_rb);
#pragma unroll
    for (int it = 0; it < BufStager<DT, BMQ, NT>::kIters; ++it) {
      qst.piece(qt(buf), rq, it);
      ost.piece(ot(buf), ro, it);
    }
    if (wu < 2) {
      const uint32_t lds = __builtin_amdgcn_readfirstlane(lds_addr(st(buf))) + wu * BMQ * 4;
      int t = threadIdx.x;
      asm volatile("" : "+v"(t));
      blds4_lo32((uint32_t)(t & 31) * 4u, make_rsrc((wu == 0 ? p.lse : p.delta) + nl, BMQ * 4), lds);
    }
    if (++st_mt == n_mt) {
      st_mt = 0;
      nm = m_last;
      nq = uniform64(nq + q_wrap);
      no = uniform64(no + o_wrap);
      nl = uniform64(nl + l_wrap);
    } else {
      nm -= BMQ;
      nq = uniform64(nq - BMQ * q_rb);
      no = uniform64(no - BMQ * o_rb);
      nl = uniform64(nl - BMQ);
    }
  };

  // this wave's bias tiles (BIASL): [32 query rows from m][32 keys from kw0] of step (hq, m)
  using BiasStager = BufStager<32, 32, 64>;
  BiasStager bst;
  int brows = 0;
  char* const bwk = smem + VT + 4 * QT + 2 * ST + w * kBiasKTile;
  if constexpr (BIASL) {
    bst.init(lane, p.bias_stride[2], 32);
    brows = BiasStager::max_rows(p.bias_stride[2]);
  }
  auto bias_issue = [&](int hq_, int m_) {
    if constexpr (BIASL) {
      const uint16_t* bg = (const uint16_t*)p.bias + b * p.bias_stride[0] + hq_ * p.bias_stride[1] + kw0;
      const i32x4 r = bias_tile_rsrc(bg, p.bias_stride[2], m_, p.seqlen_q, brows, p.seqlen_k - kw0, 32);
#pragma unroll
      for (int it = 0; it < BiasStager::kIters; ++it) bst.piece(bwk, r, it);
    }
  };
  // the bias of register i (query row m + (i & 3) + 8 (i >> 2) + 4 hh, this lane's key): element
  // i & 7 of transposed read i >> 3
  auto bias_rd = [&](int half) -> u32x4 { return lds_tr_frag<32, 32>(bwk, 16 * half, 0, lane); };
  auto bias_of = [&](const u32x4* bt2, int i) -> float {
    const int j = i & 7;
    const u32x2 pair = {bt2[i >> 3][(j >> 2) * 2], bt2[i >> 3][(j >> 2) * 2 + 1]};
    return bias_elem<BIASK>(pair, j & 3);
  };

  u32x4 kf[KS];
  {
    const uint16_t* krow = (const uint16_t*)p.k + b * p.k_stride[0] + hkv * p.k_stride[2] + (int64_t)(kval ? kj : 0) * p.k_stride[1];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) kf[ks] = load_row_frag<ALIGNED>(krow, 16 * ks + 8 * hh, D, kval);
  }
  if (total > 0) {
    const uint16_t* vg = (const uint16_t*)p.v + b * p.v_stride[0] + hkv * p.v_stride[2];
    stage_tile<DT, BNK, NT, ALIGNED>(Vs, vg, p.v_stride[1], n0, Lk, D, tid);
    if constexpr (ALIGNED) stage_desc(0);
    else stage(0);
    bias_issue(h0, tile_row(0));
  }
  f32x16 dk[NDT], dv[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) { dk[dt] = zero16(); dv[dt] = zero16(); }


  // dropout keep words (the forward's saved mask, tiled layout of fa2_amd.h) of a step: lane
  // (r32, hh) loads row r32 of the step's 32 x 32 tile; loaded one step ahead so the loop's
  // vm_wait_all retires them (a load consumed in its own step would wait for the Q / dO DMA)
  uint32_t mw_cur = 0u, mw_nxt = 0u;
  auto load_mw = [&](int hq_, int m_) -> uint32_t {
    if constexpr (DROPOUT && DT <= 128) {
      if (p.dropout_mask && kw0 < p.seqlen_k) {
        const int nrb = (p.seqlen_q + 31) >> 5, ncw = (p.seqlen_k + 31) >> 5;
        return p.dropout_mask[(((int64_t)(b * p.heads_q + hq_) * nrb + (m_ >> 5)) * ncw + (kw0 >> 5)) * 32 + r32];
      }
    }
    return 0u;
  };
  // Phases (sched_barrier-separated so each phase's LDS fragments stay inside it and the
  // register peak stays under 256): S, dP -> P, dS -> dV, dK.
  auto body = [&](auto mask_c, const char* Q, const char* O, const char* S, int hq, int m, auto next_bias) {
    constexpr bool MASK = decltype(mask_c)::value;
    // the forward's keep mask M of this lane's key and the 16 rows m + o + 4 hh, first: no score
    // or fragment registers are live yet
    uint32_t keep16 = 0u;
    if constexpr (DROPOUT) {
      // (D = 256: redrawn -- the mask read there crashes ROCm 7.2's AGPR-copy rewrite pass)
      if (DT <= 128 && p.dropout_mask) {
        // the forward's saved 32 x 32 bit tile of this step (rows m.., keys kw0..), loaded one
        // step ahead: lane (r32, hh) holds row r32's word (bit k = key kw0 + k).  Transposed
        // across each 32-lane half (5 ds_swizzle xor stages), lane r32 then holds key kw0 + r32's
        // column (bit r = row m + r); register i of the lane is row (i & 3) + 8 (i >> 2) + 4 hh.
        const uint32_t xs = transpose32_lanes(mw_cur, r32) >> (4 * hh);
        keep16 = (xs & 0xFu) | ((xs >> 4) & 0xF0u) | ((xs >> 8) & 0xF00u) | ((xs >> 12) & 0xF000u);
      } else {
        keep16 = dropout_keep16(p.dropout_seed, drop_base(hq) + (uint64_t)(m + 4 * hh) * (uint64_t)Lk + (uint64_t)kj,
                                (uint64_t)Lk, p.dropout_p);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x16 s = zero16(), dp = zero16();
    u32x4 bt2[2];
    if constexpr (BIASL) {
      bt2[0] = bias_rd(0);
      bt2[1] = bias_rd(1);
    }
    {
      // fenced steps: the S chain (one fragment per MFMA, read kDkdvLS MFMAs ahead), then the dP
      // chain (two fragments per MFMA, kDkdvLD ahead): deeper prefetch than alternating chains
      // for the same registers in flight
      constexpr int LS = kDkdvLS < KS ? kDkdvLS : KS, LD = kDkdvLD < KS ? kDkdvLD : KS;
      u32x4 fq[KS], fo[KS], fv[KS];
#pragma unroll
      for (int j = 0; j < LS; ++j) fq[j] = lds_row_frag<DT, BMQ>(Q, 0, r32, j, hh);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        if (ks + LS < KS) fq[ks + LS] = lds_row_frag<DT, BMQ>(Q, 0, r32, ks + LS, hh);
        // the dP chain's first fragments ride in the S chain's last steps
        if (ks + LD >= KS) {
          const int j = ks + LD - KS;
          fo[j] = lds_row_frag<DT, BMQ>(O, 0, r32, j, hh);
          fv[j] = lds_row_frag<DT, BNK>(Vs, 32 * w, r32, j, hh);
        }
        s = E::mfma(fq[ks], kf[ks], s);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        if (ks + LD < KS) {
          fo[ks + LD] = lds_row_frag<DT, BMQ>(O, 0, r32, ks + LD, hh);
          fv[ks + LD] = lds_row_frag<DT, BNK>(Vs, 32 * w, r32, ks + LD, hh);
        }
        dp = E::mfma(fo[ks], fv[ks], dp);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    // rows of register i: m + (i & 3) + 8 (i >> 2) + 4 hh.  The row window [q_lo, q_hi) of this
    // lane's key is recomputed from an opaque lane id: hoisted out of the loop it gets spilled
    // and its scratch reload would drain the LDS-DMA prefetch (vmcnt(0)).
    int lo = 0, hi = 0;
    if (MASK) {
      int ln = threadIdx.x;
      asm volatile("" : "+v"(ln));
      const int kl = n0 + 32 * (ln >> 6) + (ln & 31);
      int qlo = CAUSAL ? max(kl - diag, 0) : 0;
      int qhi = kl < Lk ? Lq : -1;
      if constexpr (LOCAL) {
        qlo = max(kl - diag - wright, 0);
        qhi = kl < Lk ? min(Lq, kl - diag + wleft + 1) : -1;
      }
      lo = qlo - m - 4 * ((ln >> 5) & 1);  // (hh, likewise from the opaque id)
      hi = qhi - m - 4 * ((ln >> 5) & 1);
    }
    u32x4 pp[2], dsp[2];
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const f32x4 l4 = *(const f32x4*)(S + 4 * (8 * g4 + 4 * hh));
      const f32x4 d4 = *(const f32x4*)(S + 4 * BMQ + 4 * (8 * g4 + 4 * hh));
      float pv[4], dsv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = 4 * g4 + j;
        const int o = j + 8 * g4;
        float x = s[i];
        if constexpr (BIASL) {
          x = fmaf(x, scale2, kLog2e * bias_of(bt2, i));
        } else if constexpr (BIAS) {
          const int qr = m + o + 4 * hh;
          const int qc = qr < Lq ? qr : Lq - 1;
          const int kc = kval ? kj : Lk - 1;
          x = fmaf(x, scale2, kLog2e * load_bias(p.bias, b * p.bias_stride[0] + hq * p.bias_stride[1] +
                                                           (int64_t)qc * p.bias_stride[2] + kc, p.bias_dtype));
        }
        float pr = __builtin_amdgcn_exp2f(fmaf(x, sc, -l4[j]));
        if (MASK) pr = (o >= lo && o < hi) ? pr : 0.f;
        if (DROPOUT) {
          // the forward's keep mask (same Philox offsets), P~ = P M / (1 - p):
          // dV += P~^T dO, dS = P (dP~ M / (1 - p) - delta)
          const float kp = (keep16 >> i) & 1u ? inv_keep : 0.f;
          pv[j] = pr * kp;
          dsv[j] = pr * (dp[i] * kp + d4[j]);  // d4 = -delta (workspace convention)
        } else {
          pv[j] = pr;
          dsv[j] = pr * (dp[i] + d4[j]);  // softmax_scale is applied to dK once, at the end
        }
      }
      pp[g4 >> 1][2 * (g4 & 1) + 0] = E::pack2(pv[0], pv[1]);
      pp[g4 >> 1][2 * (g4 & 1) + 1] = E::pack2(pv[2], pv[3]);
      dsp[g4 >> 1][2 * (g4 & 1) + 0] = E::pack2(dsv[0], dsv[1]);
      dsp[g4 >> 1][2 * (g4 & 1) + 1] = E::pack2(dsv[2], dsv[3]);
    }
    next_bias();  // this step's bias tile is consumed: the next one may land in its buffer
    __builtin_amdgcn_sched_barrier(0);
    {
      // steps m: dt = m % NDT (independent chains back to back), r = m / NDT: (sp, dV | dK);
      // transposed fragments two steps ahead
      constexpr int N = 4 * NDT, L = 2 < N ? 2 : N;
      u32x4 fr[N];
      auto rd = [&](int m) {
        const int dt = m % NDT, r = m / NDT;
        return lds_tr_frag<DT, BMQ>((r & 1) ? Q : O, 16 * (r >> 1), 32 * dt, lane);
      };
#pragma unroll
      for (int j = 0; j < L; ++j) fr[j] = rd(j);
#pragma unroll
      for (int m = 0; m < N; ++m) {
        if (m + L < N) fr[m + L] = rd(m + L);
        const int dt = m % NDT, r = m / NDT;
        if (r & 1) dk[dt] = E::mfma(fr[m], dsp[r >> 1], dk[dt]);
        else dv[dt] = E::mfma(fr[m], pp[r >> 1], dv[dt]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };

  // The plain step (no bias, no dropout), software-pipelined inside the wave so that the
  // softmax-gradient VALU work sits beside MFMAs of the same wave instead of in a VALU-only phase:
  //   [S chain] [dP chain | P = exp2(S sc - LSE2)] [dV, dK chains | dS = P dP', packs]
  // The dP accumulator starts at -delta (the delta workspace holds -rowsum(O dO)), so the chain
  // yields dP - delta and dS is one multiply; the LSE2 and -delta rows are read from LDS at the
  // start of the step, long before their use.
  auto body_pipe = [&](auto mask_c, const char* Q, const char* O, const char* S, int m, auto next_bias) {
    constexpr bool MASK = decltype(mask_c)::value;
    // A bias (BIASL) enters as the S chain's initial accumulator together with the LSE2 rows,
    // b / scale - LSE2 / (scale log2 e): the chain yields x with P = exp2(x scale log2 e), so the
    // P phase needs neither the bias nor the LSE2 registers (at the 256-register limit both spilled
    // there, and the spilled DMA offsets' reloads drained the Q / dO prefetch).
    f32x16 binit;
    if constexpr (BIASL) {
      const u32x4 bt2[2] = {bias_rd(0), bias_rd(1)};
      const float rs = 1.f / scale, rl = -1.f / scale2;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const f32x4 lg = *(const f32x4*)(S + 4 * (8 * g4 + 4 * hh));
#pragma unroll
        for (int j = 0; j < 4; ++j) binit[4 * g4 + j] = fmaf(bias_of(bt2, 4 * g4 + j), rs, lg[j] * rl);
      }
    }
    constexpr int LS = kDkdvLS < KS ? kDkdvLS : KS, LD = kDkdvLD < KS ? kDkdvLD : KS;
    constexpr int EP = 16 / KS;          // P elements per dP step
    constexpr int N = 4 * NDT;           // dV / dK steps
    constexpr int ED = 8 / NDT;          // dS elements per dV / dK step (first 2 NDT steps)
    constexpr int LT = kDkdvLT < N ? kDkdvLT : N;  // transposed fragments in flight
    f32x16 s, dp;
    f32x4 l4[4];  // LSE2 rows of register group g4 (rows 8 g4 + 4 hh + 0..3), read just ahead
    auto rd_lse = [&](int g4) { l4[g4] = *(const f32x4*)(S + 4 * (8 * g4 + 4 * hh)); };
    auto rd_nd = [&](int g4) {  // -delta rows of group g4 into the dP accumulator
      const f32x4 d4 = *(const f32x4*)(S + 4 * BMQ + 4 * (8 * g4 + 4 * hh));
#pragma unroll
      for (int j = 0; j < 4; ++j) dp[4 * g4 + j] = d4[j];
    };
    u32x4 fq[KS], fo[KS], fv[KS];
#pragma unroll
    for (int j = 0; j < LS; ++j) fq[j] = lds_row_frag<DT, BMQ>(Q, 0, r32, j, hh);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (ks + LS < KS) fq[ks + LS] = lds_row_frag<DT, BMQ>(Q, 0, r32, ks + LS, hh);
      if (ks + LD >= KS) {
        const int j = ks + LD - KS;
        fo[j] = lds_row_frag<DT, BMQ>(O, 0, r32, j, hh);
        fv[j] = lds_row_frag<DT, BNK>(Vs, 32 * w, r32, j, hh);
      }
      // the -delta rows land in the dP accumulator over the last S steps, LSE group 0 last
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
        if ((KS >= 4 ? ks == KS - 4 + g4 : ks == KS - 2 + g4 / 2)) rd_nd(g4);
      // LSE group g4 is first used at dP step 4 g4 / EP and read one step ahead; the groups
      // needed in dP step 0 are read here
      if (!BIASL && ks == KS - 1) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4)
          if ((4 * g4) / EP == 0) rd_lse(g4);
      }
      if constexpr (BIASL) s = E::mfma(fq[ks], kf[ks], ks == 0 ? binit : s);
      else s = E::mfma(fq[ks], kf[ks], ks == 0 ? zero16() : s);
      __builtin_amdgcn_sched_barrier(0);
    }
    int lo = 0, hi = 0;  // as in body(): the visible row window of this lane's key
    if (MASK) {
      int ln = threadIdx.x;
      asm volatile("" : "+v"(ln));
      const int kl = n0 + 32 * (ln >> 6) + (ln & 31);
      int qlo = CAUSAL ? max(kl - diag, 0) : 0;
      int qhi = kl < Lk ? Lq : -1;
      if constexpr (LOCAL) {
        qlo = max(kl - diag - wright, 0);
        qhi = kl < Lk ? min(Lq, kl - diag + wleft + 1) : -1;
      }
      lo = qlo - m - 4 * ((ln >> 5) & 1);  // (hh, likewise from the opaque id)
      hi = qhi - m - 4 * ((ln >> 5) & 1);
    }
    u32x4 pp[2], dsp[2];
    auto p_elem = [&](int i) {  // P in place of S, packed pairwise
      const int o = (i & 3) + 8 * (i >> 2);
      float pr;
      if constexpr (BIASL) pr = __builtin_amdgcn_exp2f(s[i] * scale2);
      else pr = __builtin_amdgcn_exp2f(fmaf(s[i], sc, -l4[i >> 2][i & 3]));
      if (MASK) pr = (o >= lo && o < hi) ? pr : 0.f;
      s[i] = pr;
    };
    auto p_pack = [&](int sp) {  // P packed for the dV product, right before its first use
#pragma unroll
      for (int t = 0; t < 4; ++t) pp[sp][t] = E::pack2(s[8 * sp + 2 * t], s[8 * sp + 2 * t + 1]);
    };
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (ks + LD < KS) {
        fo[ks + LD] = lds_row_frag<DT, BMQ>(O, 0, r32, ks + LD, hh);
        fv[ks + LD] = lds_row_frag<DT, BNK>(Vs, 32 * w, r32, ks + LD, hh);
      }
      dp = E::mfma(fo[ks], fv[ks], dp);
#pragma unroll
      for (int e = ks * EP; e < (ks + 1) * EP; ++e) p_elem(e);
#pragma unroll
      for (int g4 = 1; g4 < 4; ++g4)
        if (!BIASL && (4 * g4) / EP > 0 && ks == (4 * g4) / EP - 1) rd_lse(g4);
      __builtin_amdgcn_sched_barrier(0);
    }
    auto ds_elem = [&](int i) {  // dS = P (dP - delta) in place of dP, packed pairwise
      dp[i] = s[i] * dp[i];
      if (i & 1) dsp[i >> 3][(i & 7) >> 1] = E::pack2(dp[i - 1], dp[i]);
    };
    // steps m: dt = m % NDT, r = m / NDT: dV (sp 0), dK (sp 0), dV (sp 1), dK (sp 1); dS elements
    // 0..7 ride on the first NDT steps, 8..15 on the next NDT (dsp[1] is first read at r = 3)
    u32x4 fr[N];
    auto rd = [&](int mm) {
      const int dt = mm % NDT, r = mm / NDT;
      return lds_tr_frag<DT, BMQ>((r & 1) ? Q : O, 16 * (r >> 1), 32 * dt, lane);
    };
    next_bias();  // P is formed: the next step's bias tile may land in this wave's buffer
#pragma unroll
    for (int j = 0; j < LT; ++j) fr[j] = rd(j);
    p_pack(0);
#pragma unroll
    for (int mm = 0; mm < N; ++mm) {
      if (mm + LT < N) fr[mm + LT] = rd(mm + LT);
      const int dt = mm % NDT, r = mm / NDT;
      if (mm == 2 * NDT - 1) p_pack(1);  // pp[1] is first read at r = 2
      if (r & 1) dk[dt] = E::mfma(fr[mm], dsp[r >> 1], dk[dt]);
      else dv[dt] = E::mfma(fr[mm], pp[r >> 1], dv[dt]);
      if (mm < 2 * NDT) {
#pragma unroll
        for (int e = mm * ED; e < (mm + 1) * ED; ++e) ds_elem(e);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  __builtin_amdgcn_s_waitcnt(0);  // prologue: Q fragments (compiler-tracked) + first tiles
  __syncthreads();
  if (ALIGNED && D < DT && total > 0) {
    // dP = dO V^T reads both operands from LDS, whose clamped staging repeats the last real
    // chunk in the padding columns: zero V's padding once so those columns contribute nothing.
    constexpr int kChunks = DT / 8;
    const int c0 = D >> 3;
    for (int idx = tid; idx < BNK * kChunks; idx += NT) {
      const int r = idx / kChunks, c = idx % kChunks;
      if (c >= c0) *(u32x4*)(Vs + Tile<DT, BNK>::off(r, c)) = u32x4{0u, 0u, 0u, 0u};
    }
    __syncthreads();
  }

  if (total > 0) mw_cur = load_mw(h0, tile_row(0));
  int g = 0, mt = 0;  // (q-head in group, query tile) of the current step
  for (int step = 0; step < total; ++step) {
    const int cur = step & 1;
    if (DROPOUT && step + 1 < total) {
      const bool wrap = mt + 1 == n_mt;
      mw_nxt = load_mw(h0 + g + (wrap ? 1 : 0), tile_row(wrap ? 0 : mt + 1));
    }
    if (step + 1 < total) {
      if constexpr (ALIGNED) stage_desc(cur ^ 1);
      else stage(cur ^ 1);
    }
    const int hq = h0 + g;
    const int m = tile_row(mt);
    // wave-uniform tile class
    // (LOCAL: the tile's rows see keys [m + diag - left, m + BMQ - 1 + diag + right])
    bool dead = kw0 >= Lk || (CAUSAL && kw0 > m + BMQ - 1 + diag);
    bool need_mask = (m + BMQ > Lq) || (kw0 + 31 >= Lk) || (CAUSAL && kw0 + 31 > m + diag);
    if constexpr (LOCAL) {
      dead = dead || kw0 > m + BMQ - 1 + diag + wright || kw0 + 31 < m + diag - wleft;
      need_mask = need_mask || kw0 + 31 > m + diag + wright || kw0 < m + BMQ - 1 + diag - wleft;
    }
    // the bias tile of the next step (BIASL), issued once this step's P no longer needs the buffer
    auto next_bias = [&]() {
      if (step + 1 < total) {
        const bool wrap = mt + 1 == n_mt;
        bias_issue(hq + (wrap ? 1 : 0), tile_row(wrap ? 0 : mt + 1));
      }
    };
    if (!dead) {
      if constexpr (LOCAL) {
        // masked steps (the band's edges, where a row may see one key alone) take the plain body,
        // whose dP chain starts from zero and has -delta added after it: with the windowed dQ's
        // MFMA-ordered delta, dP - delta is exactly 0 when O equals the key's V row.  (body_pipe
        // seeds the chain with -delta: the same value within rounding, summed in another order.)
        if (need_mask)
          body(std::true_type{}, qt(cur), ot(cur), st(cur), hq, m, next_bias);
        else
          body_pipe(std::false_type{}, qt(cur), ot(cur), st(cur), m, next_bias);
      } else if constexpr ((!BIAS || BIASL) && !DROPOUT) {
        if (need_mask)
          body_pipe(std::true_type{}, qt(cur), ot(cur), st(cur), m, next_bias);
        else
          body_pipe(std::false_type{}, qt(cur), ot(cur), st(cur), m, next_bias);
      } else {
        if (need_mask)
          body(std::true_type{}, qt(cur), ot(cur), st(cur), hq, m, next_bias);
        else
          body(std::false_type{}, qt(cur), ot(cur), st(cur), hq, m, next_bias);
      }
    } else {
      next_bias();
    }
    vm_wait_all();
    __syncthreads();
    if constexpr (DROPOUT) mw_cur = mw_nxt;
    if (++mt == n_mt) {
      mt = 0;
      ++g;
    }
  }

  // ---- store dK, dV (kv heads; fp32 group sum rounded once) ----------------------------
  if (nsplit > 1) {
    // partial sums of this split: [split][b][hkv][key][D] fp32, unscaled (dkv_reduce_kernel)
    if (kj < p.seqlen_k) {
      const int64_t row = (((int64_t)split * p.batch + b) * p.heads_kv + hkv) * p.seqlen_k + kj;
      float* pk = p.dkv_workspace + row * D;
      float* pv = p.dkv_workspace + ((int64_t)nsplit * p.batch * p.heads_kv * p.seqlen_k + row) * D;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int d0 = 32 * dt + 8 * g4 + 4 * hh;
          float a[4], c[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            a[j] = kval ? dk[dt][4 * g4 + j] : 0.f;
            c[j] = kval ? dv[dt][4 * g4 + j] : 0.f;
          }
          if (ALIGNED) {  // D % 8 == 0: whole 4-column groups
            if (d0 < D) {
              *(f32x4*)(pk + d0) = f32x4{a[0], a[1], a[2], a[3]};
              *(f32x4*)(pv + d0) = f32x4{c[0], c[1], c[2], c[3]};
            }
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (d0 + j < D) {
                pk[d0 + j] = a[j];
                pv[d0 + j] = c[j];
              }
          }
        }
      }
    }
    return;
  }
  if constexpr (ALIGNED) {
    // every wave passed the last step's barrier: V and Q/dO buffers hold the staging images
    uint16_t* k0 = (uint16_t*)p.dk + b * p.dk_stride[0] + hkv * p.dk_stride[2] + (int64_t)kw0 * p.dk_stride[1];
    uint16_t* v0 = (uint16_t*)p.dv + b * p.dv_stride[0] + hkv * p.dv_stride[2] + (int64_t)kw0 * p.dv_stride[1];
    const int nrows = min(32, p.seqlen_k - kw0);
    store_rows_lds<BF16, DT>(smem + w * 32 * DT * 2, dk, scale, kval, k0, p.dk_stride[1], nrows, D, lane);
    store_rows_lds<BF16, DT>(smem + (4 + w) * 32 * DT * 2, dv, 1.f, kval, v0, p.dv_stride[1], nrows, D, lane);
    return;
  }
  if (kj < p.seqlen_k) {
    uint16_t* dkrow = (uint16_t*)p.dk + b * p.dk_stride[0] + hkv * p.dk_stride[2] + (int64_t)kj * p.dk_stride[1];
    uint16_t* dvrow = (uint16_t*)p.dv + b * p.dv_stride[0] + hkv * p.dv_stride[2] + (int64_t)kj * p.dv_stride[1];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d0 = 32 * dt + 8 * g4 + 4 * hh;
        float a[4], c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a[j] = kval ? dk[dt][4 * g4 + j] * scale : 0.f;
          c[j] = kval ? dv[dt][4 * g4 + j] : 0.f;
        }
        if (ALIGNED) {
          if (d0 < D) {
            *(u32x2*)(dkrow + d0) = u32x2{E::pack2(a[0], a[1]), E::pack2(a[2], a[3])};
            *(u32x2*)(dvrow + d0) = u32x2{E::pack2(c[0], c[1]), E::pack2(c[2], c[3])};
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (d0 + j < D) {
              dkrow[d0 + j] = E::from_f32(a[j]);
              dvrow[d0 + j] = E::from_f32(c[j]);
            }
        }
      }
    }
  }
