// kvcache_kernel_body.h -- the body of the KV-cache decode kernel, shared textually by the two
// __global__ functions of kvcache_kernel.h that run it: kvcache_split_kernel (PAGED = false, the
// contiguous [B, capacity, Hkv, D] cache) and kvcache_paged_split_kernel (PAGED = true, a pool of
// blocks addressed through a block table).  In scope at the point of
// inclusion: the constants BF16, DT, PAGED, the arguments `p` (fa2_kvcache_args) and `nsplit`, and
// `pg` with the paging fields (block_table, block_table_stride, page_block_size, num_blocks).
// Included text rather than a __device__ function template: DESIGN 11 records what that route did
// to register allocation.  Every paging statement is an `if constexpr (PAGED)` beside the original.
  using E = Elem<BF16>;
  using C = KvCfg<DT>;
  constexpr int NW = C::NW, NDT = DT / 32, KS = DT / 16;
  __shared__ __attribute__((aligned(1024))) char smem[NW * C::kWave];
  __shared__ float ml[NW][2][32];

  const int tid = threadIdx.x, lane = tid & 63, r32 = lane & 31, hh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Hq = p.heads_q, Hkv = p.heads_kv, Sq = p.seqlen_q, D = p.head_dim;
  const int G = Hq / Hkv, rows = G * Sq, ntiles = (rows + 31) / 32;
  int u = blockIdx.x;
  const int split = u % nsplit;
  u /= nsplit;
  const int rt = u % ntiles;
  u /= ntiles;
  const int hkv = u % Hkv, b = u / Hkv;

  // valid keys of this batch (after the append, which ran before this kernel)
  int L = p.cache_seqlens ? p.cache_seqlens[b] : p.capacity;
  L = min(max(L, 0), p.capacity);
  L = (int)min((int64_t)L + p.seqlen_new, (int64_t)p.capacity);
  L = __builtin_amdgcn_readfirstlane(L);
  const int diag = L - Sq;
  const int wl = window_bound(p.window_left);
  const int wr = p.causal ? 0 : window_bound(p.window_right);

  // key run of this split, in whole tiles from the span's (tile-aligned) start
  const int start = p.window_left >= 0 ? (max(0, diag - wl) & ~63) : 0;
  const int span_tiles = L > start ? (L - start + 63) >> 6 : 0;
  const int per = (span_tiles + nsplit - 1) / nsplit;
  const int s_begin = start + min(split * per, span_tiles) * 64;
  const int s_end = min(L, start + min(split * per + per, span_tiles) * 64);
  const int my_tiles = s_end > s_begin ? (s_end - s_begin + 63) >> 6 : 0;
  const int nsteps = (my_tiles + NW - 1) / NW;

  // this lane's row: query position qi of q-head hkv * G + g
  const int rho = rt * 32 + r32;
  const bool valid = rho < rows;
  const int qi = valid ? rho / G : 0, hq = hkv * G + (valid ? rho % G : 0);
  const int lo = valid ? qi + diag - wl : (1 << 30);
  const int hi = valid ? min(L - 1, qi + diag + wr) : -1;
  const float scale = p.softmax_scale * kLog2e;

  const uint16_t* qrow = (const uint16_t*)p.q + b * p.q_stride[0] + qi * p.q_stride[1] + hq * p.q_stride[2];
  u32x4 qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) qf[ks] = load_row_frag<true>(qrow, 16 * ks + 8 * hh, D, valid);

  const uint16_t* kg = (const uint16_t*)p.k_cache + b * p.k_cache_stride[0] + hkv * p.k_cache_stride[2];
  const uint16_t* vg = (const uint16_t*)p.v_cache + b * p.v_cache_stride[0] + hkv * p.v_cache_stride[2];
  const int64_t krs = p.k_cache_stride[1], vrs = p.v_cache_stride[1];
  // PAGED: the caches are pools [num_blocks, P, Hkv, D]; logical key j of this batch is row j % P of
  // block tbl[j / P].  pid0 .. pid3 hold the clamped block ids of the tile staged next (kv_page_ids).
  int pid0 = 0, pid1 = 0, pid2 = 0, pid3 = 0;
  int log_p = 6;
  const int32_t* tbl = nullptr;
  if constexpr (PAGED) {
    kg = (const uint16_t*)p.k_cache + hkv * p.k_cache_stride[2];
    vg = (const uint16_t*)p.v_cache + hkv * p.v_cache_stride[2];
    log_p = __builtin_ctz(pg.page_block_size);
    tbl = pg.block_table + (int64_t)b * pg.block_table_stride;
  }
  char* Kt = smem + wave * C::kWave;
  char* Vt = Kt + C::kTile;

  float m_run = kNegInf, l_run = 0.f;
  f32x16 acc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) acc[dt] = zero16();

  // rows at or past L re-read row L - 1 (stage_tile clamps): L >= 1 whenever a tile is staged
  if (wave < my_tiles) {
    const int n0 = s_begin + wave * 64;
    if constexpr (PAGED) {
      kv_page_ids(pid0, pid1, pid2, pid3, tbl, log_p, pg.num_blocks, n0, L);
      stage_tile_paged<DT>(Kt, kg, p.k_cache_stride[0], krs, pid0, pid1, pid2, pid3, log_p, n0, L, D, lane);
      stage_tile_paged<DT>(Vt, vg, p.v_cache_stride[0], vrs, pid0, pid1, pid2, pid3, log_p, n0, L, D, lane);
      // the ids of tile wave + NW, staged in step 0: one step ahead of their use
      if (wave + NW < my_tiles) kv_page_ids(pid0, pid1, pid2, pid3, tbl, log_p, pg.num_blocks, n0 + NW * 64, L);
    } else {
      stage_tile<DT, 64, 64, true>(Kt, kg, krs, n0, L, D, lane);
      stage_tile<DT, 64, 64, true>(Vt, vg, vrs, n0, L, D, lane);
    }
  }
  for (int t = 0; t < nsteps; ++t) {
    const int tile = t * NW + wave;
    const bool act = tile < my_tiles, nxt = tile + NW < my_tiles;  // wave-uniform
    const int n0 = s_begin + tile * 64;
    // K(t) has landed once only V(t)'s pieces are outstanding; the barrier orders the DMA's LDS
    // writes before the reads below (every wave runs every step's barriers, active or not)
    if (act) vm_wait_but<C::kPieces>();
    __builtin_amdgcn_s_barrier();
    f32x16 s[2];
    u32x4 pf[2][2];
    if (act) {
      s[0] = zero16();
      s[1] = zero16();
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) s[kt] = E::mfma(lds_row_frag<DT, 64>(Kt, 32 * kt, r32, ks, hh), qf[ks], s[kt]);
      }
      lds_wait_all();  // K(t) is in registers: its tile may be overwritten
      if constexpr (PAGED) {
        if (nxt) stage_tile_paged<DT>(Kt, kg, p.k_cache_stride[0], krs, pid0, pid1, pid2, pid3, log_p, n0 + NW * 64, L, D, lane);
      } else {
        if (nxt) stage_tile<DT, 64, 64, true>(Kt, kg, krs, n0 + NW * 64, L, D, lane);
      }
      // lane (r32, hh) holds keys n0 + 32 kt + 4 hh + (i & 3) + 8 (i >> 2) of row r32
      float mx = kNegInf;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = n0 + 32 * kt + 4 * hh + (i & 3) + 8 * (i >> 2);
          const float v = (key >= lo && key <= hi) ? s[kt][i] * scale : kNegInf;
          s[kt][i] = v;
          mx = fmaxf(mx, v);
        }
      }
      mx = half_max(mx);
      const float m_new = fmaxf(m_run, mx);
      const float m_use = m_new == kNegInf ? 0.f : m_new;  // no key yet: exponentiate against 0
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
      m_run = m_new;
      float rs = 0.f;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float e = __builtin_amdgcn_exp2f(s[kt][i] - m_use);
          s[kt][i] = e;
          rs += e;
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
          for (int j = 0; j < 4; ++j) pf[kt][kk][j] = E::pack2(s[kt][8 * kk + 2 * j], s[kt][8 * kk + 2 * j + 1]);
        }
      }
      l_run = l_run * alpha + rs;  // lane-partial row sum (the partner lane holds the rest)
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[dt][i] *= alpha;
      }
      // V(t) has landed once only K(t+1)'s pieces are outstanding
      if (nxt) vm_wait_but<C::kPieces>();
      else vm_wait_all();
    }
    __builtin_amdgcn_s_barrier();
    if (act) {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt)
            acc[dt] = E::mfma(lds_tr_frag<DT, 64>(Vt, 32 * kt + 16 * kk, 32 * dt, lane), pf[kt][kk], acc[dt]);
        }
      }
      lds_wait_all();
      if constexpr (PAGED) {
        if (nxt) stage_tile_paged<DT>(Vt, vg, p.v_cache_stride[0], vrs, pid0, pid1, pid2, pid3, log_p, n0 + NW * 64, L, D, lane);
        // the ids of tile + 2 NW, which the next step stages
        if (tile + 2 * NW < my_tiles) kv_page_ids(pid0, pid1, pid2, pid3, tbl, log_p, pg.num_blocks, n0 + 2 * NW * 64, L);
      } else {
        if (nxt) stage_tile<DT, 64, 64, true>(Vt, vg, vrs, n0 + NW * 64, L, D, lane);
      }
    }
  }
  l_run = half_sum(l_run);

  // merge the waves' (m, l, O) in wave order.  Every DMA of a wave was retired in its last step, so
  // its tiles are free for its fp32 O image: [dt][4-register group][lane] 16-byte slots.
  {
    f32x4* ow = (f32x4*)(smem + wave * C::kWave);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
        ow[(dt * 4 + g4) * 64 + lane] = f32x4{acc[dt][4 * g4], acc[dt][4 * g4 + 1], acc[dt][4 * g4 + 2], acc[dt][4 * g4 + 3]};
    }
    if (hh == 0) {
      ml[wave][0][r32] = m_run;
      ml[wave][1][r32] = l_run;
    }
  }
  __syncthreads();
  float M = kNegInf;
#pragma unroll
  for (int w = 0; w < NW; ++w) M = fmaxf(M, ml[w][0][r32]);
  float wgt[NW], lsum = 0.f;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const float mw = ml[w][0][r32];
    wgt[w] = mw == kNegInf ? 0.f : __builtin_amdgcn_exp2f(mw - M);
    lsum += ml[w][1][r32] * wgt[w];
  }
  const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
  const float lse = lsum > 0.f ? M + __builtin_amdgcn_logf(lsum) : kNegInf;  // v_log_f32 is log2

  const int64_t nrow = (int64_t)p.batch * Hq * Sq;
  const int64_t orow_ws = (((int64_t)split * p.batch + b) * Hq + hq) * Sq + qi;
  float* ws_o = (float*)p.workspace;
  float* ws_l = ws_o + (int64_t)nsplit * nrow * D;
  uint16_t* orow = (uint16_t*)p.o + b * p.o_stride[0] + qi * p.o_stride[1] + hq * p.o_stride[2];
  for (int dt = wave; dt < NDT; dt += NW) {
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        const f32x4 x = ((const f32x4*)(smem + w * C::kWave))[(dt * 4 + g4) * 64 + lane];
        o += x * wgt[w];
      }
      o *= inv;
      const int d0 = 32 * dt + 8 * g4 + 4 * hh;
      if (valid && d0 < D) {
        if (nsplit == 1) *(u32x2*)(orow + d0) = u32x2{E::pack2(o[0], o[1]), E::pack2(o[2], o[3])};
        else *(f32x4*)(ws_o + orow_ws * D + d0) = o;
      }
    }
  }
  if (wave == 0 && hh == 0 && valid) {
    if (nsplit == 1) {
      if (p.lse) p.lse[((int64_t)b * Hq + hq) * Sq + qi] = lse;
    } else {
      ws_l[orow_ws] = lse;
    }
  }
