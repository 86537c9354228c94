// kvcache_fp8_kernel.h -- KV-cache decode attention over fp8 (OCP e4m3fn) caches for gfx950
// (fa2_fwd_kvcache_fp8): kvcache_kernel.h's unit, key split, masks and merge, with K / V
// tiles staged as bytes and converted to q's dtype in registers.
//
//  * A cache element's value is its exact e4m3 value (every finite e4m3 value is a bf16 and an
//    fp16 value), so the conversion is lossless and the MFMAs are those of the 16-bit kernel.  The
//    per-(batch, kv head) descales never touch K or V: kd goes into the score multiplier
//    (softmax_scale * kd) * log2e, vd multiplies O in fp32 before its one rounding (on the split
//    path the fp32 partials, so kvcache_combine_kernel runs unchanged).
//  * LDS image: a 64-key x DT-byte tile is the Tile<DT / 2, 64> image of its rows read as DT / 2
//    16-bit words (byte pairs), so stage_tile / stage_tile_paged stage it as they are: DT / 16
//    LDS-DMA pieces of 16 bytes = 16 elements per lane.
//  * K rows: lane (r32, hh) reads the 8 bytes 16 ks + 8 hh .. + 7 of key r32 (ds_read_b64) and
//    converts them to one 16-byte MFMA fragment.
//  * V^T: ds_read_b64_tr_b16 on the byte pairs (lds_tr_frag on the 16-bit view).  Lane (r32, h)
//    then holds the pair (d, d + 1), d = 64 su + 2 r32, of the eight keys of a k-step in the
//    permuted key order of P; v_perm_b32 separates the even and the odd column, and the two feed two
//    accumulators: acc[2 su] holds columns 64 su + 2 m, acc[2 su + 1] columns 64 su + 2 m + 1 (m the
//    accumulator row).  The epilogue interleaves them: registers 4 g4 + e of the two accumulators
//    are the eight consecutive columns 64 su + 16 g4 + 8 hh + 2 e + parity.
//  * Bytes in flight: a workgroup's LDS is half the 16-bit kernel's (64 KiB + 1 KiB at DT = 128),
//    and the kernel is bounded to 256 VGPRs, so two workgroups share a CU: per CU the same K and V
//    bytes are ahead as in the 16-bit kernel (which fits one).
#pragma once
#include "kvcache_kernel.h"

namespace fa2 {

template <int DT>
struct KvFp8Cfg {
  static constexpr int NW = 4;              // waves per workgroup
  static constexpr int DH = DT / 2;         // the tile's width in 16-bit words (byte pairs)
  static constexpr int kTile = 64 * DT;     // bytes of a 64-key K or V tile
  static constexpr int kWave = 2 * kTile;   // a wave's K and V tile (its fp32 O image at the merge)
  static constexpr int kPieces = DT / 16;   // LDS-DMA instructions of one tile, per lane
};

// two e4m3 bytes (the low or the high half of w) as two elements of q's dtype, exactly
template <bool BF16>
FA2_DEV uint32_t fp8x2_to_elem(uint32_t w, bool high) {
  if constexpr (BF16) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const bf16x2 r = high ? __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true) : __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false);
    return __builtin_bit_cast(uint32_t, r);
  } else {
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    const f16x2 r = high ? __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true) : __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false);
    return __builtin_bit_cast(uint32_t, r);
  }
}
template <bool BF16>
FA2_DEV u32x4 fp8x8_to_frag(uint32_t lo, uint32_t hi) {
  return u32x4{fp8x2_to_elem<BF16>(lo, false), fp8x2_to_elem<BF16>(lo, true), fp8x2_to_elem<BF16>(hi, false),
               fp8x2_to_elem<BF16>(hi, true)};
}

// K fragment of k-step ks: bytes 16 ks + 8 hh .. + 7 of tile row row0 + r32 (chunk ks of the row,
// its half hh), converted.
template <bool BF16, int DH>
FA2_DEV u32x4 lds_row_frag_fp8(const char* tile, int row0, int r32, int ks, int hh) {
  const int off = (ks >> 2) * Tile<DH, 64>::kSub + (row0 + r32) * 64 + (((ks & 3) ^ ((r32 >> 2) & 3)) << 4) + 8 * hh;
  const u32x2 w = *(const u32x2*)(tile + off);
  return fp8x8_to_frag<BF16>(w[0], w[1]);
}

// V^T fragments of keys row0 .. row0 + 15 (the permuted order of lds_tr_frag) for the byte pair
// (64 su + 2 r32, + 1): `even` and `odd` are the two columns' A operands.
template <bool BF16, int DH>
FA2_DEV void lds_tr_frag_fp8(u32x4& even, u32x4& odd, const char* tile, int row0, int su, int lane) {
  const u32x4 t = lds_tr_frag<DH, 64>(tile, row0, 32 * su, lane);  // dword i: keys 2 i, 2 i + 1 as (even, odd) bytes
  const uint32_t e0 = __builtin_amdgcn_perm(t[1], t[0], 0x06040200u), e1 = __builtin_amdgcn_perm(t[3], t[2], 0x06040200u);
  const uint32_t o0 = __builtin_amdgcn_perm(t[1], t[0], 0x07050301u), o1 = __builtin_amdgcn_perm(t[3], t[2], 0x07050301u);
  even = fp8x8_to_frag<BF16>(e0, e1);
  odd = fp8x8_to_frag<BF16>(o0, o1);
}

// A 64-key byte tile through either layout: the 16-bit stagers on the byte-pair view (strides and
// D halved: 16-byte aligned rows make every stride even).
template <int DT, bool PAGED>
FA2_DEV void stage_tile_fp8(char* tile, const uint8_t* g, int64_t block_stride, int64_t row_stride, int e0, int e1, int e2, int e3,
                            int log_p, int n0, int L, int D, int lane) {
  constexpr int DH = DT / 2;
  if constexpr (PAGED) stage_tile_paged<DH>(tile, (const uint16_t*)g, block_stride >> 1, row_stride >> 1, e0, e1, e2, e3, log_p, n0, L, D >> 1, lane);
  else stage_tile<DH, 64, 64, true>(tile, (const uint16_t*)g, row_stride >> 1, n0, L, D >> 1, lane);
}

// 256 threads, two workgroups per CU (at most 256 VGPRs): see "bytes in flight" above
template <bool BF16, int DT, bool PAGED>
__global__ void __launch_bounds__(256, 2) kvcache_fp8_split_kernel(const fa2_fp8_kvcache_args fa, const int nsplit) {
  using E = Elem<BF16>;
  using C = KvFp8Cfg<DT>;
  constexpr int NW = C::NW, DH = C::DH, NDT = DT / 32, NSU = DT / 64, KS = DT / 16;
  const fa2_paged_kvcache_args& pg = fa.paged;
  const fa2_kvcache_args& p = fa.paged.base;
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

  // the descales of this (batch, kv head), read before any DMA is issued and pinned to SGPRs there
  // (no load of the kernel's may sit between a tile's pieces and their counted wait)
  float kd = fa.k_descale ? fa.k_descale[b * fa.k_descale_stride[0] + hkv * fa.k_descale_stride[1]] : 1.f;
  float vd = fa.v_descale ? fa.v_descale[b * fa.v_descale_stride[0] + hkv * fa.v_descale_stride[1]] : 1.f;
  kd = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(kd)));
  vd = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(vd)));
  asm volatile("" : "+s"(kd), "+s"(vd)::"memory");

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
  const float scale = (p.softmax_scale * kd) * kLog2e;

  const uint16_t* qrow = (const uint16_t*)p.q + b * p.q_stride[0] + qi * p.q_stride[1] + hq * p.q_stride[2];
  u32x4 qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) qf[ks] = load_row_frag<true>(qrow, 16 * ks + 8 * hh, D, valid);
  // Q is complete here, before the first DMA: the compiler does not see the DMAs or the counted
  // waits, so it would otherwise retire these loads with its own vmcnt(0) at their first use --
  // inside the loop, every step, draining the V tile that S = K Q^T is meant to overlap
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks]));

  // cache strides are in elements = bytes.  PAGED: pools [num_blocks, P, Hkv, D], logical key j of
  // this batch in row j % P of block tbl[j / P]; pid0 .. pid3 are the clamped block ids of the
  // tile staged next (kv_page_ids)
  const uint8_t* kg = (const uint8_t*)p.k_cache + (PAGED ? 0 : b * p.k_cache_stride[0]) + hkv * p.k_cache_stride[2];
  const uint8_t* vg = (const uint8_t*)p.v_cache + (PAGED ? 0 : b * p.v_cache_stride[0]) + hkv * p.v_cache_stride[2];
  const int64_t kbs = p.k_cache_stride[0], vbs = p.v_cache_stride[0], krs = p.k_cache_stride[1], vrs = p.v_cache_stride[1];
  int pid0 = 0, pid1 = 0, pid2 = 0, pid3 = 0;
  int log_p = 6;
  const int32_t* tbl = nullptr;
  if constexpr (PAGED) {
    log_p = __builtin_ctz(pg.page_block_size);
    tbl = pg.block_table + (int64_t)b * pg.block_table_stride;
  }
  char* Kt = smem + wave * C::kWave;
  char* Vt = Kt + C::kTile;

  float m_run = kNegInf, l_run = 0.f;
  f32x16 acc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) acc[dt] = zero16();

  // rows at or past L re-read row L - 1 (the stagers clamp): L >= 1 whenever a tile is staged
  if (wave < my_tiles) {
    const int n0 = s_begin + wave * 64;
    if constexpr (PAGED) kv_page_ids(pid0, pid1, pid2, pid3, tbl, log_p, pg.num_blocks, n0, L);
    stage_tile_fp8<DT, PAGED>(Kt, kg, kbs, krs, pid0, pid1, pid2, pid3, log_p, n0, L, D, lane);
    stage_tile_fp8<DT, PAGED>(Vt, vg, vbs, vrs, pid0, pid1, pid2, pid3, log_p, n0, L, D, lane);
    if constexpr (PAGED) {
      // the ids of tile wave + NW, staged in step 0: one step ahead of their use
      if (wave + NW < my_tiles) kv_page_ids(pid0, pid1, pid2, pid3, tbl, log_p, pg.num_blocks, n0 + NW * 64, L);
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
        for (int kt = 0; kt < 2; ++kt) s[kt] = E::mfma(lds_row_frag_fp8<BF16, DH>(Kt, 32 * kt, r32, ks, hh), qf[ks], s[kt]);
      }
      lds_wait_all();  // K(t) is in registers: its tile may be overwritten
      if (nxt) stage_tile_fp8<DT, PAGED>(Kt, kg, kbs, krs, pid0, pid1, pid2, pid3, log_p, n0 + NW * 64, L, D, lane);
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
          for (int su = 0; su < NSU; ++su) {
            u32x4 ve, vo;
            lds_tr_frag_fp8<BF16, DH>(ve, vo, Vt, 32 * kt + 16 * kk, su, lane);
            acc[2 * su] = E::mfma(ve, pf[kt][kk], acc[2 * su]);
            acc[2 * su + 1] = E::mfma(vo, pf[kt][kk], acc[2 * su + 1]);
          }
        }
      }
      lds_wait_all();
      if (nxt) stage_tile_fp8<DT, PAGED>(Vt, vg, vbs, vrs, pid0, pid1, pid2, pid3, log_p, n0 + NW * 64, L, D, lane);
      if constexpr (PAGED) {
        // the ids of tile + 2 NW, which the next step stages
        if (tile + 2 * NW < my_tiles) kv_page_ids(pid0, pid1, pid2, pid3, tbl, log_p, pg.num_blocks, n0 + 2 * NW * 64, L);
      }
    }
  }
  l_run = half_sum(l_run);

  // merge the waves' (m, l, O) in wave order.  Every DMA of a wave was retired in its last step, so
  // its tiles are free for its fp32 O image: [accumulator][4-register group][lane] 16-byte slots
  // (NDT * 4 KiB = a wave's two byte tiles exactly).
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
  for (int su = wave; su < NSU; su += NW) {
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      // the even and the odd accumulator's registers 4 g4 .. 4 g4 + 3: columns d0 + 2 e and d0 + 2 e + 1
      f32x4 oe = f32x4{0.f, 0.f, 0.f, 0.f}, oo = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        const f32x4* img = (const f32x4*)(smem + w * C::kWave);
        oe += img[((2 * su) * 4 + g4) * 64 + lane] * wgt[w];
        oo += img[((2 * su + 1) * 4 + g4) * 64 + lane] * wgt[w];
      }
      oe *= inv;
      oo *= inv;
      oe *= vd;
      oo *= vd;
      const int d0 = 64 * su + 16 * g4 + 8 * hh;
      if (valid && d0 < D) {
        if (nsplit == 1) {
          *(u32x4*)(orow + d0) = u32x4{E::pack2(oe[0], oo[0]), E::pack2(oe[1], oo[1]), E::pack2(oe[2], oo[2]), E::pack2(oe[3], oo[3])};
        } else {
          *(f32x4*)(ws_o + orow_ws * D + d0) = f32x4{oe[0], oo[0], oe[1], oo[1]};
          *(f32x4*)(ws_o + orow_ws * D + d0 + 4) = f32x4{oe[2], oo[2], oe[3], oo[3]};
        }
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
}

template <bool BF16, int DT, bool PAGED>
hipError_t launch_kvcache_fp8_split(const fa2_fp8_kvcache_args& a, int nsplit, hipStream_t st) {
  const dim3 grid((unsigned)(kv_units(a.paged.base) * nsplit)), block(KvFp8Cfg<DT>::NW * 64);
  hipLaunchKernelGGL((kvcache_fp8_split_kernel<BF16, DT, PAGED>), grid, block, 0, st, a, nsplit);
  return hipGetLastError();
}

}  // namespace fa2
