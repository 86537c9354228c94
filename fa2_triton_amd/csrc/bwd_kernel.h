// bwd_kernel.h -- FlashAttention-2 backward for gfx950 (CDNA4).
//
// Replaces the reference's backward launches (/root/reference/src/backward/caller.py:95-165):
//   delta_kernel  <- _compute_delta        (/root/reference/src/backward/compute_delta.py:17-73);
//                    the default backward folds it into dq_kernel, which runs first
//   dkdv_kernel   <- _bwd_kernel, pid < NUM_BLOCKS_KV branch + the host GQA sum
//                    (/root/reference/src/backward/kernel.py:154-166, compute_dkdv.py:7-296,
//                     caller.py:162-165)
//   dq_kernel     <- _bwd_kernel, dQ branch (kernel.py:168-182, compute_dq.py:7-261)
// Same math (src/backward/compute_dkdv.py:89-110, compute_dq.py:70-76):
//   P = exp2(s * scale * log2e - LSE2), dV = P^T dO, dP = dO V^T, dS = P (dP - delta) scale,
//   dK = dS^T Q, dQ = dS K; P and dS rounded to the input dtype before their MFMAs; fp32
//   accumulation; no atomics (bitwise reproducible, as tests/test_repeatability.py demands).
// Differences by design: the GQA group sum of dK/dV is done in fp32 registers inside
// dkdv_kernel (the reference sums bf16/fp16 tensors on the host), dQ is written directly in
// the requested dtype, and padded varlen rows are handled in place (no pack/unpack).
#include <type_traits>

#include <stdlib.h>

#include "common.h"
#include "fa2_internal.h"
#include "dkdv_hp_kernel.h"
#include "dq_hp_kernel.h"

// Schedule constants (measured; the variants they replaced are recorded in DESIGN.md):
//  dK/dV: S chain with its Q fragments kDkdvLS MFMAs ahead, then the dP chain with its
//         (dO, V) fragment pairs kDkdvLD ahead, then the dV/dK steps kDkdvLT transposed
//         fragments ahead -- at the 256-register limit a deeper prefetch spills;
//  dQ (recompute): fragments kDqLead k-steps ahead; interior tiles software-pipelined by
//         32-key halves with kDqPipeLead step of fragments in flight.

namespace fa2 {

constexpr int kDkdvLS = 2;
constexpr int kDkdvLD = 1;
constexpr int kDkdvLT = 2;
constexpr int kDqLead = 2;
constexpr int kDqPipeLead = 1;

// ---------------------------------------------------------------------------------------------
// delta[b, h, i] = -sum_d O[b, i, h, d] * dO[b, i, h, d]   (fp32; 0 for padded rows).  The
// workspace holds the NEGATED row sum: it is the initial dP accumulator of dkdv_kernel.
template <bool BF16, bool ALIGNED>
__global__ void __launch_bounds__(256) delta_kernel(const fa2_bwd_args p) {
  using E = Elem<BF16>;
  constexpr int LPR = 16;             // lanes per row
  constexpr int ROWS = 256 / LPR;     // rows per block
  const int tid = threadIdx.x;
  const int row = blockIdx.x * ROWS + tid / LPR;
  const int sub = tid % LPR;
  const int bh = blockIdx.y;
  const int b = bh / p.heads_q, h = bh - b * p.heads_q;
  int Lq = p.seqlen_q;
  if (p.cu_seqlens) Lq = p.cu_seqlens[b + 1] - p.cu_seqlens[b];
  float acc = 0.f;
  if (row < Lq) {
    const uint16_t* orow = (const uint16_t*)p.o + b * p.o_stride[0] + h * p.o_stride[2] + (int64_t)row * p.o_stride[1];
    const uint16_t* drow = (const uint16_t*)p.dout + b * p.do_stride[0] + h * p.do_stride[2] + (int64_t)row * p.do_stride[1];
    for (int d0 = sub * 8; d0 < p.head_dim; d0 += LPR * 8) {
      const u32x4 ov = load_row_frag<ALIGNED>(orow, d0, p.head_dim, true);
      const u32x4 dv = load_row_frag<ALIGNED>(drow, d0, p.head_dim, true);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc += E::to_f32((uint16_t)(ov[j] & 0xFFFF)) * E::to_f32((uint16_t)(dv[j] & 0xFFFF));
        acc += E::to_f32((uint16_t)(ov[j] >> 16)) * E::to_f32((uint16_t)(dv[j] >> 16));
      }
    }
  }
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, LPR);
  // rows [Lq, lse_row_stride) get 0 so that masked rows can never inject NaN/Inf garbage
  // stored negated: the dK/dV kernel starts its dP accumulator at -delta
  if (sub == 0 && row < p.lse_row_stride) p.delta[(int64_t)bh * p.lse_row_stride + row] = -acc;
}

// ---------------------------------------------------------------------------------------------
// dK, dV: one workgroup = 4 waves = 128 keys of one (batch, kv-head); wave w owns keys
// n0 + 32 w + (lane & 31).  K stays in VGPRs (B operand of S = Q K^T), the workgroup's V rows
// sit in LDS (B operand of dP = dO V^T, read as row fragments), and the workgroup sweeps the
// q-heads of its GQA group and 32-row query tiles (Q, dO, LSE2 and delta staged in LDS by
// LDS-DMA, double buffered).  Per tile and wave:
//   S[q][key], dP[q][key]   8 + 8 MFMA (A = Q / dO row fragments)
//   dV^T[d][key] += dO^T P  NDT*2 MFMA (A = dO^T via ds_read_b64_tr_b16, B = P registers)
//   dK^T[d][key] += Q^T dS  NDT*2 MFMA
// dK/dV accumulate the whole GQA group in fp32 and are rounded once.  <= 256 VGPRs, so two
// workgroups share a CU (DT <= 128).
// q-head split (nsplit > 1, small grids: GQA / MQA with few (batch, kv-head, key block) items):
// the group's q-heads are dealt to nsplit workgroups per key block, each writes its fp32 partial
// dK/dV sums to p.dkv_workspace ([nsplit][B][Hkv][Sk][D], unscaled) and dkv_reduce_kernel adds
// them in split order (deterministic).
// BIASK as dq_kernel: 0 none, 1 element loads from global memory, 16 / 17 a 16-bit bias with
// 16-byte aligned rows staged per wave by LDS-DMA: [32 query rows x 32 keys] of the step (2 KiB,
// single buffered), read with the transposing ds_read_b64_tr_b16 straight into the register
// order of the S accumulator (key on the lane).  The tile of step j+1 goes out as soon as step j
// has formed P, so it lands under the dV / dK chains (the step's closing wait covers it).
// The body is dkdv_kernel_body.h, shared with the sliding-window dK/dV (local_kernel.h), which
// includes it with LOCAL = true (CAUSAL, BIASK and DROPOUT off): key j
// is visible to the rows max(0, j - diag - right) <= i < min(Lq, j - diag + left + 1), so the
// block sweeps only the query tiles of [m_begin, m_end) and every mask is two-sided.  A block whose
// range is empty stages nothing and writes zeros.
template <bool BF16, int DT, bool CAUSAL, int BIASK, bool DROPOUT, bool ALIGNED>
__global__ void __launch_bounds__(256, DT >= 256 ? 1 : 2) dkdv_kernel(const fa2_bwd_args p, int nsplit) {
  constexpr bool LOCAL = false;
#include "dkdv_kernel_body.h"
}

// ---------------------------------------------------------------------------------------------
// dK/dV of a q-head split (dkdv_kernel, nsplit > 1): dK = scale * sum_s dK_s, dV = sum_s dV_s
// over the fp32 partials in split order (deterministic), rounded once.  One thread per four
// columns of one (batch, kv-head, key) row; HBM-bound (2 nsplit fp32 reads per output element).
template <bool BF16>
__global__ void __launch_bounds__(256) dkv_reduce_kernel(const fa2_bwd_args p, int nsplit) {
  using E = Elem<BF16>;
  const int D = p.head_dim;
  const int cpr = (D + 3) >> 2;
  const int64_t rows = (int64_t)p.batch * p.heads_kv * p.seqlen_k;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * cpr) return;
  const int64_t row = idx / cpr;
  const int d0 = (int)(idx - row * cpr) * 4;
  const int kj = (int)(row % p.seqlen_k);
  const int64_t bh = row / p.seqlen_k;
  const int hkv = (int)(bh % p.heads_kv), b = (int)(bh / p.heads_kv);
  const int64_t half = (int64_t)nsplit * rows * D;
  float a[4] = {0.f, 0.f, 0.f, 0.f}, c[4] = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < nsplit; ++s) {
    const float* pk = p.dkv_workspace + ((int64_t)s * rows + row) * D + d0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (d0 + j < D) {
        a[j] += pk[j];
        c[j] += pk[half + j];
      }
  }
  uint16_t* dkrow = (uint16_t*)p.dk + b * p.dk_stride[0] + hkv * p.dk_stride[2] + (int64_t)kj * p.dk_stride[1];
  uint16_t* dvrow = (uint16_t*)p.dv + b * p.dv_stride[0] + hkv * p.dv_stride[2] + (int64_t)kj * p.dv_stride[1];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (d0 + j < D) {
      dkrow[d0 + j] = E::from_f32(a[j] * p.softmax_scale);
      dvrow[d0 + j] = E::from_f32(c[j]);
    }
}

// ---------------------------------------------------------------------------------------------
template <int DT>
struct DqCfg {
  static constexpr int NW = 4;  // two independent workgroups per CU (measured faster than 8 waves)
  static constexpr int kWavesPerSimd = DT >= 256 ? 1 : 2;
};

// dQ: one workgroup = 4 waves = 128 query rows of one (batch, q-head); K/V tiles of 64 keys in
// LDS (double buffered).  Per tile and wave:
//   S^T, dP^T [key][q]   2 x (8 + 8) MFMA (A = K / V row fragments, B = Q / dO in VGPRs)
//   dQ^T[d][q] += K^T dS^T   NDT*4 MFMA (A = K^T via ds_read_b64_tr_b16)
// BIASK: 0 no bias; 1 any bias, read element by element from global memory; 16 / 17 an fp16 /
// bf16 bias with 16-byte aligned rows, staged per wave by LDS-DMA like the forward's
// (fwd_pipe_kernel.h): each wave's [32 rows x 64 keys] bias tile of tile i goes out first at the
// top of tile i and is waited for (counted vmcnt, the next K/V tile left in flight) right before
// the softmax gradient of its first key half.
#ifndef FA2_DQ_BIAS_WPS
#define FA2_DQ_BIAS_WPS 2
#endif
// The body is dq_kernel_body.h, shared with the sliding-window dQ (local_kernel.h), which includes
// it with LOCAL = true (CAUSAL, BIASK and DROPOUT off, so the grid is the plain one block per
// workgroup): the tile loop confined to the block's band and every mask two-sided, as in the
// forward.
template <bool BF16, int DT, bool CAUSAL, int BIASK, bool DROPOUT, bool ALIGNED, bool DQF32>
__global__ void __launch_bounds__(DqCfg<DT>::NW * 64, BIASK != 0 && DT == 128 ? FA2_DQ_BIAS_WPS : DqCfg<DT>::kWavesPerSimd)
    dq_kernel(const fa2_bwd_args p) {
  constexpr bool LOCAL = false;
#include "dq_kernel_body.h"
}

// ---------------------------------------------------------------------------------------------
// Bias gradient (ABI 5; the reference has none, /root/reference/src/wrapper.py:86):
//   dbias[b', h', i, j] = sum over the (batch, q-head) pairs the bias broadcasts to of
//                         dS[b, hq, i, j] = P (dP~ - delta),   P = exp2(s scale log2e + bias log2e - LSE2)
// (dP~ = dP M / (1 - p) under dropout, M the forward's keep mask), in fp32, deterministic.
// One workgroup owns a 128-row x (64 kDbiasChunk)-key block of one bias slice (b', h') and sums
// the pairs of its broadcast group into registers, pair after pair in index order, then stores
// the block once: no read-modify-write of the output, and the memory is the bias-shaped output
// alone -- no [B, Hq, Sq, Sk] buffer.  The bias values are the same for every pair of the group
// (the summed dimensions have stride 0), so the block's bias is read once, into registers.
// Per pair the structure is dq_kernel's (query on the lane, Q / dO in registers, 64-key K/V tiles
// in LDS): S^T = K Q^T and dP^T = V dO^T (the same products as compute_dq.py:38-69), without the
// dQ GEMM; the next K/V tile and the next pair's Q/dO rows stream into LDS while the current
// pair computes.
// delta comes from the dQ (or delta) kernel that ran before (-rowsum(O dO), negated).
// 64-key tiles per dbias workgroup.  One: the block's sums and bias (32 + 32 fp32 per lane) leave
// the arch VGPRs room to read the K/V fragments ahead of the MFMAs; with two (64 + 64) the
// compiler read each fragment just before its MFMA and waited out the LDS latency every time.
#ifndef FA2_DBIAS_CHUNK
#define FA2_DBIAS_CHUNK 1
#endif
constexpr int kDbiasChunk = FA2_DBIAS_CHUNK;

// XCD-aware block order: workgroup g runs on XCD g % 8 as that XCD's (g / 8)-th; the blocks go
// out in 8 x 8 squares of (row block, key chunk), so the workgroups an XCD runs together share
// 8 row blocks' Q / dO and 8 key chunks' K / V in its L2 (each read by 8 workgroups instead of
// 1).  Square (r, c) goes to XCD (r + c) % 8: anti-diagonals, so that the causal triangle's
// squares spread evenly over the XCDs (square columns would give XCD 0 fifteen times XCD 7's
// work).  The square columns are padded to a multiple of 8 (dbias_blocks); padding
// workgroups get mb = -1.
// (grids under 32 x 32 blocks use 1 x 1 "squares": whole squares would crowd them onto few XCDs)
__host__ __device__ inline int dbias_side(int nmb, int nkc) { return nmb >= 32 && nkc >= 32 ? 8 : 1; }
__host__ __device__ inline int dbias_blocks(int nmb, int nkc) {  // the padded grid
  const int e = dbias_side(nmb, nkc);
  const int sqr = (nmb + e - 1) / e, sqk = (nkc + e - 1) / e;
  return sqr * ((sqk + 7) / 8 * 8) * e * e;
}
FA2_DEV void dbias_block(int g, int nmb, int nkc, int& mb, int& kc) {
  const int e = dbias_side(nmb, nkc);
  const int x = g & 7, j = g >> 3;
  const int q = j / (e * e), within = j % (e * e);
  const int sqk = (nkc + e - 1) / e, per_row = (sqk + 7) / 8;
  const int r = q / per_row, m = q - r * per_row;
  const int c = ((x - r) & 7) + 8 * m;  // (r + c) % 8 == x
  mb = r * e + within / e;
  kc = c * e + within % e;
  if (c >= sqk || mb >= nmb || kc >= nkc) mb = -1;
}

template <bool BF16, int DT, bool CAUSAL, bool DROPOUT, bool ALIGNED>
__global__ void __launch_bounds__(256, DT <= 64 && !DROPOUT ? 2 : 1) dbias_kernel(const fa2_bwd_args p) {
  using E = Elem<BF16>;
  constexpr int NT = 256, BM = 128, BN = 64, C = kDbiasChunk;
  constexpr int KS = DT / 16;
  constexpr int TILE = BN * DT * 2;
  // D <= 128: the pair's Q / dO rows go through LDS (coalesced 16-byte DMA pieces, then one
  // fragment read per lane): loaded straight into the row-per-lane registers, every load
  // instruction would touch 32 rows x 32 bytes and the address unit, not the MFMAs, would set
  // the pace.  D = 256 loads them into registers directly (the LDS would not hold both tiles).
  constexpr bool QLDS = DT <= 128;
  constexpr int QTILE = QLDS ? BM * DT * 2 : 0;
  // K/V tiles: a ring of 3 (D <= 128; staged two steps ahead) or 2 (D = 256, one step ahead)
  constexpr int RING = QLDS ? 3 : 2;
  // the deep pipeline counts its loads: fixed VMEM instructions per step (LDS-DMA pieces per
  // K/V tile and per Q/dO block; the two -LSE / -delta loads land before those go out)
  constexpr int KV_VM = 2 * BufStager<DT, BN, NT>::kIters, QO_VM = 2 * BufStager<DT, BM, NT>::kIters;
  constexpr bool DEEP = QLDS && ALIGNED && !DROPOUT;
  __shared__ __attribute__((aligned(16))) char smem[2 * RING * TILE + 2 * QTILE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, hh = lane >> 5;
  const int nkt = (p.seqlen_k + BN - 1) / BN;        // key tiles of the output rows
  const int nkc = (nkt + C - 1) / C;
  int mb, kc;
  dbias_block(blockIdx.x, (p.seqlen_q + BM - 1) / BM, nkc, mb, kc);
  if (mb < 0) return;                                // grid padding
  const int t0 = kc * C, t1 = min(nkt, t0 + C);     // this workgroup's key tiles
  const int Hb = p.bias_stride[1] != 0 ? p.heads_q : 1;
  const int slice = blockIdx.y;                       // (b', h') of the bias
  const int bb = slice / Hb, hb = slice - bb * Hb;
  const bool sum_b = p.bias_stride[0] == 0, sum_h = p.bias_stride[1] == 0;
  const int nb = sum_b ? p.batch : 1, nh = sum_h ? p.heads_q : 1;
  const int np = nb * nh;
  const int D = p.head_dim;
  const int m0 = mb * BM;
  const int qi = m0 + 32 * w + r32;                  // this lane's row
  const float scale2 = p.softmax_scale * kLog2e;
  const bool row_in = qi < p.seqlen_q;

  auto kt = [&](int buf) { return smem + buf * 2 * TILE; };
  auto vt = [&](int buf) { return smem + TILE + buf * 2 * TILE; };
  char* const qt = smem + 2 * RING * TILE;
  char* const ot = smem + 2 * RING * TILE + QTILE;
  BufStager<DT, BN, NT> kst;
  BufStager<DT, BM, NT> qst, ost;
  int mrows = 0, qrows = 0, orows = 0;
  if (ALIGNED) {
    kst.init(tid, p.k_stride[1], D);
    mrows = BufStager<DT, BN, NT>::max_rows(p.k_stride[1]);
    if (QLDS) {
      qst.init(tid, p.q_stride[1], D);
      ost.init(tid, p.do_stride[1], D);
      qrows = BufStager<DT, BM, NT>::max_rows(p.q_stride[1]);
      orows = BufStager<DT, BM, NT>::max_rows(p.do_stride[1]);
    }
  }

  // element i of half t of tile c: key (t0 + c) 64 + 32 t + 8 (i / 4) + 4 hh + i % 4
  float acc[C][2][16], bl[C][2][16];
  {
    const int64_t brow = bb * p.bias_stride[0] + hb * p.bias_stride[1] + (int64_t)(row_in ? qi : 0) * p.bias_stride[2];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int kj = (t0 + c) * BN + 32 * t + (i & 3) + 8 * (i >> 2) + 4 * hh;
          acc[c][t][i] = 0.f;
          bl[c][t][i] = kLog2e * load_bias(p.bias, brow + (kj < p.seqlen_k ? kj : p.seqlen_k - 1), p.bias_dtype);
        }
  }

  // The pair cursor: the pair's index with its (batch, q-head, kv-head) carried along, so a step
  // moves it by increments (index -> (b, hq) -> kv-head by division costs ~25 instructions per
  // division, seven per step, on a one-wave-per-SIMD kernel whose step is short).  Pair order:
  // index = b nh + hq over the summed dims (as the dims of the bias's broadcast group).
  const int group = p.heads_q / p.heads_kv;
  struct Cur {
    int i, b, hq, hkv, gi;  // gi = hq - hkv group
  };
  Cur first;
  first.i = 0;
  first.b = sum_b ? 0 : bb;
  first.hq = sum_h ? 0 : hb;
  first.hkv = first.hq / group;
  first.gi = first.hq - first.hkv * group;
  auto step_cur = [&](Cur c) {
    ++c.i;
    if (sum_h) {
      if (++c.gi == group) {
        c.gi = 0;
        ++c.hkv;
      }
      if (++c.hq == nh) {
        c.hq = c.hkv = c.gi = 0;
        ++c.b;
      }
    } else {
      ++c.b;  // (a single pair when neither dim is summed: past the end)
    }
    return c;
  };
  // the pair's visible key tiles are [t0, tend); a pair with none adds nothing
  struct Pair {
    int b, hq, hkv, Lq, Lk, tend;
  };
  auto pair_of = [&](const Cur& c) {
    Pair r;
    r.b = c.b;
    r.hq = c.hq;
    r.hkv = c.hkv;
    r.Lq = p.seqlen_q;
    r.Lk = p.seqlen_k;
    if (p.cu_seqlens) r.Lq = r.Lk = p.cu_seqlens[r.b + 1] - p.cu_seqlens[r.b];
    int n_end = 0;
    if (m0 < r.Lq) n_end = max(CAUSAL ? min(r.Lk, m0 + BM + r.Lk - r.Lq) : r.Lk, 0);
    r.tend = min(t1, (n_end + BN - 1) / BN);
    return r;
  };
  auto next_visible = [&](Cur c) {
    while (c.i < np && pair_of(c).tend <= t0) c = step_cur(c);
    return c;
  };
  auto stage_kv = [&](int buf, const Pair& r, int n) {
    const uint16_t* kg = (const uint16_t*)p.k + r.b * p.k_stride[0] + r.hkv * p.k_stride[2];
    const uint16_t* vg = (const uint16_t*)p.v + r.b * p.v_stride[0] + r.hkv * p.v_stride[2];
    if constexpr (ALIGNED) {
      kst.issue(kt(buf), kg, p.k_stride[1], n, r.Lk, mrows);
      kst.issue(vt(buf), vg, p.v_stride[1], n, r.Lk, mrows);
    } else {
      stage_tile<DT, BN, NT, false>(kt(buf), kg, p.k_stride[1], n, r.Lk, D, tid);
      stage_tile<DT, BN, NT, false>(vt(buf), vg, p.v_stride[1], n, r.Lk, D, tid);
    }
  };
  auto q_base = [&](const Pair& r) { return (const uint16_t*)p.q + r.b * p.q_stride[0] + r.hq * p.q_stride[2]; };
  auto o_base = [&](const Pair& r) { return (const uint16_t*)p.dout + r.b * p.do_stride[0] + r.hq * p.do_stride[2]; };
  auto stage_qo = [&](const Pair& r) {  // the pair's 128 Q / dO rows of this block into LDS
    if constexpr (QLDS) {
      if constexpr (ALIGNED) {
        qst.issue(qt, q_base(r), p.q_stride[1], m0, r.Lq, qrows);
        ost.issue(ot, o_base(r), p.do_stride[1], m0, r.Lq, orows);
      } else {
        stage_tile<DT, BM, NT, false>(qt, q_base(r), p.q_stride[1], m0, r.Lq, D, tid);
        stage_tile<DT, BM, NT, false>(ot, o_base(r), p.do_stride[1], m0, r.Lq, D, tid);
      }
    }
  };
  // the lane's row of the pair's LSE2 and -delta (row 0 exists: Lq > 0)
  auto rowstats = [&](const Pair& r, float& l, float& d) {
    const int64_t srow = (int64_t)(r.b * p.heads_q + r.hq) * p.lse_row_stride + (qi < r.Lq ? qi : 0);
    l = p.lse[srow];
    d = p.delta[srow];
  };

  Cur cur = next_visible(first);
  int buf = 0;
  // staging cursor (pair, tile) of the K/V ring, RING - 1 steps ahead of the compute; past the
  // last pair it re-stages a tile of the current pair (unused) so every step issues the same loads
  Cur scur = cur;
  int sc = 0;
  auto advance = [&]() {
    if (++sc == C) {
      sc = 0;
      scur = next_visible(step_cur(scur));
    }
  };
  float lse_v = 0.f, del_v = 0.f;
  if (cur.i < np) {
    const Pair r = pair_of(cur);
    rowstats(r, lse_v, del_v);
    stage_qo(r);
    for (int k = 0; k < RING - 1; ++k) {
      stage_kv(k, scur.i < np ? pair_of(scur) : r, t0 * BN + (scur.i < np ? sc : 0) * BN);
      advance();
    }
  }
  vm_wait_all();
  __syncthreads();
  while (cur.i < np) {
    const Pair r = pair_of(cur);
    const Cur nxc = next_visible(step_cur(cur));
    const bool has_next = nxc.i < np;
    const int b = r.b, hq = r.hq, Lq = r.Lq, Lk = r.Lk;
    const bool qvalid = qi < Lq;
    // this pair's LSE2 / -delta were loaded a step ago: landed before this step's LDS-DMA goes out
    // (the compiler's own wait for them counts no LDS-DMA: waited at their use it would be a
    // vmcnt(0) that drains this step's prefetches)
    asm volatile("" : "+v"(lse_v), "+v"(del_v));
    const float nlse = qvalid ? -lse_v : 0.f;
    const float ndel = qvalid ? del_v : 0.f;  // the workspace holds -delta
    // the next pair's go out ahead of this step's LDS-DMA, so the step-end wait retires them
    // (loaded at the step start and waited at once, each step had exposed one load latency)
    float lse_n = 0.f, del_n = 0.f;
    if (has_next) rowstats(pair_of(nxc), lse_n, del_n);
    u32x4 qf[KS], of[KS];
    if constexpr (QLDS) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        qf[ks] = lds_row_frag<DT, BM>(qt, 32 * w, r32, ks, hh);
        of[ks] = lds_row_frag<DT, BM>(ot, 32 * w, r32, ks, hh);
      }
    } else {
      const uint16_t* qrow = q_base(r) + (int64_t)(qvalid ? qi : 0) * p.q_stride[1];
      const uint16_t* orow = o_base(r) + (int64_t)(qvalid ? qi : 0) * p.do_stride[1];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        qf[ks] = load_row_frag<ALIGNED>(qrow, 16 * ks + 8 * hh, D, qvalid);
        of[ks] = load_row_frag<ALIGNED>(orow, 16 * ks + 8 * hh, D, qvalid);
      }
    }
    if constexpr (QLDS) {
      // every wave holds its fragments: the next pair's rows may overwrite the tiles
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
      __syncthreads();
      if (has_next) stage_qo(pair_of(nxc));
      else if (DEEP) stage_qo(r);  // (unused: keeps the step's load count)
    }
    const int lim_lane = !qvalid ? 0 : (CAUSAL ? min(Lk, qi + Lk - Lq + 1) : Lk);
    uint64_t drop_row = 0;
    float inv_keep = 1.f;
    if (DROPOUT) {
      const uint64_t cu0 = p.cu_seqlens ? (uint64_t)p.cu_seqlens[b] : 0;
      drop_row = (uint64_t)Lk * (cu0 + (uint64_t)Lq * ((uint64_t)hq + (uint64_t)p.heads_q * (p.cu_seqlens ? 0 : b))) +
                 (uint64_t)qi * (uint64_t)Lk;
      inv_keep = 1.f / (1.f - p.dropout_p);
    }

#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int it = t0 + c;
      if (RING == 3 || it < r.tend) {
        const int n0 = it * BN;
        if constexpr (RING == 3) {  // the tile RING - 1 steps ahead (every step of a pair runs)
          stage_kv(buf == 0 ? 2 : buf - 1, scur.i < np ? pair_of(scur) : r, (t0 + (scur.i < np ? sc : 0)) * BN);
          advance();
        } else {  // the next tile: this pair's, else the next visible pair's first
          if (it + 1 < r.tend) stage_kv(buf ^ 1, r, n0 + BN);
          else if (has_next) stage_kv(buf ^ 1, pair_of(nxc), t0 * BN);
        }
        const char* K = kt(buf);
        const char* V = vt(buf);
        const int rel = lim_lane - n0 - 4 * hh;
        // the tile's K / V fragments of both key halves, read ahead of the MFMAs (read next to
        // each MFMA, every one of them waited out the LDS latency)
        // (D = 256: read next to the MFMAs, the register file would not hold them)
        u32x4 kf[2][QLDS ? KS : 1], vf[2][QLDS ? KS : 1];
        if (QLDS && it < r.tend) {
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
              kf[t][QLDS ? ks : 0] = lds_row_frag<DT, BN>(K, 32 * t, r32, ks, hh);
              vf[t][QLDS ? ks : 0] = lds_row_frag<DT, BN>(V, 32 * t, r32, ks, hh);
            }
          __builtin_amdgcn_sched_barrier(0);  // (the scheduler would sink each read to its MFMA)
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if (it >= r.tend) break;  // a ring step over a tile this pair does not see
          uint32_t mwd = 0u;  // the forward's saved keep word of this row and key half
          if (DROPOUT && p.dropout_mask && qvalid && n0 + 32 * t < p.seqlen_k) {
            const int nrb = (p.seqlen_q + 31) >> 5, ncw = (p.seqlen_k + 31) >> 5;
            mwd = p.dropout_mask[((((int64_t)(b * p.heads_q + hq) * nrb + (qi >> 5)) * ncw + ((n0 >> 5) + t)) * 32) + (qi & 31)];
          }
          f32x16 s = zero16(), dp = zero16();
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            if constexpr (QLDS) {
              s = E::mfma(kf[t][ks], qf[ks], s);
              dp = E::mfma(vf[t][ks], of[ks], dp);
            } else {
              s = E::mfma(lds_row_frag<DT, BN>(K, 32 * t, r32, ks, hh), qf[ks], s);
              dp = E::mfma(lds_row_frag<DT, BN>(V, 32 * t, r32, ks, hh), of[ks], dp);
            }
          }
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int o = 32 * t + (i & 3) + 8 * (i >> 2);
            float pr = __builtin_amdgcn_exp2f(fmaf(s[i], scale2, bl[c][t][i]) + nlse);
            pr = o < rel ? pr : 0.f;
            float dpv = dp[i];
            if (DROPOUT) {
              const bool keep = p.dropout_mask ? ((mwd >> ((i & 3) + 8 * (i >> 2) + 4 * hh)) & 1u) != 0
                                               : philox_uniform(p.dropout_seed, drop_row + (uint64_t)(n0 + o + 4 * hh)) > p.dropout_p;
              dpv *= keep ? inv_keep : 0.f;
            }
            acc[c][t][i] += pr * (dpv + ndel);
          }
        }
        if constexpr (DEEP) {
          // all but the loads this step issued after what the next step needs: the next step's
          // tile, and at a pair's last step the next pair's Q / dO (issued at its first step,
          // before that step's K/V); s_waitcnt vmcnt(n): bits 3:0 and 15:14 of the count
          static_assert(KV_VM + QO_VM < 64, "vmcnt range");
          constexpr int n0c = KV_VM + QO_VM, n1c = KV_VM;
          if (c < C - 1)
            __builtin_amdgcn_s_waitcnt((n0c & 15) | ((n0c >> 4) << 14) | 0x0f70);
          else
            __builtin_amdgcn_s_waitcnt((n1c & 15) | ((n1c >> 4) << 14) | 0x0f70);
        } else {
          vm_wait_all();
        }
        __syncthreads();
        buf = RING == 3 ? (buf == 2 ? 0 : buf + 1) : buf ^ 1;
      }
    }
    cur = nxc;
    lse_v = lse_n;
    del_v = del_n;
  }

  // one store of the block (16-byte stores when the rows allow them: a group's 4 keys are contiguous)
  if (!row_in) return;
  float* drow = p.dbias + bb * p.dbias_stride[0] + hb * p.dbias_stride[1] + (int64_t)qi * p.dbias_stride[2];
  const bool vec4 = ((uintptr_t)p.dbias & 15) == 0 && p.dbias_stride[0] % 4 == 0 && p.dbias_stride[1] % 4 == 0 &&
                    p.dbias_stride[2] % 4 == 0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    if (t0 + c >= t1) break;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int k0 = (t0 + c) * BN + 32 * t + 8 * g + 4 * hh;
        if (vec4 && k0 + 4 <= p.seqlen_k) {
          *(f32x4*)(drow + k0) = f32x4{acc[c][t][4 * g], acc[c][t][4 * g + 1], acc[c][t][4 * g + 2], acc[c][t][4 * g + 3]};
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (k0 + j < p.seqlen_k) drow[k0 + j] = acc[c][t][4 * g + j];
        }
      }
  }
}

// ---------------------------------------------------------------------------------------------
// the standalone delta launch, shared with the windowed backward (local_kernel.h)
template <bool BF16, bool ALIGNED>
static void launch_delta(const fa2_bwd_args& a, hipStream_t st) {
  dim3 grid((a.lse_row_stride + 15) / 16, a.batch * a.heads_q);
  hipLaunchKernelGGL((delta_kernel<BF16, ALIGNED>), grid, dim3(256), 0, st, a);
}

// The stages of a plan (select_bwd) that is not local, in the plan's order: standalone delta (bit
// 0), dQ (bit 2; also writes delta), the bias gradient (bit 3), dK/dV (bit 1, reads delta).  What
// no plan holds is ruled out here: BIASK 16 / 17 (LDS-staged bias tiles) exist only with aligned
// rows, the hand-placed kernels only at DT == 128 && BIASK == 0 && ALIGNED (D = 128 exactly;
// dropout: with the forward's saved keep words).
template <bool BF16, int DT, bool CAUSAL, int BIASK, bool DROPOUT, bool ALIGNED>
static hipError_t launch_bwd_t(const fa2_bwd_args& a, const BwdPlan& p, LaunchCtx ctx) {
  if constexpr (BIASK >= 16 && !ALIGNED) {
    return hipErrorInvalidValue;
  } else {
    constexpr bool HP = DT == 128 && BIASK == 0 && ALIGNED;
    hipStream_t st = ctx.stream;
    for (int i = 0; i < p.nstages; ++i)
      if (p.stage[i].path == Path::hand_placed && !HP) return hipErrorInvalidValue;
    for (int i = 0; i < p.nstages; ++i) {
      const bool hp = p.stage[i].path == Path::hand_placed;
      switch (p.stage[i].kind) {
        case Stage::delta: launch_delta<BF16, ALIGNED>(a, st); break;
        case Stage::dq:
          if (hp) {
            if constexpr (HP) launch_dq_hp<BF16, CAUSAL, DROPOUT>(a, ctx);
          } else {
            constexpr int NW = DqCfg<DT>::NW, BM = NW * 32;
            const int nmb = (a.seqlen_q + BM - 1) / BM;
            dim3 grid((CAUSAL ? (nmb + 1) / 2 : nmb) * a.batch * a.heads_q);  // causal: mirrored pairs of blocks
            dispatch(  // dQ in fp32 concerns this launch alone
                [&](auto f32) {
                  hipLaunchKernelGGL((dq_kernel<BF16, DT, CAUSAL, BIASK, DROPOUT, ALIGNED, f32.value>), grid, dim3(NW * 64), 0, st, a);
                  return hipSuccess;
                },
                p.dq_f32, bools{});
          }
          break;
        case Stage::dbias: {
          const int bb = a.bias_stride[0] != 0 ? a.batch : 1, hb = a.bias_stride[1] != 0 ? a.heads_q : 1;
          const int nkc = ((a.seqlen_k + 63) / 64 + kDbiasChunk - 1) / kDbiasChunk;
          dim3 grid(dbias_blocks((a.seqlen_q + 127) / 128, nkc), bb * hb);
          hipLaunchKernelGGL((dbias_kernel<BF16, DT, CAUSAL, DROPOUT, ALIGNED>), grid, dim3(256), 0, st, a);
          break;
        }
        case Stage::dkdv:
          if (hp) {
            if constexpr (HP) launch_dkdv_hp<BF16, CAUSAL, DROPOUT>(a, p.nsplit, ctx);
          } else {
            dim3 grid(((a.seqlen_k + 127) / 128) * a.batch * a.heads_kv * p.nsplit);
            hipLaunchKernelGGL((dkdv_kernel<BF16, DT, CAUSAL, BIASK, DROPOUT, ALIGNED>), grid, dim3(256), 0, st, a, p.nsplit);
          }
          if (p.reduce) {
            const int64_t n = (int64_t)a.batch * a.heads_kv * a.seqlen_k * ((a.head_dim + 3) / 4);
            hipLaunchKernelGGL((dkv_reduce_kernel<BF16>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, p.nsplit);
          }
          break;
      }
    }
    return hipGetLastError();
  }
}

template <bool BF16, int DT>
hipError_t launch_bwd_dt(const fa2_bwd_args& a, LaunchCtx ctx, int stages) {
  const BwdPlan p = select_bwd(a, ctx.aligned, stages, ctx.policy);
  // a sliding window (normalised by api.hip) comes first: no other kernel knows one
  if (a.local) return launch_bwd_local<BF16, DT>(a, p, ctx.stream);
  return dispatch(
      [&](auto causal, auto biask, auto dropout, auto aligned) {
        return launch_bwd_t<BF16, DT, causal.value, biask.value, dropout.value, aligned.value>(a, p, ctx);
      },
      p.causal, bools{}, p.biask, values<0, 1, 16, 17>{}, p.dropout, bools{}, p.aligned, bools{});
}

}  // namespace fa2
