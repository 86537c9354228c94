// select.h -- which kernels a call launches, as pure functions of its arguments and policy.
//
// The authority for the selection table of DESIGN.md 1: the launchers (fwd_kernel.h, bwd_kernel.h,
// local_kernel.h, kvcache_kernel.h) compute a plan here and launch exactly what it names, and
// tests/test_select_host.py pins the plans on the CPU.  Host arithmetic only: no HIP call, no
// global, nothing but the C ABI header and the standard library.
#pragma once
#include <stdint.h>

#include "fa2_amd.h"  // include/ (build.py passes -I)

namespace fa2 {

// ---------------------------------------------------------------------------------------------
// The path policy of one call (fa2_policy, ABI 9; nullptr: every path on, no grid cap).
inline bool path_enabled(const fa2_policy* policy, uint32_t bit) { return !(policy && (policy->disable & bit)); }
// grid of a persistent kernel over `items` work units: one workgroup per compute unit, capped by
// the policy, never more workgroups than items
inline int hp_grid(int64_t items, int ncu, const fa2_policy* policy) {
  const int cap = policy ? policy->grid_cap : 0;
  if (cap > 0 && cap < ncu) ncu = cap;
  return (int)(items < ncu ? items : ncu);
}

// head-dim tile of the kernels' DT template argument; 0: head_dim > 256
inline int head_dim_tile(int d) { return d <= 32 ? 32 : d <= 64 ? 64 : d <= 128 ? 128 : d <= 256 ? 256 : 0; }

// a bias the LDS-staged paths take (16-bit, every row 16-byte aligned)
inline bool bias16_rows(const void* bias, int dtype, const int64_t* stride) {
  return bias && (dtype == 16 || dtype == 17) && ((uintptr_t)bias & 15) == 0 && stride[0] % 8 == 0 &&
         stride[1] % 8 == 0 && stride[2] % 8 == 0;
}

// The hand-placed forward (fwd_hp_kernel.h) applies to D = 128 exactly (the emitted statements: 8
// k-steps, 4 d-tiles), aligned rows, equal K / V row strides, no bias, dropout only with a
// keep-mask buffer (whose words it reads; byte offsets within 32 bits), and K / V slices whose
// byte range fits the 32-bit descriptor arithmetic of the statement.
inline bool fwd_hp_ok(const fa2_fwd_args& a, bool aligned, const fa2_policy* policy) {
  if (!path_enabled(policy, FA2_PATH_FWD_HP) || !aligned || a.head_dim != 128 || a.bias) return false;
#if FA2_HP_STAMPS
  if (a.dropout_p > 0.f) return false;  // (stamp builds: no dropout statement)
#endif
  if (a.dropout_p > 0.f &&
      (!a.dropout_mask || (int64_t)a.batch * a.heads_q * ((a.seqlen_q + 31) / 32) * ((a.seqlen_k + 31) / 32) * 128 >= ((int64_t)1 << 31)))
    return false;
  if (a.k_stride[1] != a.v_stride[1]) return false;
  return (int64_t)(a.seqlen_k + 128) * a.k_stride[1] * 2 < ((int64_t)1 << 31);
}

// The hand-placed dQ (dq_hp_kernel.h): D = 128 exactly, aligned rows, equal K / V row strides, dQ
// in the input dtype, no bias, dropout only with the forward's saved keep words, and K / V slices
// within the statement's 32-bit descriptor arithmetic.
inline bool dq_hp_ok(const fa2_bwd_args& a, bool aligned, const fa2_policy* policy) {
  if (!path_enabled(policy, FA2_PATH_DQ_HP) || !aligned || a.head_dim != 128 || a.bias || a.dq_dtype != a.dtype) return false;
  if (a.dropout_p > 0.f) {  // dropout: the forward's saved keep words, byte offsets within 2^31
    if (!a.dropout_mask) return false;
    const int64_t nrb = (a.seqlen_q + 31) / 32, ncw = (a.seqlen_k + 31) / 32;
    if ((int64_t)a.batch * a.heads_q * nrb * ncw * 128 >= ((int64_t)1 << 31)) return false;
  }
  if (a.k_stride[1] != a.v_stride[1]) return false;
  const int64_t lim = (int64_t)1 << 31;
  return (int64_t)(a.seqlen_k + 128) * a.k_stride[1] * 2 < lim && (int64_t)64 * a.q_stride[1] * 2 < lim &&
         (int64_t)64 * a.do_stride[1] * 2 < lim;
}

// The hand-placed dK/dV (dkdv_hp_kernel.h) applies to D = 128 exactly, aligned rows, no bias,
// dropout only with the forward's saved keep words and Q / dO of one row stride (the dropout
// statement shares their DMA offsets), and problems whose Q / dO / LSE / keep-word byte offsets fit
// the statement's 32-bit cursor arithmetic.
inline bool dkdv_hp_ok(const fa2_bwd_args& a, bool aligned, const fa2_policy* policy) {
  if (!path_enabled(policy, FA2_PATH_DKDV_HP) || !aligned || a.head_dim != 128 || a.bias) return false;
  const int64_t lim = (int64_t)1 << 31;
  if (a.dropout_p > 0.f) {
    if (!a.dropout_mask || a.q_stride[1] != a.do_stride[1]) return false;
    const int64_t nrb = (a.seqlen_q + 31) / 32, ncw = (a.seqlen_k + 31) / 32;
    if ((int64_t)(a.heads_q / a.heads_kv) * nrb * ncw * 128 >= lim) return false;
  }
  const int64_t lse_bytes = (int64_t)a.batch * a.heads_q * a.lse_row_stride * 4;
  // the statement's cursors move by 32-bit amounts: one tile, and at a q-head wrap back over the
  // head's tiles plus one head stride (qwrap / owrap / lwrap)
  if (a.q_stride[2] < 0 || a.do_stride[2] < 0) return false;
  return (int64_t)(a.seqlen_q + 64) * a.q_stride[1] * 2 + 2 * a.q_stride[2] < lim &&
         (int64_t)(a.seqlen_q + 64) * a.do_stride[1] * 2 + 2 * a.do_stride[2] < lim && lse_bytes < lim;
}

// q-head split of dK/dV (ABI 4): the smallest divisor s of the GQA group size G = Hq / Hkv with
// s * B * Hkv * ceil(Sk / 128) >= kDkvTargetGrid workgroups (two per CU), G if none is; 1 when
// G == 1 or the grid is already that large.
constexpr int kDkvTargetGrid = 512;
inline int dkv_split_count(int B, int Hq, int Hkv, int Sk) {
  if (B < 1 || Hkv < 1 || Hq % Hkv != 0 || Sk < 1) return 1;
  const int G = Hq / Hkv;
  const int64_t grid = (int64_t)((Sk + 127) / 128) * B * Hkv;
  if (G <= 1 || grid >= kDkvTargetGrid) return 1;
  for (int s = 2; s < G; ++s)
    if (G % s == 0 && grid * s >= kDkvTargetGrid) return s;
  return G;
}
inline int64_t dkv_workspace_bytes(int B, int Hq, int Hkv, int Sk, int D) {
  const int s = dkv_split_count(B, Hq, Hkv, Sk);
  return s > 1 ? 2 * (int64_t)s * B * Hkv * Sk * D * 4 : 0;
}
// the split a launch uses: only with a large enough workspace (checked by fa2_bwd_stages)
inline int dkv_split(const fa2_bwd_args& a) {
  return a.dkv_workspace ? dkv_split_count(a.batch, a.heads_q, a.heads_kv, a.seqlen_k) : 1;
}

// ---------------------------------------------------------------------------------------------
// The plans.  Path: which family of kernels; the flags are the kernels' template arguments.
enum class Path : int { general, pipelined, hand_placed, local };

// Forward: an optional dropout_mask_kernel launch (misc.hip), then one kernel --
//   local        fwd_local_kernel<BF16, DT, aligned>
//   hand_placed  fwd_hp_kernel<BF16, causal, 128, drop != 0>
//   pipelined    fwd_pipe_kernel<BF16, DT, causal, 4, biask>          (biask 0 / 16 / 17)
//   general      fwd_kernel<BF16, DT, causal, biask != 0, drop, aligned>
// biask: 0 no bias, 1 element loads, 16 / 17 an fp16 / bf16 bias staged by LDS-DMA.  drop: 0 none,
// 1 Philox draws in the softmax, 2 the keep words dropout_mask_kernel wrote just before are read.
struct FwdPlan {
  Path path;
  bool causal, aligned, mask_first;
  int biask, drop;
};

inline FwdPlan select_fwd(const fa2_fwd_args& a, bool aligned, const fa2_policy* policy) {
  const bool bias = a.bias != nullptr, dropout = a.dropout_p > 0.f;
  // a sliding window (normalised by api.hip) comes first: no other kernel knows one
  if (a.local) return {Path::local, false, aligned, false, 0, 0};
  const int drop = dropout ? (a.dropout_mask ? 2 : 1) : 0, dt = head_dim_tile(a.head_dim);
  FwdPlan p = {Path::general, a.causal != 0, aligned, drop == 2, bias ? 1 : 0, drop};
  if (fwd_hp_ok(a, aligned, policy)) {
    p.path = Path::hand_placed;
  } else if ((dt == 64 || dt == 128) && aligned && !dropout && a.k_stride[1] == a.v_stride[1] &&
             (!bias || bias16_rows(a.bias, a.bias_dtype, a.bias_stride))) {
    // the software-pipelined kernel, also with a 16-bit bias whose rows are 16-byte aligned (its
    // tiles are staged by LDS-DMA)
    p.path = Path::pipelined;
    p.biask = !bias ? 0 : (a.bias_dtype == FA2_BF16 ? 17 : 16);
  }
  return p;
}

// Backward: the stages launch in the order of `stage` --
//   delta  delta_kernel<BF16, aligned>                                 (stage bit 0)
//   dq     dq_hp_kernel<BF16, causal, dropout> | dq_local_kernel<BF16, DT, aligned, dq_f32> |
//          dq_kernel<BF16, DT, causal, biask, dropout, aligned, dq_f32>  (bit 2; writes delta too)
//   dbias  dbias_kernel<BF16, DT, causal, dropout, aligned>             (bit 3)
//   dkdv   dkdv_hp_kernel<BF16, causal, dropout> | dkdv_local_kernel<BF16, DT, aligned> |
//          dkdv_kernel<BF16, DT, causal, biask, dropout, aligned>, over nsplit q-head splits,
//          then dkv_reduce_kernel<BF16> when `reduce`                  (bit 1; reads delta)
// Zero-sized problems launch nothing for that side: Sk == 0 -> dQ = 0 (dq_kernel sees no key tile
// and writes zeros), no dK/dV rows; Sq == 0 -> dK/dV = 0, no dQ rows.
enum class Stage : int { delta, dq, dbias, dkdv };
struct BwdPlan {
  bool causal, dropout, aligned, dq_f32;
  int biask;
  struct {
    Stage kind;
    Path path;
  } stage[4];
  int nstages;
  int nsplit;
  bool reduce;
};

inline BwdPlan select_bwd(const fa2_bwd_args& a, bool aligned, int stages, const fa2_policy* policy) {
  BwdPlan p = {};
  const bool bias = a.bias != nullptr;
  p.causal = !a.local && a.causal != 0;
  p.dropout = a.dropout_p > 0.f;
  p.aligned = aligned;
  p.dq_f32 = a.dq_dtype == FA2_F32;
  p.nsplit = 1;
  // a 16-bit bias with 16-byte aligned rows: LDS-staged bias tiles
  if (bias) p.biask = aligned && bias16_rows(a.bias, a.bias_dtype, a.bias_stride) ? (a.bias_dtype == FA2_BF16 ? 17 : 16) : 1;
  const Path local_or = a.local ? Path::local : Path::general;  // a window knows no other kernel
  auto add = [&](Stage kind, Path path) {
    p.stage[p.nstages].kind = kind;
    p.stage[p.nstages++].path = path;
  };
  if ((stages & 1) && a.lse_row_stride > 0) add(Stage::delta, Path::general);
  if ((stages & 4) && a.seqlen_q > 0) add(Stage::dq, !a.local && dq_hp_ok(a, aligned, policy) ? Path::hand_placed : local_or);
  if ((stages & 8) && bias && a.dbias && a.seqlen_q > 0 && a.seqlen_k > 0) add(Stage::dbias, Path::general);
  if ((stages & 2) && a.seqlen_k > 0) {
    add(Stage::dkdv, !a.local && dkdv_hp_ok(a, aligned, policy) ? Path::hand_placed : local_or);
    // the windowed dK/dV sums each GQA group in one workgroup
    if (!a.local) p.nsplit = dkv_split(a);
    p.reduce = p.nsplit > 1;
  }
  return p;
}

// ---------------------------------------------------------------------------------------------
// KV-cache decode (kvcache_kernel.h): the unit count, the split heuristic and the workspace size.
// Functions of the shapes only -- never of the cache lengths, which stay on the device.  A paged
// call uses those of its `base`, an fp8 call those of its `paged.base`.
inline const fa2_kvcache_args& kv_base(const fa2_kvcache_args& a) { return a; }
inline const fa2_kvcache_args& kv_base(const fa2_paged_kvcache_args& a) { return a.base; }
inline const fa2_kvcache_args& kv_base(const fa2_fp8_kvcache_args& a) { return a.paged.base; }

// 32-row tiles of a kv head's rows (the Hq / Hkv q-heads of the group x the Sq query positions)
inline int kv_row_tiles(const fa2_kvcache_args& a) {
  return (int)(((int64_t)(a.heads_q / a.heads_kv) * a.seqlen_q + 31) / 32);
}
inline int64_t kv_units(const fa2_kvcache_args& a) { return (int64_t)a.batch * a.heads_kv * kv_row_tiles(a); }

// 64-key tiles of the longest key span a batch can have: the capacity, or with a left window bound
// the band of the Sq rows (left + Sq keys, up to 63 more for the tile-aligned start)
inline int kv_span_tiles(const fa2_kvcache_args& a) {
  int64_t span = a.capacity;
  if (a.window_left >= 0) {
    const int64_t band = (int64_t)a.window_left + a.seqlen_q + 63;
    if (band < span) span = band;
  }
  const int64_t t = (span + 63) / 64;
  return (int)(t < 1 ? 1 : t);
}

// the smallest split count that gives two workgroups per compute unit, never cutting the span
// into runs of fewer than FA2_KVCACHE_MIN_SPLIT_TILES tiles, at most FA2_KVCACHE_MAX_SPLITS
inline int kv_auto_splits(const fa2_kvcache_args& a, int ncu) {
  const int64_t units = kv_units(a);
  int64_t want = (2 * (int64_t)ncu + units - 1) / units;
  const int64_t most = kv_span_tiles(a) / FA2_KVCACHE_MIN_SPLIT_TILES;
  if (want > most) want = most;
  if (want > FA2_KVCACHE_MAX_SPLITS) want = FA2_KVCACHE_MAX_SPLITS;
  return (int)(want < 1 ? 1 : want);
}

inline int64_t kv_workspace_bytes(const fa2_kvcache_args& a, int nsplit) {
  if (nsplit <= 1) return 0;
  return (int64_t)nsplit * a.batch * a.heads_q * a.seqlen_q * ((int64_t)a.head_dim + 1) * 4;
}

// ---------------------------------------------------------------------------------------------
// fp8 caches (kvcache_kernel.h, FP8): the kernels exist for the head-dim tiles 64 and 128 (a tile's
// rows are DT bytes, 16-byte pieces of 16 elements) and both layouts.  Units, splits and workspace
// are those of `paged.base` above.
constexpr int kFp8MaxHeadDim = 128;
// head-dim tile of the fp8 kernels' DT; 0: head_dim > 128
inline int fp8_head_dim_tile(int d) { return d <= 64 ? 64 : d <= kFp8MaxHeadDim ? 128 : 0; }
// a NULL block table is the contiguous layout
inline bool fp8_paged(const fa2_fp8_kvcache_args& a) { return a.paged.block_table != nullptr; }
// every row of a byte cache starts on a 16-byte boundary
inline bool fp8_rows16(const void* cache, const int64_t* stride) {
  return ((uintptr_t)cache & 15) == 0 && stride[0] % 16 == 0 && stride[1] % 16 == 0 && stride[2] % 16 == 0;
}

}  // namespace fa2
