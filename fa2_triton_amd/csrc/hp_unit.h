// hp_unit.h -- what fwd_hp_kernel.h, dq_hp_kernel.h and dkdv_hp_kernel.h share around their
// generated statements: the 256-row unit of the forward and dQ, its tile classes, the persistent
// schedule's dimensions and walk, buffer-descriptor words and ranges.  The first part is integer
// arithmetic a host compiler takes as it is (tests/test_hp_unit_host.py: brute force over rows and
// keys); the second (PersistSched, readfirstlane) is device code.
// Each function has the form that left every kernel's bytes as they were (compare_code_objects.py).
#pragma once
#include <stdint.h>

#ifdef __HIP__
#define FA2_HD __host__ __device__ __forceinline__
#else
#define FA2_HD inline
#endif

namespace fa2 {
constexpr int kHpBlock = 256;  // query rows of a unit, keys of a dK/dV block: 4 waves x 64
constexpr int kHpTile = 64;    // keys of a K / V tile

FA2_HD int hp_min(int a, int b) { return a < b ? a : b; }
FA2_HD int hp_max(int a, int b) { return a > b ? a : b; }

// One work unit of the forward and dQ = 256 query rows (4 waves x 64) of one (batch, q-head), its
// valid lengths (varlen: Lq == Lk from cu_seqlens) and the 64-key tiles it visits: up to the last
// one any of its rows sees (key j is visible to row i iff j < Lk and, causal,
// j <= i + Lk - Lq).  init returns the kv head (stored as a seventh int it moved the forward's code).
template <bool CAUSAL>
struct HpRowUnit {
  int b, hq, Lq, Lk, m0, ntiles;
  FA2_HD int init(int heads_q, int heads_kv, int seqlen_q, int seqlen_k, const int32_t* cu_seqlens, int bh, int mb) {
    b = bh / heads_q;
    hq = bh - b * heads_q;
    const int hkv = hq / (heads_q / heads_kv);
    Lq = seqlen_q;
    Lk = seqlen_k;
    if (cu_seqlens) {
      const int cu = cu_seqlens[b];
      Lq = Lk = cu_seqlens[b + 1] - cu;
    }
    m0 = mb * kHpBlock;
    int n_end = 0;
    if (m0 < Lq) {
      n_end = Lk;
      if (CAUSAL) n_end = hp_min(Lk, m0 + kHpBlock + Lk - Lq);
      n_end = hp_max(n_end, 0);
    }
    ntiles = (n_end + kHpTile - 1) / kHpTile;
    return hkv;
  }
};

// Wave-uniform tile classes of the wave whose 64 rows start at qw0 (diag = Lk - Lq): the n_full
// leading tiles lie wholly below Lk and the wave's first row sees them whole (so all do: no mask);
// `last` is the last tile any of its rows sees, at most ntiles - 1 (-1: none, live0 false).  na and
// mask0 are each kernel's own.  The forward calls hp_last_tile; its n_full and both of dQ's are
// written out there to this definition (as calls, in every form tried, they moved those kernels'
// code), as is fwd_pipe_kernel's, whose waves are 32 rows.
template <bool CAUSAL>
FA2_HD int hp_n_full(int Lk, int diag, int qw0) {
  int n_full = Lk / kHpTile;
  if (CAUSAL) n_full = hp_min(n_full, qw0 + diag + 1 >= 0 ? (qw0 + diag + 1) / kHpTile : 0);
  return n_full;
}
template <bool CAUSAL>
FA2_HD int hp_last_tile(int diag, int qw0, int ntiles) {
  const bool live0 = ntiles > 0 && !(CAUSAL && 0 > qw0 + 63 + diag);
  int last = -1;
  if (live0) {
    last = ntiles - 1;
    if (CAUSAL) last = hp_min(last, (qw0 + 63 + diag) / kHpTile);
  }
  return last;
}

// The persistent schedule's dimensions (PersistSched): blocks of 256 rows along a sequence, items
// per group (a causal mirrored pair of blocks, or one block), and the launchers' item count
FA2_HD int hp_blocks(int seqlen) { return (seqlen + kHpBlock - 1) / kHpBlock; }
template <bool PAIR>
FA2_HD int hp_items_per_group(int n) { return PAIR ? (n + 1) / 2 : n; }
template <bool PAIR>
FA2_HD int64_t hp_sched_items(int seqlen, int64_t groups) { return hp_items_per_group<PAIR>(hp_blocks(seqlen)) * groups; }

// a descriptor's range: a K / V slice's valid rows, at most the mrows that fit 32 bits; rows
// 0 .. nrows - 1 of Q / dO, the last one only up to its 256 bytes
FA2_HD uint32_t kv_range_bytes(int Lk, int mrows, uint32_t rowb) { return (uint32_t)hp_min(Lk, mrows) * rowb; }
FA2_HD uint32_t row_range_bytes(int nrows, uint32_t rowb) { return nrows > 0 ? (uint32_t)(nrows - 1) * rowb + 256u : 0u; }
}  // namespace fa2

#ifdef __HIP__
#include "common.h"
namespace fa2 {
// (bh, mb) of a unit of the schedule: items are head-major, and under a causal mask rep 0 of an
// item is the heavy row block nmb - 1 - i of the mirrored pair, rep 1 the light one i
struct HpWalk { int bh, mb; };
FA2_DEV HpWalk hp_walk_unit(const PersistSched& s, int nmb, int per_bh, bool pair) {
  HpWalk r;
  r.bh = s.item / per_bh;
  const int mbi = s.item - r.bh * per_bh;
  r.mb = pair && s.rep == 0 ? nmb - 1 - mbi : mbi;
  return r;
}

// words 0 and 1 of a buffer descriptor in SGPRs (word 1: 16 address bits, see kAddr48)
FA2_DEV uint32_t sgpr_lo(uint64_t a) { return __builtin_amdgcn_readfirstlane((uint32_t)a); }
FA2_DEV uint32_t sgpr_hi(uint64_t a) { return __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32)); }
FA2_DEV uint32_t sgpr_lo(const void* p) { return sgpr_lo((uint64_t)(uintptr_t)p); }
FA2_DEV uint32_t sgpr_hi(const void* p) { return sgpr_hi((uint64_t)(uintptr_t)p); }
constexpr uint64_t kAddr48 = 0xFFFFFFFFFFFFull;
}  // namespace fa2
#endif
