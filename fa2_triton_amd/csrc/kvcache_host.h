// kvcache_host.h -- host arithmetic of the KV-cache decode path shared by api.hip and the kernel
// launchers: the unit count, the split heuristic and the workspace size.  Functions of the shapes
// only -- never of the cache lengths, which stay on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa2_amd.h"

namespace fa2 {

// kvcache_kernel.h, one translation unit per (dtype, head-dim tile): the split attention kernel
template <bool BF16, int DT>
hipError_t launch_kvcache_split(const fa2_kvcache_args& a, int nsplit, hipStream_t st);
// kvcache.hip: the append of k_new / v_new and the combination of nsplit > 1 partial results
hipError_t launch_kvcache_append(const fa2_kvcache_args& a, hipStream_t st);
hipError_t launch_kvcache_combine(const fa2_kvcache_args& a, int nsplit, hipStream_t st);
// kvcache_paged_kernel.h and kvcache.hip: the same two over a paged cache (the combination is shared)
template <bool BF16, int DT>
hipError_t launch_kvcache_paged_split(const fa2_paged_kvcache_args& a, int nsplit, hipStream_t st);
hipError_t launch_kvcache_paged_append(const fa2_paged_kvcache_args& a, hipStream_t st);

// compute units of the current device, 256 (an MI355X) when there is none to ask
inline int kv_cu_count() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 256;
  return n;
}

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

}  // namespace fa2
