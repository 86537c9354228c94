// kvcache_paged_kernel.h -- KV-cache decode attention over a paged cache (fa2_fwd_kvcache_paged).
//
// The kernel of kvcache_kernel.h with paged staging: the caches are pools of blocks
// [num_blocks, P, Hkv, D] and logical key j of batch b is row j % P of block block_table[b, j / P].
// Units, the round-robin of tiles over waves, the step, the masks, the merge and the workspace
// are kvcache_kernel_body.h unchanged; what differs is the source address of a tile's rows
// (stage_tile_paged) and the lookup of the block ids one step ahead of it (kv_page_ids).
#pragma once
#include "kvcache_kernel.h"

namespace fa2 {

template <bool BF16, int DT>
__global__ void __launch_bounds__(KvCfg<DT>::NW * 64) kvcache_paged_split_kernel(const fa2_paged_kvcache_args pg, const int nsplit) {
  constexpr bool PAGED = true;
  const fa2_kvcache_args& p = pg.base;
#include "kvcache_kernel_body.h"
}

template <bool BF16, int DT>
hipError_t launch_kvcache_paged_split(const fa2_paged_kvcache_args& a, int nsplit, hipStream_t st) {
  const int64_t grid = kv_units(a.base) * nsplit;
  hipLaunchKernelGGL((kvcache_paged_split_kernel<BF16, DT>), dim3((unsigned)grid), dim3(KvCfg<DT>::NW * 64), 0, st, a, nsplit);
  return hipGetLastError();
}

}  // namespace fa2
