// kvcache_append_pos.h -- the position rule of the three append kernels (kvcache.hip,
// kvcache_fp8.hip), included as text at the head of each.  In scope at the point of inclusion: the
// constants CW (elements per thread: 8 or 16) and PAGED, `p` (fa2_kvcache_args) and `pg` with the
// paging fields.  It leaves b, n, h, c, slab and row, or returns from the enclosing function.
// Thread idx owns chunk c of head h of new row n of batch b, which goes to logical row
// pos = L_b + n, L_b = cache_seqlens[b] clamped to [0, capacity] on the device.  A row at or past
// the capacity is dropped, so whatever cache_seqlens holds, only rows [0, capacity) of a batch are
// written.  Logical row pos is row `row` of slab `slab` (the index of the caches' first stride):
// row pos of the batch's own slab, or PAGED row pos % P of block block_table[b, pos / P], the entry
// clamped into [0, num_blocks - 1].  capacity = max_blocks * P, so only table entries
// [0, max_blocks) are read and only blocks of the pool are written, whatever the table holds.
// Included text rather than a function: the fp8 kernel's code came out different through a
// __device__ function or a callback ("One body").
  const int chunks = p.head_dim >> (CW == 16 ? 4 : 3);
  const int64_t total = (int64_t)p.batch * p.seqlen_new * p.heads_kv * chunks;
  int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % chunks);
  idx /= chunks;
  const int h = (int)(idx % p.heads_kv);
  idx /= p.heads_kv;
  const int n = (int)(idx % p.seqlen_new), b = (int)(idx / p.seqlen_new);
  int L = p.cache_seqlens ? p.cache_seqlens[b] : p.capacity;
  L = min(max(L, 0), p.capacity);
  const int64_t pos = (int64_t)L + n;
  if (pos >= p.capacity) return;
  int64_t slab = b, row = pos;
  if constexpr (PAGED) {
    const int log_p = __builtin_ctz(pg.page_block_size);
    slab = min(max(pg.block_table[(int64_t)b * pg.block_table_stride + (pos >> log_p)], 0), pg.num_blocks - 1);
    row = pos & (pg.page_block_size - 1);
  }
