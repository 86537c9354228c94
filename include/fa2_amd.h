/*
 * fa2_amd.h -- C ABI of the MI355X (gfx950) FlashAttention-2 forward/backward kernels.
 *
 * This library replaces the three Triton launches of the reference
 * (remi-or/fa2_triton @ 2024-10-08):
 *   fa2_fwd  <- _fwd_kernel[grid](...)      /root/reference/src/forward/caller.py:83-116
 *   fa2_bwd  <- _compute_delta[grid](...)   /root/reference/src/backward/caller.py:95-114
 *             + _bwd_kernel[grid](...)      /root/reference/src/backward/caller.py:122-160
 *             + the host GQA dK/dV sum      /root/reference/src/backward/caller.py:162-165
 * and the host varlen pack/unpack loops (/root/reference/src/utils.py:8-31) through
 *   fa2_cu_seqlens_from_mask  (device-side cumulative lengths of a right-padded mask).
 *
 * Conventions
 *  - All tensors live in device memory and are addressed by element strides; the last
 *    (head_dim) stride must be 1 (/root/reference/src/wrapper.py:41-43).  Q/K/V/O/dO/dQ/dK/dV
 *    use the reference's [batch, seqlen, heads, head_dim] (BSHD) indexing, but any stride
 *    order works (e.g. BHSD views), so no copies are needed.
 *  - lse / delta are [batch, heads_q, lse_row_stride] fp32, lse_row_stride >= seqlen_q
 *    (the reference rounds it up to a multiple of 128, src/forward/caller.py:73-74).
 *    lse holds the base-2 log-sum-exp: LSE2 = ln(sum_j exp(s_ij)) * log2(e); rows with no
 *    visible key (causal seqlen_q > seqlen_k, padded rows) hold -inf.
 *  - Nothing is allocated inside the library; every buffer is caller-owned.
 *  - Launches are asynchronous on `stream` (a hipStream_t; NULL = default stream).
 *  - Return 0 on success or a negative FA2_E* code; fa2_last_error() then describes it
 *    (thread-local string).  The Python host layer raises RuntimeError with that text.
 */
#ifndef FA2_AMD_H
#define FA2_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FA2_ABI_VERSION 10

/* dtype codes: same numbers as the reference's encode_dtype (src/utils.py:102-109). */
enum fa2_dtype { FA2_F16 = 16, FA2_BF16 = 17, FA2_F32 = 32 };

enum fa2_status {
  FA2_OK = 0,
  FA2_E_INVALID = -1,     /* bad shape / stride / pointer */
  FA2_E_UNSUPPORTED = -2, /* valid but not implemented (e.g. head_dim > 256) */
  FA2_E_HIP = -3          /* a HIP runtime call failed */
};

/* Forward: O = softmax(scale * Q K^T + bias, masks) V  (dropout optional), plus LSE2.
 * Mirrors the argument list of _fwd_kernel (/root/reference/src/forward/kernel.py:61-96). */
typedef struct fa2_fwd_args {
  const void* q;      /* [B, Sq, Hq, D] */
  const void* k;      /* [B, Sk, Hkv, D] */
  const void* v;      /* [B, Sk, Hkv, D] */
  void* o;            /* [B, Sq, Hq, D], same dtype as q; every element is written */
  float* lse;         /* [B, Hq, lse_row_stride]; rows [0, Sq) written */
  const void* bias;   /* optional additive bias [1|B, 1|Hq, Sq, Sk] (strides below), or NULL */
  const int32_t* cu_seqlens; /* optional [B+1] cumulative valid lengths (varlen, Sq == Sk), or NULL */
  int64_t q_stride[3];    /* batch, seq, head strides (elements) */
  int64_t k_stride[3];
  int64_t v_stride[3];
  int64_t o_stride[3];
  int64_t bias_stride[3]; /* batch, head, row strides; 0 = broadcast */
  int32_t batch, heads_q, heads_kv, seqlen_q, seqlen_k, head_dim;
  int32_t lse_row_stride;
  int32_t causal;         /* bottom-right aligned causal mask */
  int32_t dtype;          /* FA2_F16 or FA2_BF16 (q, k, v, o) */
  int32_t bias_dtype;     /* FA2_F16, FA2_BF16 or FA2_F32 when bias != NULL */
  float softmax_scale;
  float dropout_p;        /* 0 <= p < 1 */
  uint64_t dropout_seed;  /* Philox4x32-10 key, identical to Triton's tl.rand */
  /* optional dropout keep mask out (ABI 6): when non-NULL and dropout_p > 0, the forward also
   * writes the keep bits it drew (keep = tl.rand > p) into this buffer of
   * fa2_dropout_mask_bytes(batch, heads_q, seqlen_q, seqlen_k) bytes (ABI 8: the tiles below plus
   * one 128-byte tile of slack the backward may read past the last one), so that the backward reads
   * them instead of regenerating Philox (fa2_bwd_args.dropout_mask).  Layout: 32 x 32 bit tiles,
   * word[((b * Hq + h) * ceil(Sq / 32) + i / 32) * ceil(Sk / 32) + j / 32][i % 32], bit j % 32 =
   * keep(b, h, i, j).  Only the tiles the (causal) mask leaves visible are written.  The buffer is
   * also the forward's input: with it the forward first draws every visible word (an all-VALU
   * Philox launch) and then reads them (the D = 128 hand-placed forward runs with dropout only
   * then); O equals the no-buffer forward's within rounding, not bitwise. */
  uint32_t* dropout_mask;
  /* sliding-window (local) attention (ABI 10).  local == 0: no window, the two fields below are
   * ignored (a zero-initialised struct means what it meant before).  local != 0: with
   * diag = Lk - Lq over the valid lengths (cu_seqlens under varlen), key j is visible to query i
   * iff j < Lk and i + diag - window_left <= j <= i + diag + window_right; a negative bound means
   * no bound on that side, and causal != 0 forces window_right = 0.  Rows with no visible key give
   * O = 0 and LSE2 = -inf.  A window that bounds nothing (both negative) or only restates the
   * causal mask (left < 0, right == 0) runs the kernels of the call without a window.  Not
   * implemented together with a bias or dropout_p > 0: FA2_E_UNSUPPORTED. */
  int32_t local, window_left, window_right;
} fa2_fwd_args;

/* Backward: dQ, dK, dV of the forward above.  dK/dV are written with heads_kv heads: the GQA
 * group sum is done in fp32 inside the kernel.  dropout_p > 0 is supported (the reference
 * raises NotImplementedError, /root/reference/src/utils.py:80-88): the kernels read the keep
 * mask the forward saved (dropout_mask) or regenerate it with Philox, so dropout_p and
 * dropout_seed must equal the forward's. */
typedef struct fa2_bwd_args {
  const void* q;
  const void* k;
  const void* v;
  const void* o;
  const void* dout;       /* dO, [B, Sq, Hq, D] */
  const float* lse;       /* as written by fa2_fwd */
  float* delta;           /* workspace [B, Hq, lse_row_stride] fp32: -rowsum(O * dO) (scratch) */
  void* dq;               /* [B, Sq, Hq, D] in dq_dtype */
  void* dk;               /* [B, Sk, Hkv, D] in dtype */
  void* dv;               /* [B, Sk, Hkv, D] in dtype */
  const void* bias;
  const int32_t* cu_seqlens;
  int64_t q_stride[3];
  int64_t k_stride[3];
  int64_t v_stride[3];
  int64_t o_stride[3];
  int64_t do_stride[3];
  int64_t dq_stride[3];
  int64_t dk_stride[3];
  int64_t dv_stride[3];
  int64_t bias_stride[3];
  int32_t batch, heads_q, heads_kv, seqlen_q, seqlen_k, head_dim;
  int32_t lse_row_stride;
  int32_t causal;
  int32_t dtype;
  int32_t bias_dtype;
  int32_t dq_dtype;       /* dtype, or FA2_F32 */
  float softmax_scale;
  float dropout_p;
  uint64_t dropout_seed;
  /* optional bias gradient (ABI 5): when non-NULL (bias must be non-NULL too), the backward
   * also writes dL/d(bias) in fp32 into this buffer, which has the BIAS's shape
   * [1|B, 1|Hq, Sq, Sk] (element strides below: batch, head, row; unit key stride): element
   * (b', h', i, j) = sum over the batches and q-heads the bias broadcasts over (a zero batch /
   * head stride in bias_stride) of dS[b, hq, i, j] = P (dP - delta), summed in a fixed order
   * (bitwise reproducible), 0 where no pair is visible.  Every element is written; no
   * initialisation needed; no workspace beyond this buffer.  (The reference returns no bias
   * gradient, /root/reference/src/wrapper.py:86.) */
  float* dbias;
  int64_t dbias_stride[3];
  /* optional dK/dV split workspace (ABI 4): when non-NULL and at least
   * fa2_bwd_dkv_workspace_bytes(args) bytes (> 0 only for GQA / MQA problems whose
   * B * Hkv * ceil(Sk / 128) key blocks are too few to fill the GPU), the q-heads of each GQA
   * group are split over several dK/dV workgroups that write fp32 partial sums here, and a
   * reduction kernel adds them in a fixed order (bitwise reproducible).  NULL: one workgroup
   * per key block sums the whole group (the reference launches per q-head and sums on the
   * host, /root/reference/src/backward/caller.py:118-121,162-165).  Contents are scratch. */
  float* dkv_workspace;
  int64_t dkv_workspace_bytes;
  /* optional (ABI 6): the keep mask a forward with the same dropout_p / dropout_seed wrote
   * (fa2_fwd_args.dropout_mask); NULL = regenerate it with Philox (dQ, dK/dV and the bias
   * gradient each draw it again).  The backward kernels may READ words the forward never wrote
   * (tiles the causal mask hides, prefetches one tile past the last live one): such a word only
   * ever gates a (row, key) pair whose probability is 0, so its contents never reach a result and
   * the buffer needs no initialisation. */
  const uint32_t* dropout_mask;
  /* sliding window (ABI 10), as in fa2_fwd_args and equal to the forward's.  Rows with no visible
   * key get dQ = 0 and add nothing to dK / dV.  Not implemented together with a bias, a dbias
   * buffer or dropout_p > 0: FA2_E_UNSUPPORTED.  The windowed dK/dV sums each GQA group in one
   * workgroup: a dkv_workspace is accepted and left unused. */
  int32_t local, window_left, window_right;
} fa2_bwd_args;

int fa2_fwd(const fa2_fwd_args* args, void* stream);
int fa2_bwd(const fa2_bwd_args* args, void* stream);

/* The backward's launches selected by a bit mask, for per-kernel timing and profiling.
 * Launch order: bit 0 delta = rowsum(O * dO) (standalone kernel), bit 2 dQ (which also computes
 * delta for its rows and writes it to args->delta), bit 1 dK/dV (reads delta), bit 3 the bias
 * gradient (reads delta; needs args->dbias).  A mask must produce delta before dK/dV or the
 * bias gradient read it (bit 0 or bit 2, now or in an earlier call);
 * fa2_bwd == fa2_bwd_stages(args, 6, stream), 14 when args->dbias is set. */
int fa2_bwd_stages(const fa2_bwd_args* args, int stages, void* stream);
/* Bytes of dK/dV split workspace for these sizes (batch, heads_q, heads_kv, seqlen_k, head_dim):
 * 2 * nsplit * B * Hkv * Sk * D * 4, with nsplit the smallest divisor of the group size Hq / Hkv
 * that gives at least 512 dK/dV workgroups (two per CU), or 0 when no split applies (Hq == Hkv,
 * or the grid is already that large). */
int64_t fa2_bwd_dkv_workspace_bytes(const fa2_bwd_args* args);
/* Bytes of a dropout keep mask (ABI 6): batch * heads_q * ceil(seqlen_q / 32) * ceil(seqlen_k / 32) * 128. */
int64_t fa2_dropout_mask_bytes(int32_t batch, int32_t heads_q, int32_t seqlen_q, int32_t seqlen_k);

/* cu_seqlens[0] = 0, cu_seqlens[b+1] = cu_seqlens[b] + sum_s mask[b, s]  (mask: uint8/bool,
 * row stride mask_row_stride bytes).  Replaces attention_mask.sum(1).cumsum(0) and the
 * .item() syncs of the reference callers (src/forward/caller.py:48-50, src/utils.py:8-17). */
int fa2_cu_seqlens_from_mask(const uint8_t* mask, int64_t mask_row_stride, int32_t batch,
                             int32_t seqlen, int32_t* cu_seqlens, void* stream);

/* Kernel-path policy of ONE call (ABI 9; replaces ABI 7's process-wide fa2_set_path_policy: the
 * library keeps no mutable state between calls), for tests and A/B timing.  Bits of `disable`
 * turn a specialised path off so that the general kernels of the same launch run instead (same
 * math; the tests compare the two): FA2_PATH_FWD_HP the hand-placed D = 128 forward,
 * FA2_PATH_DQ_HP / FA2_PATH_DKDV_HP the hand-placed D = 128 dQ / dK-dV.  grid_cap > 0 caps the
 * grid of the persistent (one workgroup per CU) kernels, so that small problems run several work
 * units per workgroup.  A NULL policy, or {0, 0}, is the default: every path on, one workgroup
 * per CU (fa2_fwd / fa2_bwd_stages).  The environment is never read. */
enum fa2_path { FA2_PATH_FWD_HP = 1, FA2_PATH_DQ_HP = 2, FA2_PATH_DKDV_HP = 4 };
typedef struct fa2_policy {
  uint32_t disable;  /* fa2_path bits */
  int32_t grid_cap;  /* 0: no cap */
} fa2_policy;
int fa2_fwd_ex(const fa2_fwd_args* args, const fa2_policy* policy, void* stream);
int fa2_bwd_stages_ex(const fa2_bwd_args* args, int stages, const fa2_policy* policy, void* stream);

/* KV-cache decode attention (ABI 10, minor 1): O = softmax(scale * Q K^T, masks) V for a few query
 * tokens against a pre-allocated key / value cache whose sequences have their own filled lengths,
 * read on the device (no host synchronisation; the call can be captured in a graph).  Forward
 * only.  Paged caches (block tables): fa2_fwd_kvcache_paged below.  Not implemented: rotary
 * embedding, bias, dropout, backward.
 *
 *  - L_b, the valid keys of batch b: cache_seqlens[b] clamped to [0, capacity] (NULL: capacity);
 *    with k_new / v_new, min(that + seqlen_new, capacity) after the new rows n = 0 .. seqlen_new - 1
 *    were written to the cache rows cache_seqlens[b] + n (rows that would land at or past capacity
 *    are not written; nothing outside [0, capacity) of a batch row is ever written).  cache_seqlens
 *    itself is not modified.
 *  - query i sees key j iff j < L_b and, with diag = L_b - seqlen_q (bottom-right aligned),
 *    i + diag - window_left <= j <= i + diag + window_right; a negative bound means no bound on
 *    that side and causal != 0 forces window_right = 0.  Rows with no visible key give O = 0 and
 *    LSE2 = -inf.
 *  - work is cut into (batch, kv head, 32-row tile of the group's heads_q / heads_kv x seqlen_q
 *    rows, key split) units; with more than one split the units write fp32 partial results into
 *    `workspace` and a second kernel combines them in split order (bitwise reproducible).
 *  - every row of q, k_cache, v_cache, o, k_new, v_new must be 16-byte aligned (head_dim % 8 == 0,
 *    aligned pointers, strides % 8 == 0), else FA2_E_UNSUPPORTED. */
typedef struct fa2_kvcache_args {
  const void* q;          /* [B, Sq, Hq, D] */
  void* k_cache;          /* [B, capacity, Hkv, D]; written only when k_new is given */
  void* v_cache;          /* [B, capacity, Hkv, D] */
  void* o;                /* [B, Sq, Hq, D], same dtype as q; every element is written */
  float* lse;             /* optional [B, Hq, Sq] contiguous fp32 LSE2, or NULL */
  const void* k_new;      /* optional [B, seqlen_new, Hkv, D] rows to append first, or NULL */
  const void* v_new;      /* given exactly when k_new is */
  const int32_t* cache_seqlens; /* optional [B] device int32, or NULL (every sequence fills the cache) */
  void* workspace;        /* fa2_kvcache_workspace_bytes(args) bytes, 16-byte aligned; scratch */
  int64_t workspace_bytes;
  int64_t q_stride[3];    /* batch, seq, head strides (elements) */
  int64_t k_cache_stride[3];
  int64_t v_cache_stride[3];
  int64_t o_stride[3];
  int64_t k_new_stride[3];
  int64_t v_new_stride[3];
  int32_t batch, heads_q, heads_kv, seqlen_q, capacity, head_dim;
  int32_t seqlen_new;     /* 0 without k_new / v_new */
  int32_t causal;
  int32_t window_left, window_right; /* negative: no bound */
  int32_t dtype;          /* FA2_F16 or FA2_BF16 (q, caches, new rows, o) */
  int32_t num_splits;     /* 0: chosen by fa2_kvcache_num_splits; 1 .. 128: forced */
  float softmax_scale;
} fa2_kvcache_args;

int fa2_fwd_kvcache(const fa2_kvcache_args* args, void* stream);
/* The key splits the call will use: num_splits when forced, else the smallest count that gives
 * about two workgroups per compute unit over the B * Hkv * ceil(Hq / Hkv * Sq / 32) units, never
 * leaving a split fewer than FA2_KVCACHE_MIN_SPLIT_TILES 64-key tiles of the key span (capacity,
 * or the window's span when window_left >= 0), at most 128.  A function of the shapes only (host
 * arithmetic; 1 for arguments fa2_fwd_kvcache would reject). */
#define FA2_KVCACHE_MIN_SPLIT_TILES 4
#define FA2_KVCACHE_MAX_SPLITS 128
int fa2_kvcache_num_splits(const fa2_kvcache_args* args);
/* Bytes of workspace: 0 with one split, else nsplit * B * Hq * Sq * (D + 1) * 4 (the fp32 partial
 * outputs [nsplit, B, Hq, Sq, D] followed by the partial LSE2 [nsplit, B, Hq, Sq]). */
int64_t fa2_kvcache_workspace_bytes(const fa2_kvcache_args* args);

/* The same attention over a paged cache (added within ABI 10 minor 1: detect it by the presence of
 * the symbol fa2_fwd_kvcache_paged).  k_cache / v_cache of `base` are pools of blocks
 * [num_blocks, page_block_size, Hkv, D] and logical key j of batch b is row j % P of block
 * block_table[b, j / P] (P = page_block_size).  In `base`:
 *  - k_cache_stride / v_cache_stride are the (block, row-in-block, head) strides, in elements;
 *  - capacity = max_blocks * P, the keys a row of the table can address; max_blocks is not stated
 *    separately, it is capacity / P (capacity % P != 0 is rejected).
 * Everything else is fa2_fwd_kvcache's semantics with that capacity: L_b clamped to [0, capacity],
 * the bottom-right aligned masks, the append (row n of batch b goes to logical position L_b + n
 * through the table; positions >= capacity are dropped; the blocks must already be in the table),
 * the split count and the workspace (the same functions of the same shapes).
 *  - table entries of pages at or past ceil(L_b / P) (L_b after the append) are never read and may
 *    hold anything; an entry that is read is clamped into [0, num_blocks - 1] on the device, so a
 *    wrong table reads or writes a wrong block of the pool, never memory outside it.
 *  - several table rows may name the same block (shared prefixes) as long as the call does not
 *    append into it: appending through tables that alias is the caller's error.
 *  - neither block_table nor cache_seqlens is modified. */
typedef struct fa2_paged_kvcache_args {
  fa2_kvcache_args base;
  const int32_t* block_table;  /* [B, max_blocks] device int32, unit stride in the last dimension */
  int64_t block_table_stride;  /* elements between batch rows, >= max_blocks */
  int32_t page_block_size;     /* P: a power of two >= 16 */
  int32_t num_blocks;          /* blocks in each pool, >= 1 */
} fa2_paged_kvcache_args;

int fa2_fwd_kvcache_paged(const fa2_paged_kvcache_args* args, void* stream);
/* fa2_kvcache_num_splits / fa2_kvcache_workspace_bytes of args->base: a paged call and a
 * contiguous call of the same shapes use the same split count and workspace. */
int fa2_paged_kvcache_num_splits(const fa2_paged_kvcache_args* args);
int64_t fa2_paged_kvcache_workspace_bytes(const fa2_paged_kvcache_args* args);

/* The same attention over fp8 caches (added within ABI 10 minor 1: detect it by the presence of the
 * symbol fa2_fwd_kvcache_fp8).  k_cache / v_cache of `paged.base` hold OCP e4m3fn bytes; q, o and
 * the new rows keep `paged.base.dtype` (fp16 or bf16).  A NULL paged.block_table means the
 * contiguous layout [B, capacity, Hkv, D] (the paging fields are then ignored), otherwise the
 * caches are pools as in fa2_fwd_kvcache_paged.  Cache strides are in elements, here bytes.
 *  - a cache element's value is its exact e4m3 value times the descale of its (batch, kv head):
 *    k_descale / v_descale point to fp32 device values read on the device, element
 *    b * stride[0] + h * stride[1] (a stride of 0 broadcasts); NULL means 1.
 *  - the score multiplier is (softmax_scale * k_descale) * log2(e) in fp32; v_descale multiplies O
 *    in fp32 before its one rounding to the output dtype; LSE2 is that of the scaled scores.
 *  - k_new / v_new (in `dtype`) are quantised on the way in: the byte written is
 *    e4m3_rne(clamp(float(x) / descale, -448, 448)), the division correctly rounded, NaN kept.
 *  - head_dim is a multiple of 16 up to 128 and every cache row is 16-byte aligned (pointers and
 *    strides multiples of 16), else FA2_E_UNSUPPORTED.
 * Masks, lengths, the append positions, the split count and the workspace are fa2_fwd_kvcache's
 * (fa2_fwd_kvcache_paged's with a block table). */
typedef struct fa2_fp8_kvcache_args {
  fa2_paged_kvcache_args paged;
  const float* k_descale;       /* device fp32, or NULL (1) */
  const float* v_descale;
  int64_t k_descale_stride[2];  /* (batch, kv head) strides in elements; 0 broadcasts */
  int64_t v_descale_stride[2];
} fa2_fp8_kvcache_args;

int fa2_fwd_kvcache_fp8(const fa2_fp8_kvcache_args* args, void* stream);
/* fa2_kvcache_num_splits / fa2_kvcache_workspace_bytes of args->paged.base. */
int fa2_fp8_kvcache_num_splits(const fa2_fp8_kvcache_args* args);
int64_t fa2_fp8_kvcache_workspace_bytes(const fa2_fp8_kvcache_args* args);

/* Shared-prefix (cascade) decode attention (added within ABI 10 minor 1: detect it by the presence of
 * the symbol fa2_fwd_kvcache_prefix).  Every query row of `seq` (the call fa2_fwd_kvcache or, with a
 * block table, fa2_fwd_kvcache_paged would take) attends to the first Lp keys of one prefix cache
 * that all batch rows share, and to the keys of its own sequence under seq's rule (lengths, append,
 * causal, window_right); one softmax runs over the union.  Lp is prefix.base.cache_seqlens[0] read
 * on the device and clamped to [0, prefix.base.capacity] (NULL: the capacity).  A row that sees no
 * key at all (Lp = 0 and no visible key of its own) gives O = 0 and LSE2 = -inf.
 *  - the prefix is attended once for the whole batch: the library runs the split kernel of the
 *    prefix's layout on batch 1 with seqlen_q = B * Sq, no mask and no append, reading q row
 *    b * Sq + i at q + (b * Sq + i) * row stride.  That needs q_stride[0] == Sq * q_stride[1]; with
 *    Sq == 1 the batch stride is the row stride and with B == 1 the sequence stride is; anything
 *    else is FA2_E_UNSUPPORTED.
 *  - both passes always write fp32 partial results into `seq.base.workspace`, never a rounded O, so
 *    each runs with at least two key splits: max(2, the automatic count of the pass), or a forced
 *    2 .. 128 in seq.base.num_splits / prefix.base.num_splits.  A forced 1 is FA2_E_INVALID.  One
 *    merge kernel sums the prefix splits, then the sequence splits, weighted by their LSE2, and
 *    rounds O once (bitwise reproducible).
 *  - workspace: the prefix region [ns_p, 1, Hq, B * Sq, D] fp32 + [ns_p, 1, Hq, B * Sq], then the
 *    sequence region [ns_s, B, Hq, Sq, D] + [ns_s, B, Hq, Sq], each rounded up to 16 bytes.
 *  - window_left >= 0 is FA2_E_UNSUPPORTED (the band may or may not reach into the prefix); there is
 *    no fp8 form.  The layouts of the two sides are independent: a NULL block_table on a side means
 *    its cache is contiguous ([B, capacity, Hkv, D]; the prefix [1, capacity, Hkv, D]), otherwise
 *    pools as in fa2_fwd_kvcache_paged (the prefix table is one row), which may be the same pools. */
typedef struct fa2_prefix_kvcache_args {
  fa2_paged_kvcache_args seq;     /* the per-sequence call; q, o, lse, k_new / v_new, the masks, the scale and the workspace live here */
  fa2_paged_kvcache_args prefix;  /* read: k_cache, v_cache, their strides, capacity, cache_seqlens (one int32 or NULL), the paging
                                     fields and num_splits.  Every other field must be zero */
} fa2_prefix_kvcache_args;

int fa2_fwd_kvcache_prefix(const fa2_prefix_kvcache_args* args, void* stream);
/* The key splits of the two passes, into *prefix_splits and *seq_splits (either may be NULL): both
 * are >= 2 and functions of the shapes only.  Returns FA2_OK, or the status fa2_fwd_kvcache_prefix
 * would reject the sizes with (both counts are then 0). */
int fa2_prefix_kvcache_num_splits(const fa2_prefix_kvcache_args* args, int* prefix_splits, int* seq_splits);
/* Bytes of workspace: round16(ns_p * R) + round16(ns_s * R) with R = B * Hq * Sq * (D + 1) * 4 and
 * round16 rounding up to a multiple of 16; 0 for sizes the call would reject. */
int64_t fa2_prefix_kvcache_workspace_bytes(const fa2_prefix_kvcache_args* args);

const char* fa2_last_error(void);
int fa2_version(void);
/* Additive revisions of one ABI version (FA2_ABI_VERSION stays what callers compiled against):
 * minor 1 added the fa2_kvcache_* entry points and this function. */
#define FA2_ABI_MINOR 1
int fa2_abi_minor(void);

#ifdef __cplusplus
}
#endif
#endif /* FA2_AMD_H */
