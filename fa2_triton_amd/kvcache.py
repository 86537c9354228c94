"""KV-cache decode attention: `flash_attn_with_kvcache` (C ABI `fa2_fwd_kvcache`, ABI 10 minor 1)
over one contiguous cache slab per sequence, and `flash_attn_with_paged_kvcache`
(`fa2_fwd_kvcache_paged`) over a pool of fixed-size blocks addressed through a block table, and
`flash_attn_with_fp8_kvcache` (`fa2_fwd_kvcache_fp8`) over caches of either layout that hold
`float8_e4m3fn` bytes with a descale per (batch, kv head), and `flash_attn_with_prefix_kvcache`
(`fa2_fwd_kvcache_prefix`) over 16-bit caches of either layout behind a prefix that all sequences
share and that is attended once for the whole batch.

One query token, or a few, per sequence against a pre-allocated key / value cache whose sequences
have their own filled lengths.  The lengths stay on the device: nothing here reads a tensor's
contents, synchronises with the host or sizes an allocation by a length, so a decode step can be
captured in a HIP graph and replayed while `cache_seqlens` changes in place.
"""
import ctypes
import math
from typing import Optional, Tuple, Union

import torch
from torch import Tensor

from . import _lib
from .utils import bshd_strides, check_window_size, encode_dtype, launch_on

MAX_SPLITS = _lib.KVCACHE_MAX_SPLITS


def _check_plain_args(k, v, window_size, num_splits, cache_seqlens) -> Tuple[int, int]:
    """What can be judged without looking at a tensor."""
    left, right = check_window_size(window_size)
    if not isinstance(num_splits, int) or isinstance(num_splits, bool) or not 0 <= num_splits <= MAX_SPLITS:
        raise ValueError(f"num_splits must be an int in 0 .. {MAX_SPLITS}, got {num_splits!r}")
    if (k is None) != (v is None):
        raise ValueError("k and v (the rows to append) must be given together")
    if isinstance(cache_seqlens, bool) or not (cache_seqlens is None or isinstance(cache_seqlens, (int, Tensor))):
        raise TypeError(f"cache_seqlens must be None, an int or an int32 tensor, got {type(cache_seqlens).__name__}")
    return min(max(left, -1), 2**30), min(max(right, -1), 2**30)


def _check_tensors(q, k_cache, v_cache, k, v, cache_shape: str, cache_dtype=None, max_head_dim: int = 256):
    """The checks both cache layouts share: q, the two caches and the optional new rows.  Returns
    (batch, seqlen_q, heads_q, head_dim, heads_kv, new) with `new` the (name, tensor) pairs of k, v.
    cache_dtype: the dtype the caches must have when it is not q's (the fp8 call)."""
    for name, t in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache)):
        if not isinstance(t, Tensor) or t.dim() != 4:
            raise ValueError(f"{name} must be a 4-d tensor [{'batch, seqlen' if name == 'q' else cache_shape}, heads, head_dim]")
    batch, seqlen_q, heads_q, head_dim = q.shape
    lead, rows, heads_kv, _ = k_cache.shape
    if k_cache.shape[3] != head_dim or (cache_shape == "batch, cap" and lead != batch) or v_cache.shape != k_cache.shape:
        raise ValueError(f"{k_cache.shape = } and {v_cache.shape = } must both be ({cache_shape}, heads_kv, "
                         f"head_dim={head_dim}) with batch={batch}")
    if heads_kv < 1 or heads_q % heads_kv != 0:
        raise ValueError(f"{heads_q = } is not divisible by {heads_kv = }")
    if seqlen_q < 1 or rows < 1 or lead < 1:
        raise ValueError(f"{seqlen_q = } and the cache sizes {lead} x {rows} must be at least 1")
    new = () if k is None else (("k", k), ("v", v))
    for name, t in new:
        if not isinstance(t, Tensor) or t.dim() != 4 or t.shape != (batch, t.shape[1], heads_kv, head_dim) or t.shape[1] < 1:
            raise ValueError(f"{name} must be [batch={batch}, seqlen_new >= 1, heads_kv={heads_kv}, head_dim={head_dim}]")
    if new and k.shape != v.shape:
        raise ValueError(f"{k.shape = } <> {v.shape = }")
    tensors = (("q", q), ("k_cache", k_cache), ("v_cache", v_cache)) + new
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise TypeError(f"only fp16 and bf16 are supported, got {q.dtype}")
    for name, t in tensors:
        if cache_dtype is not None and name.endswith("_cache"):
            if t.dtype != cache_dtype:
                raise TypeError(f"{name} is {t.dtype}: the caches must be {cache_dtype}")
        elif t.dtype != q.dtype:
            raise TypeError(f"{name} is {t.dtype}, q is {q.dtype}: all tensors must have the same dtype")
    for name, t in tensors:
        if not t.is_cuda or t.device != q.device:
            raise ValueError(f"{name} must be on q's GPU device, got {t.device}")
        if t.stride(-1) != 1:
            raise ValueError(f"{name} must have a unit head-dim stride")
    if head_dim > max_head_dim:
        raise NotImplementedError(f"{head_dim = } > {max_head_dim} is not supported")
    return batch, seqlen_q, heads_q, head_dim, heads_kv, new


def _seqlens_on_device(cache_seqlens, batch: int, cap: int, device) -> Optional[Tensor]:
    if isinstance(cache_seqlens, Tensor):
        if cache_seqlens.dtype != torch.int32 or cache_seqlens.shape != (batch,) or cache_seqlens.device != device:
            raise ValueError(f"cache_seqlens must be an int32 tensor of shape ({batch},) on {device}, got "
                             f"{cache_seqlens.dtype} {tuple(cache_seqlens.shape)} on {cache_seqlens.device}")
        return cache_seqlens.contiguous()
    if cache_seqlens is None:
        return None
    return torch.full((batch,), min(max(cache_seqlens, 0), cap), dtype=torch.int32, device=device)


def _check_block_table(block_table, k_cache, q) -> int:
    """The block table of a paged call against its pool and q; returns the capacity max_blocks * P."""
    batch, page = q.shape[0], k_cache.shape[1]
    if page < 16 or page & (page - 1):
        raise ValueError(f"page_block_size (k_cache.shape[1] = {page}) must be a power of two >= 16")
    if block_table.dtype != torch.int32:
        raise TypeError(f"block_table must be int32, got {block_table.dtype}")
    if block_table.shape[0] != batch or block_table.shape[1] < 1:
        raise ValueError(f"block_table must be [batch={batch}, max_blocks >= 1], got {tuple(block_table.shape)}")
    if block_table.device != q.device:
        raise ValueError(f"block_table must be on q's GPU device, got {block_table.device}")
    if block_table.stride(1) != 1 and block_table.shape[1] > 1:
        raise ValueError("block_table must have a unit stride in its last dimension")
    cap = block_table.shape[1] * page
    if cap > 2**30:
        raise NotImplementedError(f"max_blocks * page_block_size = {cap} > 2^30 is not supported")
    return cap


def _fill_paging(paged, block_table, k_cache) -> None:
    """The paging fields of a fa2_paged_kvcache_args."""
    batch, max_blocks = block_table.shape
    paged.block_table = block_table.data_ptr()
    paged.block_table_stride = block_table.stride(0) if batch > 1 else max(block_table.stride(0), max_blocks)
    paged.page_block_size, paged.num_blocks = k_cache.shape[1], k_cache.shape[0]


def _run(args, base, workspace_bytes, entry, q, k_cache, v_cache, new, seqlens, cap, softmax_scale, causal, left, right,
         num_splits, return_lse):
    """Fill `base` (the fa2_kvcache_args of `args`: `args` itself, or its first member), allocate the
    outputs and the workspace, and launch `entry(args, stream)` on q's stream."""
    batch, seqlen_q, heads_q, head_dim = q.shape
    with torch.no_grad():
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        lse = torch.empty((batch, heads_q, seqlen_q), dtype=torch.float32, device=q.device) if return_lse else None
        base.q, base.k_cache, base.v_cache, base.o = q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr()
        base.lse = lse.data_ptr() if return_lse else None
        base.q_stride[:] = bshd_strides(q)
        base.k_cache_stride[:] = bshd_strides(k_cache)
        base.v_cache_stride[:] = bshd_strides(v_cache)
        base.o_stride[:] = bshd_strides(out)
        if new:
            (_, k), (_, v) = new
            base.k_new, base.v_new = k.data_ptr(), v.data_ptr()
            base.k_new_stride[:] = bshd_strides(k)
            base.v_new_stride[:] = bshd_strides(v)
            base.seqlen_new = k.shape[1]
        base.cache_seqlens = seqlens.data_ptr() if seqlens is not None else None
        base.batch, base.heads_q, base.heads_kv = batch, heads_q, k_cache.shape[2]
        base.seqlen_q, base.capacity, base.head_dim = seqlen_q, cap, head_dim
        base.causal = int(bool(causal))
        base.window_left, base.window_right = left, right
        base.dtype = encode_dtype(q)
        base.num_splits = num_splits
        base.softmax_scale = 1.0 / math.sqrt(head_dim) if softmax_scale is None else float(softmax_scale)
        need = workspace_bytes(ctypes.byref(args))
        workspace = None
        if need > 0:  # a function of the shapes only
            workspace = torch.empty(need, dtype=torch.uint8, device=q.device)
            base.workspace, base.workspace_bytes = workspace.data_ptr(), need
        _lib.check(launch_on(q, lambda st: entry(ctypes.byref(args), st)))
    return (out, lse) if return_lse else out


def flash_attn_with_kvcache(
    q: Tensor,
    k_cache: Tensor,
    v_cache: Tensor,
    k: Optional[Tensor] = None,
    v: Optional[Tensor] = None,
    cache_seqlens: Union[None, int, Tensor] = None,
    softmax_scale: Optional[float] = None,
    causal: bool = False,
    window_size: Tuple[int, int] = (-1, -1),
    num_splits: int = 0,
    return_lse: bool = False,
):
    """Attention of `q` [B, Sq, Hq, D] over the first L_b keys of `k_cache` / `v_cache`
    [B, cap, Hkv, D] (fp16 or bf16, Hq % Hkv == 0, any strides with a unit head-dim stride).

    Inference only: no autograd graph is built and the result never requires grad, whatever the
    inputs require.  For paged caches (a pool of blocks and a block table) see
    `flash_attn_with_paged_kvcache`, for fp8 caches `flash_attn_with_fp8_kvcache`.  Not implemented:
    rotary embedding, bias, dropout, backward.

    cache_seqlens: None (every sequence is `cap` long), a Python int, or an int32 device tensor [B]
        that is read on the device; each value is clamped to [0, cap].  It is not modified.
    k, v: optional new rows [B, Sn, Hkv, D], both or neither.  They are first written into the caches
        at positions L_b .. L_b + Sn - 1 (rows at or past `cap` are dropped) and attention then runs
        over min(L_b + Sn, cap) keys.
    causal, window_size=(left, right): bottom-right aligned on the valid length.  With
        diag = L_b - Sq, query i sees key j iff j < L_b and i + diag - left <= j <= i + diag + right;
        a negative bound is no bound and causal forces right = 0.  Rows that see no key give 0.
    num_splits: 0 lets the library choose how many ways the keys are split over workgroups (from
        the shapes alone); 1 .. 128 forces the count.
    return_lse: also return the base-2 log-sum-exp [B, Hq, Sq] in fp32 (-inf for rows that see no key).

    Returns `out` [B, Sq, Hq, D] in q's dtype, or `(out, lse)`.
    """
    left, right = _check_plain_args(k, v, window_size, num_splits, cache_seqlens)
    batch, _, _, _, _, new = _check_tensors(q, k_cache, v_cache, k, v, "batch, cap")
    cap = k_cache.shape[1]
    seqlens = _seqlens_on_device(cache_seqlens, batch, cap, q.device)
    lib = _lib.load()
    args = _lib.KvCacheArgs()
    return _run(args, args, lib.fa2_kvcache_workspace_bytes, lib.fa2_fwd_kvcache, q, k_cache, v_cache, new, seqlens, cap,
                softmax_scale, causal, left, right, num_splits, return_lse)


def flash_attn_with_paged_kvcache(
    q: Tensor,
    k_cache: Tensor,
    v_cache: Tensor,
    block_table: Tensor,
    cache_seqlens: Union[int, Tensor],
    k: Optional[Tensor] = None,
    v: Optional[Tensor] = None,
    softmax_scale: Optional[float] = None,
    causal: bool = False,
    window_size: Tuple[int, int] = (-1, -1),
    num_splits: int = 0,
    return_lse: bool = False,
):
    """`flash_attn_with_kvcache` over a paged cache: `k_cache` / `v_cache` are pools
    [num_blocks, page_block_size, Hkv, D] (any strides with a unit head-dim stride, so a pool stored
    [N, Hkv, P, D] and viewed [N, P, Hkv, D] needs no copy) and logical key j of batch b is row
    j % P of block `block_table[b, j // P]`.  P is a power of two >= 16.

    Inference only, as the contiguous function.  fp8 pools: `flash_attn_with_fp8_kvcache`.  Not
    implemented: rotary embedding, a batch-index indirection, page sizes that are not powers of two,
    bias, dropout, backward.

    block_table: int32 device tensor [B, max_blocks] with a unit stride in its last dimension (a
        column slice of a wider table is fine).  The capacity of a sequence is max_blocks * P.
        Entries of pages at or past ceil(L_b / P) (after the append) are never read and may hold
        anything; an entry that is read is clamped into [0, num_blocks - 1] on the device, so a wrong
        table reads or writes a wrong block of the pool, never memory outside it.  Rows may share
        blocks (a common prefix) as long as the call does not append into a shared block: writing
        through tables that alias is the caller's error.  It is not modified.
    cache_seqlens: required: an int32 device tensor [B] read on the device, or a Python int; each
        value is clamped to [0, max_blocks * P].  It is not modified.
    k, v: optional new rows [B, Sn, Hkv, D]; row n of batch b is written to logical position L_b + n
        through the table (positions at or past the capacity are dropped).  The blocks must already
        be in the table: nothing is allocated here.
    softmax_scale, causal, window_size, num_splits, return_lse: as `flash_attn_with_kvcache`; the
        split count is the same function of the same shapes, with cap = max_blocks * P.

    Returns `out` [B, Sq, Hq, D] in q's dtype, or `(out, lse)`; the same bits as the contiguous
    function on the gathered cache.
    """
    if cache_seqlens is None:
        raise TypeError("cache_seqlens is required with a paged cache: an int or an int32 tensor")
    left, right = _check_plain_args(k, v, window_size, num_splits, cache_seqlens)
    if not isinstance(block_table, Tensor) or block_table.dim() != 2:
        raise ValueError("block_table must be a 2-d int32 tensor [batch, max_blocks]")
    batch, _, _, _, _, new = _check_tensors(q, k_cache, v_cache, k, v, "num_blocks, page_block_size")
    cap = _check_block_table(block_table, k_cache, q)
    seqlens = _seqlens_on_device(cache_seqlens, batch, cap, q.device)
    lib = _lib.load()
    args = _lib.PagedKvCacheArgs()
    _fill_paging(args, block_table, k_cache)
    return _run(args, args.base, lib.fa2_paged_kvcache_workspace_bytes, lib.fa2_fwd_kvcache_paged, q, k_cache, v_cache,
                new, seqlens, cap, softmax_scale, causal, left, right, num_splits, return_lse)


def _fill_cache_side(side, k_cache, v_cache, block_table, seqlens, cap, num_splits) -> None:
    """What both sides of a fa2_prefix_kvcache_args state: the caches, their strides, the capacity,
    the lengths, the paging fields and the split count."""
    base = side.base
    base.k_cache, base.v_cache = k_cache.data_ptr(), v_cache.data_ptr()
    base.k_cache_stride[:] = bshd_strides(k_cache)
    base.v_cache_stride[:] = bshd_strides(v_cache)
    base.cache_seqlens = seqlens.data_ptr() if seqlens is not None else None
    base.capacity, base.num_splits = cap, num_splits
    if block_table is not None:
        _fill_paging(side, block_table, k_cache)


def flash_attn_with_prefix_kvcache(
    q: Tensor,
    prefix_k: Tensor,
    prefix_v: Tensor,
    k_cache: Tensor,
    v_cache: Tensor,
    prefix_seqlen: Union[None, int, Tensor] = None,
    cache_seqlens: Union[None, int, Tensor] = None,
    prefix_block_table: Optional[Tensor] = None,
    block_table: Optional[Tensor] = None,
    k: Optional[Tensor] = None,
    v: Optional[Tensor] = None,
    softmax_scale: Optional[float] = None,
    causal: bool = False,
    window_size: Tuple[int, int] = (-1, -1),
    num_splits: int = 0,
    prefix_num_splits: int = 0,
    return_lse: bool = False,
):
    """Shared-prefix (cascade) decode attention: every query of `q` [B, Sq, Hq, D] attends to the
    first Lp keys of one prefix (`prefix_k` / `prefix_v`) that all batch rows share, and to the keys
    of its own sequence in `k_cache` / `v_cache` exactly as `flash_attn_with_kvcache` (with
    `block_table`: `flash_attn_with_paged_kvcache`) would show them; one softmax runs over the union.
    With every L_b >= Sq that is bottom-right aligned causal attention over the concatenation
    [prefix[:Lp]; cache_b[:L_b]].

    The prefix is attended once for the whole batch, as B * Sq query positions of one batch row (full
    32-row tiles in place of B mostly empty ones, and the prefix keys staged once per kv head rather
    than once per batch row); the two partial results are merged by their log-sum-exp in fp32 and
    rounded once.  When it pays (bf16, D = 128, Hq = 32, Hkv = 8, Sq = 1, one
    MI355X, against `flash_attn_with_paged_kvcache` over block tables that alias the prefix blocks):
    0.58 x the time at B = 64 with a prefix of 75 % of the keys, 0.78 x at B = 8 with 87.5 %, even
    at B = 64 with 12.5 %, and 1.32 x (slower: one more launch and a workspace round trip) at B = 1.
    Use it for batches of 8 and more whose shared prefix is the larger part of the keys, never for
    B = 1.

    Inference only: no autograd graph is built and the result never requires grad.  Not implemented:
    a left window bound, fp8 caches, more than one prefix level, rotary embedding, bias, dropout,
    backward.

    prefix_k, prefix_v: [1, cap_p, Hkv, D], or with `prefix_block_table` (int32 [1, max_blocks_p])
        pools [num_blocks, P, Hkv, D], which may be the very pools of `k_cache` / `v_cache`.
    prefix_seqlen: Lp: None (cap_p), a Python int, or an int32 device tensor [1] that is read on the
        device; clamped to [0, cap_p].  It is not modified.
    k_cache, v_cache, cache_seqlens, block_table: the per-sequence caches, [B, cap, Hkv, D] or, with
        `block_table` (then `cache_seqlens` is required), pools; the rules of the two functions named
        above.  The two sides choose their layouts independently.
    k, v: optional new rows [B, Sn, Hkv, D], appended to the per-sequence caches only.
    causal, window_size=(left, right): apply to the keys of the sequence, bottom-right aligned on L_b
        as in `flash_attn_with_kvcache`; every prefix key is always visible.  `left` must be negative
        (NotImplementedError otherwise).  A row that sees no key at all (Lp = 0 and no visible key of
        its own) gives 0 and an LSE of -inf.
    num_splits, prefix_num_splits: the key splits of the per-sequence pass and of the prefix pass:
        0 lets the library choose (at least 2), 2 .. 128 forces the count.  1 is rejected: both passes
        hand fp32 partial results to the merge, which a pass with one split does not write.
    return_lse: also return the base-2 log-sum-exp [B, Hq, Sq] in fp32.

    q must collapse to [1, B * Sq, Hq, D]: with Sq == 1 any batch stride does (a slice of a fused QKV
    buffer needs no copy), otherwise a q with `q.stride(0) != Sq * q.stride(1)` is copied first.

    Returns `out` [B, Sq, Hq, D] in q's dtype, or `(out, lse)`.
    """
    paged, prefix_paged = block_table is not None, prefix_block_table is not None
    if paged and cache_seqlens is None:
        raise TypeError("cache_seqlens is required with a paged cache: an int or an int32 tensor")
    left, right = _check_plain_args(k, v, window_size, num_splits, cache_seqlens)
    if not isinstance(prefix_num_splits, int) or isinstance(prefix_num_splits, bool) or not 0 <= prefix_num_splits <= MAX_SPLITS:
        raise ValueError(f"prefix_num_splits must be an int in 0 .. {MAX_SPLITS}, got {prefix_num_splits!r}")
    if isinstance(prefix_seqlen, bool) or not (prefix_seqlen is None or isinstance(prefix_seqlen, (int, Tensor))):
        raise TypeError(f"prefix_seqlen must be None, an int or an int32 tensor, got {type(prefix_seqlen).__name__}")
    if left >= 0:
        raise NotImplementedError(f"window_size[0] = {left}: a left window bound is not supported with a shared prefix")
    for name, n in (("num_splits", num_splits), ("prefix_num_splits", prefix_num_splits)):
        if n == 1:
            raise ValueError(f"{name} = 1: both passes hand fp32 partial results to the merge, which a pass with one split "
                             f"does not write; pass 0 or 2 .. {MAX_SPLITS}")
    for name, t in (("prefix_k", prefix_k), ("prefix_v", prefix_v), ("k_cache", k_cache), ("v_cache", v_cache)):
        if isinstance(t, Tensor) and str(t.dtype).startswith("torch.float8"):
            raise NotImplementedError(f"{name} is {t.dtype}: fp8 caches are not supported with a shared prefix")
    for name, t in (("block_table", block_table), ("prefix_block_table", prefix_block_table)):
        if t is not None and (not isinstance(t, Tensor) or t.dim() != 2):
            raise ValueError(f"{name} must be a 2-d int32 tensor [batch, max_blocks]")
    for name, t in (("prefix_k", prefix_k), ("prefix_v", prefix_v)):
        if not isinstance(t, Tensor) or t.dim() != 4 or (not prefix_paged and t.shape[0] != 1):
            raise ValueError(f"{name} must be a 4-d tensor [1, cap_p, heads_kv, head_dim] (one prefix for the whole batch), or with "
                             f"prefix_block_table a pool [num_blocks, page_block_size, heads_kv, head_dim]")
    pool = "num_blocks, page_block_size"
    batch, seqlen_q, heads_q, head_dim, heads_kv, new = _check_tensors(q, k_cache, v_cache, k, v, pool if paged else "batch, cap")
    try:  # the prefix is the cache of a batch of one
        _check_tensors(q[:1], prefix_k, prefix_v, None, None, pool if prefix_paged else "batch, cap")
        if prefix_k.shape[2] != heads_kv:
            raise ValueError(f"{prefix_k.shape[2]} kv heads, k_cache has {heads_kv}")
        cap_p = _check_block_table(prefix_block_table, prefix_k, q[:1]) if prefix_paged else prefix_k.shape[1]
        prefix_len = _seqlens_on_device(prefix_seqlen, 1, cap_p, q.device)
    except (ValueError, TypeError, NotImplementedError) as e:
        raise type(e)(f"prefix_k / prefix_v / prefix_block_table / prefix_seqlen (the k_cache / v_cache / block_table / "
                      f"cache_seqlens of a batch of 1): {e}") from None
    cap = _check_block_table(block_table, k_cache, q) if paged else k_cache.shape[1]
    seqlens = _seqlens_on_device(cache_seqlens, batch, cap, q.device)
    lib = _lib.load()
    args = _lib.PrefixKvCacheArgs()
    base = args.seq.base
    with torch.no_grad():
        if seqlen_q > 1 and batch > 1 and q.stride(0) != seqlen_q * q.stride(1):
            q = q.contiguous()  # the prefix pass reads q as [1, B * Sq, Hq, D]
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        lse = torch.empty((batch, heads_q, seqlen_q), dtype=torch.float32, device=q.device) if return_lse else None
        _fill_cache_side(args.seq, k_cache, v_cache, block_table, seqlens, cap, num_splits)
        _fill_cache_side(args.prefix, prefix_k, prefix_v, prefix_block_table, prefix_len, cap_p, prefix_num_splits)
        base.q, base.o = q.data_ptr(), out.data_ptr()
        base.lse = lse.data_ptr() if return_lse else None
        base.q_stride[:] = bshd_strides(q)
        base.o_stride[:] = bshd_strides(out)
        if new:
            base.k_new, base.v_new = k.data_ptr(), v.data_ptr()
            base.k_new_stride[:] = bshd_strides(k)
            base.v_new_stride[:] = bshd_strides(v)
            base.seqlen_new = k.shape[1]
        base.batch, base.heads_q, base.heads_kv = batch, heads_q, heads_kv
        base.seqlen_q, base.head_dim = seqlen_q, head_dim
        base.causal = int(bool(causal))
        base.window_left, base.window_right = left, right
        base.dtype = encode_dtype(q)
        base.softmax_scale = 1.0 / math.sqrt(head_dim) if softmax_scale is None else float(softmax_scale)
        need = lib.fa2_prefix_kvcache_workspace_bytes(ctypes.byref(args))  # a function of the shapes only
        workspace = None
        if need > 0:
            workspace = torch.empty(need, dtype=torch.uint8, device=q.device)
            base.workspace, base.workspace_bytes = workspace.data_ptr(), need
        _lib.check(launch_on(q, lambda st: lib.fa2_fwd_kvcache_prefix(ctypes.byref(args), st)))
    return (out, lse) if return_lse else out


def _check_descale(name: str, d) -> None:
    """A descale judged without looking at a tensor: None, a float > 0 or a tensor."""
    if d is None or isinstance(d, Tensor):
        return
    if isinstance(d, bool) or not isinstance(d, (int, float)):
        raise TypeError(f"{name} must be None, a float > 0 or an fp32 tensor, got {type(d).__name__}")
    if not (d > 0 and math.isfinite(d)):
        raise ValueError(f"{name} must be a finite float > 0, got {d!r}")


def _descale_on_device(name: str, d, batch: int, heads_kv: int, device) -> Optional[Tensor]:
    """None (1.0), or an fp32 [batch, heads_kv] view on `device` (strides may be 0)."""
    if d is None:
        return None
    if not isinstance(d, Tensor):
        return torch.full((1, 1), float(d), dtype=torch.float32, device=device).expand(batch, heads_kv)
    if d.dtype != torch.float32:
        raise TypeError(f"{name} must be an fp32 tensor, got {d.dtype}")
    if d.device != device:
        raise ValueError(f"{name} must be on q's GPU device, got {d.device}")
    try:
        d = d.expand(batch, heads_kv) if d.dim() <= 2 else None
    except RuntimeError:
        d = None
    if d is None:
        raise ValueError(f"{name} must be broadcastable to [batch={batch}, heads_kv={heads_kv}]")
    return d


def flash_attn_with_fp8_kvcache(
    q: Tensor,
    k_cache: Tensor,
    v_cache: Tensor,
    k_descale: Union[None, float, Tensor] = None,
    v_descale: Union[None, float, Tensor] = None,
    block_table: Optional[Tensor] = None,
    cache_seqlens: Union[None, int, Tensor] = None,
    k: Optional[Tensor] = None,
    v: Optional[Tensor] = None,
    softmax_scale: Optional[float] = None,
    causal: bool = False,
    window_size: Tuple[int, int] = (-1, -1),
    num_splits: int = 0,
    return_lse: bool = False,
):
    """`flash_attn_with_kvcache` (with `block_table`: `flash_attn_with_paged_kvcache`) over caches that
    hold `torch.float8_e4m3fn` bytes: half the bytes of a 16-bit cache, on the path that is bound by
    reading them.  q, the new rows and the result are fp16 or bf16; head_dim is a multiple of 16 up
    to 128 and every cache row must start on a 16-byte boundary.

    Inference only: no autograd graph is built and the result never requires grad.  Not implemented:
    e5m2 or fnuz caches, fp8 q, per-token or per-block scales, head dims above 128, rotary embedding,
    a batch-index indirection.

    k_descale, v_descale: the value of a cache element is its exact e4m3 value times the descale of
        its (batch, kv head): None (1.0), a Python float > 0, or an fp32 device tensor broadcastable
        to [B, Hkv] (an expanded view is fine) that is read on the device.  The scores are
        (softmax_scale * k_descale) * q . k8 and the result is v_descale * (P v8), scaled in fp32
        before its one rounding; K and V themselves are converted exactly, never scaled.
    block_table: None for contiguous caches [B, cap, Hkv, D]; with an int32 table [B, max_blocks]
        the caches are pools [num_blocks, P, Hkv, D], `cache_seqlens` is required and the rules are
        those of `flash_attn_with_paged_kvcache`.
    k, v: optional new rows [B, Sn, Hkv, D] in q's dtype, quantised on the way into the caches:
        the byte written is e4m3(clamp(float(x) / descale, -448, 448)), rounded to nearest even, NaN
        kept.  Attention in the same call reads the quantised bytes.
    cache_seqlens, softmax_scale, causal, window_size, num_splits, return_lse: as
        `flash_attn_with_kvcache`.

    Returns `out` [B, Sq, Hq, D] in q's dtype, or `(out, lse)`.  With descales that are powers of two
    the same bits as the 16-bit call on `k_cache.to(q.dtype)`, `v_cache.to(q.dtype)` with
    softmax_scale * k_descale, times v_descale.
    """
    _check_descale("k_descale", k_descale)
    _check_descale("v_descale", v_descale)
    if block_table is not None and cache_seqlens is None:
        raise TypeError("cache_seqlens is required with a paged cache: an int or an int32 tensor")
    left, right = _check_plain_args(k, v, window_size, num_splits, cache_seqlens)
    paged = block_table is not None
    if paged and (not isinstance(block_table, Tensor) or block_table.dim() != 2):
        raise ValueError("block_table must be a 2-d int32 tensor [batch, max_blocks]")
    batch, _, _, _, heads_kv, new = _check_tensors(q, k_cache, v_cache, k, v, "num_blocks, page_block_size" if paged else "batch, cap",
                                                   cache_dtype=torch.float8_e4m3fn, max_head_dim=128)
    cap = _check_block_table(block_table, k_cache, q) if paged else k_cache.shape[1]
    kd = _descale_on_device("k_descale", k_descale, batch, heads_kv, q.device)
    vd = _descale_on_device("v_descale", v_descale, batch, heads_kv, q.device)
    seqlens = _seqlens_on_device(cache_seqlens, batch, cap, q.device)
    lib = _lib.load()
    args = _lib.Fp8KvCacheArgs()
    if paged:
        _fill_paging(args.paged, block_table, k_cache)
    for name, d in (("k_descale", kd), ("v_descale", vd)):
        if d is not None:
            setattr(args, name, d.data_ptr())
            getattr(args, name + "_stride")[:] = (d.stride(0) if batch > 1 else 0, d.stride(1) if heads_kv > 1 else 0)
    return _run(args, args.paged.base, lib.fa2_fp8_kvcache_workspace_bytes, lib.fa2_fwd_kvcache_fp8, q, k_cache, v_cache,
                new, seqlens, cap, softmax_scale, causal, left, right, num_splits, return_lse)
