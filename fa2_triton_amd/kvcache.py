"""KV-cache decode attention: `flash_attn_with_kvcache` (C ABI `fa2_fwd_kvcache`, ABI 10 minor 1).

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
    inputs require.  Not implemented: paged caches (block tables), rotary embedding, bias, dropout,
    backward.

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
    for name, t in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache)):
        if not isinstance(t, Tensor) or t.dim() != 4:
            raise ValueError(f"{name} must be a 4-d tensor [batch, seqlen, heads, head_dim]")
    batch, seqlen_q, heads_q, head_dim = q.shape
    _, cap, heads_kv, _ = k_cache.shape
    if k_cache.shape != (batch, cap, heads_kv, head_dim) or v_cache.shape != k_cache.shape:
        raise ValueError(f"{k_cache.shape = } and {v_cache.shape = } must both be (batch={batch}, cap, heads_kv, "
                         f"head_dim={head_dim})")
    if heads_kv < 1 or heads_q % heads_kv != 0:
        raise ValueError(f"{heads_q = } is not divisible by {heads_kv = }")
    if seqlen_q < 1 or cap < 1:
        raise ValueError(f"{seqlen_q = } and the cache capacity {cap} must be at least 1")
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
        if t.dtype != q.dtype:
            raise TypeError(f"{name} is {t.dtype}, q is {q.dtype}: all tensors must have the same dtype")
    for name, t in tensors:
        if not t.is_cuda or t.device != q.device:
            raise ValueError(f"{name} must be on q's GPU device, got {t.device}")
        if t.stride(-1) != 1:
            raise ValueError(f"{name} must have a unit head-dim stride")
    if head_dim > 256:
        raise NotImplementedError(f"{head_dim = } > 256 is not supported")
    if isinstance(cache_seqlens, Tensor):
        if cache_seqlens.dtype != torch.int32 or cache_seqlens.shape != (batch,) or cache_seqlens.device != q.device:
            raise ValueError(f"cache_seqlens must be an int32 tensor of shape ({batch},) on {q.device}, got "
                             f"{cache_seqlens.dtype} {tuple(cache_seqlens.shape)} on {cache_seqlens.device}")
        seqlens = cache_seqlens.contiguous()
    elif cache_seqlens is None:
        seqlens = None
    else:
        seqlens = torch.full((batch,), min(max(cache_seqlens, 0), cap), dtype=torch.int32, device=q.device)
    softmax_scale = 1.0 / math.sqrt(head_dim) if softmax_scale is None else float(softmax_scale)

    with torch.no_grad():
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        lse = torch.empty((batch, heads_q, seqlen_q), dtype=torch.float32, device=q.device) if return_lse else None
        args = _lib.KvCacheArgs()
        args.q, args.k_cache, args.v_cache, args.o = q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr()
        args.lse = lse.data_ptr() if return_lse else None
        args.q_stride[:] = bshd_strides(q)
        args.k_cache_stride[:] = bshd_strides(k_cache)
        args.v_cache_stride[:] = bshd_strides(v_cache)
        args.o_stride[:] = bshd_strides(out)
        if new:
            args.k_new, args.v_new = k.data_ptr(), v.data_ptr()
            args.k_new_stride[:] = bshd_strides(k)
            args.v_new_stride[:] = bshd_strides(v)
            args.seqlen_new = k.shape[1]
        args.cache_seqlens = seqlens.data_ptr() if seqlens is not None else None
        args.batch, args.heads_q, args.heads_kv = batch, heads_q, heads_kv
        args.seqlen_q, args.capacity, args.head_dim = seqlen_q, cap, head_dim
        args.causal = int(bool(causal))
        args.window_left, args.window_right = left, right
        args.dtype = encode_dtype(q)
        args.num_splits = num_splits
        args.softmax_scale = softmax_scale
        lib = _lib.load()
        need = lib.fa2_kvcache_workspace_bytes(ctypes.byref(args))
        workspace = None
        if need > 0:  # a function of the shapes only
            workspace = torch.empty(need, dtype=torch.uint8, device=q.device)
            args.workspace, args.workspace_bytes = workspace.data_ptr(), need
        _lib.check(launch_on(q, lambda st: lib.fa2_fwd_kvcache(ctypes.byref(args), st)))
    return (out, lse) if return_lse else out
