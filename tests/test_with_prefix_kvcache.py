"""Shared-prefix (cascade) decode attention on the GPU (`flash_attn_with_prefix_kvcache`,
fa2_fwd_kvcache_prefix): parity with the oracle on the per-batch concatenation [prefix[:Lp];
cache_b[:L_b]] under a key-padding mask, both cache layouts on either side, the bitwise anchors that
pin the prefix pass's row remap and the merge order, reads that stop at the lengths, the append,
strided q, graph capture with lengths that change between replays, and the rejections.
"""
import functools

import pytest
import torch

from tests.test_kvcache import _check, _data, _lens

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
NAN = float("nan")


def _prefix(hkv, d, cap_p, dtype, seed=7):
    """prefix_k, prefix_v [1, cap_p, Hkv, D], normal(0, 0.5) as the caches of tests/test_kvcache.py."""
    _, pk, pv = _data(1, 1, hkv, hkv, d, cap_p, dtype, seed=seed)
    return pk, pv


def _concat(pk, pv, kc, vc, lp, lens):
    """The caches the oracle sees: row b is cat(prefix[:Lp], cache_b[:L_b]), zero-padded to the longest,
    and the lengths Lp + L_b (its key-padding mask)."""
    b, _, hkv, d = kc.shape
    total = tuple(lp + n for n in lens)
    kcat = torch.zeros((b, max(max(total), 1), hkv, d), dtype=kc.dtype, device="cuda")
    vcat = torch.zeros_like(kcat)
    for i, n in enumerate(lens):
        kcat[i, :lp + n] = torch.cat((pk[0, :lp], kc[i, :n]))
        vcat[i, :lp + n] = torch.cat((pv[0, :lp], vc[i, :n]))
    return kcat, vcat, total


def _one_pool(pk, pv, kc, vc, page, spare=3, seed=1):
    """The prefix [1, cap_p, Hkv, D] and the slabs [B, cap, Hkv, D] in one pair of pools, their pages
    scattered by one random permutation.  Capacities are rounded up to whole pages; the rows that
    adds and the `spare` blocks no table names hold NaN.  Returns (k_pool, v_pool, prefix table
    [1, nb_p] int32, table [B, nb] int32, spare ids)."""
    hkv, d = kc.shape[2], kc.shape[3]

    def pages(x):
        n, cap = x.shape[0], x.shape[1]
        nb = -(-cap // page)
        padded = torch.full((n, nb * page, hkv, d), NAN, dtype=x.dtype, device="cuda")
        padded[:, :cap] = x
        return padded.reshape(n * nb, page, hkv, d), nb

    (kpp, nb_p), (vpp, _), (ksp, nb), (vsp, _) = pages(pk), pages(pv), pages(kc), pages(vc)
    used = nb_p + kc.shape[0] * nb
    perm = torch.randperm(used + spare, generator=torch.Generator().manual_seed(seed))
    ids = perm[:used].cuda()
    kp = torch.full((used + spare, page, hkv, d), NAN, dtype=kc.dtype, device="cuda")
    vp = torch.full_like(kp, NAN)
    kp[ids] = torch.cat((kpp, ksp))
    vp[ids] = torch.cat((vpp, vsp))
    return kp, vp, ids[:nb_p].reshape(1, nb_p).to(torch.int32), ids[nb_p:].reshape(-1, nb).to(torch.int32), perm[used:].cuda()


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# (B, Hq, Hkv, Sq, D, Lp, cap_p, lengths, cap, causal, (prefix_num_splits, num_splits))
CASES = {
    "one-row-auto": (4, 8, 2, 1, 128, 300, 512, (256, 1, 63, 130), 256, True, (0, 0)),
    # 40 rows per kv head in the prefix pass: two row tiles, the second partly filled, the rows of
    # batch 4 (rows 32 .. 39) and of batch 3 on either side of the tile edge
    "two-row-tiles": (5, 8, 2, 2, 128, 65, 128, (64, 2, 100, 7, 33), 128, True, (3, 2)),
    "short-and-empty-suffix": (3, 16, 1, 3, 64, 1, 64, (0, 2, 70), 128, False, (2, 4)),
    "prefix-splits-mostly-empty": (2, 4, 4, 1, 128, 1000, 1024, (5, 5), 64, True, (16, 2)),
    "d32": (2, 8, 2, 2, 32, 131, 192, (300, 131), 300, True, (0, 0)),
    "d96": (2, 8, 2, 2, 96, 131, 192, (300, 131), 300, True, (0, 0)),
    "d256": (2, 8, 2, 2, 256, 131, 192, (300, 131), 300, True, (0, 0)),
}


@functools.lru_cache(maxsize=None)
def _contiguous(case, dtype):
    """The inputs of a case and the result of the contiguous arm, computed once and never modified."""
    from fa2_triton_amd import flash_attn_with_prefix_kvcache

    b, hq, hkv, sq, d, lp, cap_p, lens, cap, causal, (ns_p, ns_s) = CASES[case]
    q, kc, vc = _data(b, sq, hq, hkv, d, cap, dtype)
    pk, pv = _prefix(hkv, d, cap_p, dtype)
    got = flash_attn_with_prefix_kvcache(q, pk, pv, kc, vc, prefix_seqlen=_lens((lp,)), cache_seqlens=_lens(lens), causal=causal,
                                         num_splits=ns_s, prefix_num_splits=ns_p, return_lse=True)
    return (q, pk, pv, kc, vc), got


@DTYPES
@pytest.mark.parametrize("case", sorted(CASES))
def test_parity(case, dtype):
    """The reference tests' forward rule with no escape taken, on the concatenated caches."""
    b, hq, hkv, sq, d, lp, cap_p, lens, cap, causal, _ = CASES[case]
    assert not causal or min(lens) >= sq  # only then is the union's mask the oracle's bottom-right causal one
    (q, pk, pv, kc, vc), (out, lse) = _contiguous(case, dtype)
    kcat, vcat, total = _concat(pk, pv, kc, vc, lp, lens)
    _check(q, kcat, vcat, total, out, lse, causal, (-1, -1))


@DTYPES
@pytest.mark.parametrize("page", [16, 64, 256])
@pytest.mark.parametrize("case", ["one-row-auto", "two-row-tiles"])
def test_paged_arms_give_the_bits_of_the_contiguous_arm(case, page, dtype):
    """Prefix and sequences in one pool behind two tables; and, at P = 64, a contiguous prefix with
    paged sequences and the reverse."""
    from fa2_triton_amd import flash_attn_with_prefix_kvcache

    b, hq, hkv, sq, d, lp, cap_p, lens, cap, causal, (ns_p, ns_s) = CASES[case]
    (q, pk, pv, kc, vc), want = _contiguous(case, dtype)
    kp, vp, table_p, table, _ = _one_pool(pk, pv, kc, vc, page)
    kw = dict(prefix_seqlen=_lens((lp,)), cache_seqlens=_lens(lens), causal=causal, num_splits=ns_s, prefix_num_splits=ns_p,
              return_lse=True)
    got = flash_attn_with_prefix_kvcache(q, kp, vp, kp, vp, prefix_block_table=table_p, block_table=table, **kw)
    assert _same(got, want)
    if page == 64:
        got = flash_attn_with_prefix_kvcache(q, pk, pv, kp, vp, block_table=table, **kw)
        assert _same(got, want)
        got = flash_attn_with_prefix_kvcache(q, kp, vp, kc, vc, prefix_block_table=table_p, **kw)
        assert _same(got, want)


@DTYPES
def test_without_a_prefix_it_is_the_plain_call_bitwise(dtype):
    """Lp = 0: the prefix splits have weight 0 and the merge is kvcache_combine_kernel's sum."""
    from fa2_triton_amd import flash_attn_with_kvcache, flash_attn_with_prefix_kvcache

    lens = (300, 2, 65)
    q, kc, vc = _data(3, 2, 8, 2, 128, 320, dtype)
    pk, pv = _prefix(2, 128, 64, dtype)
    for ns_s, ns_p in ((3, 2), (2, 5)):
        want = flash_attn_with_kvcache(q, kc, vc, cache_seqlens=_lens(lens), causal=True, num_splits=ns_s, return_lse=True)
        got = flash_attn_with_prefix_kvcache(q, pk, pv, kc, vc, prefix_seqlen=_lens((0,)), cache_seqlens=_lens(lens), causal=True,
                                             num_splits=ns_s, prefix_num_splits=ns_p, return_lse=True)
        assert _same(got, want), (ns_s, ns_p)


@DTYPES
def test_without_suffix_keys_it_is_the_prefix_pass_bitwise(dtype):
    """Every L_b = 0, non-causal: the batch-1 call on q as [1, B * Sq, Hq, D], row b * Sq + i."""
    from fa2_triton_amd import flash_attn_with_kvcache, flash_attn_with_prefix_kvcache

    b, sq, hq, hkv, d, lp = 5, 2, 8, 2, 128, 200
    q, kc, vc = _data(b, sq, hq, hkv, d, 64, dtype)
    pk, pv = _prefix(hkv, d, 256, dtype)
    for ns_p, ns_s in ((3, 2), (2, 4)):
        out1, lse1 = flash_attn_with_kvcache(q.reshape(1, b * sq, hq, d), pk, pv, cache_seqlens=lp, num_splits=ns_p, return_lse=True)
        want = out1.reshape(b, sq, hq, d), lse1.reshape(hq, b, sq).transpose(0, 1)
        got = flash_attn_with_prefix_kvcache(q, pk, pv, kc, vc, prefix_seqlen=lp, cache_seqlens=0, num_splits=ns_s,
                                             prefix_num_splits=ns_p, return_lse=True)
        assert _same(got, want), (ns_p, ns_s)


def test_no_key_at_all_gives_zero_and_minus_inf():
    from fa2_triton_amd import flash_attn_with_prefix_kvcache

    q, kc, vc = _data(2, 3, 8, 2, 64, 64, torch.bfloat16)
    pk, pv = _prefix(2, 64, 64, torch.bfloat16)
    # causal, Sq 3 over 1 and 0 keys, Lp = 0: rows 0, 1 of batch 0 and every row of batch 1 see no key
    out, lse = flash_attn_with_prefix_kvcache(q, pk, pv, kc, vc, prefix_seqlen=0, cache_seqlens=_lens((1, 0)), causal=True,
                                              return_lse=True)
    assert torch.all(torch.isneginf(lse[0, :, :2])) and torch.all(torch.isneginf(lse[1]))
    assert torch.count_nonzero(out[0, :2]) == 0 and torch.count_nonzero(out[1]) == 0
    assert torch.isfinite(lse[0, :, 2]).all() and torch.isfinite(out).all()


def test_deterministic_and_batch_invariant():
    """Two runs give equal bits, and with the split counts forced, batch row b of a B = 4 call has
    the bits of the B = 1 call on that row alone (whose prefix pass has other rows in its tile)."""
    from fa2_triton_amd import flash_attn_with_prefix_kvcache

    lens = (500, 3, 257, 64)
    q, kc, vc = _data(4, 2, 16, 4, 128, 512, torch.bfloat16)
    pk, pv = _prefix(4, 128, 384, torch.bfloat16)
    kw = dict(prefix_seqlen=_lens((333,)), causal=True, num_splits=3, prefix_num_splits=4, return_lse=True)
    a = flash_attn_with_prefix_kvcache(q, pk, pv, kc, vc, cache_seqlens=_lens(lens), **kw)
    b = flash_attn_with_prefix_kvcache(q, pk, pv, kc, vc, cache_seqlens=_lens(lens), **kw)
    assert _same(a, b)
    for i, n in enumerate(lens):
        one = flash_attn_with_prefix_kvcache(q[i:i + 1], pk, pv, kc[i:i + 1], vc[i:i + 1], cache_seqlens=_lens((n,)), **kw)
        assert torch.equal(one[0][0], a[0][i]) and torch.equal(one[1][0], a[1][i]), i


@pytest.mark.parametrize("page", [0, 16], ids=["contiguous", "p16"])
def test_nothing_past_a_length_is_read(page):
    """NaN in the prefix rows >= Lp, in the sequence rows >= L_b and (paged) in the blocks no table
    names changes no bit against zeros there; and the result is the oracle's."""
    from fa2_triton_amd import flash_attn_with_prefix_kvcache

    b, sq, hq, hkv, d, lp, lens = 3, 1, 8, 2, 128, 70, (100, 1, 64)
    q, kc, vc = _data(b, sq, hq, hkv, d, 128, torch.bfloat16)
    pk, pv = _prefix(hkv, d, 128, torch.bfloat16)
    results = []
    for fill in (0.0, NAN):
        pk2, pv2, kc2, vc2 = pk.clone(), pv.clone(), kc.clone(), vc.clone()
        pk2[:, lp:], pv2[:, lp:] = fill, fill
        for i, n in enumerate(lens):
            kc2[i, n:], vc2[i, n:] = fill, fill
        kw = dict(prefix_seqlen=_lens((lp,)), cache_seqlens=_lens(lens), causal=True, return_lse=True)
        if page:
            kp, vp, table_p, table, spare = _one_pool(pk2, pv2, kc2, vc2, page)
            kp[spare], vp[spare] = fill, fill
            results.append(flash_attn_with_prefix_kvcache(q, kp, vp, kp, vp, prefix_block_table=table_p, block_table=table, **kw))
        else:
            results.append(flash_attn_with_prefix_kvcache(q, pk2, pv2, kc2, vc2, **kw))
    assert _same(results[0], results[1])
    kcat, vcat, total = _concat(pk, pv, kc, vc, lp, lens)
    _check(q, kcat, vcat, total, results[1][0], results[1][1], True, (-1, -1))


def test_prefix_seqlen_is_clamped_on_the_device():
    from fa2_triton_amd import flash_attn_with_prefix_kvcache

    q, kc, vc = _data(2, 1, 8, 2, 128, 128, torch.bfloat16)
    pk, pv = _prefix(2, 128, 192, torch.bfloat16)
    run = lambda lp: flash_attn_with_prefix_kvcache(q, pk, pv, kc, vc, prefix_seqlen=lp, cache_seqlens=_lens((100, 7)), causal=True,
                                                    return_lse=True)
    full, none = run(None), run(_lens((0,)))
    assert _same(run(_lens((10**9,))), full) and _same(run(_lens((192,))), full) and _same(run(10**9), full)
    assert _same(run(_lens((-5,))), none) and _same(run(-5), none)
    assert not torch.equal(full[0], none[0])


@DTYPES
@pytest.mark.parametrize("sn", [1, 3])
def test_append(sn, dtype):
    """k, v land at rows L_b .. L_b + Sn - 1 of the per-sequence caches only; the prefix keeps its
    bits; the result is that of a call without append on the updated caches."""
    from fa2_triton_amd import flash_attn_with_prefix_kvcache

    b, hq, hkv, d, cap, lp = 3, 8, 2, 128, 192, 90
    lens = (100, 0, 189)
    q, kc, vc = _data(b, sn, hq, hkv, d, cap, dtype)
    _, kn, vn = _data(b, sn, hq, hkv, d, sn, dtype, seed=3)
    pk, pv = _prefix(hkv, d, 128, dtype)
    k0, v0, pk0, pv0 = kc.clone(), vc.clone(), pk.clone(), pv.clone()
    seqlens, plen = _lens(lens), _lens((lp,))
    got = flash_attn_with_prefix_kvcache(q, pk, pv, kc, vc, prefix_seqlen=plen, cache_seqlens=seqlens, k=kn, v=vn, causal=True,
                                         return_lse=True)
    assert torch.equal(seqlens, _lens(lens)) and torch.equal(plen, _lens((lp,)))  # not modified
    assert torch.equal(pk, pk0) and torch.equal(pv, pv0)
    for i, n in enumerate(lens):
        k0[i, n:n + sn], v0[i, n:n + sn] = kn[i], vn[i]
    assert torch.equal(kc, k0) and torch.equal(vc, v0)
    after = tuple(n + sn for n in lens)
    want = flash_attn_with_prefix_kvcache(q, pk, pv, kc, vc, prefix_seqlen=plen, cache_seqlens=_lens(after), causal=True,
                                          return_lse=True)
    assert _same(got, want)
    kcat, vcat, total = _concat(pk, pv, kc, vc, lp, after)
    _check(q, kcat, vcat, total, got[0], got[1], True, (-1, -1))


def test_append_through_a_table_shared_with_the_prefix():
    """Paged on both sides in one pool: the new rows go through the sequences' table, the prefix's
    blocks keep their bits, and the result has the bits of the contiguous call."""
    from fa2_triton_amd import flash_attn_with_prefix_kvcache

    b, hq, hkv, d, lp, lens, sn = 2, 8, 2, 64, 40, (31, 16), 2
    q, kc, vc = _data(b, sn, hq, hkv, d, 64, torch.bfloat16)
    _, kn, vn = _data(b, sn, hq, hkv, d, sn, torch.bfloat16, seed=3)
    pk, pv = _prefix(hkv, d, 48, torch.bfloat16)
    kp, vp, table_p, table, _ = _one_pool(pk, pv, kc, vc, 16)
    kw = dict(prefix_seqlen=lp, cache_seqlens=_lens(lens), k=kn, v=vn, causal=True, return_lse=True)
    got = flash_attn_with_prefix_kvcache(q, kp, vp, kp, vp, prefix_block_table=table_p, block_table=table, **kw)
    want = flash_attn_with_prefix_kvcache(q, pk, pv, kc, vc, **kw)
    assert _same(got, want)
    assert torch.equal(kp[table_p[0].long()].reshape(1, 48, hkv, d), pk) and torch.equal(vp[table_p[0].long()].reshape(1, 48, hkv, d), pv)
    assert torch.equal(kp[table.long()].reshape(b, 64, hkv, d), kc) and torch.equal(vp[table.long()].reshape(b, 64, hkv, d), vc)


@DTYPES
def test_strided_q(dtype):
    """Sq = 1: q as a slice of a fused QKV buffer (its batch stride serves as the prefix pass's row
    stride); Sq = 2: a q that does not collapse to [1, B * Sq, Hq, D].  Both give the bits of a
    contiguous copy."""
    from fa2_triton_amd import flash_attn_with_prefix_kvcache

    b, hq, hkv, d = 5, 8, 2, 128
    pk, pv = _prefix(hkv, d, 128, dtype)
    for sq in (1, 2):
        q, kc, vc = _data(b, sq, hq, hkv, d, 128, dtype)
        kw = dict(prefix_seqlen=100, cache_seqlens=_lens((128, 2, 77, 64, 5)), causal=True, num_splits=2, prefix_num_splits=3,
                  return_lse=True)
        want = flash_attn_with_prefix_kvcache(q, pk, pv, kc, vc, **kw)
        if sq == 1:
            qkv = torch.full((b, 1, hq + 2 * hkv, d), NAN, dtype=dtype, device="cuda")
            view = qkv[:, :, :hq]
        else:
            big = torch.full((b, sq + 1, hq, d), NAN, dtype=dtype, device="cuda")
            view = big[:, :sq]
            assert view.stride(0) != sq * view.stride(1)
        view.copy_(q)
        assert not view.is_contiguous()
        assert _same(flash_attn_with_prefix_kvcache(view, pk, pv, kc, vc, **kw), want), sq


def test_graph_capture_follows_the_device_lengths():
    """One decode step (append + cascade) captured once on one stream: after `cache_seqlens` is
    advanced and `prefix_seqlen` changed in place, a replay equals a fresh eager call on the same
    state bitwise."""
    from fa2_triton_amd import flash_attn_with_prefix_kvcache

    b, hq, hkv, d, cap = 3, 16, 4, 128, 512
    dtype = torch.bfloat16
    q, kc, vc = _data(b, 1, hq, hkv, d, cap, dtype)
    _, kn, vn = _data(b, 1, hq, hkv, d, 1, dtype, seed=1)
    pk, pv = _prefix(hkv, d, 384, dtype)
    seqlens, plen = _lens((300, 63, 0)), _lens((200,))

    def step(kc_, vc_):
        return flash_attn_with_prefix_kvcache(q, pk, pv, kc_, vc_, prefix_seqlen=plen, cache_seqlens=seqlens, k=kn, v=vn,
                                              causal=True, return_lse=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(kc, vc)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(kc, vc)
    graph.replay()
    torch.cuda.synchronize()
    fresh = step(kc.clone(), vc.clone())
    assert _same(captured, fresh)

    for seed, lp in ((11, 384), (12, 1)):  # two more decode steps through the same graph
        q2, _, _ = _data(b, 1, hq, hkv, d, 1, dtype, seed=seed)
        _, k2, v2 = _data(b, 1, hq, hkv, d, 1, dtype, seed=seed + 100)
        seqlens += 1
        plen.fill_(lp)
        q.copy_(q2)
        kn.copy_(k2)
        vn.copy_(v2)
        graph.replay()
        torch.cuda.synchronize()
        kf, vf = kc.clone(), vc.clone()
        fresh = step(kf, vf)
        assert _same(captured, fresh)
        assert torch.equal(kf, kc) and torch.equal(vf, vc)
    lens = tuple(int(n) + 1 for n in seqlens.tolist())
    kcat, vcat, total = _concat(pk, pv, kc, vc, 1, lens)
    _check(q, kcat, vcat, total, captured[0], captured[1], True, (-1, -1))


def test_inference_only_and_rejections():
    from fa2_triton_amd import flash_attn_with_prefix_kvcache

    q, kc, vc = _data(2, 1, 4, 2, 64, 128, torch.bfloat16)
    pk, pv = _prefix(2, 64, 64, torch.bfloat16)
    out = flash_attn_with_prefix_kvcache(q.requires_grad_(), pk.requires_grad_(), pv.requires_grad_(), kc.requires_grad_(),
                                         vc.requires_grad_())
    assert not out.requires_grad and out.grad_fn is None
    with pytest.raises(NotImplementedError, match="window"):
        flash_attn_with_prefix_kvcache(q, pk, pv, kc, vc, window_size=(16, -1))
    with pytest.raises(NotImplementedError, match="window"):
        flash_attn_with_prefix_kvcache(q, pk, pv, kc, vc, causal=True, window_size=(0, 0))
    with pytest.raises(NotImplementedError, match="fp8"):
        flash_attn_with_prefix_kvcache(q, pk.to(torch.float8_e4m3fn), pv.to(torch.float8_e4m3fn), kc, vc)
    with pytest.raises(ValueError, match="num_splits = 1"):
        flash_attn_with_prefix_kvcache(q, pk, pv, kc, vc, num_splits=1)
    with pytest.raises(ValueError, match="prefix_k"):
        flash_attn_with_prefix_kvcache(q, kc, vc, kc, vc)  # a prefix per batch row
    with pytest.raises(ValueError, match="prefix_k.*kv heads"):
        flash_attn_with_prefix_kvcache(q, pk[:, :, :1], pv[:, :, :1], kc, vc)
    with pytest.raises(TypeError, match="prefix_k.*dtype"):
        flash_attn_with_prefix_kvcache(q, pk.half(), pv.half(), kc, vc)
    with pytest.raises(ValueError, match="prefix_k.*shape"):
        flash_attn_with_prefix_kvcache(q, pk, pv[:, :32], kc, vc)
    with pytest.raises(ValueError, match="prefix_k.*cache_seqlens"):
        flash_attn_with_prefix_kvcache(q, pk, pv, kc, vc, prefix_seqlen=_lens((5, 5)))
    with pytest.raises((ValueError, TypeError)):
        flash_attn_with_prefix_kvcache(q, pk.cpu(), pv.cpu(), kc, vc)
    with pytest.raises(TypeError, match="cache_seqlens is required"):
        flash_attn_with_prefix_kvcache(q, pk, pv, kc, vc, block_table=torch.zeros(2, 2, dtype=torch.int32, device="cuda"))
