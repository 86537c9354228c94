"""Paged KV-cache decode attention on the GPU (`flash_attn_with_paged_kvcache`, fa2_fwd_kvcache_paged).

The main assertion is bitwise equality with `flash_attn_with_kvcache` on the gathered slab: the paged
kernel stages the same rows into the same LDS image and runs the same step, so every bit of `out`
and `lse` agrees, with forced and with automatic split counts.  Around it: oracle parity, that
nothing unreferenced is read, shared prefixes, pool and table layouts, the append and its bounds,
the device-side clamp of table entries, graph capture with a table that grows between replays,
determinism and batch invariance, and the rejections.
"""
import pytest
import torch

from tests.test_kvcache import _check, _data, _lens

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
NAN = float("nan")


def _pool(kc, vc, page, spare=3, seed=1):
    """Pools and a block table holding the slabs kc / vc [B, cap, Hkv, D]: a random permutation of
    B * max_blocks + spare block ids, slab pages copied into their blocks, the spare blocks (zeros)
    referenced by no table entry.  Returns (k_pool, v_pool, table [B, max_blocks] int32, spare ids)."""
    b, cap, hkv, d = kc.shape
    assert cap % page == 0
    nb = cap // page
    perm = torch.randperm(b * nb + spare, generator=torch.Generator().manual_seed(seed))
    ids = perm[:b * nb].cuda()
    kp = torch.zeros((b * nb + spare, page, hkv, d), dtype=kc.dtype, device="cuda")
    vp = torch.zeros_like(kp)
    kp[ids] = kc.reshape(b * nb, page, hkv, d)
    vp[ids] = vc.reshape(b * nb, page, hkv, d)
    return kp, vp, ids.reshape(b, nb).to(torch.int32), perm[b * nb:].cuda()


def _slab(pool, table):
    """The contiguous cache [B, max_blocks * P, Hkv, D] a table describes."""
    b, nb = table.shape
    return pool[table.long()].reshape(b, nb * pool.shape[1], pool.shape[2], pool.shape[3]).contiguous()


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# (B, Hq, Hkv, Sq, cap, D, lengths, causal, window, num_splits, P)
CASES = {
    "p16-gqa": (3, 32, 8, 1, 304, 128, (304, 17, 16), True, (-1, -1), 0, 16),
    "p16-splits3": (2, 8, 2, 2, 704, 64, (700, 129), False, (-1, -1), 3, 16),
    "p32": (2, 8, 2, 1, 320, 128, (320, 33), True, (-1, -1), 2, 32),
    "p64-boundaries": (4, 8, 8, 1, 512, 128, (512, 1, 63, 65), True, (-1, -1), 0, 64),
    "p128-two-row-tiles": (2, 16, 2, 5, 640, 128, (640, 7), True, (-1, -1), 0, 128),
    "p256-splits16-mostly-empty": (1, 8, 2, 1, 2048, 128, (65,), True, (-1, -1), 16, 256),
    "p64-window": (2, 8, 2, 3, 1024, 64, (1000, 50), True, (64, -1), 0, 64),
    "p16-window-two-sided": (2, 4, 4, 4, 512, 128, (500, 200), False, (30, 10), 0, 16),
    "d32": (2, 8, 2, 2, 320, 32, (300, 131), True, (-1, -1), 2, 64),
    "d96": (2, 8, 2, 2, 320, 96, (300, 131), True, (-1, -1), 2, 64),
    "d256": (2, 8, 2, 2, 320, 256, (300, 131), True, (-1, -1), 2, 64),
}


@DTYPES
@pytest.mark.parametrize("case", sorted(CASES))
def test_bitwise_equal_to_the_contiguous_path(case, dtype):
    """`out` and `lse` equal the contiguous call on the slab bit for bit, with the case's split count
    and with the other kind (automatic where the case forces one, forced where it is automatic)."""
    from fa2_triton_amd import flash_attn_with_kvcache, flash_attn_with_paged_kvcache

    b, hq, hkv, sq, cap, d, lens, causal, window, nsplit, page = CASES[case]
    q, kc, vc = _data(b, sq, hq, hkv, d, cap, dtype)
    kp, vp, table, _ = _pool(kc, vc, page)
    for n in (nsplit, 0 if nsplit else 3):
        kw = dict(cache_seqlens=_lens(lens), causal=causal, window_size=window, num_splits=n, return_lse=True)
        want = flash_attn_with_kvcache(q, kc, vc, **kw)
        got = flash_attn_with_paged_kvcache(q, kp, vp, table, **kw)
        assert torch.equal(got[0], want[0]), (n, (got[0].float() - want[0].float()).abs().max())
        assert torch.equal(got[1], want[1]), n
    # a Python int for the lengths is the same call
    got = flash_attn_with_paged_kvcache(q, kp, vp, table, 40, causal=causal, return_lse=True)
    assert _same(got, flash_attn_with_kvcache(q, kc, vc, cache_seqlens=40, causal=causal, return_lse=True))


@DTYPES
def test_length_zero(dtype):
    """A batch row with no key gives O = 0 and LSE2 = -inf exactly; all bits as the contiguous call."""
    from fa2_triton_amd import flash_attn_with_kvcache, flash_attn_with_paged_kvcache

    q, kc, vc = _data(2, 2, 8, 2, 128, 256, dtype)
    kp, vp, table, _ = _pool(kc, vc, 64)
    for nsplit in (1, 3):
        kw = dict(cache_seqlens=_lens((0, 200)), num_splits=nsplit, return_lse=True)
        out, lse = flash_attn_with_paged_kvcache(q, kp, vp, table, **kw)
        assert torch.count_nonzero(out[0]) == 0 and torch.all(torch.isneginf(lse[0]))
        assert _same((out, lse), flash_attn_with_kvcache(q, kc, vc, **kw))


@DTYPES
@pytest.mark.parametrize("case", ["p16-gqa", "p64-window", "p256-splits16-mostly-empty"])
def test_oracle_parity(case, dtype):
    """One case per page-size class against the oracle by the reference rule, no escape taken.  The
    low-precision reordered oracle must itself be off the fp32 one, so that the rule has a scale."""
    from fa2_triton_amd import flash_attn_with_paged_kvcache

    b, hq, hkv, sq, cap, d, lens, causal, window, nsplit, page = CASES[case]
    assert min(lens) >= 2
    q, kc, vc = _data(b, sq, hq, hkv, d, cap, dtype)
    kp, vp, table, _ = _pool(kc, vc, page)
    out, lse = flash_attn_with_paged_kvcache(q, kp, vp, table, _lens(lens), causal=causal, window_size=window,
                                             num_splits=nsplit, return_lse=True)
    ref, pt = _check(q, kc, vc, lens, out, lse, causal, window)
    assert (pt.float() - ref.float()).abs().max() > 0


@pytest.mark.parametrize("page", [16, 64, 256])
def test_what_is_not_referenced_is_not_read(page):
    """NaN in the spare blocks and in the rows at or past L_b of each sequence's pages, and table
    entries of pages at or past ceil(L_b / P) set to -7 and 2^30: no bit of the result changes."""
    from fa2_triton_amd import flash_attn_with_paged_kvcache

    b, cap, lens = 3, 512, (500, 65, 2)
    q, kc, vc = _data(b, 2, 8, 2, 128, cap, torch.bfloat16)
    kp, vp, table, spare = _pool(kc, vc, page)
    kn, vn, bad = kp.clone(), vp.clone(), table.clone()
    kn[spare], vn[spare] = NAN, NAN
    for i, n in enumerate(lens):
        used = -(-n // page)
        if n % page:  # the rows of the last page past the length
            last = table[i, used - 1].item()
            kn[last, n % page:], vn[last, n % page:] = NAN, NAN
        for j in range(used, cap // page):  # blocks the table no longer names: NaN, and a wild id
            kn[table[i, j].item()], vn[table[i, j].item()] = NAN, NAN
            bad[i, j] = -7 if j % 2 else 2**30
    for nsplit in (0, 3):
        kw = dict(causal=True, num_splits=nsplit, return_lse=True)
        clean = flash_attn_with_paged_kvcache(q, kp, vp, table, _lens(lens), **kw)
        dirty = flash_attn_with_paged_kvcache(q, kn, vn, bad, _lens(lens), **kw)
        assert _same(clean, dirty)
        assert torch.isfinite(dirty[0]).all() and torch.isfinite(dirty[1]).all()


@DTYPES
def test_shared_prefix(dtype):
    """Two table rows name the same blocks for their first 3 pages and then diverge: reading through
    aliased tables gives the bits of the contiguous call on the materialised slabs."""
    from fa2_triton_amd import flash_attn_with_kvcache, flash_attn_with_paged_kvcache

    page, nb = 16, 8
    q, kc, vc = _data(2, 1, 8, 2, 128, nb * page, dtype)
    kp, vp, table, _ = _pool(kc, vc, page)
    table[1, :3] = table[0, :3]
    ks, vs = _slab(kp, table), _slab(vp, table)
    assert torch.equal(ks[0, :3 * page], ks[1, :3 * page]) and not torch.equal(ks[0, 3 * page:], ks[1, 3 * page:])
    for nsplit in (0, 2):
        kw = dict(cache_seqlens=_lens((100, 77)), causal=True, num_splits=nsplit, return_lse=True)
        assert _same(flash_attn_with_paged_kvcache(q, kp, vp, table, **kw), flash_attn_with_kvcache(q, ks, vs, **kw))


@DTYPES
@pytest.mark.parametrize("page", [16, 64])
def test_layouts_need_no_copy(page, dtype):
    """A pool stored [N, Hkv, P, D] and viewed [N, P, Hkv, D], a pool that is a slice of a larger
    buffer, and a table that is a column slice of a wider one give the bits of the plain call."""
    from fa2_triton_amd import flash_attn_with_paged_kvcache

    q, kc, vc = _data(2, 2, 8, 2, 128, 320, dtype)
    kp, vp, table, _ = _pool(kc, vc, page)
    kw = dict(cache_seqlens=_lens((300, 97)), causal=True, return_lse=True)
    want = flash_attn_with_paged_kvcache(q, kp, vp, table, **kw)
    k_hnd, v_hnd = kp.transpose(1, 2).contiguous(), vp.transpose(1, 2).contiguous()  # [N, Hkv, P, D]
    assert not k_hnd.transpose(1, 2).is_contiguous()
    assert _same(flash_attn_with_paged_kvcache(q, k_hnd.transpose(1, 2), v_hnd.transpose(1, 2), table, **kw), want)
    n = kp.shape[0]
    k_big = torch.full((n + 4,) + tuple(kp.shape[1:]), NAN, dtype=dtype, device="cuda")
    v_big = torch.full_like(k_big, NAN)
    k_big[2:2 + n], v_big[2:2 + n] = kp, vp
    assert _same(flash_attn_with_paged_kvcache(q, k_big[2:2 + n], v_big[2:2 + n], table, **kw), want)
    wide = torch.full((2, table.shape[1] + 7), -1, dtype=torch.int32, device="cuda")
    wide[:, 3:3 + table.shape[1]] = table
    cols = wide[:, 3:3 + table.shape[1]]
    assert cols.stride(0) > cols.shape[1] and not cols.is_contiguous()
    assert _same(flash_attn_with_paged_kvcache(q, kp, vp, cols, **kw), want)


@DTYPES
@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("sn", [1, 3])
def test_append(sn, page, dtype):
    """Row n of batch b lands at logical position L_b + n through the table, positions at or past the
    capacity are dropped, every other element of the pools keeps its bits, and attention is that of
    the contiguous append call.  Lengths straddle a page boundary and the capacity."""
    from fa2_triton_amd import flash_attn_with_kvcache, flash_attn_with_paged_kvcache

    cap = 4 * page
    lens = (page - 1, page, cap - 1, cap)
    q, kc, vc = _data(4, sn, 8, 2, 128, cap, dtype)
    _, kn, vn = _data(4, sn, 8, 2, 128, sn, dtype, seed=3)
    kp, vp, table, _ = _pool(kc, vc, page)
    k_want, v_want, table0, seqlens = kp.clone(), vp.clone(), table.clone(), _lens(lens)
    for i, length in enumerate(lens):
        for n in range(sn):
            pos = length + n
            if pos < cap:
                blk = table[i, pos // page].item()
                k_want[blk, pos % page], v_want[blk, pos % page] = kn[i, n], vn[i, n]
    got = flash_attn_with_paged_kvcache(q, kp, vp, table, seqlens, k=kn, v=vn, causal=True, return_lse=True)
    assert torch.equal(seqlens, _lens(lens)) and torch.equal(table, table0)  # not modified
    assert torch.equal(kp, k_want) and torch.equal(vp, v_want)
    assert torch.equal(_slab(kp, table)[0, page - 1:page - 1 + sn], kn[0])
    want = flash_attn_with_kvcache(q, kc, vc, k=kn, v=vn, cache_seqlens=seqlens, causal=True, return_lse=True)
    assert _same(got, want)
    assert torch.equal(_slab(kp, table), kc) and torch.equal(_slab(vp, table), vc)  # kc / vc were appended to as well


@DTYPES
def test_clamping_stays_inside_the_pool(dtype):
    """Table entries just outside [0, num_blocks) on the pages the append and the attention use, and
    lengths of 10^9 and -5: the pools are the middle of sentinel-filled allocations with two blocks
    of margin on each side, and no element of the margins changes.  An unclamped id would land in a
    margin (inside the allocation) and fail the comparison."""
    from fa2_triton_amd import flash_attn_with_paged_kvcache

    page, nb, sn, sentinel = 16, 8, 2, 7.0
    q, _, _ = _data(3, sn, 4, 2, 64, page, dtype)
    _, kn, vn = _data(3, sn, 4, 2, 64, sn, dtype, seed=5)
    k_big = torch.full((nb + 4, page, 2, 64), sentinel, dtype=dtype, device="cuda")
    v_big = torch.full_like(k_big, sentinel)
    kp, vp = k_big[2:2 + nb], v_big[2:2 + nb]
    kp.normal_(0.0, 0.5)
    vp.normal_(0.0, 0.5)
    k0, v0 = kp.clone(), vp.clone()
    # batch 0 appends at positions 15, 16 (pages 0, 1), batch 1 is full (clamped from 10^9) and reads
    # all four pages, batch 2 starts at 0 (clamped from -5) and appends into page 0
    table = torch.tensor([[nb, nb + 1, 3, 4], [-1, nb, nb + 1, 2], [-1, 5, 6, 7]], dtype=torch.int32, device="cuda")
    out, lse = flash_attn_with_paged_kvcache(q, kp, vp, table, _lens((15, 10**9, -5)), k=kn, v=vn, causal=True,
                                             return_lse=True)
    for big in (k_big, v_big):
        assert torch.all(big[:2] == sentinel) and torch.all(big[2 + nb:] == sentinel)
    assert torch.isfinite(out).all() and torch.isfinite(lse).all()
    # the rows went where the clamped ids say: nb, nb + 1 -> nb - 1 and -1 -> 0
    k0[nb - 1, 15], k0[nb - 1, 0], k0[0, 0], k0[0, 1] = kn[0, 0], kn[0, 1], kn[2, 0], kn[2, 1]
    v0[nb - 1, 15], v0[nb - 1, 0], v0[0, 0], v0[0, 1] = vn[0, 0], vn[0, 1], vn[2, 0], vn[2, 1]
    assert torch.equal(kp, k0) and torch.equal(vp, v0)


def test_graph_capture_follows_the_table_and_the_lengths():
    """One paged decode step (append + attention) captured once on a single stream.  Between replays
    the lengths advance in place across a page boundary, the next block id is written into the table
    in place and new q / k / v are copied in: every replay equals a fresh eager call on the same
    state bitwise."""
    from fa2_triton_amd import flash_attn_with_paged_kvcache

    b, hq, hkv, d, page, max_blocks, nb = 2, 16, 4, 128, 16, 8, 20
    dtype = torch.bfloat16
    q, _, _ = _data(b, 1, hq, hkv, d, 1, dtype)
    _, kn, vn = _data(b, 1, hq, hkv, d, 1, dtype, seed=1)
    torch.manual_seed(2)
    kp = torch.empty((nb, page, hkv, d), dtype=dtype, device="cuda").normal_(0.0, 0.5)
    vp = torch.empty((nb, page, hkv, d), dtype=dtype, device="cuda").normal_(0.0, 0.5)
    table = torch.full((b, max_blocks), -7, dtype=torch.int32, device="cuda")  # pages not yet allocated: garbage
    table[0, 0], table[1, 0], table[1, 1] = 11, 4, 17
    seqlens = _lens((14, 30))

    def step(kp_, vp_):
        return flash_attn_with_paged_kvcache(q, kp_, vp_, table, seqlens, k=kn, v=vn, causal=True, return_lse=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(kp, vp)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(kp, vp)

    for it in range(3):
        if it:
            q2, _, _ = _data(b, 1, hq, hkv, d, 1, dtype, seed=10 + it)
            _, k2, v2 = _data(b, 1, hq, hkv, d, 1, dtype, seed=110 + it)
            seqlens += 1  # (15, 31), then (16, 32): the new rows open pages 1 and 2
            if it == 2:
                table[0, 1], table[1, 2] = 2, 9
            q.copy_(q2)
            kn.copy_(k2)
            vn.copy_(v2)
        graph.replay()
        torch.cuda.synchronize()
        kf, vf = kp.clone(), vp.clone()
        fresh = step(kf, vf)
        assert _same(captured, fresh), it
        assert torch.equal(kf, kp) and torch.equal(vf, vp)
    assert seqlens.tolist() == [16, 32]
    assert torch.equal(kp[2, 0], kn[0, 0]) and torch.equal(vp[9, 0], vn[1, 0])  # the rows that opened the new pages


def test_deterministic_and_batch_invariant():
    """Two runs give equal bits, and with the split count forced, batch row b of a B = 4 call equals
    that row run alone (its own table row over the same pool)."""
    from fa2_triton_amd import flash_attn_with_paged_kvcache

    lens = (1000, 3, 513, 64)
    q, kc, vc = _data(4, 2, 16, 4, 128, 1024, torch.bfloat16)
    kp, vp, table, _ = _pool(kc, vc, 16)
    for nsplit in (1, 5):
        kw = dict(causal=True, num_splits=nsplit, return_lse=True)
        a = flash_attn_with_paged_kvcache(q, kp, vp, table, _lens(lens), **kw)
        b = flash_attn_with_paged_kvcache(q, kp, vp, table, _lens(lens), **kw)
        assert _same(a, b)
        for i, n in enumerate(lens):
            one = flash_attn_with_paged_kvcache(q[i:i + 1], kp, vp, table[i:i + 1], _lens((n,)), **kw)
            assert torch.equal(one[0][0], a[0][i]) and torch.equal(one[1][0], a[1][i]), (nsplit, i)


def test_inference_only_and_rejections():
    from fa2_triton_amd import flash_attn_with_paged_kvcache

    q, kc, vc = _data(1, 1, 4, 2, 64, 192, torch.bfloat16)
    kp, vp, table, _ = _pool(kc, vc, 16)
    out = flash_attn_with_paged_kvcache(q.requires_grad_(), kp.requires_grad_(), vp.requires_grad_(), table, 100)
    assert not out.requires_grad and out.grad_fn is None
    kp, vp = kp.detach(), vp.detach()
    with pytest.raises(ValueError, match="power of two"):  # 4 blocks of 48 rows
        flash_attn_with_paged_kvcache(q, kc.reshape(4, 48, 2, 64), vc.reshape(4, 48, 2, 64), table[:, :4], 100)
    with pytest.raises(ValueError, match="power of two"):  # 24 blocks of 8 rows
        flash_attn_with_paged_kvcache(q, kc.reshape(24, 8, 2, 64), vc.reshape(24, 8, 2, 64), table, 100)
    with pytest.raises(TypeError, match="int32"):
        flash_attn_with_paged_kvcache(q, kp, vp, table.long(), 100)
    with pytest.raises(ValueError, match="block_table must be on"):
        flash_attn_with_paged_kvcache(q, kp, vp, table.cpu(), 100)
    with pytest.raises(ValueError, match="block_table"):
        flash_attn_with_paged_kvcache(q, kp, vp, table[:, ::2], 100)  # no unit stride
    with pytest.raises(ValueError, match="block_table"):
        flash_attn_with_paged_kvcache(q, kp, vp, table.expand(2, -1), 100)  # batch of q is 1
    with pytest.raises(TypeError):
        flash_attn_with_paged_kvcache(q, kp, vp, table, None)
