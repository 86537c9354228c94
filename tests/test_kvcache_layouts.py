"""Decode attention (`flash_attn_with_kvcache`, `flash_attn_with_paged_kvcache`, `flash_attn_with_fp8_kvcache`)
on the inputs a serving stack passes in every step and the other decode suites leave out.

A. q, the new rows and the fp8 descales as strided views: slices of one fused QKV projection buffer,
   BHSD storage, a head-dim window of a wider buffer at a 16-byte offset, a stride-0 batch, and the
   descales as a column slice, a transpose and two broadcasts.  Every call on views gives the bits of
   the call on `.contiguous()` copies: `out`, `lse` and, after an append, the caches.  Whatever the
   backing buffers hold outside the views is NaN and reaches nothing.  Rows at an 8-byte offset are
   refused with the library's "16-byte" error and leave the caches alone.
B. Every head dim the kernels accept: the multiples of 8 up to 256 (16-bit caches) and of 16 up to
   128 (fp8).  Most of them fill their head-dim tile (32 / 64 / 128 / 256) only partly; the stagers
   fill the padded 16-byte chunks with copies of the last real chunk, so the result rests on Q being
   loaded as zero there, on the padded output columns never being stored and on the last 4-column
   group of the combine.  16-bit results are held to the oracle by tests/test_kvcache._check and the
   paged call to the contiguous one bitwise; fp8 results to their 16-bit twin (vouched for by the
   same D here) and to the oracle with general descales.  With the caches, q and the new rows as
   views `[..., :D]` of buffers a whole tile wide whose other columns are NaN, nothing past column
   D is read or written.
C. Cache rows at byte offsets past 2^31 and 2^32 (element offsets past 2^31 for 16-bit caches): one
   allocation of 4 - 6 GiB of which only the referenced rows are written.  A block or batch offset
   truncated to 32 bits lands on a lower block or row of the same allocation; those hold NaN.  The
   results are the bits of the same call on a small dense copy, the NaN stays where it was and the
   appended rows are found at their true places.

The shapes are the smallest at which these paths differ: more than one wave-tile of keys (cap 320
and 200), a forced split with a combine beside the direct path, two query rows, GQA.  The
combinations of A and B (entry point, view, dtype, head dim) run as loops inside three cases, by
`each` of tests/test_kvcache_fp8.py, which prints the one it is on: the suite grows by six cases.
"""
import math

import pytest
import torch

from oracle.reference import attention_reference
from tests.test_kvcache import _check, _data, _key_mask, _lens
from tests.test_kvcache_fp8 import POW2_DESCALES, _assert_equals_scaled, _check_dequantised, _paged, _per_head, each, f8
from tests.test_kvcache_fp8 import _data as _data8
from tests.test_kvcache_paged import _pool, _slab

pytestmark = pytest.mark.gpu

BOTH = [torch.bfloat16, torch.float16]
F8 = torch.float8_e4m3fn
NAN = float("nan")
NAN8 = 0x7F  # the e4m3fn NaN
ENTRIES = ("kvcache", "paged", "fp8", "fp8-paged")


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _no_nan(cache):
    """No NaN in a cache: 16-bit values, or e4m3 bytes (uint8)."""
    if cache.dtype == torch.uint8:
        return bool(((cache & 0x7F) != NAN8).all())
    return bool(torch.isfinite(cache).all())


class _Call:
    """One of the four decode calls over caches of its own: [B, cap, Hkv, D] slabs, or pools of pages
    of 16 rows behind a permuted table; 16-bit values or e4m3 bytes (with distinct descales per
    (batch, kv head), none a power of two).  `run` works on fresh copies of the caches."""

    def __init__(self, entry, dtype, d, b, sq, hq, hkv, cap, lens, page=16):
        self.fp8, self.paged, self.lens, self.table = entry.startswith("fp8"), entry.endswith("paged"), lens, None
        self.q, k, v = (_data8 if self.fp8 else _data)(b, sq, hq, hkv, d, cap, dtype)
        if self.paged:
            k, v, self.table, _ = (_paged if self.fp8 else _pool)(k, v, page)
        self.k0, self.v0 = k, v
        self.kd = (0.3 + 0.11 * torch.arange(b * hkv, device="cuda").float()).reshape(b, hkv)
        self.vd = (1.7 - 0.13 * torch.arange(b * hkv, device="cuda").float()).reshape(b, hkv)

    def run(self, q, k=None, v=None, num_splits=0, caches=None, kd=None, vd=None):
        """(out, lse, k_cache, v_cache) of the call, the caches as the call left them."""
        from fa2_triton_amd import flash_attn_with_fp8_kvcache, flash_attn_with_kvcache, flash_attn_with_paged_kvcache

        kc, vc = caches if caches is not None else (self.k0.clone(), self.v0.clone())
        kw = dict(cache_seqlens=_lens(self.lens), causal=True, num_splits=num_splits, return_lse=True)
        if k is not None:
            kw.update(k=k, v=v)
        if self.fp8:
            out, lse = flash_attn_with_fp8_kvcache(q, f8(kc), f8(vc), self.kd if kd is None else kd,
                                                   self.vd if vd is None else vd, block_table=self.table, **kw)
        elif self.paged:
            out, lse = flash_attn_with_paged_kvcache(q, kc, vc, self.table, **kw)
        else:
            out, lse = flash_attn_with_kvcache(q, kc, vc, **kw)
        return out, lse, kc, vc

    def appended(self, sn):
        """bool [slabs, rows]: the cache rows an append of `sn` rows writes."""
        mask = torch.zeros(self.k0.shape[:2], dtype=torch.bool, device="cuda")
        page = self.k0.shape[1]
        for i, n in enumerate(self.lens):
            for pos in range(n, n + sn):
                if self.paged:
                    mask[self.table[i, pos // page].item(), pos % page] = True
                else:
                    mask[i, pos] = True
        return mask


# ---------------------------------------------------------------------------------------------
# A. strided q, new rows and descales
A = dict(b=2, sq=2, hq=8, hkv=2, cap=320, lens=(300, 97))


def _window(t, offset, width):
    """`t` as the columns [offset, offset + D) of a NaN-filled buffer `width` columns wide."""
    buf = torch.full(tuple(t.shape[:-1]) + (width,), NAN, dtype=t.dtype, device=t.device)
    view = buf[..., offset:offset + t.shape[-1]]
    view.copy_(t)
    return buf, view


def _strided(variant, q, kn, vn):
    """Views with the values of q [B, S, Hq, D] and the new rows kn, vn [B, S, Hkv, D], none contiguous."""
    hq, hkv, d = q.shape[2], kn.shape[2], q.shape[3]
    if variant == "fused-qkv":  # one projection buffer [B, S, Hq + 2 Hkv, D]
        buf = torch.cat([q, kn, vn], dim=2)
        views = buf[:, :, :hq], buf[:, :, hq:hq + hkv], buf[:, :, hq + hkv:]
    elif variant == "bhsd":  # stored [B, H, S, D]
        views = tuple(t.transpose(1, 2).contiguous().transpose(1, 2) for t in (q, kn, vn))
    elif variant == "padded-head-dim":  # [..., 8:8 + D] of [..., D + 16]: the pointer moves by 16 bytes
        views = tuple(_window(t, 8, d + 16)[1] for t in (q, kn, vn))
    else:  # every batch row is row 0
        assert variant == "batch-stride-0"
        views = tuple(t[:1].expand(t.shape[0], -1, -1, -1) for t in (q, kn, vn))
        assert all(t.stride(0) == 0 for t in views)
    assert not any(t.is_contiguous() for t in views)
    if variant != "batch-stride-0":
        assert all(torch.equal(t, u) for t, u in zip(views, (q, kn, vn)))
    return views


VARIANTS = [("fused-qkv", 128), ("fused-qkv", 64), ("bhsd", 128), ("padded-head-dim", 128), ("batch-stride-0", 128)]


def _views_give_the_bits_of_copies(entry, variant, head_dim, dtype):
    """`out`, `lse` and the caches after an append are those of the call on contiguous copies, with
    three forced splits (the combine) and the automatic count (one split here); no NaN of the backing
    buffers arrives anywhere and only the appended rows of the caches change."""
    call = _Call(entry, dtype, head_dim, **A)
    sn = A["sq"]
    _, kn, vn = _data(A["b"], sn, A["hq"], A["hkv"], head_dim, sn, dtype, seed=3)
    views = _strided(variant, call.q, kn, vn)
    dense = tuple(t.contiguous() for t in views)
    rows = call.appended(sn)
    for nsplit in (3, 0):
        want, got = call.run(dense[0], num_splits=nsplit), call.run(views[0], num_splits=nsplit)
        assert _same(got, want), (nsplit, (got[0].float() - want[0].float()).abs().max())
        assert torch.equal(got[2], call.k0) and torch.equal(got[3], call.v0)
        want, got = call.run(*dense, num_splits=nsplit), call.run(*views, num_splits=nsplit)
        assert _same(got, want), (nsplit, "append", (got[0].float() - want[0].float()).abs().max())
        assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
        for cache, twin, first in ((got[2], want[2], call.k0), (got[3], want[3], call.v0)):
            assert torch.equal(cache, twin) and _no_nan(cache), nsplit
            assert torch.equal(cache[~rows], first[~rows]) and not torch.equal(cache[rows], first[rows]), nsplit


def _descale_views_give_the_bits_of_copies(entry, dtype):
    """k_descale / v_descale as a column slice of a wider tensor, the transpose of an [Hkv, B] tensor
    and the two broadcasts give the bits of the materialised contiguous [B, Hkv] tensor: the attention
    and the bytes the append quantises.  The values are distinct and no powers of two, and what lies
    around the slice is NaN."""
    b, hkv = A["b"], A["hkv"]
    call = _Call(entry, dtype, 128, **A)
    _, kn, vn = _data(b, A["sq"], A["hq"], hkv, 128, A["sq"], dtype, seed=3)

    def forms(full):  # full: [B, Hkv]
        wide = torch.full((b, hkv + 3), NAN, device="cuda")
        wide[:, 2:2 + hkv] = full
        return {"column-slice": wide[:, 2:2 + hkv], "transposed": full.T.contiguous().T,
                "per-head": full[1:2].clone(), "per-batch": full[:, 1:2].clone()}

    k_forms, v_forms = forms(call.kd), forms(call.vd)
    assert k_forms["column-slice"].stride() == (hkv + 3, 1) and k_forms["transposed"].stride() == (1, b)
    for name in k_forms:
        kd, vd = k_forms[name], v_forms[name]
        kd_c, vd_c = kd.expand(b, hkv).contiguous(), vd.expand(b, hkv).contiguous()
        assert len(set(kd_c.flatten().tolist())) >= 2 and all(math.log2(x) % 1 for x in kd_c.flatten().tolist())
        for nsplit in (3, 0):
            want = call.run(call.q, kn, vn, num_splits=nsplit, kd=kd_c, vd=vd_c)
            got = call.run(call.q, kn, vn, num_splits=nsplit, kd=kd, vd=vd)
            assert _same(got, want), (name, nsplit)
            assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3]), (name, nsplit)
        # (the bytes are the definition's: the new rows quantised with their (batch, kv head)'s descale)
        kq, vq = _per_head(kn, kd_c), _per_head(vn, vd_c)
        k_slab, v_slab = (_slab(c, call.table) if call.paged else c for c in got[2:])
        for i, n in enumerate(A["lens"]):
            assert torch.equal(k_slab[i, n:n + A["sq"]], kq[i]) and torch.equal(v_slab[i, n:n + A["sq"]], vq[i]), (name, i)


def _rows_at_an_8_byte_offset_are_refused(entry):
    """q, k or v as the columns [4, 4 + D) of a wider buffer: rows 8-byte aligned.  The library's
    "16-byte" unsupported error, before anything is written."""
    d, dtype = 128, torch.bfloat16
    call = _Call(entry, dtype, d, **A)
    _, kn, vn = _data(A["b"], A["sq"], A["hq"], A["hkv"], d, A["sq"], dtype, seed=3)
    for which in ("q", "k", "v"):
        q_, k_, v_ = (_window(t, 4 if name == which else 8, d + 16)[1] for name, t in (("q", call.q), ("k", kn), ("v", vn)))
        caches = call.k0.clone(), call.v0.clone()
        with pytest.raises(NotImplementedError, match="16-byte"):
            call.run(q_, k_, v_, caches=caches)
        if which == "q":
            with pytest.raises(NotImplementedError, match="16-byte"):
                call.run(q_, caches=caches)
        torch.cuda.synchronize()
        assert torch.equal(caches[0], call.k0) and torch.equal(caches[1], call.v0), which
    call.run(*(_window(t, 8, d + 16)[1] for t in (call.q, kn, vn)))  # at 16 bytes the same views are taken


@each(entry=ENTRIES, dtype=BOTH)
def test_strided_q_new_rows_and_descales(entry, dtype):
    """Part A for one entry point and dtype (the combinations run inside one case and are printed):
    every view variant, for the fp8 calls the descale views, and the refusal of 8-byte rows."""
    for variant, head_dim in VARIANTS:
        print(" ", variant, head_dim)
        _views_give_the_bits_of_copies(entry, variant, head_dim, dtype)
    if entry.startswith("fp8"):
        _descale_views_give_the_bits_of_copies(entry, dtype)
    if dtype == torch.bfloat16:
        _rows_at_an_8_byte_offset_are_refused(entry)


# ---------------------------------------------------------------------------------------------
# B. every head dim
HB = dict(b=2, sq=2, hq=4, hkv=2, cap=200, lens=(200, 67))
PAGE = 16


def _padded_to_pages(k, v, page=PAGE):
    """The slabs with zero rows up to a whole number of pages (the capacity a paged twin has)."""
    b, cap, hkv, d = k.shape
    zeros = torch.zeros((b, -cap % page, hkv, d), dtype=k.dtype, device="cuda")
    return torch.cat([k, zeros], 1), torch.cat([v, zeros], 1)


def _head_dim_against_the_oracle(head_dim, dtype):
    """Every multiple of 8 up to 256, direct and with two splits: the contiguous call by the project's
    rule against the oracle (no escape taken) and the LSE2 rule; the paged call at P = 16 equal to the
    contiguous one bit for bit, also when one new row is appended first (and that call against the
    oracle on the cache it left)."""
    from fa2_triton_amd import flash_attn_with_kvcache, flash_attn_with_paged_kvcache

    b, sq, hq, hkv, cap, lens = (HB[key] for key in ("b", "sq", "hq", "hkv", "cap", "lens"))
    q, kc, vc = _data(b, sq, hq, hkv, head_dim, cap, dtype)
    _, kn, vn = _data(b, 1, hq, hkv, head_dim, 1, dtype, seed=3)
    ks, vs = _padded_to_pages(kc, vc)
    kp, vp, table, _ = _pool(ks, vs, PAGE)
    for nsplit in (1, 2):
        kw = dict(cache_seqlens=_lens(lens), causal=True, num_splits=nsplit, return_lse=True)
        out, lse = flash_attn_with_kvcache(q, kc, vc, **kw)
        _check(q, kc, vc, lens, out, lse, True, (-1, -1))
        assert _same(flash_attn_with_kvcache(q, ks, vs, **kw), (out, lse)), nsplit
        assert _same(flash_attn_with_paged_kvcache(q, kp, vp, table, **kw), (out, lse)), nsplit
        ks2, vs2, kp2, vp2 = ks.clone(), vs.clone(), kp.clone(), vp.clone()
        want = flash_attn_with_kvcache(q, ks2, vs2, k=kn, v=vn, **kw)
        got = flash_attn_with_paged_kvcache(q, kp2, vp2, table, k=kn, v=vn, **kw)
        assert _same(got, want), (nsplit, "append")
        assert torch.equal(_slab(kp2, table), ks2) and torch.equal(_slab(vp2, table), vs2)
        for i, n in enumerate(lens):
            assert torch.equal(ks2[i, n], kn[i, 0]) and torch.equal(vs2[i, n], vn[i, 0])
            ks2[i, n], vs2[i, n] = ks[i, n], vs[i, n]
        assert torch.equal(ks2, ks) and torch.equal(vs2, vs)  # nothing else was written
        if nsplit == 2:
            for i, n in enumerate(lens):
                ks2[i, n], vs2[i, n] = kn[i, 0], vn[i, 0]
            _check(q, ks2, vs2, tuple(n + 1 for n in lens), want[0], want[1], True, (-1, -1))


@each(dtype=BOTH, head_dim=list(range(16, 129, 16)))
def test_every_fp8_head_dim(dtype, head_dim):
    """Every multiple of 16 up to 128.  Power-of-two descales: the bits of the 16-bit call on the
    upcast cache (the relation of tests/test_kvcache_fp8.py; that call is held to the oracle at the
    same D above).  General descales per (batch, kv head): the project's rule against the oracle on
    the dequantised values, and the bytes a one-row append writes."""
    from fa2_triton_amd import flash_attn_with_fp8_kvcache, flash_attn_with_kvcache, flash_attn_with_paged_kvcache

    b, sq, hq, hkv, cap, lens = (HB[key] for key in ("b", "sq", "hq", "hkv", "cap", "lens"))
    q, k8, v8 = _data8(b, sq, hq, hkv, head_dim, cap, dtype)
    kp, vp, table, _ = _paged(k8, v8, PAGE)
    s = 1.0 / math.sqrt(head_dim)
    for (kd, vd), nsplit in ((x, n) for x in POW2_DESCALES for n in (1, 2)):
        kw = dict(cache_seqlens=_lens(lens), causal=True, num_splits=nsplit, return_lse=True)
        want = flash_attn_with_kvcache(q, f8(k8).to(dtype), f8(v8).to(dtype), softmax_scale=s * kd, **kw)
        got = flash_attn_with_fp8_kvcache(q, f8(k8), f8(v8), kd, vd, **kw)
        _assert_equals_scaled(got[0], want[0], vd, (kd, vd, nsplit))
        assert torch.equal(got[1], want[1]), (kd, vd, nsplit)
        want = flash_attn_with_paged_kvcache(q, f8(kp).to(dtype), f8(vp).to(dtype), table, softmax_scale=s * kd, **kw)
        got = flash_attn_with_fp8_kvcache(q, f8(kp), f8(vp), kd, vd, block_table=table, **kw)
        _assert_equals_scaled(got[0], want[0], vd, (kd, vd, nsplit, "paged"))
        assert torch.equal(got[1], want[1]), (kd, vd, nsplit, "paged")

    kd = (0.3 + 0.11 * torch.arange(b * hkv, device="cuda").float()).reshape(b, hkv)
    vd = (1.7 - 0.13 * torch.arange(b * hkv, device="cuda").float()).reshape(b, hkv)
    kf, vf = f8(k8).float() * kd[:, None, :, None], f8(v8).float() * vd[:, None, :, None]
    common = dict(key_padding_mask=_key_mask(lens, cap), causal=True, window_size=(-1, -1))
    ref = attention_reference(q, kf, vf, **common)
    pt = attention_reference(q, kf.to(dtype), vf.to(dtype), upcast=False, reorder_ops=True, **common)
    for nsplit in (1, 2):
        kw = dict(cache_seqlens=_lens(lens), causal=True, num_splits=nsplit, return_lse=True)
        out, lse = flash_attn_with_fp8_kvcache(q, f8(k8), f8(v8), kd, vd, **kw)
        _check_dequantised(q, kf, vf, lens, out, lse, ref, pt, True, (-1, -1))
        out, lse = flash_attn_with_fp8_kvcache(q, f8(kp), f8(vp), kd, vd, block_table=table, **kw)
        _check_dequantised(q, kf, vf, lens, out, lse, ref, pt, True, (-1, -1))
    # one new row through both layouts (the slab padded to the pool's capacity, so that neither drops it)
    _, kn, vn = _data(b, 1, hq, hkv, head_dim, 1, dtype, seed=3)
    ks, vs = _padded_to_pages(k8, v8)
    ks2, vs2, kp2, vp2 = ks.clone(), vs.clone(), kp.clone(), vp.clone()
    kw = dict(cache_seqlens=_lens(lens), causal=True, k=kn, v=vn, return_lse=True)
    want = flash_attn_with_fp8_kvcache(q, f8(ks2), f8(vs2), kd, vd, **kw)
    got = flash_attn_with_fp8_kvcache(q, f8(kp2), f8(vp2), kd, vd, block_table=table, **kw)
    assert _same(got, want)
    assert torch.equal(_slab(kp2, table), ks2) and torch.equal(_slab(vp2, table), vs2)
    kq, vq = _per_head(kn, kd), _per_head(vn, vd)
    for i, n in enumerate(lens):
        assert torch.equal(ks2[i, n], kq[i, 0]) and torch.equal(vs2[i, n], vq[i, 0])
        ks2[i, n], vs2[i, n] = ks[i, n], vs[i, n]
    assert torch.equal(ks2, ks) and torch.equal(vs2, vs)


def _tile(d):
    """The head-dim tile of the 16-bit kernels (select.h: head_dim_tile)."""
    return next(t for t in (32, 64, 128, 256) if d <= t)


def _nothing_past_column_d_is_read(head_dim, dtype):
    """The caches (slabs and pools), q and the new rows are the columns [0, D) of buffers a whole
    head-dim tile wide whose columns [D, tile) hold NaN: the neighbour of every padded chunk.  `out`,
    `lse` and the appended rows are those of the dense call, and the pad is still all NaN."""
    from fa2_triton_amd import flash_attn_with_kvcache, flash_attn_with_paged_kvcache

    b, sq, hq, hkv, cap, lens = (HB[key] for key in ("b", "sq", "hq", "hkv", "cap", "lens"))
    d, width = head_dim, _tile(head_dim)
    q, kc, vc = _data(b, sq, hq, hkv, d, cap, dtype)
    _, kn, vn = _data(b, 1, hq, hkv, d, 1, dtype, seed=3)
    ks, vs = _padded_to_pages(kc, vc)
    kp, vp, table, _ = _pool(ks, vs, PAGE)
    for nsplit in (1, 2):
        kw = dict(cache_seqlens=_lens(lens), causal=True, num_splits=nsplit, return_lse=True)
        (_, q_), (_, kn_), (_, vn_) = (_window(t, 0, width) for t in (q, kn, vn))
        for fn, tab, dense in ((flash_attn_with_kvcache, (), (ks, vs)), (flash_attn_with_paged_kvcache, (table,), (kp, vp))):
            (k_buf, k_), (v_buf, v_) = (_window(t, 0, width) for t in dense)
            assert k_.stride(2) == width and not k_.is_contiguous()
            assert _same(fn(q_, k_, v_, *tab, **kw), fn(q, *dense, *tab, **kw)), nsplit
            k2, v2 = dense[0].clone(), dense[1].clone()
            assert _same(fn(q_, k_, v_, *tab, k=kn_, v=vn_, **kw), fn(q, k2, v2, *tab, k=kn, v=vn, **kw)), (nsplit, "append")
            assert torch.equal(k_, k2) and torch.equal(v_, v2) and not torch.equal(k2, dense[0])
            assert torch.isnan(k_buf[..., d:]).all() and torch.isnan(v_buf[..., d:]).all()


@each(dtype=BOTH, head_dim=list(range(8, 257, 8)))
def test_every_head_dim(dtype, head_dim):
    """Part B for 16-bit caches (the head dims run inside one case and are printed): every multiple
    of 8 against the oracle and the paged twin, and at the head dims whose last 32-column sub-tile is
    only partly real, one per tile size and position, the NaN neighbour."""
    _head_dim_against_the_oracle(head_dim, dtype)
    if head_dim in (8, 40, 72, 104, 136, 200, 248):
        _nothing_past_column_d_is_read(head_dim, dtype)


# ---------------------------------------------------------------------------------------------
# C. rows beyond 4 GiB
def _need(nbytes):
    free, _ = torch.cuda.mem_get_info()
    if free < 3 * nbytes:
        pytest.skip(f"{free / 2**30:.1f} GiB free on the device, this test wants 3 x {nbytes / 2**30:.1f} GiB")


def _values(shape, dtype, fp8, seed):
    torch.manual_seed(seed)
    x = torch.empty(shape, device="cuda").normal_()
    return x.to(F8).view(torch.uint8) if fp8 else (0.5 * x).to(dtype)


def _poison(t, fp8):
    t.fill_(NAN8 if fp8 else NAN)


def _poisoned(t, fp8):
    return bool((t == NAN8).all() if fp8 else torch.isnan(t).all())


def _decode(fp8, q, kc, vc, kd, vd, **kw):
    from fa2_triton_amd import flash_attn_with_fp8_kvcache, flash_attn_with_kvcache, flash_attn_with_paged_kvcache

    if fp8:
        return flash_attn_with_fp8_kvcache(q, f8(kc), f8(vc), kd, vd, **kw)
    if "block_table" in kw:
        return flash_attn_with_paged_kvcache(q, kc, vc, kw.pop("block_table"), **kw)
    return flash_attn_with_kvcache(q, kc, vc, **kw)


def _pool_beyond(dtype, fp8):
    """Pools k = big[:, 0], v = big[:, 1] of one buffer [N, 2, P, Hkv, D] (never filled as a whole) whose
    last blocks lie past byte offset 2^32.  The table names blocks on both sides of every 32-bit
    threshold (byte offset 2^32, which is element offset 2^31 for 16-bit caches; for byte caches also
    2^31), block 0 and block N - 1; the appended rows land past a threshold each.  `wrapped`: the
    blocks a named block's offset would come down to mod 2^31 or 2^32 bytes -- NaN, unless the table
    names them as well (block 0 is the wrap of the block that starts at the threshold: there equal
    bits with the dense twin, whose blocks all differ, are the check)."""
    page, hkv, d, hq, b = 16, 2, 128, 8, 2
    esize = 1 if fp8 else 2
    stride = 2 * page * hkv * d  # elements from block to block: K and V blocks alternate
    marks = [2**31 // stride, 2**32 // stride] if fp8 else [2**32 // (stride * esize)]
    n = marks[-1] + 8
    _need(n * stride * esize)
    big = torch.empty(n * stride, dtype=torch.uint8 if fp8 else dtype, device="cuda").view(n, 2, page, hkv, d)
    kp, vp = big[:, 0], big[:, 1]
    assert kp.stride(0) == stride and (n - 1) * stride * esize > 2**32 and kp.shape == (n, page, hkv, d)
    if fp8:
        lo, hi = marks
        blocks, lens = [[0, lo - 1, lo, lo + 1], [n - 1, hi - 1, hi, hi + 1]], (56, 49)
    else:
        (hi,) = marks
        blocks, lens = [[hi - 1, hi, hi + 1], [n - 1, 0, hi + 2]], (40, 33)
    named = sorted({x for row in blocks for x in row})
    wrapped = sorted({x % m for x in named for m in marks if x >= m} - set(named))
    assert wrapped and all(blocks[i][lens[i] // page] > marks[min(i, len(marks) - 1)] for i in range(b))  # where the new rows go
    ks, vs = _values((len(named), page, hkv, d), dtype, fp8, 1), _values((len(named), page, hkv, d), dtype, fp8, 2)
    for i, x in enumerate(named):
        kp[x].copy_(ks[i])
        vp[x].copy_(vs[i])
    for x in wrapped:
        _poison(big[x], fp8)
    table = torch.tensor(blocks, dtype=torch.int32, device="cuda")
    small = torch.tensor([[named.index(x) for x in row] for row in blocks], dtype=torch.int32, device="cuda")
    q = _data(b, 1, hq, hkv, d, 1, dtype)[0]
    _, kn, vn = _data(b, 1, hq, hkv, d, 1, dtype, seed=3)
    kd = torch.tensor([[0.7, 0.3], [1.3, 0.9]], device="cuda") if fp8 else None
    vd = torch.tensor([[1.1, 0.6], [0.4, 1.9]], device="cuda") if fp8 else None
    for nsplit in (0, 2):
        kw = dict(cache_seqlens=_lens(lens), causal=True, num_splits=nsplit, return_lse=True)
        want = _decode(fp8, q, ks, vs, kd, vd, block_table=small, **kw)
        got = _decode(fp8, q, kp, vp, kd, vd, block_table=table, **kw)
        assert _same(got, want) and torch.isfinite(got[0]).all(), nsplit
    k_first = ks.clone()
    want = _decode(fp8, q, ks, vs, kd, vd, block_table=small, k=kn, v=vn, **kw)
    got = _decode(fp8, q, kp, vp, kd, vd, block_table=table, k=kn, v=vn, **kw)
    assert _same(got, want) and torch.isfinite(got[0]).all()
    assert not torch.equal(ks, k_first)
    for i, x in enumerate(named):  # the new rows are in their true blocks, and no named block changed otherwise
        assert torch.equal(kp[x], ks[i]) and torch.equal(vp[x], vs[i]), x
    for i in range(b):
        x, row = blocks[i][lens[i] // page], lens[i] % page
        new = (_per_head(kn, kd)[i, 0], _per_head(vn, vd)[i, 0]) if fp8 else (kn[i, 0], vn[i, 0])
        assert torch.equal(kp[x, row], new[0]) and torch.equal(vp[x, row], new[1]), x
    assert all(_poisoned(big[x], fp8) for x in wrapped)


def _slab_beyond(dtype, fp8):
    """Caches k = big[:, :cap], v = big[:, cap:2 cap] of one buffer [3, R, Hkv, D] (never filled as a
    whole) whose batch stride is 2^31 bytes and 512 rows, so that batch 1 starts past byte offset 2^31
    and batch 2 past 2^32 (element offset 2^31 for 16-bit caches).  An offset of batch 1 or 2 cut to
    31 or 32 bits comes down in batch 0 at rows 512 or 1024: NaN there."""
    b, cap, hkv, d, hq, lens = 3, 128, 2, 128, 8, (100, 37, 64)
    row_bytes = hkv * d * (1 if fp8 else 2)
    r = 2**31 // row_bytes + 512
    _need(b * r * row_bytes)
    big = torch.empty((b, r, hkv, d), dtype=torch.uint8 if fp8 else dtype, device="cuda")
    kc, vc = big[:, :cap], big[:, cap:2 * cap]
    assert kc.stride(0) * kc.element_size() > 2**31 and 2 * kc.stride(0) * kc.element_size() > 2**32
    wrapped = sorted({(i * r * row_bytes) % m // row_bytes for i in (1, 2) for m in (2**31, 2**32) if i * r * row_bytes >= m})
    assert wrapped == [512, 1024]
    ks, vs = _values((b, cap, hkv, d), dtype, fp8, 1), _values((b, cap, hkv, d), dtype, fp8, 2)
    kc.copy_(ks)
    vc.copy_(vs)
    for x in wrapped:
        _poison(big[0, x:x + 2 * cap], fp8)
    q = _data(b, 1, hq, hkv, d, 1, dtype)[0]
    _, kn, vn = _data(b, 1, hq, hkv, d, 1, dtype, seed=3)
    kd = torch.tensor([[0.7, 0.3], [1.3, 0.9], [0.45, 2.1]], device="cuda") if fp8 else None
    vd = torch.tensor([[1.1, 0.6], [0.4, 1.9], [0.75, 1.4]], device="cuda") if fp8 else None
    for nsplit in (0, 2):
        kw = dict(cache_seqlens=_lens(lens), causal=True, num_splits=nsplit, return_lse=True)
        assert _same(_decode(fp8, q, kc, vc, kd, vd, **kw), _decode(fp8, q, ks, vs, kd, vd, **kw)), nsplit
    want = _decode(fp8, q, ks, vs, kd, vd, k=kn, v=vn, **kw)
    got = _decode(fp8, q, kc, vc, kd, vd, k=kn, v=vn, **kw)
    assert _same(got, want) and torch.isfinite(got[0]).all()
    assert torch.equal(kc, ks) and torch.equal(vc, vs)
    for i, n in enumerate(lens):
        new = (_per_head(kn, kd)[i, 0], _per_head(vn, vd)[i, 0]) if fp8 else (kn[i, 0], vn[i, 0])
        assert torch.equal(kc[i, n], new[0]) and torch.equal(vc[i, n], new[1]), i
    assert all(_poisoned(big[0, x:x + 2 * cap], fp8) for x in wrapped)


def _release(fn, *args):
    try:
        fn(*args)
    finally:
        torch.cuda.empty_cache()  # hand the allocation back: the rest of the suite does not need it cached


def test_paged_pool_beyond_4_gib():
    _release(_pool_beyond, torch.bfloat16, False)


def test_contiguous_cache_beyond_4_gib():
    _release(_slab_beyond, torch.float16, False)


@each(layout=["contiguous", "paged"])
def test_fp8_cache_beyond_4_gib(layout):
    _release(_pool_beyond if layout == "paged" else _slab_beyond, torch.bfloat16, True)
