"""fp8 (e4m3fn) KV caches on the GPU (`flash_attn_with_fp8_kvcache`, fa2_fwd_kvcache_fp8).

The yardstick is bitwise: a cache element's value is its exact e4m3 value, which bf16 and fp16 hold
exactly, so with descales that are uniform powers of two `out` and `lse` are the bits of the 16-bit
call on the upcast cache with softmax_scale * k_descale, times v_descale -- contiguous and paged,
forced and automatic splits.  Before that, exact small-integer data (one-hot probabilities, integer
V) pins the byte order of the K fragments and of the even / odd V^T route.  Around it: general
descales against the oracle, the quantising append over every 16-bit input pattern, its placement
and bounds, what is never read, layouts, determinism, batch invariance and graph capture.

The caches are built as uint8 tensors and viewed as float8_e4m3fn for the call.
"""
import functools
import inspect
import itertools
import math

import pytest
import torch

from oracle import tolerance
from oracle.reference import attention_reference
from oracle.tolerance import check_fa_tolerance
from tests.test_kvcache import CASES as BASE_CASES
from tests.test_kvcache import _key_mask, _lens, _lse2
from tests.test_kvcache_paged import _pool

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
NAN8 = 0x7F  # the e4m3fn NaN


def each(**values):
    """Run the test body for every combination of the named arguments inside one test case (the
    combination is printed, so a failure names it): the suite grows by one case, not by the product."""
    def wrap(fn):
        @functools.wraps(fn)
        def run(*args, **kw):
            for combo in itertools.product(*values.values()):
                print(fn.__name__, dict(zip(values, combo)))
                fn(*args, **kw, **dict(zip(values, combo)))
        del run.__wrapped__  # pytest reads the signature below, without the looped arguments
        sig = inspect.signature(fn)
        run.__signature__ = sig.replace(parameters=[p for n, p in sig.parameters.items() if n not in values])
        return run
    return wrap


DTYPES = each(dtype=[torch.bfloat16, torch.float16])


def f8(u8):
    return u8.view(F8)


def _data(b, sq, hq, hkv, d, cap, dtype, seed=0):
    """q in `dtype` and the two caches as e4m3 bytes (uint8) of N(0, 1) values."""
    torch.manual_seed(seed)
    q = torch.empty((b, sq, hq, d), dtype=dtype, device="cuda").normal_(0.0, 0.5)
    k8 = torch.empty((b, cap, hkv, d), device="cuda").normal_().to(F8).view(torch.uint8)
    v8 = torch.empty((b, cap, hkv, d), device="cuda").normal_().to(F8).view(torch.uint8)
    return q, k8, v8


def _paged(k8, v8, page):
    """Pools and a permuted table for the slabs, zero-padded to a whole number of pages."""
    b, cap, hkv, d = k8.shape
    pad = -cap % page
    if pad:
        zeros = torch.zeros((b, pad, hkv, d), dtype=torch.uint8, device="cuda")
        k8, v8 = torch.cat([k8, zeros], 1), torch.cat([v8, zeros], 1)
    return _pool(k8, v8, page)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _assert_equals_scaled(got, want, vd, what):
    """got == want * vd bit for bit, vd a power of two.  The fp8 call rounds O * vd once; `want * vd`
    is round(O) * vd.  Rounding commutes with a power of two only inside the normal range: where
    round(O) or the product is subnormal (fp16 outputs below 6.1e-5, and that over vd) one of the two
    sides was rounded at the fixed subnormal spacing and the other was not.  There -- rare, and
    counted -- they may differ by that spacing (times vd when vd > 1), the most the extra rounding
    can do; everywhere else every bit agrees."""
    tiny = torch.finfo(got.dtype).smallest_normal
    normal = (want.float().abs() >= tiny) & ((want.float() * vd).abs() >= tiny)
    assert torch.equal(got[normal], (want * vd)[normal]), (what, (got.float() - want.float() * vd)[normal].abs().max())
    assert normal[want != 0].float().mean() > 0.98, (what, normal.float().mean())  # (rows without keys are exact zeros)
    spacing = tiny * 2.0 ** -(10 if got.dtype == torch.float16 else 7) * max(1.0, vd)
    assert ((got.float() - want.float() * vd)[~normal].abs() <= spacing).all(), what


# ---------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("head_dim", [64, 128])
def test_exact_small_integers(head_dim, dtype):
    """K rows are +-2 codes of the key index in 8 columns (at a per-head column offset), q is 32 x the
    code of one target key per row and softmax_scale = 1: the target's score leads by >= 128, every
    other probability underflows to an exact 0 and O is the target's V row, integers in [-8, 8].
    A permuted byte, column or key anywhere on the K or V route picks other integers."""
    from fa2_triton_amd import flash_attn_with_fp8_kvcache

    b, sq, hq, hkv, cap, lens = 2, 2, 8, 4, 256, (200, 77)
    offs = [0, 24, head_dim - 24, head_dim - 8]
    gen = torch.Generator().manual_seed(0)
    code = lambda j: torch.tensor([2.0 if (j >> i) & 1 else -2.0 for i in range(8)])
    k = torch.zeros(b, cap, hkv, head_dim)
    for j in range(cap):
        for h in range(hkv):
            k[:, j, h, offs[h]:offs[h] + 8] = code(j)
    v = torch.randint(-8, 9, (b, cap, hkv, head_dim), generator=gen).float()
    q = torch.zeros(b, sq, hq, head_dim)
    want = torch.zeros(b, sq, hq, head_dim)
    for bi in range(b):
        for i in range(sq):
            for h in range(hq):
                j = int(torch.randint(0, lens[bi], (1,), generator=gen))
                q[bi, i, h, offs[h // 2]:offs[h // 2] + 8] = 16.0 * code(j)
                want[bi, i, h] = v[bi, j, h // 2]
    q, want = q.to(dtype).cuda(), want.to(dtype).cuda()
    k8, v8 = k.to(F8).view(torch.uint8).cuda(), v.to(F8).view(torch.uint8).cuda()
    assert torch.equal(f8(v8).float().cpu(), v)  # the integers are e4m3 values
    kp, vp, table, _ = _paged(k8, v8, 16)
    for nsplit in (1, 3):
        kw = dict(cache_seqlens=_lens(lens), softmax_scale=1.0, num_splits=nsplit)
        out = flash_attn_with_fp8_kvcache(q, f8(k8), f8(v8), **kw)
        assert torch.equal(out, want), (nsplit, (out.float() - want.float()).abs().max())
        out = flash_attn_with_fp8_kvcache(q, f8(kp), f8(vp), block_table=table, **kw)
        assert torch.equal(out, want), (nsplit, "paged")


# ---------------------------------------------------------------------------------------------
# (B, Hq, Hkv, Sq, cap, D, lengths, causal, window, num_splits): tests/test_kvcache.py's with D <= 128,
# a second padded tile (D = 48) and a batch row without keys
CASES = {name: c for name, c in BASE_CASES.items() if c[5] <= 128}
CASES["d48"] = (2, 8, 2, 2, 300, 48, (300, 131), True, (-1, -1), 2)
CASES["length-zero-splits3"] = (2, 8, 2, 2, 256, 128, (0, 200), False, (-1, -1), 3)
POW2_DESCALES = [(1.0, 1.0), (0.5, 2.0), (4.0, 0.25)]


@DTYPES
@pytest.mark.parametrize("case", sorted(CASES))
def test_bitwise_equal_to_the_16_bit_call_on_the_upcast_cache(case, dtype):
    from fa2_triton_amd import flash_attn_with_fp8_kvcache, flash_attn_with_kvcache, flash_attn_with_paged_kvcache

    b, hq, hkv, sq, cap, d, lens, causal, window, nsplit = CASES[case]
    q, k8, v8 = _data(b, sq, hq, hkv, d, cap, dtype)
    assert {"d48", "d96", "window-100-causal", "window-30-10-sq4", "rows-without-keys"} <= set(CASES)
    s = 1.0 / math.sqrt(d)
    pools = {page: _paged(k8, v8, page) for page in (16, 64, 256)}
    for kd, vd in POW2_DESCALES:
        for n in sorted({nsplit, 0}):
            kw = dict(cache_seqlens=_lens(lens), causal=causal, window_size=window, num_splits=n, return_lse=True)
            want = flash_attn_with_kvcache(q, f8(k8).to(dtype), f8(v8).to(dtype), softmax_scale=s * kd, **kw)
            got = flash_attn_with_fp8_kvcache(q, f8(k8), f8(v8), kd, vd, **kw)
            _assert_equals_scaled(got[0], want[0], vd, (kd, vd, n))
            assert torch.equal(got[1], want[1]), (kd, vd, n)
            for page, (kp, vp, table, _) in pools.items():
                want = flash_attn_with_paged_kvcache(q, f8(kp).to(dtype), f8(vp).to(dtype), table, softmax_scale=s * kd, **kw)
                got = flash_attn_with_fp8_kvcache(q, f8(kp), f8(vp), kd, vd, block_table=table, **kw)
                _assert_equals_scaled(got[0], want[0], vd, (kd, vd, n, page))
                assert torch.equal(got[1], want[1]), (kd, vd, n, page)
    if case in ("rows-without-keys", "length-zero-splits3"):
        empty = (got[1] == float("-inf"))
        assert empty.any() and torch.count_nonzero(got[0].transpose(1, 2)[empty]) == 0
    # descales given as device tensors (uniform, one an expanded view) are the same call
    kd_t = torch.full((b, hkv), 0.5, device="cuda")
    vd_t = torch.full((1, 1), 2.0, device="cuda").expand(b, hkv)
    kw = dict(cache_seqlens=_lens(lens), causal=causal, window_size=window, num_splits=nsplit, return_lse=True)
    assert _same(flash_attn_with_fp8_kvcache(q, f8(k8), f8(v8), kd_t, vd_t, **kw),
                 flash_attn_with_fp8_kvcache(q, f8(k8), f8(v8), 0.5, 2.0, **kw))


# ---------------------------------------------------------------------------------------------
def _check_dequantised(q, kf, vf, lens, out, lse, ref, pt, causal, window):
    """The project's rule for an fp8 call with general descales (2 x the low-precision oracle's error
    + 5e-5, no escape taken) against the oracle outputs `ref`, `pt` on the dequantised kf, vf, and
    LSE2 as tests/test_kvcache.py.  (shared with tests/test_kvcache_layouts.py)"""
    before = dict(tolerance.ESCAPES)
    report = check_fa_tolerance(q, kf, vf, None, out, ref, pt, out_error_mul=2, out_error_bias=5e-5)
    print({key: f"{val:.3e}" for key, val in report.items()})
    assert tolerance.ESCAPES["ulp"] == before["ulp"] and tolerance.ESCAPES["dv_sum"] == before["dv_sum"], report
    assert out.dtype == q.dtype and torch.isfinite(out).all()
    want = _lse2(q, kf, lens, causal, window)
    finite = torch.isfinite(want)
    assert torch.allclose(lse[finite], want[finite], rtol=1e-3, atol=1e-3), (lse[finite] - want[finite]).abs().max()
    assert torch.all(torch.isneginf(lse[~finite]))


@DTYPES
@pytest.mark.parametrize("case", ["gqa-32x8-splits4", "two-row-tiles-causal", "d96", "window-30-10-sq4"])
def test_general_descales_against_the_oracle(case, dtype):
    """Distinct descales per (batch, kv head), none a power of two.  ref: the fp32 oracle on the
    dequantised values float(k8) * kd, float(v8) * vd; pt: the low-precision reordered oracle on those
    values rounded to q's dtype.  The project's rule, no escape taken; LSE2 as tests/test_kvcache.py."""
    from fa2_triton_amd import flash_attn_with_fp8_kvcache

    b, hq, hkv, sq, cap, d, lens, causal, window, nsplit = CASES[case]
    q, k8, v8 = _data(b, sq, hq, hkv, d, cap, dtype)
    kd = (0.3 + 0.11 * torch.arange(b * hkv, device="cuda").float()).reshape(b, hkv)
    vd = (1.7 - 0.13 * torch.arange(b * hkv, device="cuda").float()).reshape(b, hkv)
    kf, vf = f8(k8).float() * kd[:, None, :, None], f8(v8).float() * vd[:, None, :, None]
    common = dict(key_padding_mask=_key_mask(lens, cap), causal=causal, window_size=window)
    ref = attention_reference(q, kf, vf, **common)
    pt = attention_reference(q, kf.to(dtype), vf.to(dtype), upcast=False, reorder_ops=True, **common)
    kp, vp, table, _ = _paged(k8, v8, 16)
    for paged in (False, True):
        kw = dict(cache_seqlens=_lens(lens), causal=causal, window_size=window, num_splits=nsplit, return_lse=True)
        if paged:
            out, lse = flash_attn_with_fp8_kvcache(q, f8(kp), f8(vp), kd, vd, block_table=table, **kw)
        else:
            out, lse = flash_attn_with_fp8_kvcache(q, f8(k8), f8(v8), kd, vd, **kw)
        _check_dequantised(q, kf, vf, lens, out, lse, ref, pt, causal, window)


# ---------------------------------------------------------------------------------------------
def _quantise_cpu(x, d):
    """The definition, by torch on the CPU: e4m3_rne(clamp(float(x) / d, -448, 448)) as bytes."""
    return (x.float().cpu() / d).clamp(-448, 448).to(F8).view(torch.uint8)


def _assert_bytes(got, want, what):
    """Equal bytes; where the definition gives NaN (0x7f / 0xff), any NaN byte."""
    got, want = got.cpu(), want.cpu()
    nan = (want & 0x7F) == NAN8
    assert torch.equal(got[~nan], want[~nan]), (what, int((got[~nan] != want[~nan]).sum()))
    assert torch.all((got[nan] & 0x7F) == NAN8), what


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@each(paged=[False, True], descale=[1.0, 0.5, 0.3])
def test_append_quantises_every_input_pattern(paged, descale, dtype):
    """All 65 536 bit patterns of q's dtype as the new K rows (and, reversed, as the V rows): the
    bytes in the cache are the definition's."""
    from fa2_triton_amd import flash_attn_with_fp8_kvcache

    b, sn, hkv, d = 4, 16, 8, 128
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).cuda()
    kn = bits.view(dtype).reshape(b, sn, hkv, d)
    vn = bits.flip(0).view(dtype).reshape(b, sn, hkv, d)
    q = torch.zeros((b, 1, hkv, d), dtype=dtype, device="cuda")
    kd = torch.full((b, hkv), descale, device="cuda")
    if paged:
        k8 = torch.zeros((b + 1, 16, hkv, d), dtype=torch.uint8, device="cuda")
        v8 = torch.zeros_like(k8)
        table = torch.tensor([[3], [0], [4], [1]], dtype=torch.int32, device="cuda")
        flash_attn_with_fp8_kvcache(q, f8(k8), f8(v8), kd, descale, block_table=table, cache_seqlens=0, k=kn, v=vn)
        k8, v8 = k8[table[:, 0].long()], v8[table[:, 0].long()]
    else:
        k8 = torch.zeros((b, sn, hkv, d), dtype=torch.uint8, device="cuda")
        v8 = torch.zeros_like(k8)
        flash_attn_with_fp8_kvcache(q, f8(k8), f8(v8), kd, descale, cache_seqlens=0, k=kn, v=vn)
    _assert_bytes(k8, _quantise_cpu(kn, descale), "k")
    _assert_bytes(v8, _quantise_cpu(vn, descale), "v")


def _new_rows(b, sn, hkv, d, dtype, seed):
    torch.manual_seed(seed)
    kn = torch.empty((b, sn, hkv, d), dtype=dtype, device="cuda").normal_(0.0, 2.0)
    vn = torch.empty((b, sn, hkv, d), dtype=dtype, device="cuda").normal_(0.0, 2.0)
    return kn, vn


def _per_head(x, d):
    """x [B, n, Hkv, D] quantised with the descales d [B, Hkv], on the CPU."""
    return (x.float().cpu() / d.cpu()[:, None, :, None]).clamp(-448, 448).to(F8).view(torch.uint8).cuda()


@DTYPES
@pytest.mark.parametrize("sn", [1, 3])
def test_append(sn, dtype):
    """The quantised rows land at L_b .. L_b + Sn - 1 with their (batch, kv head)'s descale, no other
    cache byte changes, and attention in the same call reads the quantised bytes."""
    from fa2_triton_amd import flash_attn_with_fp8_kvcache

    b, hq, hkv, d, cap, lens = 3, 8, 2, 128, 320, (100, 0, 317)
    q, k8, v8 = _data(b, sn, hq, hkv, d, cap, dtype)
    kn, vn = _new_rows(b, sn, hkv, d, dtype, 3)
    kd = torch.tensor([[0.5, 0.3], [1.0, 0.7], [2.0, 0.11]], device="cuda")
    vd = torch.tensor([[0.9, 1.3], [0.25, 1.0], [0.6, 3.0]], device="cuda")
    k0, v0, seqlens = k8.clone(), v8.clone(), _lens(lens)
    got = flash_attn_with_fp8_kvcache(q, f8(k8), f8(v8), kd, vd, cache_seqlens=seqlens, k=kn, v=vn, causal=True, return_lse=True)
    assert torch.equal(seqlens, _lens(lens))  # not modified
    kq, vq = _per_head(kn, kd), _per_head(vn, vd)
    for i, n in enumerate(lens):
        k0[i, n:n + sn], v0[i, n:n + sn] = kq[i], vq[i]
    assert torch.equal(k8, k0) and torch.equal(v8, v0)
    after = flash_attn_with_fp8_kvcache(q, f8(k0), f8(v0), kd, vd, cache_seqlens=seqlens + sn, causal=True, return_lse=True)
    assert _same(got, after)


@DTYPES
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_append_stays_inside_the_cache(paged, dtype):
    """Lengths (cap - 1, cap, 0, far too large, negative) with Sn = 2, and with a table, entries just
    outside [0, num_blocks): rows at or past cap are dropped, and no byte outside the caches -- the
    middle of sentinel-filled buffers owned by this test -- changes."""
    from fa2_triton_amd import flash_attn_with_fp8_kvcache

    b, hq, hkv, d, sn, sentinel, page = 5, 4, 2, 64, 2, 0x55, 16
    cap = 128 if paged else 130
    lens, clamped = (cap - 1, cap, 0, 10**9, -5), (cap - 1, cap, 0, cap, 0)
    q, kc0, vc0 = _data(b, sn, hq, hkv, d, cap, dtype)
    kn, vn = _new_rows(b, sn, hkv, d, dtype, 5)
    kq, vq = _per_head(kn, torch.full((b, hkv), 0.3)), _per_head(vn, torch.full((b, hkv), 1.0))
    for i, n in enumerate(clamped):
        w = min(n + sn, cap) - n  # rows that fit
        kc0[i, n:n + w], vc0[i, n:n + w] = kq[i, :w], vq[i, :w]
    if not paged:
        pad = 8
        k_big = torch.full((b, cap + 2 * pad, hkv, d), sentinel, dtype=torch.uint8, device="cuda")
        v_big = torch.full_like(k_big, sentinel)
        k8, v8 = k_big[:, pad:pad + cap], v_big[:, pad:pad + cap]
        k8.copy_(_data(b, sn, hq, hkv, d, cap, dtype)[1])
        v8.copy_(_data(b, sn, hq, hkv, d, cap, dtype)[2])
        out, lse = flash_attn_with_fp8_kvcache(q, f8(k8), f8(v8), 0.3, None, cache_seqlens=_lens(lens), k=kn, v=vn,
                                               causal=True, return_lse=True)
        for big in (k_big, v_big):
            assert torch.all(big[:, :pad] == sentinel) and torch.all(big[:, pad + cap:] == sentinel)
        assert torch.equal(k8, kc0) and torch.equal(v8, vc0)
    else:
        # blocks in order, batch i's pages at blocks 8 i .. 8 i + 7; the ids of the first and the last
        # block are written as -1 and num_blocks, which the device clamps back onto them
        nb = b * cap // page
        k_big = torch.full((nb + 4, page, hkv, d), sentinel, dtype=torch.uint8, device="cuda")
        v_big = torch.full_like(k_big, sentinel)
        kp, vp = k_big[2:2 + nb], v_big[2:2 + nb]
        _, k_init, v_init = _data(b, sn, hq, hkv, d, cap, dtype)
        kp.copy_(k_init.reshape(nb, page, hkv, d))
        vp.copy_(v_init.reshape(nb, page, hkv, d))
        table = torch.arange(nb, dtype=torch.int32, device="cuda").reshape(b, cap // page).clone()
        table[0, 0], table[-1, -1] = -1, nb
        out, lse = flash_attn_with_fp8_kvcache(q, f8(kp), f8(vp), 0.3, None, block_table=table, cache_seqlens=_lens(lens),
                                               k=kn, v=vn, causal=True, return_lse=True)
        for big in (k_big, v_big):
            assert torch.all(big[:2] == sentinel) and torch.all(big[2 + nb:] == sentinel)
        assert torch.equal(kp.reshape(b, cap, hkv, d), kc0) and torch.equal(vp.reshape(b, cap, hkv, d), vc0)
    want = flash_attn_with_fp8_kvcache(q, f8(kc0), f8(vc0), 0.3, None, cache_seqlens=_lens(tuple(min(n + sn, cap) for n in clamped)),
                                       causal=True, return_lse=True)
    assert _same((out, lse), want)


# ---------------------------------------------------------------------------------------------
@each(head_dim=[64, 128])
def test_keys_below_the_band_are_never_read(head_dim):
    """cap = L = 1024, Sq 1, causal, left = 63: the smallest visible key is 960.  NaN bytes in the
    cache rows [0, 512) (at least 385 keys below the band) change no bit of the result."""
    from fa2_triton_amd import flash_attn_with_fp8_kvcache

    q, k8, v8 = _data(1, 1, 8, 2, head_dim, 1024, torch.bfloat16)
    k8[:, :512], v8[:, :512] = 0, 0
    kn, vn = k8.clone(), v8.clone()
    kn[:, :512], vn[:, :512] = NAN8, NAN8
    for nsplit in (0, 2):
        kw = dict(causal=True, window_size=(63, -1), num_splits=nsplit, return_lse=True)
        zero = flash_attn_with_fp8_kvcache(q, f8(k8), f8(v8), 0.7, 1.3, **kw)
        nan = flash_attn_with_fp8_kvcache(q, f8(kn), f8(vn), 0.7, 1.3, **kw)
        assert _same(zero, nan) and torch.isfinite(nan[0]).all()


@each(page=[16, 64, 256])
def test_what_is_not_referenced_is_not_read(page):
    """NaN bytes in the rows at or past L_b (contiguous and paged), in the spare blocks and in the
    blocks the table no longer names, whose entries are set to -7 and 2^30: no bit changes."""
    from fa2_triton_amd import flash_attn_with_fp8_kvcache

    b, cap, lens = 3, 512, (500, 65, 2)
    q, k8, v8 = _data(b, 2, 8, 2, 128, cap, torch.bfloat16)
    kp, vp, table, spare = _paged(k8, v8, page)
    kn, vn, bad = kp.clone(), vp.clone(), table.clone()
    kn[spare], vn[spare] = NAN8, NAN8
    kc, vc = k8.clone(), v8.clone()
    for i, n in enumerate(lens):
        kc[i, n:], vc[i, n:] = NAN8, NAN8
        used = -(-n // page)
        if n % page:  # the rows of the last page past the length
            last = table[i, used - 1].item()
            kn[last, n % page:], vn[last, n % page:] = NAN8, NAN8
        for j in range(used, cap // page):
            kn[table[i, j].item()], vn[table[i, j].item()] = NAN8, NAN8
            bad[i, j] = -7 if j % 2 else 2**30
    for nsplit in (0, 3):
        kw = dict(cache_seqlens=_lens(lens), causal=True, num_splits=nsplit, return_lse=True)
        clean = flash_attn_with_fp8_kvcache(q, f8(kp), f8(vp), 0.7, 1.3, block_table=table, **kw)
        dirty = flash_attn_with_fp8_kvcache(q, f8(kn), f8(vn), 0.7, 1.3, block_table=bad, **kw)
        assert _same(clean, dirty)
        assert torch.isfinite(dirty[0]).all() and torch.isfinite(dirty[1]).all()
        assert _same(flash_attn_with_fp8_kvcache(q, f8(k8), f8(v8), 0.7, 1.3, **kw),
                     flash_attn_with_fp8_kvcache(q, f8(kc), f8(vc), 0.7, 1.3, **kw))


@DTYPES
def test_layouts_need_no_copy(dtype):
    """A BHSD-allocated cache viewed as BSHD, a slice of a larger buffer and a pool stored
    [N, Hkv, P, D] give the bits of a contiguous copy."""
    from fa2_triton_amd import flash_attn_with_fp8_kvcache

    b, hq, hkv, d, cap = 2, 8, 2, 128, 320
    q, k8, v8 = _data(b, 2, hq, hkv, d, cap, dtype)
    kw = dict(cache_seqlens=_lens((300, 97)), causal=True, return_lse=True)
    want = flash_attn_with_fp8_kvcache(q, f8(k8), f8(v8), 0.7, 1.3, **kw)
    k_bhsd, v_bhsd = k8.transpose(1, 2).contiguous(), v8.transpose(1, 2).contiguous()  # [B, Hkv, cap, D]
    assert not k_bhsd.transpose(1, 2).is_contiguous()
    assert _same(flash_attn_with_fp8_kvcache(q, f8(k_bhsd).transpose(1, 2), f8(v_bhsd).transpose(1, 2), 0.7, 1.3, **kw), want)
    k_big = torch.full((b, cap + 128, hkv, d), NAN8, dtype=torch.uint8, device="cuda")
    v_big = torch.full_like(k_big, NAN8)
    k_big[:, 64:64 + cap], v_big[:, 64:64 + cap] = k8, v8
    assert _same(flash_attn_with_fp8_kvcache(q, f8(k_big)[:, 64:64 + cap], f8(v_big)[:, 64:64 + cap], 0.7, 1.3, **kw), want)
    kp, vp, table, _ = _paged(k8, v8, 16)
    k_hnd, v_hnd = kp.transpose(1, 2).contiguous(), vp.transpose(1, 2).contiguous()  # [N, Hkv, P, D]
    assert _same(flash_attn_with_fp8_kvcache(q, f8(k_hnd).transpose(1, 2), f8(v_hnd).transpose(1, 2), 0.7, 1.3, block_table=table, **kw),
                 want)


@each(paged=[False, True])
def test_deterministic_and_batch_invariant(paged):
    """Two runs give equal bits, and with the split count forced, batch row b of a B = 4 call equals
    that row run alone (with its own descales)."""
    from fa2_triton_amd import flash_attn_with_fp8_kvcache

    lens = (1000, 3, 513, 64)
    q, k8, v8 = _data(4, 2, 16, 4, 128, 1024, torch.bfloat16)
    kd = torch.rand((4, 4), device="cuda") + 0.5
    vd = torch.rand((4, 4), device="cuda") + 0.5
    kp, vp, table, _ = _paged(k8, v8, 16)

    def call(rows, n, nsplit):
        kw = dict(cache_seqlens=_lens(n), causal=True, num_splits=nsplit, return_lse=True)
        if paged:
            return flash_attn_with_fp8_kvcache(q[rows], f8(kp), f8(vp), kd[rows], vd[rows], block_table=table[rows], **kw)
        return flash_attn_with_fp8_kvcache(q[rows], f8(k8)[rows], f8(v8)[rows], kd[rows], vd[rows], **kw)

    for nsplit in (1, 5):
        a, b = call(slice(0, 4), lens, nsplit), call(slice(0, 4), lens, nsplit)
        assert _same(a, b)
        for i, n in enumerate(lens):
            one = call(slice(i, i + 1), (n,), nsplit)
            assert torch.equal(one[0][0], a[0][i]) and torch.equal(one[1][0], a[1][i]), (nsplit, i)


def test_graph_capture_follows_the_table_and_the_lengths():
    """One paged fp8 decode step (quantising append + attention) captured once on a single stream.
    Between replays the lengths advance in place across a page boundary, the next block id is written
    into the table in place and new q / k / v are copied in: every replay equals a fresh eager call
    on the same state bitwise."""
    from fa2_triton_amd import flash_attn_with_fp8_kvcache

    b, hq, hkv, d, page, max_blocks, nb = 2, 16, 4, 128, 16, 8, 20
    dtype = torch.bfloat16
    q, _, _ = _data(b, 1, hq, hkv, d, 1, dtype)
    kn, vn = _new_rows(b, 1, hkv, d, dtype, 1)
    _, kp, vp = _data(nb, 1, hq, hkv, d, page, dtype, seed=2)  # [nb, page, hkv, d] bytes
    kd = torch.tensor([[0.5, 0.3, 0.9, 1.1], [1.0, 0.7, 0.4, 2.0]], device="cuda")
    vd = torch.full((1, 1), 0.8, device="cuda").expand(b, hkv)
    table = torch.full((b, max_blocks), -7, dtype=torch.int32, device="cuda")  # pages not yet allocated: garbage
    table[0, 0], table[1, 0], table[1, 1] = 11, 4, 17
    seqlens = _lens((14, 30))

    def step(kp_, vp_):
        return flash_attn_with_fp8_kvcache(q, f8(kp_), f8(vp_), kd, vd, block_table=table, cache_seqlens=seqlens, k=kn, v=vn,
                                           causal=True, return_lse=True)

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
            k2, v2 = _new_rows(b, 1, hkv, d, dtype, 110 + it)
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
    assert torch.equal(kp[2, 0], _per_head(kn, kd)[0, 0]) and torch.equal(vp[9, 0], _per_head(vn, vd)[1, 0])


def test_inference_only_and_rejections():
    from fa2_triton_amd import flash_attn_with_fp8_kvcache, flash_attn_with_kvcache, flash_attn_with_paged_kvcache

    q, k8, v8 = _data(1, 1, 4, 2, 64, 192, torch.bfloat16)
    out = flash_attn_with_fp8_kvcache(q.requires_grad_(), f8(k8), f8(v8), 0.5, torch.full((1, 2), 2.0, device="cuda").requires_grad_())
    assert not out.requires_grad and out.grad_fn is None
    q = q.detach()
    table = torch.arange(12, dtype=torch.int32, device="cuda").reshape(1, 12)
    with pytest.raises(TypeError, match="float8_e4m3fn"):
        flash_attn_with_fp8_kvcache(q, k8.view(torch.float8_e5m2), v8.view(torch.float8_e5m2))
    with pytest.raises(TypeError, match="float8_e4m3fn"):
        flash_attn_with_fp8_kvcache(q, f8(k8).to(torch.bfloat16), f8(v8).to(torch.bfloat16))
    with pytest.raises(TypeError, match="dtype"):  # the 16-bit functions keep refusing fp8 caches
        flash_attn_with_kvcache(q, f8(k8), f8(v8))
    with pytest.raises(TypeError, match="dtype"):
        flash_attn_with_paged_kvcache(q, f8(k8).reshape(12, 16, 2, 64), f8(v8).reshape(12, 16, 2, 64), table, 100)
    with pytest.raises(NotImplementedError, match="128"):
        flash_attn_with_fp8_kvcache(torch.zeros((1, 1, 4, 144), dtype=torch.bfloat16, device="cuda"),
                                    f8(torch.zeros((1, 64, 2, 144), dtype=torch.uint8, device="cuda")),
                                    f8(torch.zeros((1, 64, 2, 144), dtype=torch.uint8, device="cuda")))
    with pytest.raises(NotImplementedError, match="multiple of 16"):
        flash_attn_with_fp8_kvcache(q[..., :40], f8(k8)[..., :48][..., :40], f8(v8)[..., :48][..., :40])
    with pytest.raises(NotImplementedError, match="16-byte"):  # rows at an 8-byte offset
        flash_attn_with_fp8_kvcache(q[..., :48], f8(k8)[..., 8:56], f8(v8)[..., 8:56])
    with pytest.raises(ValueError, match="k_descale"):
        flash_attn_with_fp8_kvcache(q, f8(k8), f8(v8), torch.ones((3, 2), device="cuda"))
    with pytest.raises(TypeError, match="v_descale"):
        flash_attn_with_fp8_kvcache(q, f8(k8), f8(v8), None, torch.ones((1, 2), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="v_descale"):
        flash_attn_with_fp8_kvcache(q, f8(k8), f8(v8), None, torch.ones((1, 2)))
    with pytest.raises(TypeError, match="cache_seqlens"):
        flash_attn_with_fp8_kvcache(q, f8(k8).reshape(12, 16, 2, 64), f8(v8).reshape(12, 16, 2, 64), block_table=table)
    with pytest.raises(ValueError, match="power of two"):
        flash_attn_with_fp8_kvcache(q, f8(k8).reshape(4, 48, 2, 64), f8(v8).reshape(4, 48, 2, 64), block_table=table[:, :4],
                                    cache_seqlens=100)
