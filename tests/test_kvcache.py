"""KV-cache decode attention on the GPU (`flash_attn_with_kvcache`, fa2_fwd_kvcache): parity with the
oracle under a key-padding mask built from the cache lengths (bottom-right aligned on the valid
length), the split / combine paths, cache layouts, the append and its bounds, determinism, batch
invariance and graph capture with lengths that change between replays.
"""
import math

import pytest
import torch

from oracle import tolerance
from oracle.reference import LOG2E, attention_reference, window_mask
from oracle.tolerance import check_fa_tolerance

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
NAN = float("nan")


def _data(b, sq, hq, hkv, d, cap, dtype, seed=0):
    torch.manual_seed(seed)
    q = torch.empty((b, sq, hq, d), dtype=dtype, device="cuda").normal_(0.0, 0.5)
    kc = torch.empty((b, cap, hkv, d), dtype=dtype, device="cuda").normal_(0.0, 0.5)
    vc = torch.empty((b, cap, hkv, d), dtype=dtype, device="cuda").normal_(0.0, 0.5)
    return q, kc, vc


def _lens(lens, device="cuda"):
    return torch.tensor(lens, dtype=torch.int32, device=device)


def _key_mask(lens, cap):
    return torch.arange(cap, device="cuda")[None, :] < _lens(lens)[:, None]


def _oracle(q, kc, vc, lens, causal, window, softmax_scale=None):
    """(fp32-upcast oracle, low-precision reordered oracle) with the cache lengths as a key mask."""
    common = dict(key_padding_mask=_key_mask(lens, kc.size(1)), causal=causal, window_size=window,
                  softmax_scale=softmax_scale)
    return attention_reference(q, kc, vc, **common), attention_reference(q, kc, vc, upcast=False, reorder_ops=True, **common)


def _lse2(q, kc, lens, causal, window, softmax_scale=None):
    """Base-2 log-sum-exp of the scaled scores over the same mask: [B, Hq, Sq] fp32, -inf on empty rows."""
    mask = _key_mask(lens, kc.size(1))
    if causal:
        window = (window[0], 0)
    kf = torch.repeat_interleave(kc.float(), q.size(2) // kc.size(2), dim=2)
    scores = torch.einsum("bqhd,bkhd->bhqk", q.float(), kf)
    scores = scores / math.sqrt(q.size(3)) if softmax_scale is None else scores * softmax_scale
    scores = scores.masked_fill(~mask[:, None, None, :], float("-inf"))
    if window[0] >= 0 or window[1] >= 0:
        scores = scores.masked_fill(window_mask(q.size(1), kc.size(1), window, None, mask, q.device), float("-inf"))
    return torch.logsumexp(scores, dim=-1) * LOG2E


def _check(q, kc, vc, lens, out, lse, causal, window, softmax_scale=None):
    """The reference tests' forward rule with no escape taken, and LSE2 by the rule of test_golden."""
    ref, pt = _oracle(q, kc, vc, lens, causal, window, softmax_scale)
    before = dict(tolerance.ESCAPES)
    report = check_fa_tolerance(q, kc, vc, None, out, ref, pt)
    print({key: f"{val:.3e}" for key, val in report.items()})
    assert tolerance.ESCAPES["ulp"] == before["ulp"] and tolerance.ESCAPES["dv_sum"] == before["dv_sum"], report
    assert out.shape == q.shape and out.dtype == q.dtype and torch.isfinite(out).all()
    if lse is not None:
        want = _lse2(q, kc, lens, causal, window, softmax_scale)
        assert lse.shape == want.shape and lse.dtype == torch.float32
        finite = torch.isfinite(want)
        assert torch.allclose(lse[finite], want[finite], rtol=1e-3, atol=1e-3), (lse[finite] - want[finite]).abs().max()
        assert torch.all(torch.isneginf(lse[~finite]))
    return ref, pt


# (B, Hq, Hkv, Sq, cap, D, lengths, causal, window, num_splits)
CASES = {
    "mha-one-row": (4, 8, 8, 1, 512, 128, (512, 1, 63, 300), True, (-1, -1), 0),
    "gqa-32x8-splits4": (3, 32, 8, 1, 1024, 128, (1024, 65, 64), True, (-1, -1), 4),
    "mqa-full-tile-splits3": (2, 32, 1, 1, 700, 64, (700, 129), False, (-1, -1), 3),
    "two-row-tiles-causal": (2, 16, 2, 5, 640, 128, (640, 7), True, (-1, -1), 0),
    "rows-without-keys": (2, 4, 2, 3, 64, 64, (2, 1), True, (-1, -1), 0),
    "full-sq4": (2, 4, 2, 4, 300, 128, (300, 77), False, (-1, -1), 0),
    "splits16-mostly-empty": (1, 8, 2, 1, 2048, 128, (65,), True, (-1, -1), 16),
    "direct-one-split": (2, 8, 2, 1, 1000, 128, (1000, 333), True, (-1, -1), 1),
    "d32": (2, 8, 2, 2, 300, 32, (300, 131), True, (-1, -1), 2),
    "d96": (2, 8, 2, 2, 300, 96, (300, 131), True, (-1, -1), 2),
    "d256": (2, 8, 2, 2, 300, 256, (300, 131), True, (-1, -1), 2),
    # windows: causal or two-sided only (the oracle reads a negative right bound differently)
    "window-100-causal": (1, 8, 2, 1, 2048, 128, (2048,), True, (100, -1), 0),
    "window-64-causal-sq3": (2, 8, 2, 3, 1000, 64, (1000, 50), True, (64, -1), 0),
    "window-30-10-sq4": (2, 4, 4, 4, 500, 128, (500, 200), False, (30, 10), 0),
}


@DTYPES
@pytest.mark.parametrize("case", sorted(CASES))
def test_parity(case, dtype):
    from fa2_triton_amd import flash_attn_with_kvcache

    b, hq, hkv, sq, cap, d, lens, causal, window, nsplit = CASES[case]
    q, kc, vc = _data(b, sq, hq, hkv, d, cap, dtype)
    out, lse = flash_attn_with_kvcache(q, kc, vc, cache_seqlens=_lens(lens), causal=causal, window_size=window,
                                       num_splits=nsplit, return_lse=True)
    _check(q, kc, vc, lens, out, lse, causal, window)
    if case == "rows-without-keys":
        # causal, Sq 3 over 2 and 1 keys: rows 0 (and 1) of the batches see no key
        assert torch.all(torch.isneginf(lse[0, :, 0])) and torch.all(torch.isneginf(lse[1, :, :2]))
        assert torch.count_nonzero(out[0, 0]) == 0 and torch.count_nonzero(out[1, :2]) == 0


@DTYPES
def test_cache_seqlens_forms(dtype):
    """None (every sequence fills the cache), a Python int and a device tensor."""
    from fa2_triton_amd import flash_attn_with_kvcache

    q, kc, vc = _data(2, 1, 8, 2, 128, 333, dtype)
    out = flash_attn_with_kvcache(q, kc, vc, causal=True)
    _check(q, kc, vc, (333, 333), out, None, True, (-1, -1))
    out_i, lse_i = flash_attn_with_kvcache(q, kc, vc, cache_seqlens=200, causal=True, return_lse=True)
    _check(q, kc, vc, (200, 200), out_i, lse_i, True, (-1, -1))
    out_t, lse_t = flash_attn_with_kvcache(q, kc, vc, cache_seqlens=_lens((200, 200)), causal=True, return_lse=True)
    assert torch.equal(out_t, out_i) and torch.equal(lse_t, lse_i)
    # values outside [0, cap] are clamped on the device
    out_c = flash_attn_with_kvcache(q, kc, vc, cache_seqlens=_lens((10**6, 333)), causal=True)
    assert torch.equal(out_c, out)


@DTYPES
def test_length_zero(dtype):
    """A batch row with no key gives O = 0 and LSE2 = -inf exactly; the other row is checked against
    the oracle on its own slice (the oracle gives NaN for an empty non-causal row)."""
    from fa2_triton_amd import flash_attn_with_kvcache

    q, kc, vc = _data(2, 2, 8, 2, 128, 256, dtype)
    for nsplit in (1, 3):
        out, lse = flash_attn_with_kvcache(q, kc, vc, cache_seqlens=_lens((0, 200)), num_splits=nsplit, return_lse=True)
        assert torch.count_nonzero(out[0]) == 0 and torch.all(torch.isneginf(lse[0]))
        _check(q[1:], kc[1:, :200], vc[1:, :200], (200,), out[1:], lse[1:], False, (-1, -1))


@DTYPES
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_against_the_existing_forward(causal, dtype):
    """With equal lengths both entry points pass the rule against the same oracle outputs."""
    from fa2_triton_amd import flash_attn_func, flash_attn_with_kvcache

    q, kc, vc = _data(2, 4, 8, 2, 128, 384, dtype)
    out = flash_attn_with_kvcache(q, kc, vc, causal=causal)
    ref, pt = _check(q, kc, vc, (384, 384), out, None, causal, (-1, -1))
    with torch.no_grad():
        old = flash_attn_func(q, kc, vc, causal=causal)
    check_fa_tolerance(q, kc, vc, None, old, ref, pt)


@pytest.mark.parametrize("head_dim", [64, 128])
def test_keys_below_the_band_are_never_read(head_dim):
    """cap = L = 1024, Sq 1, causal, left = 63: the smallest visible key is 960.  NaN in the cache
    rows [0, 512) (at least 385 keys below the band) changes no bit of the result."""
    from fa2_triton_amd import flash_attn_with_kvcache

    q, kc, vc = _data(1, 1, 8, 2, head_dim, 1024, torch.bfloat16)
    kc[:, :512], vc[:, :512] = 0, 0
    kn, vn = kc.clone(), vc.clone()
    kn[:, :512], vn[:, :512] = NAN, NAN
    for nsplit in (0, 2):
        zero = flash_attn_with_kvcache(q, kc, vc, causal=True, window_size=(63, -1), num_splits=nsplit, return_lse=True)
        nan = flash_attn_with_kvcache(q, kn, vn, causal=True, window_size=(63, -1), num_splits=nsplit, return_lse=True)
        assert torch.equal(zero[0], nan[0]) and torch.equal(zero[1], nan[1])
        _check(q, kc, vc, (1024,), zero[0], zero[1], True, (63, -1))


@DTYPES
def test_layouts_need_no_copy(dtype):
    """A BHSD-allocated cache viewed as BSHD, and a slice of a larger buffer, give the bits of a
    contiguous copy."""
    from fa2_triton_amd import flash_attn_with_kvcache

    b, hq, hkv, d, cap = 2, 8, 2, 128, 300
    q, kc, vc = _data(b, 2, hq, hkv, d, cap, dtype)
    lens = _lens((300, 97))
    want = flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, return_lse=True)
    k_bhsd, v_bhsd = kc.transpose(1, 2).contiguous(), vc.transpose(1, 2).contiguous()  # [B, Hkv, cap, D]
    got = flash_attn_with_kvcache(q, k_bhsd.transpose(1, 2), v_bhsd.transpose(1, 2), cache_seqlens=lens, causal=True,
                                  return_lse=True)
    assert not k_bhsd.transpose(1, 2).is_contiguous()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    k_big = torch.full((b, cap + 128, hkv, d), NAN, dtype=dtype, device="cuda")
    v_big = torch.full((b, cap + 128, hkv, d), NAN, dtype=dtype, device="cuda")
    k_big[:, 64:64 + cap], v_big[:, 64:64 + cap] = kc, vc
    got = flash_attn_with_kvcache(q, k_big[:, 64:64 + cap], v_big[:, 64:64 + cap], cache_seqlens=lens, causal=True,
                                  return_lse=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@DTYPES
@pytest.mark.parametrize("sn", [1, 3])
def test_append(sn, dtype):
    """k, v are written at rows L_b .. L_b + Sn - 1 bitwise, no other cache row changes, and the
    output is that of the updated cache with lengths L_b + Sn."""
    from fa2_triton_amd import flash_attn_with_kvcache

    b, hq, hkv, d, cap = 3, 8, 2, 128, 320
    lens = (100, 0, 317)
    q, kc, vc = _data(b, sn, hq, hkv, d, cap, dtype)
    _, kn, vn = _data(b, sn, hq, hkv, d, sn, dtype, seed=3)
    k0, v0 = kc.clone(), vc.clone()
    seqlens = _lens(lens)
    out, lse = flash_attn_with_kvcache(q, kc, vc, k=kn, v=vn, cache_seqlens=seqlens, causal=True, return_lse=True)
    assert torch.equal(seqlens, _lens(lens))  # not modified
    for i, n in enumerate(lens):
        assert torch.equal(kc[i, n:n + sn], kn[i]) and torch.equal(vc[i, n:n + sn], vn[i])
        k0[i, n:n + sn], v0[i, n:n + sn] = kn[i], vn[i]
    assert torch.equal(kc, k0) and torch.equal(vc, v0)
    _check(q, kc, vc, tuple(n + sn for n in lens), out, lse, True, (-1, -1))


@DTYPES
def test_append_stays_inside_the_cache(dtype):
    """Lengths (cap - 1, cap, 0, far too large, negative) with Sn = 2: rows that would land at or
    past cap are dropped, no element outside the caches (slices of sentinel-filled buffers owned by
    this test) changes, and the attended length is min(L_b + Sn, cap)."""
    from fa2_triton_amd import flash_attn_with_kvcache

    b, hq, hkv, d, cap, sn, pad = 5, 4, 2, 64, 130, 2, 8
    lens = (cap - 1, cap, 0, 10**9, -5)
    clamped = (cap - 1, cap, 0, cap, 0)
    q, kc0, vc0 = _data(b, sn, hq, hkv, d, cap, dtype)
    _, kn, vn = _data(b, sn, hq, hkv, d, sn, dtype, seed=5)
    sentinel = 7.0
    k_big = torch.full((b, cap + 2 * pad, hkv, d), sentinel, dtype=dtype, device="cuda")
    v_big = torch.full((b, cap + 2 * pad, hkv, d), sentinel, dtype=dtype, device="cuda")
    kc, vc = k_big[:, pad:pad + cap], v_big[:, pad:pad + cap]
    kc.copy_(kc0)
    vc.copy_(vc0)
    out, lse = flash_attn_with_kvcache(q, kc, vc, k=kn, v=vn, cache_seqlens=_lens(lens), causal=True, return_lse=True)
    for big in (k_big, v_big):
        assert torch.all(big[:, :pad] == sentinel) and torch.all(big[:, pad + cap:] == sentinel)
    for i, n in enumerate(clamped):
        w = min(n + sn, cap) - n  # rows that fit
        kc0[i, n:n + w], vc0[i, n:n + w] = kn[i, :w], vn[i, :w]
    assert torch.equal(kc, kc0) and torch.equal(vc, vc0)
    _check(q, kc, vc, tuple(min(n + sn, cap) for n in clamped), out, lse, True, (-1, -1))


def test_deterministic_and_batch_invariant():
    """Two runs give equal bits, and with the split count forced, batch row b of a B = 4 call equals
    that row run alone."""
    from fa2_triton_amd import flash_attn_with_kvcache

    lens = (1000, 3, 513, 64)
    q, kc, vc = _data(4, 2, 16, 4, 128, 1000, torch.bfloat16)
    for nsplit in (1, 5):
        kw = dict(causal=True, num_splits=nsplit, return_lse=True)
        a = flash_attn_with_kvcache(q, kc, vc, cache_seqlens=_lens(lens), **kw)
        b = flash_attn_with_kvcache(q, kc, vc, cache_seqlens=_lens(lens), **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for i, n in enumerate(lens):
            one = flash_attn_with_kvcache(q[i:i + 1], kc[i:i + 1], vc[i:i + 1], cache_seqlens=_lens((n,)), **kw)
            assert torch.equal(one[0][0], a[0][i]) and torch.equal(one[1][0], a[1][i]), (nsplit, i)


def test_graph_capture_follows_the_device_lengths():
    """One decode step (append + attention, device cache_seqlens) captured once: after the lengths
    are advanced in place and new q / k / v copied in, a replay equals a fresh eager call on the
    same state bitwise -- no length is baked into the capture and nothing synchronises."""
    from fa2_triton_amd import flash_attn_with_kvcache

    b, hq, hkv, d, cap = 3, 16, 4, 128, 1024
    dtype = torch.bfloat16
    q, kc, vc = _data(b, 1, hq, hkv, d, cap, dtype)
    _, kn, vn = _data(b, 1, hq, hkv, d, 1, dtype, seed=1)
    seqlens = _lens((700, 63, 0))

    def step(kc_, vc_):
        return flash_attn_with_kvcache(q, kc_, vc_, k=kn, v=vn, cache_seqlens=seqlens, causal=True, return_lse=True)

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
    assert torch.equal(captured[0], fresh[0]) and torch.equal(captured[1], fresh[1])

    for seed in (11, 12):  # two more decode steps through the same graph
        q2, _, _ = _data(b, 1, hq, hkv, d, 1, dtype, seed=seed)
        _, k2, v2 = _data(b, 1, hq, hkv, d, 1, dtype, seed=seed + 100)
        seqlens += 1
        q.copy_(q2)
        kn.copy_(k2)
        vn.copy_(v2)
        graph.replay()
        torch.cuda.synchronize()
        kf, vf = kc.clone(), vc.clone()
        fresh = step(kf, vf)
        assert torch.equal(captured[0], fresh[0]) and torch.equal(captured[1], fresh[1])
        assert torch.equal(kf, kc) and torch.equal(vf, vc)
    lens = tuple(int(n) + 1 for n in seqlens.tolist())
    _check(q, kc, vc, lens, captured[0], captured[1], True, (-1, -1))


def test_inference_only_and_rejections():
    from fa2_triton_amd import flash_attn_with_kvcache

    q, kc, vc = _data(1, 1, 4, 2, 64, 128, torch.bfloat16)
    out = flash_attn_with_kvcache(q.requires_grad_(), kc.requires_grad_(), vc.requires_grad_())
    assert not out.requires_grad and out.grad_fn is None
    with pytest.raises((ValueError, TypeError)):
        flash_attn_with_kvcache(q.cpu(), kc.cpu(), vc.cpu())
    with pytest.raises(TypeError):
        flash_attn_with_kvcache(q, kc.half(), vc.half())
    with pytest.raises(ValueError):
        flash_attn_with_kvcache(q, kc, vc, cache_seqlens=torch.tensor([5], dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        flash_attn_with_kvcache(q, kc, vc, cache_seqlens=torch.tensor([5, 5], dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        flash_attn_with_kvcache(q, kc, vc, cache_seqlens=torch.tensor([5], dtype=torch.int32))
