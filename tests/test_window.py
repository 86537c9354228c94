"""Sliding-window (local) attention on the GPU: forward + backward against the oracle's
`window_size` (oracle/reference.py, bottom-right aligned on the valid lengths), the exact
one-key-per-row case, the normalisation of windows that bound nothing, and the functional face of
O(S * W): keys and rows outside the band are never read.
"""
import math

import pytest
import torch

from oracle import tolerance
from oracle.reference import LOG2E, attention_reference, window_mask
from oracle.tolerance import check_fa_tolerance
from tests.core import generate_test_data

pytestmark = pytest.mark.gpu

NAN = float("nan")

# (B, Hq, Hkv, Sq, Sk, D, causal, window, valid lengths or None)
CASES = [
    (2, 4, 4, 200, 200, 64, True, (64, -1), None),
    (2, 4, 2, 257, 257, 128, False, (33, 17), None),
    (1, 4, 1, 130, 333, 128, True, (100, -1), None),
    (1, 2, 2, 333, 130, 64, False, (40, 40), None),   # rows with no visible key
    (1, 2, 2, 333, 130, 64, True, (40, -1), None),    # rows with no visible key
    (1, 2, 2, 129, 129, 96, False, (-1, 20), None),
    (1, 2, 1, 300, 300, 256, True, (127, -1), None),
    (1, 2, 2, 64, 64, 128, True, (1000, -1), None),
    (2, 2, 2, 199, 199, 59, True, (64, -1), None),    # the unaligned path
    # varlen: right padding as tests.core.generate_attention_mask builds it, one full row and one
    # nearly empty row
    (3, 4, 2, 260, 260, 64, True, (50, -1), (260, 2, 137)),
    (3, 2, 2, 260, 260, 128, False, (30, 70), (137, 260, 2)),
]


def _id(c):
    b, hq, hkv, sq, sk, d, causal, w, lens = c
    return f"b{b}-h{hq}x{hkv}-s{sq}x{sk}-d{d}-{'causal' if causal else 'full'}-w{w[0]}_{w[1]}" + ("-varlen" if lens else "")


def _padding_mask(lens, seqlen, device):
    if lens is None:
        return None
    mask = torch.ones((len(lens), seqlen), dtype=torch.bool, device=device)
    for i, n in enumerate(lens):
        if seqlen - n:
            mask[i, -(seqlen - n):] = False
    return mask


def _lse2_window(q, k, causal, window, mask):
    """Base-2 log-sum-exp of the scaled scores over the oracle's window mask: [B, Hq, Sq] fp32."""
    if causal:
        window = (window[0], 0)
    qf, kf = q.detach().float(), k.detach().float()
    kf = torch.repeat_interleave(kf, q.size(2) // k.size(2), dim=2)
    scores = torch.einsum("bqhd,bkhd->bhqk", qf, kf) / math.sqrt(q.size(3))
    if mask is not None:
        scores = scores.masked_fill(~mask[:, None, None, :], float("-inf"))
    scores = scores.masked_fill(window_mask(q.size(1), k.size(1), window, mask, mask, q.device), float("-inf"))
    return torch.logsumexp(scores, dim=-1) * LOG2E


def _forward_lse(q, k, v, mask, causal, window):
    from fa2_triton_amd.forward import _flash_attn_forward

    with torch.no_grad():
        _, lse, _, _ = _flash_attn_forward(q, k, v, mask, None, 0.0, causal, None, None, window_size=window)
    return lse[:, :, : q.size(1)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_window_parity(case, dtype):
    """The reference tests' rule (oracle/tolerance.py) with the oracle's window, no escape taken;
    LSE2 as tests/test_golden.py checks it (1e-3 abs / rel, -inf on empty rows); padded rows zero."""
    from fa2_triton_amd import flash_attn_func

    b, hq, hkv, sq, sk, d, causal, window, lens = case
    q, k, v, do = generate_test_data(b, hq, hkv, sq, sk, d, dtype)
    mask = _padding_mask(lens, sq, q.device)
    common = dict(query_padding_mask=mask, key_padding_mask=mask, causal=causal, window_size=window)
    out_ref = attention_reference(q, k, v, **common)
    out_pt = attention_reference(q, k, v, upcast=False, reorder_ops=True, **common)
    out = flash_attn_func(q, k, v, attention_mask=mask, causal=causal, window_size=window)
    assert out.shape == q.shape and out.dtype == q.dtype
    grads = torch.autograd.grad(out, (q, k, v), do, retain_graph=True)
    before = dict(tolerance.ESCAPES)
    report = check_fa_tolerance(q, k, v, do, out, out_ref, out_pt, grads=grads)
    print(_id(case), dtype, {key: f"{val:.3e}" for key, val in report.items()})
    assert tolerance.ESCAPES["ulp"] == before["ulp"] and tolerance.ESCAPES["dv_sum"] == before["dv_sum"], report
    for name, g in zip(("out", "dq", "dk", "dv"), (out,) + tuple(grads)):
        assert torch.isfinite(g).all(), name

    ref_lse = _lse2_window(q, k, causal, window, mask)
    got = _forward_lse(q, k, v, mask, causal, window)
    finite = torch.isfinite(ref_lse)
    if mask is not None:
        finite &= mask[:, None, :]
    assert torch.allclose(got[finite], ref_lse[finite], rtol=1e-3, atol=1e-3), (got[finite] - ref_lse[finite]).abs().max()
    assert torch.all(torch.isneginf(got[~torch.isfinite(ref_lse)]))
    if (sq, sk) == (333, 130):
        assert (~torch.isfinite(ref_lse)).any()  # the case has rows with no visible key
    if mask is not None:
        for name, g in zip(("out", "dq", "dk", "dv"), (out,) + tuple(grads)):
            assert torch.count_nonzero(g[~mask]) == 0, name


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_negative_right_is_no_bound(dtype):
    """left >= 0 with a negative right and no causal flag: no bound on the right (fa2_amd.h), i.e.
    the oracle's window with right = Sk."""
    from fa2_triton_amd import flash_attn_func

    q, k, v, do = generate_test_data(1, 2, 1, 150, 210, 64, dtype)
    out = flash_attn_func(q, k, v, window_size=(40, -1))
    out_ref = attention_reference(q, k, v, window_size=(40, 210))
    out_pt = attention_reference(q, k, v, window_size=(40, 210), upcast=False, reorder_ops=True)
    check_fa_tolerance(q, k, v, do, out, out_ref, out_pt)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_one_key_per_row_is_exact(dtype):
    """window_size=(0, 0): each row sees its diagonal key alone, so P == 1.  O equals V bitwise,
    dV equals the fp32 group sum of dO rounded once, and dQ and dK are exactly zero: the windowed
    dQ forms delta = rowsum(O o dO) in the summation order of the dP chains,
    so with O == V the difference dP - delta is 0, not a last-bit residue."""
    from fa2_triton_amd import flash_attn_func

    q, k, v, do = generate_test_data(2, 4, 2, 192, 192, 32, dtype)
    out = flash_attn_func(q, k, v, window_size=(0, 0))
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), do)
    for h in range(4):
        assert torch.equal(out[:, :, h], v.detach()[:, :, h // 2]), h
    want = do.float().view(2, 192, 2, 2, 32).sum(dim=3).to(dtype)  # fp32 group sum, rounded once
    print("max |dq|", dq.abs().max().item(), "max |dk|", dk.abs().max().item(),
          "max |dv - want|", (dv.float() - want.float()).abs().max().item())
    assert torch.equal(dv, want), (dv.float() - want.float()).abs().max()
    assert torch.count_nonzero(dq) == 0
    assert torch.count_nonzero(dk) == 0


def _fwd_bwd(q, k, v, do, **kw):
    from fa2_triton_amd import flash_attn_func

    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    out = flash_attn_func(q, k, v, **kw)
    return (out.detach(),) + torch.autograd.grad(out, (q, k, v), do)


def test_windows_that_bound_nothing_run_the_plain_kernels():
    """A hand-placed shape: (-1, -1) is the call without a window, (-1, 0) is causal -- bitwise."""
    q, k, v, do = generate_test_data(1, 2, 2, 256, 256, 128, torch.bfloat16)
    for causal in (False, True):
        plain = _fwd_bwd(q, k, v, do, causal=causal)
        same = _fwd_bwd(q, k, v, do, causal=causal, window_size=(-1, -1))
        for name, x, y in zip(("out", "dq", "dk", "dv"), same, plain):
            assert torch.equal(x, y), (causal, name)
    causal = _fwd_bwd(q, k, v, do, causal=True)
    as_window = _fwd_bwd(q, k, v, do, causal=False, window_size=(-1, 0))
    for name, x, y in zip(("out", "dq", "dk", "dv"), as_window, causal):
        assert torch.equal(x, y), name
    also = _fwd_bwd(q, k, v, do, causal=True, window_size=(-1, 5))  # causal forces right = 0
    for name, x, y in zip(("out", "dq", "dk", "dv"), also, causal):
        assert torch.equal(x, y), name


@pytest.mark.parametrize("head_dim", [64, 128])
def test_keys_below_the_band_are_never_read(head_dim):
    """Sq = 64, Sk = 1024, causal, left = 63: the smallest visible key is 897.  NaN in K / V rows
    [0, 512) changes nothing (a gap of 385 keys, beyond any tile or prefetch distance), and those
    keys get exactly zero gradients."""
    dtype, window = torch.bfloat16, (63, -1)
    q, k, v, do = generate_test_data(1, 2, 1, 64, 1024, head_dim, dtype)
    kz, vz = k.detach().clone(), v.detach().clone()
    kz[:, :512], vz[:, :512] = 0, 0
    kn, vn = kz.clone(), vz.clone()
    kn[:, :512], vn[:, :512] = NAN, NAN
    zero = _fwd_bwd(q, kz, vz, do, causal=True, window_size=window)
    nan = _fwd_bwd(q, kn, vn, do, causal=True, window_size=window)
    out_z, dq_z, dk_z, dv_z = zero
    out_n, dq_n, dk_n, dv_n = nan
    assert torch.equal(out_n, out_z) and torch.equal(dq_n, dq_z)
    assert torch.equal(dk_n[:, 512:], dk_z[:, 512:]) and torch.equal(dv_n[:, 512:], dv_z[:, 512:])
    assert torch.count_nonzero(dk_n[:, :512]) == 0 and torch.count_nonzero(dv_n[:, :512]) == 0
    # the zero run against the oracle
    qz, kz, vz = (t.detach().clone().requires_grad_() for t in (q, kz, vz))
    out_ref = attention_reference(qz, kz, vz, causal=True, window_size=window)
    out_pt = attention_reference(qz, kz, vz, causal=True, window_size=window, upcast=False, reorder_ops=True)
    check_fa_tolerance(qz, kz, vz, do, out_z, out_ref, out_pt, grads=(dq_z, dk_z, dv_z))


@pytest.mark.parametrize("head_dim", [64, 128])
def test_rows_outside_the_band_are_never_read(head_dim):
    """The mirror image: Sq = 1024, Sk = 64, so rows below 960 see no key.  NaN in Q / dO rows
    [0, 512) reaches no dK / dV; those rows get O = 0, LSE2 = -inf and dQ = 0."""
    dtype, window = torch.bfloat16, (63, -1)
    q, k, v, do = generate_test_data(1, 2, 1, 1024, 64, head_dim, dtype)
    qz, doz = q.detach().clone(), do.clone()
    qz[:, :512], doz[:, :512] = 0, 0
    qn, don = qz.clone(), doz.clone()
    qn[:, :512], don[:, :512] = NAN, NAN
    out_z, dq_z, dk_z, dv_z = _fwd_bwd(qz, k, v, doz, causal=True, window_size=window)
    out_n, dq_n, dk_n, dv_n = _fwd_bwd(qn, k, v, don, causal=True, window_size=window)
    assert torch.equal(dk_n, dk_z) and torch.equal(dv_n, dv_z)
    assert torch.count_nonzero(out_n[:, :512]) == 0 and torch.count_nonzero(dq_n[:, :512]) == 0
    lse = _forward_lse(qn, k.detach(), v.detach(), None, True, window)
    assert torch.all(torch.isneginf(lse[:, :, :960])) and torch.isfinite(lse[:, :, 960:]).all()
    for name, t in zip(("out", "dq", "dk", "dv"), (out_n, dq_n, dk_n, dv_n)):
        assert torch.isfinite(t).all(), name
    assert torch.count_nonzero(dk_n) > 0 and torch.count_nonzero(dv_n) > 0 and torch.count_nonzero(out_n[:, 960:]) > 0


def test_window_with_bias_or_dropout_is_not_implemented():
    from fa2_triton_amd import flash_attn_func

    q, k, v, _ = generate_test_data(1, 2, 2, 64, 64, 64, torch.bfloat16)
    bias = torch.zeros(1, 1, 64, 64, dtype=torch.bfloat16, device=q.device)
    with pytest.raises(NotImplementedError, match="window"):
        flash_attn_func(q, k, v, attention_bias=bias, window_size=(8, 8))
    with pytest.raises(NotImplementedError, match="window"):
        flash_attn_func(q, k, v, dropout_p=0.1, window_size=(8, 8))
