"""GPU parity harness -- the reference's tests/core.py + tests/utils.py, Triton-free.

Mirrors /root/reference/tests/core.py:10-78 (_test_core_fn) and the generators of
/root/reference/tests/utils.py: generate_test_data (:9-26, seed 0, N(0, 0.5) Q/K/V, N(0, 1) dO),
generate_attention_mask (:40-56, right padding, one full row), generate_dropout_seed_and_mask
(:169-207, here with the torch Philox of oracle/philox.py instead of a Triton kernel) and the
acceptance rule compare_results_fa (:68-142, oracle/tolerance.py).  The oracle is run on the
same device tensors, fp32-upcast ("ref") and in the input dtype with reordered ops ("pt").
"""
from typing import Optional, Tuple

import torch
from torch import Tensor

from oracle.philox import dropout_keep_mask_torch
from oracle.reference import attention_reference
from oracle.tolerance import check_fa_tolerance


def generate_test_data(batch_size, nheads_q, nheads_kv, seqlen_q, seqlen_k, head_dim, dtype, seed=0, device="cuda"):
    torch.manual_seed(seed)
    q = torch.empty((batch_size, seqlen_q, nheads_q, head_dim), dtype=dtype, device=device).normal_(0.0, 0.5)
    k = torch.empty((batch_size, seqlen_k, nheads_kv, head_dim), dtype=dtype, device=device).normal_(0.0, 0.5)
    v = torch.empty((batch_size, seqlen_k, nheads_kv, head_dim), dtype=dtype, device=device).normal_(0.0, 0.5)
    do = torch.randn_like(q)
    return q.requires_grad_(), k.requires_grad_(), v.requires_grad_(), do


STAIR_EDGES_ALIGNED = (64, 128, 192)  # a new level at every 64-key tile
STAIR_EDGES_MID = (37, 101, 165)  # levels change inside the tiles
STAIR_A = 4.0  # q column 0 of the planted rows


def stair_levels(seqlen_k: int, edges, descending=False, valid_lens=None, batch_size=1, device="cpu") -> Tensor:
    """[B, Sk] int64: level(j) = the number of entries of `edges` (truncated to Sk) that are <= j.
    `descending` reverses the staircase along each sequence's valid keys, level(L_b - 1 - j) for
    j < L_b and 0 past them; ascending it runs over the whole (padded) length whatever L_b is."""
    edges = torch.tensor([e for e in edges if e < seqlen_k], dtype=torch.long, device=device)
    j = torch.arange(seqlen_k, device=device)
    lens = torch.tensor(list(valid_lens) if valid_lens is not None else [seqlen_k] * batch_size, device=device)
    if not descending:
        return (j[:, None] >= edges[None, :]).sum(-1)[None, :].expand(lens.numel(), -1).contiguous()
    jr = lens[:, None] - 1 - j[None, :]  # [B, Sk], negative past the valid keys
    return ((jr[:, :, None] >= edges[None, None, :]).sum(-1) * (jr >= 0)).contiguous()


def planted_row_mask(seqlen_q: int, planted_rows, device="cpu") -> Tensor:
    """[Sq] bool: "third" (i % 3 == 0: planted and control rows inside every wave) or a range
    (first, last + 1), e.g. (64, 128): the 64 rows of one wave, whose neighbours never vote."""
    i = torch.arange(seqlen_q, device=device)
    if planted_rows == "third":
        return i % 3 == 0
    lo, hi = planted_rows
    return (i >= lo) & (i < hi)


def generate_staircase_data(batch_size, nheads_q, nheads_kv, seqlen_q, seqlen_k, head_dim, dtype, edges, step,
                            planted_rows="third", descending=False, softmax_scale=None, valid_lens=None, seed=0,
                            device="cuda"):
    """generate_test_data with a staircase planted in head-dim column 0, so that the running row
    max of the planted rows climbs by `step` log2 units per level -- beyond kDeferMax (csrc/common.h),
    which the N(0, 0.5) inputs never do after the first tile.

    q[:, planted, :, 0] = STAIR_A, q[:, others, :, 0] = 0 (control rows keep the flat softmax);
    k[b, j, :, 0] = level_b(j) c with c = step / (log2e STAIR_A scale) rounded to the dtype and
    `scale` the call's softmax scale, so the planted rows get level(j) step log2 units on top of
    their scores.  Returns (q, k, v, do, levels [B, Sk], planted [Sq])."""
    from oracle.reference import LOG2E

    q, k, v, do = generate_test_data(batch_size, nheads_q, nheads_kv, seqlen_q, seqlen_k, head_dim, dtype, seed, device)
    scale = head_dim ** -0.5 if softmax_scale is None else softmax_scale
    levels = stair_levels(seqlen_k, edges, descending, valid_lens, batch_size, device)
    planted = planted_row_mask(seqlen_q, planted_rows, device)
    c = torch.tensor(step / (LOG2E * STAIR_A * scale), dtype=dtype, device=device)
    with torch.no_grad():
        q[:, :, :, 0] = (planted.to(dtype) * STAIR_A)[None, :, None]
        k[:, :, :, 0] = (levels.to(dtype) * c)[:, :, None]
    return q, k, v, do, levels, planted


def staircase_growth(scores2: Tensor, valid_lens=None, threshold: float = 8.0):
    """What a forward that defers its running max meets, from fp32 scores in log2 units
    [B, H, Sq, Sk] (bias included): 64-key blocks from key 0 of each sequence's valid keys; a row's
    max starts at its first block's and moves to a later block's max only when that outgrows the
    stale max by more than `threshold`.  Returns (growth [B, H, Sq, nblk - 1]: block max minus the
    stale max it met, -inf for blocks past the valid keys; moved: growth > threshold)."""
    b, h, sq, sk = scores2.shape
    s = scores2.float()
    if valid_lens is not None:
        lens = torch.tensor(list(valid_lens), device=s.device)
        s = s.masked_fill((torch.arange(sk, device=s.device)[None, :] >= lens[:, None])[:, None, None, :], float("-inf"))
    nblk = (sk + 63) // 64
    s = torch.nn.functional.pad(s, (0, nblk * 64 - sk), value=float("-inf"))
    bm = s.view(b, h, sq, nblk, 64).amax(-1)
    stale = bm[..., 0].clone()
    growth = []
    for i in range(1, nblk):
        g = bm[..., i] - stale
        growth.append(g)
        stale = torch.where(g > threshold, bm[..., i], stale)
    growth = torch.stack(growth, -1) if growth else s.new_empty(b, h, sq, 0)
    return growth, growth > threshold


def check_staircase_precondition(scores2: Tensor, levels: Tensor, planted: Tensor, step: float, valid_lens=None) -> dict:
    """The staircase's condition on the input, from the oracle's fp32 scores alone (log2 units):
    at every 64-key block where the planted levels say the stale max is outgrown by more than 8
    (level difference x step against the level the max last moved to), EVERY planted row's block
    max exceeds its stale max by more than 8.5; at every other block it stays below 8; and no control
    row ever outgrows its stale max by more than 8.  Returns the extreme figures."""
    growth, _ = staircase_growth(scores2, valid_lens)
    b, sk = levels.shape
    nblk = (sk + 63) // 64
    lens = list(valid_lens) if valid_lens is not None else [sk] * b
    report = {"planted_min_move": float("inf"), "planted_max_stay": float("-inf"), "control_max": float("-inf"), "moves": 0}
    for bi in range(b):
        lv = levels[bi, : lens[bi]].tolist()
        top = [max(lv[i * 64:(i + 1) * 64]) for i in range((lens[bi] + 63) // 64)]
        stale = top[0] if top else 0
        for i in range(1, nblk):
            g = growth[bi, :, :, i - 1]  # [H, Sq]
            gp, gc = g[:, planted], g[:, ~planted]
            if gc.numel():
                report["control_max"] = max(report["control_max"], gc.max().item())
            if not gp.numel():
                continue
            if i < len(top) and (top[i] - stale) * step > 8.0:
                stale = top[i]
                report["moves"] += 1
                report["planted_min_move"] = min(report["planted_min_move"], gp.min().item())
            else:
                report["planted_max_stay"] = max(report["planted_max_stay"], gp.max().item())
    assert report["planted_min_move"] > 8.5, report
    assert report["planted_max_stay"] < 8.0, report
    assert report["control_max"] <= 8.0, report
    return report


def generate_attention_mask(x: Tensor) -> Tensor:
    """Random right padding per batch row, one row unpadded (reference tests/utils.py:40-56)."""
    mask = torch.ones(size=x.shape[:2], dtype=torch.bool, device=x.device)
    if x.size(1) == 1:
        return mask
    padding = torch.randint(low=0, high=x.size(1) - 1, size=(x.size(0),)).tolist()
    padding[torch.randint(low=0, high=x.size(0), size=(1,)).item()] = 0
    for i, pad in enumerate(padding):
        if pad:
            mask[i, -pad:] = False
    return mask


def generate_dropout_seed_and_mask(dropout_p, q, k, attention_mask) -> Tuple[Optional[int], Optional[Tensor]]:
    if dropout_p == 0:
        return None, None
    seed = torch.randint(low=0, high=2**32, size=(1,)).item()
    assert attention_mask is None, "dropout + padding mask is not exercised by the reference tests"
    b, sq, hq, _ = q.shape
    return seed, dropout_keep_mask_torch(seed, dropout_p, b, hq, sq, k.size(1), device=q.device)


def run_case(
    batch_size: int,
    nheads_q: int,
    nheads_kv: int,
    seqlen_q: int,
    seqlen_k: int,
    head_dim: int,
    causal: bool,
    dropout_p: float,
    use_attention: bool,
    use_bias: bool,
    dtype: torch.dtype,
    forward_only: bool,
) -> dict:
    from fa2_triton_amd import flash_attn_func

    q, k, v, do = generate_test_data(batch_size, nheads_q, nheads_kv, seqlen_q, seqlen_k, head_dim, dtype)
    attn_mask = generate_attention_mask(q) if use_attention else None
    attn_bias = torch.rand(size=(1, 1, seqlen_q, seqlen_k), dtype=dtype, device=q.device) if use_bias else None
    dropout_seed, dropout_mask = generate_dropout_seed_and_mask(dropout_p, q, k, attn_mask)
    common = dict(query_padding_mask=attn_mask, key_padding_mask=attn_mask, attn_bias=attn_bias,
                  dropout_p=dropout_p, dropout_mask=dropout_mask, causal=causal)
    out_ref = attention_reference(q, k, v, **common)
    out_pt = attention_reference(q, k, v, upcast=False, reorder_ops=True, **common)
    out = flash_attn_func(q, k, v, attention_mask=attn_mask, attention_bias=attn_bias, dropout_p=dropout_p,
                          causal=causal, softmax_scale=None, dropout_seed=dropout_seed)
    assert out.shape == q.shape and out.dtype == q.dtype
    return check_fa_tolerance(q, k, v, None if forward_only else do, out, out_ref, out_pt)


def unpack_keep_mask(words, b, h, sq, sk):
    """Dense [B, Hq, Sq, Sk] bool view of the tiled keep mask of include/fa2_amd.h (ABI 6; the
    ABI-8 slack tile after the last one is not part of the mask)."""
    nrb, ncw = (sq + 31) // 32, (sk + 31) // 32
    t = words[: b * h * nrb * ncw * 32].view(b, h, nrb, ncw, 32)  # [.., row tile, key word, row in tile]
    bits = (t.unsqueeze(-1) >> torch.arange(32, device=words.device, dtype=torch.int32)) & 1
    dense = bits.permute(0, 1, 2, 4, 3, 5).reshape(b, h, nrb * 32, ncw * 32)
    return dense[:, :, :sq, :sk].bool()


def assert_dropout_dv_vs_oracle(dv_got, dv_other, q, k, v, do, words, p, causal):
    """dV of a dropout backward against the fp32 oracle over the SAME keep bits (the forward's
    saved words, unpacked): the rule of the reference's compare_results_fa for gradients
    (tests/utils.py:127-131, oracle/tolerance.py) with the other backward's dV (the general kernel
    over the same bits) as the baseline: max |dv - ref| <= 3 max |dv_other - ref| + 1e-5.  This
    checks the hand-placed dK/dV's P-pack masking and its one-time 1 / (1 - p) against the exact
    math, not only against the other kernel."""
    b, sq, hq, _ = q.shape
    keep = unpack_keep_mask(words, b, hq, sq, k.size(1))
    qf, kf, vf = (t.detach().float().requires_grad_() for t in (q, k, v))
    out = attention_reference(qf, kf, vf, dropout_p=p, dropout_mask=keep, causal=causal)
    ref = torch.autograd.grad(out, vf, do.float())[0]
    e_got = (dv_got.float() - ref).abs().max().item()
    e_other = (dv_other.float() - ref).abs().max().item()
    assert e_got <= 3 * e_other + 1e-5, f"dv vs fp32 oracle: {e_got:.3e} > 3 x {e_other:.3e} + 1e-5"


def assert_dropout_grads_match(got, want, names=("dq", "dk", "dv")):
    """Gradients of two dropout backwards over the same keep bits.  dQ and dK are bitwise equal
    whichever kernels ran; dV may come from the hand-placed dK/dV, which packs P M and applies
    1 / (1 - p) once to the fp32 sum where the general kernel rounds P M / (1 - p) per score
    (dkdv_hp_kernel.h): within 4 ulps (of the dtype) of the largest |dV|.  (The difference is the
    rounding of each term, so it grows with the number of terms a dV row sums: under a causal mask
    the first keys are visible to every query row and carry both the largest |dV| and the largest
    difference -- the "key % 64 == 0" pattern of DESIGN.md 5 is key 0 of the sequence, at a relative
    difference of 0.5 % like every other key.  assert_dropout_dv_vs_oracle checks dV against the
    exact math.)"""
    for name, x, y in zip(names, got, want):
        if x is None:
            continue
        assert torch.isfinite(x).all(), name
        if name != "dv":
            assert torch.equal(x, y), f"{name}: max |diff| {(x.float() - y.float()).abs().max().item():.3e}"
            continue
        ulp = 2.0 ** -7 if x.dtype == torch.bfloat16 else 2.0 ** -10
        tol = 4 * ulp * y.float().abs().max().item()
        err = (x.float() - y.float()).abs().max().item()
        assert err <= tol, f"dv: max |diff| {err:.3e} > {tol:.3e}"
