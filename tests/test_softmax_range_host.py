"""CPU side of tests/test_softmax_range.py: the staircase generator's precondition over the very
case tables the GPU file runs, and the oracle's `softmax_scale`.
"""
import math

import pytest
import torch

from oracle.reference import attention_reference
from tests.core import STAIR_EDGES_ALIGNED, STAIR_EDGES_MID, stair_levels
from tests.test_softmax_range import (ATTENTION_PARAMS, DECODE_CASES, DTYPE_IDS, DTYPE_LIST, build_decode_inputs,
                                      build_inputs, decode_precondition, precondition, precondition_key)


def _unique_attention():
    seen, params = set(), []
    for c, dtype in ATTENTION_PARAMS:
        key = precondition_key(c, dtype)
        if (c["stair"] or (c["bias"] and c["scale"] is None)) and key not in seen:
            seen.add(key)
            params.append((c, dtype))
    return params


UNIQUE = _unique_attention()


@pytest.mark.parametrize("c,dtype", UNIQUE, ids=[f"{c['id']}-{DTYPE_IDS[dt]}" for c, dt in UNIQUE])
def test_staircase_precondition(c, dtype):
    """Every (shape, dtype, edges, step, rows, scale) combination of groups a - h that plants a
    staircase, in q / k or in the bias (cases that differ only in the mask, the path or the dropout
    share their inputs).  The 12-unit staircases must move the max somewhere unless they descend."""
    report = precondition(c, build_inputs(c, dtype, "cpu"))
    print(c["id"], report)
    assert report is not None
    assert (report["moves"] > 0) == (not c["desc"])


@pytest.mark.parametrize("dtype", DTYPE_LIST, ids=[DTYPE_IDS[dt] for dt in DTYPE_LIST])
@pytest.mark.parametrize("c", [c for c in DECODE_CASES if c["stair"]], ids=[c["id"] for c in DECODE_CASES if c["stair"]])
def test_staircase_precondition_decode(c, dtype):
    report = decode_precondition(c, build_decode_inputs(c, dtype, "cpu"))
    print(c["id"], report)
    assert (report["moves"] > 0) == (not c["desc"])


def test_issue_shape_figures():
    """B = 1, Hq : Hkv = 2 : 1, 96 x 256, D = 128, tile-aligned edges, "third" rows, step 12: every
    later tile moves the max of every planted row by more than 8.5 (three moves), control rows stay
    flat, in both dtypes."""
    from tests.test_softmax_range import case

    c = case("a", 96, 256, 128, b=1, hq=2, hkv=1)
    for dtype in DTYPE_LIST:
        report = precondition(c, build_inputs(c, dtype, "cpu"))
        assert report["moves"] == 3 and report["planted_min_move"] > 8.5 and report["control_max"] < 4, report


def test_stair_levels():
    lv = stair_levels(256, STAIR_EDGES_ALIGNED)
    assert lv.shape == (1, 256) and lv[0, [0, 63, 64, 127, 128, 191, 192, 255]].tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    lv = stair_levels(150, STAIR_EDGES_MID)  # truncated to Sk: the edge at 165 is gone
    assert lv[0, [36, 37, 100, 101, 149]].tolist() == [0, 1, 1, 2, 2]
    lv = stair_levels(256, STAIR_EDGES_ALIGNED, descending=True, valid_lens=(256, 70), batch_size=2)
    assert lv[0, [0, 63, 64, 255]].tolist() == [3, 3, 2, 0]
    assert lv[1, [0, 5, 6, 69, 70, 255]].tolist() == [1, 1, 0, 0, 0, 0]  # reversed along 70 valid keys, 0 past them


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d,s", [(64, 0.5), (64, 0.03125), (16, 1.0), (256, 0.25)])
def test_oracle_softmax_scale_is_a_q_prescale(d, s, causal):
    """attention_reference(..., softmax_scale=s) in fp32 equals the default call on q (s sqrt(d))
    for s sqrt(d) a power of two (every factor exact, the fp32 products reordered): 1e-6 absolute;
    and its autograd dQ is that call's dQ by the chain rule, dQ = (s sqrt(d)) dQ'."""
    f = s * math.sqrt(d)
    assert math.log2(f) == round(math.log2(f))
    torch.manual_seed(0)
    q = torch.empty(2, 40, 4, d).normal_(0, 0.5).requires_grad_()
    k = torch.empty(2, 70, 2, d).normal_(0, 0.5)
    v = torch.empty(2, 70, 2, d).normal_(0, 0.5)
    do = torch.randn(2, 40, 4, d)
    out = attention_reference(q, k, v, causal=causal, softmax_scale=s)
    q2 = (q.detach() * f).requires_grad_()
    out2 = attention_reference(q2, k, v, causal=causal)
    assert (out - out2).abs().max().item() <= 1e-6
    dq = torch.autograd.grad(out, q, do)[0]
    dq2 = torch.autograd.grad(out2, q2, do)[0]
    assert (dq - f * dq2).abs().max().item() <= 1e-6 * max(1.0, f)
    for reorder in (False, True):  # both operand orders take the scale
        o3 = attention_reference(q, k, v, causal=causal, softmax_scale=s, reorder_ops=reorder)
        assert (o3 - out2).abs().max().item() <= 1e-6


def test_oracle_default_scale_is_bitwise_unchanged():
    """softmax_scale=None is the call without the argument, and equals the explicit 1 / sqrt(d)."""
    torch.manual_seed(1)
    q, k, v = torch.randn(1, 33, 2, 40), torch.randn(1, 50, 2, 40), torch.randn(1, 50, 2, 40)
    a = attention_reference(q, k, v, causal=True)
    assert torch.equal(a, attention_reference(q, k, v, causal=True, softmax_scale=None))
    assert torch.equal(a, attention_reference(q, k, v, causal=True, softmax_scale=1.0 / math.sqrt(40)))
