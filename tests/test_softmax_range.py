"""The softmax under a running row max that moves after the first tile, and under a softmax scale
other than 1 / sqrt(D).

The forward kernels defer the running max (kDeferMax = 8 log2 units, csrc/common.h): O and l are
rescaled only when some row of a wave outgrows its stale max by more than that.  With N(0, 0.5)
inputs and the default scale the scores of a row stay within about 2 log2 units, so the only
rescale any other test takes is the first tile's move away from -inf, on a zero accumulator.  Here
a staircase planted in head-dim column 0 (tests/core.generate_staircase_data), or made by the bias,
lifts the scores of the planted rows by 12 log2 units per level (every tile moves the max), or by
5 (the max moves on the third tile only, and P up to 2^5 is packed against a stale max before and
after), through every forward: hand-placed, pipelined, general (8-wave ping-pong and 4-wave),
sliding-window and the split-KV decode kernels; with masked keys that hold the largest scores
(causal diagonal, padding, keys outside the band, cache rows past the length), bias and dropout.
The backward kernels see the peaked P that results.  `softmax_scale` in {0.03, 0.25, 1.0} runs
through the same paths with the oracle given the same scale.

Acceptance is the project's rule everywhere (oracle/tolerance.py: 2 x + 5e-5 for O, 3 x + 1e-5 for
gradients, against the low-precision reordered oracle's own error, which must be > 0), no escape
taken, LSE2 within 1e-3 of lse2_reference where there is no window, everything finite.  The
staircase's precondition (tests/core.check_staircase_precondition) is checked on the inputs each
case really uses; tests/test_softmax_range_host.py checks it on the CPU for the same tables.
"""
import pytest
import torch

from oracle import tolerance
from oracle.reference import LOG2E, attention_reference, lse2_reference
from oracle.tolerance import check_fa_tolerance
from tests.core import (STAIR_EDGES_ALIGNED, STAIR_EDGES_MID, check_staircase_precondition, generate_staircase_data,
                        generate_test_data, planted_row_mask, stair_levels)

pytestmark = pytest.mark.gpu

DTYPE_LIST = (torch.bfloat16, torch.float16)
DTYPE_IDS = {torch.bfloat16: "bf16", torch.float16: "f16"}
DTYPES = pytest.mark.parametrize("dtype", DTYPE_LIST, ids=[DTYPE_IDS[dt] for dt in DTYPE_LIST])
AL, MID = STAIR_EDGES_ALIGNED, STAIR_EDGES_MID
WIDE = (128, 256, 384)  # decode only: cache rows past a length of 200 hold levels no visible key has
WAVE1 = (64, 128)  # planted rows 64..127: one wave's rows, the neighbouring waves never vote
BIAS_STEP_NATS = 8.0  # exact in bf16 and fp16 at levels 1..3; 11.5 log2 units
SHAPES = [(192, 256), (130, 333), (1, 239), (256, 256)]
VARLEN = (256, 150, 70)
# the forward / backward kernels of a launch, by the per-call path policy (fa2_triton_amd._lib)
PATHS = {"hp": (), "pipe": ("PATH_FWD_HP",), "general": ("PATH_FWD_HP", "PATH_DQ_HP", "PATH_DKDV_HP")}


def case(group, sq, sk, d, causal=False, edges=AL, step=12, desc=False, rows="third", path="hp", scale=None, lens=None,
         window=(-1, -1), unequal=False, bias=None, dropout=0.0, stair=True, b=2, hq=4, hkv=2):
    """One row of the tables below.  bias: None or (batch dim, head dim, dtype name) with dtype name
    "same" / "fp32"; the bias then carries the staircase (stair says whether q / k do)."""
    c = dict(group=group, sq=sq, sk=sk, d=d, causal=causal, edges=edges, step=step, desc=desc, rows=rows, path=path,
             scale=scale, lens=lens, window=window, unequal=unequal, bias=bias, dropout=dropout, stair=stair,
             b=len(lens) if lens else b, hq=hq, hkv=hkv)
    tag = [group, path, f"d{d}", f"{sq}x{sk}", "causal" if causal else "full"]
    if stair or bias:
        tag.append(("al" if edges == AL else "mid") + f"{step}" + ("desc" if desc else "asc"))
        if rows != "third":
            tag.append(f"rows{rows[0]}_{rows[1]}")
    if scale is not None:
        tag.append(f"scale{scale}")
    if lens:
        tag.append("varlen")
    if window != (-1, -1):
        tag.append(f"w{window[0]}_{window[1]}")
    if unequal:
        tag.append("kvstrides")
    if bias:
        tag.append(f"bias{bias[0]}_{bias[1]}_{bias[2]}")
    if dropout:
        tag.append(f"p{dropout}")
    c["id"] = "-".join(tag)
    return c


STAIRS3 = [dict(edges=AL, step=12), dict(edges=MID, step=5), dict(edges=MID, step=12, desc=True)]
STAIRS2 = STAIRS3[:2]
FC = (False, True)

# a. hand-placed forward (D = 128, aligned, no bias; default policy), hand-placed dQ and dK/dV
def table_d128(group, path):
    t = [case(group, 192, 256, 128, c, path=path, **st) for c in FC for st in STAIRS2]
    t += [case(group, 192, 256, 128, False, edges=AL, step=5, path=path),
          case(group, 192, 256, 128, True, edges=MID, step=12, path=path),
          case(group, 192, 256, 128, False, edges=AL, desc=True, path=path),
          case(group, 192, 256, 128, True, edges=MID, desc=True, path=path),
          case(group, 256, 256, 128, False, rows=WAVE1, path=path),
          case(group, 256, 256, 128, True, rows=WAVE1, path=path),
          case(group, 192, 256, 128, False, rows=WAVE1, path=path, **STAIRS2[1])]
    for (sq, sk) in SHAPES[1:]:
        t += [case(group, sq, sk, 128, False, path=path, **STAIRS2[0]), case(group, sq, sk, 128, True, path=path, **STAIRS2[1])]
    t.append(case(group, 130, 333, 128, True, path=path, **STAIRS3[2]))
    return t


CASES_A = table_d128("a", "hp")

# b. pipelined forward: the same D = 128 cases with the hand-placed forward off, D = 64; and with
#    all three hand-placed paths off (the general dQ and dK/dV on peaked P)
CASES_B = table_d128("b", "pipe")
for (_sq, _sk) in SHAPES:
    CASES_B += [case("b", _sq, _sk, 64, False, path="pipe", **STAIRS2[0]), case("b", _sq, _sk, 64, True, path="pipe", **STAIRS2[1])]
CASES_B += [case("b", 192, 256, 64, True, path="pipe", **STAIRS3[2]), case("b", 256, 256, 64, False, path="pipe", rows=WAVE1)]
for (_sq, _sk) in SHAPES[:2]:
    CASES_B += [case("b", _sq, _sk, 128, False, path="general", **STAIRS2[0]),
                case("b", _sq, _sk, 128, True, path="general", **STAIRS2[1])]

# c. general forward: other head-dim tiles, the unaligned head dim, unequal K / V sequence strides;
#    full is the 8-wave ping-pong form (4 waves at D = 256), causal the 4-wave one
CASES_C = [case("c", 256, 256, d, c, **st) for d in (32, 256, 59) for c in FC for st in STAIRS2]
CASES_C += [case("c", 130, 333, d, c, **st) for d in (32, 256, 59) for (c, st) in zip(FC, STAIRS2)]
CASES_C += [case("c", 256, 256, 32, True, **STAIRS3[2]), case("c", 256, 256, 32, False, rows=WAVE1), case("c", 1, 239, 32)]
CASES_C += [case("c", 256, 256, 128, False, unequal=True), case("c", 256, 256, 128, True, unequal=True),
            case("c", 256, 256, 128, True, unequal=True, **STAIRS2[1]), case("c", 130, 333, 128, False, unequal=True)]

# d. masked keys hold the largest scores: the causal mid-tile cases are in a - c; varlen with the
#    staircase ascending over the whole padded length (padded keys carry the top levels), and
#    descending over the valid length
CASES_D = [case("d", 256, 256, d, c, edges=e, lens=VARLEN, path=p)
           for (d, p) in [(128, "hp"), (64, "pipe"), (32, "hp")] for (c, e) in [(False, AL), (True, MID)]]
CASES_D += [case("d", 256, 256, 128, True, edges=MID, step=5, lens=VARLEN),
            case("d", 256, 256, 128, True, edges=MID, desc=True, lens=VARLEN),
            case("d", 256, 256, 64, False, edges=AL, desc=True, lens=VARLEN, path="pipe")]

# e. the staircase made by the bias alone (plain q, k): 16-bit bias with Sk % 8 == 0 is the
#    pipelined forward with LDS-staged bias tiles; fp32 bias and Sk = 333 the general forward
CASES_E = [case("e", 192, 256, 64, False, stair=False, bias=(1, 1, "same")),
           case("e", 192, 256, 64, True, stair=False, bias=("B", "Hq", "same")),
           case("e", 192, 256, 128, True, stair=False, bias=(1, 1, "same")),
           case("e", 192, 256, 128, False, stair=False, bias=("B", "Hq", "same")),
           case("e", 192, 256, 128, True, edges=MID, stair=False, bias=(1, 1, "same")),
           case("e", 192, 256, 128, False, stair=False, bias=("B", "Hq", "fp32")),
           case("e", 192, 256, 128, True, stair=False, bias=("B", "Hq", "fp32")),
           case("e", 130, 333, 64, False, stair=False, bias=(1, 1, "same")),
           case("e", 130, 333, 128, True, stair=False, bias=(1, 1, "same"))]

# f. dropout over the staircase: the hand-placed forward reading saved keep words (D = 128), the
#    general forward (D = 64)
CASES_F = [case("f", sq, sk, d, c, dropout=0.2, **st)
           for d in (128, 64) for c in FC for ((sq, sk), st) in zip(SHAPES[:2], STAIRS2)]

# g. sliding window (the LOCAL kernels): ascending the max moves inside the band; descending the
#    keys just left of the band, in the band's first tile, hold larger scores than any visible key
WINDOWS = [(False, (40, 40)), (True, (100, -1))]
CASES_G = [case("g", 256, 256, d, c, edges=MID, desc=ds, window=w) for d in (64, 128) for (c, w) in WINDOWS for ds in FC]
CASES_G += [case("g", 130, 333, 64, False, edges=MID, window=(40, 40)), case("g", 130, 333, 128, False, edges=MID, desc=True, window=(40, 40)),
            case("g", 130, 333, 128, True, edges=MID, window=(100, -1)), case("g", 130, 333, 64, True, edges=MID, desc=True, window=(100, -1))]

# h. softmax_scale other than 1 / sqrt(D), plain inputs (scale 1.0: organically peaked rows)
PATHS_H = [(128, "hp", False), (128, "pipe", False), (128, "general", False), (64, "pipe", False), (32, "hp", False),
           (256, "hp", False), (59, "hp", False), (128, "hp", True)]
CASES_H = [case("h", 130, 333, d, c, stair=False, scale=s, path=p, unequal=u)
           for (d, p, u) in PATHS_H for (s, c) in [(0.03, True), (1.0, False)]]
CASES_H += [case("h", 256, 256, 128, False, stair=False, scale=0.03), case("h", 256, 256, 128, True, stair=False, scale=1.0)]
CASES_H += [case("h", 192, 256, 128, False, stair=False, scale=s, bias=bi)
            for (s, bi) in [(1.0, ("B", "Hq", "same")), (0.03, (1, 1, "fp32"))]]
CASES_H += [case("h", 192, 256, 128, True, stair=False, scale=1.0, dropout=0.2),
            case("h", 256, 256, 128, False, stair=False, scale=1.0, window=(40, 40)),
            case("h", 256, 256, 128, True, stair=False, scale=1.0, lens=VARLEN),
            case("h", 192, 256, 128, False, scale=0.25), case("h", 192, 256, 128, True, edges=MID, scale=0.25)]

ATTENTION_CASES = CASES_A + CASES_B + CASES_C + CASES_D + CASES_E + CASES_F + CASES_G + CASES_H
assert len({c["id"] for c in ATTENTION_CASES}) == len(ATTENTION_CASES)


def scores_log2(q, k, scale, bias=None):
    """fp32 scores in log2 units [B, Hq, Sq, Sk], bias included, nothing masked."""
    kf = torch.repeat_interleave(k.detach().float(), q.size(2) // k.size(2), dim=2)
    s = torch.einsum("bqhd,bkhd->bhqk", q.detach().float(), kf) * scale
    if bias is not None:
        s = s + bias.detach().float()
    return s * LOG2E


def build_inputs(c, dtype, device):
    """The tensors of a case, on any device (the CPU test checks the precondition on its own draw)."""
    b, hq, hkv, sq, sk, d = c["b"], c["hq"], c["hkv"], c["sq"], c["sk"], c["d"]
    scale = d ** -0.5 if c["scale"] is None else c["scale"]
    levels = planted = None
    if c["stair"]:
        q, k, v, do, levels, planted = generate_staircase_data(
            b, hq, hkv, sq, sk, d, dtype, c["edges"], c["step"], c["rows"], c["desc"], c["scale"], c["lens"], device=device)
    else:
        q, k, v, do = generate_test_data(b, hq, hkv, sq, sk, d, dtype, device=device)
    bias = None
    if c["bias"]:
        bb, bh, bdt = c["bias"]
        bb, bh = (b if bb == "B" else 1), (hq if bh == "Hq" else 1)
        bdt = dtype if bdt == "same" else torch.float32
        if c["scale"] is None:  # the bias-made staircase
            levels = stair_levels(sk, c["edges"], False, None, b, device)
            planted = planted_row_mask(sq, c["rows"], device)
            bias = (planted[:, None] * levels[0][None, :] * BIAS_STEP_NATS).to(bdt).expand(bb, bh, sq, sk).contiguous()
        else:  # group h: the plain bias of tests/test_layouts.py under another scale
            bias = (torch.rand(bb, bh, sq, sk, device=device) * 2 - 1).to(bdt)
        bias.requires_grad_()
    if c["unequal"]:  # as test_kv_unequal_seq_strides: K's sequence stride is twice V's
        wide = torch.zeros(b, sk, 2 * hkv, d, device=device, dtype=dtype)
        wide[:, :, :hkv] = k.detach()
        k = wide[:, :, :hkv].requires_grad_()
        assert k.stride(1) != v.stride(1)
    mask = None
    if c["lens"]:
        mask = torch.arange(sk, device=device)[None, :] < torch.tensor(c["lens"], device=device)[:, None]
    return dict(q=q, k=k, v=v, do=do, bias=bias, mask=mask, levels=levels, planted=planted, scale=scale)


def precondition(c, t):
    """check_staircase_precondition on a case's own tensors; None when it plants no staircase."""
    if t["levels"] is None:
        return None
    step = BIAS_STEP_NATS * LOG2E if c["bias"] else c["step"]
    return check_staircase_precondition(scores_log2(t["q"], t["k"], t["scale"], t["bias"]), t["levels"], t["planted"],
                                        step, c["lens"])


def precondition_key(c, dtype):
    """What the precondition depends on (not the mask kind, the path or the dropout)."""
    return (c["b"], c["hq"], c["hkv"], c["sq"], c["sk"], c["d"], dtype, c["edges"], c["step"], c["desc"], c["rows"],
            c["scale"], c["lens"], c["bias"], c["stair"])


@pytest.fixture
def policy():
    from fa2_triton_amd import _lib as L

    yield L
    L.set_path_policy(0, 0)


def ratios(report, dbias=None):
    """err / (mul err_pt + bias) of the rule, per tensor: <= 1 passes."""
    r = {"out": report["out"] / (2 * report["out_pt"] + 5e-5)}
    for name in ("dq", "dk", "dv"):
        if name in report:
            r[name] = report[name] / (3 * report[name + "_pt"] + 1e-5)
    if dbias is not None:
        r["dbias"] = dbias[0] / (3 * dbias[1] + 1e-5)
    return r


# bf16 and fp16 throughout; dropout over the staircase in bf16 only
ATTENTION_PARAMS = [(c, dt) for c in ATTENTION_CASES for dt in ((torch.bfloat16,) if c["dropout"] else DTYPE_LIST)]


# Known misses of the rule, kept in as strict expected failures (the project carries one more,
# tests/test_gqa_split.py).
XFAILS = {
    ("c-hp-d59-256x256-causal-al12asc", torch.bfloat16):
        "dq_kernel (unaligned, D = 59), bf16: dQ err 1.362e-01 > 3 x err_pt 4.169e-02 + 1e-5, at dQ[1, 192, 3, 0]; O, dK, dV "
        "and every other dQ column are within 0.1 of their bounds.  Causal row 192 sees one key of the top level, so "
        "P ~ 1 there and dQ[:, 0] = scale k0 sum_j dS_ij with k0 = 70: a sum that cancels exactly in exact math and is "
        "left with scale k0 times the error of delta = rowsum(O o dO), which FlashAttention-2 (the reference too, "
        "compute_delta.py) forms from the stored 16-bit O.  Exact fp32 math over the kernel's stored O and LSE2 with dS "
        "rounded once reproduces the kernel's dQ (same 1.362e-01 at the same element), the same math over an fp32 O "
        "gives 3.1e-02; autograd through the low-precision oracle never rounds O, so err_pt has no such term.  The "
        "fp16 twin and every other path sit at 0.13 - 0.93 of the dQ bound on these inputs for the same reason "
        "(scripts/diag_softmax_range_dq.py).",
}
ATTENTION_PYTEST_PARAMS = [
    pytest.param(c, dt, id=f"{c['id']}-{DTYPE_IDS[dt]}",
                 marks=[pytest.mark.xfail(strict=True, reason=XFAILS[(c["id"], dt)])] if (c["id"], dt) in XFAILS else [])
    for c, dt in ATTENTION_PARAMS]


@pytest.mark.parametrize("c,dtype", ATTENTION_PYTEST_PARAMS)
def test_attention(c, dtype, policy):
    """Groups a - h through `flash_attn_func`: O, dQ, dK, dV (and dBias) by the rule, LSE2, padded rows."""
    from fa2_triton_amd import flash_attn_func
    from fa2_triton_amd.forward import _flash_attn_forward
    from fa2_triton_amd.utils import dropout_mask_words
    from oracle.philox import dropout_keep_mask_torch

    b, hq, sq, sk = c["b"], c["hq"], c["sq"], c["sk"]
    t = build_inputs(c, dtype, "cuda")
    q, k, v, do, bias, mask = t["q"], t["k"], t["v"], t["do"], t["bias"], t["mask"]
    pre = precondition(c, t)
    p, seed = c["dropout"], (1234 if c["dropout"] else None)
    keep = dropout_keep_mask_torch(seed, p, b, hq, sq, sk, device=q.device) if p else None
    disable = 0
    for name in PATHS[c["path"]]:
        disable |= getattr(policy, name)

    policy.set_path_policy(disable, 0)
    out = flash_attn_func(q, k, v, mask, bias, p, c["causal"], c["scale"], seed, c["window"])
    wrt = (q, k, v) + ((bias,) if bias is not None else ())
    grads = torch.autograd.grad(out, wrt, do, retain_graph=True)
    lse = None
    if c["window"] == (-1, -1):
        words = torch.empty(dropout_mask_words(b, hq, sq, sk), dtype=torch.int32, device=q.device) if p else None
        with torch.no_grad():
            _, lse, _, _ = _flash_attn_forward(q, k, v, mask, bias, p, c["causal"], c["scale"], seed, dropout_mask=words)
    torch.cuda.synchronize()
    policy.set_path_policy(0, 0)
    assert out.shape == q.shape and out.dtype == q.dtype

    common = dict(query_padding_mask=mask, key_padding_mask=mask, attn_bias=bias, dropout_p=p, dropout_mask=keep,
                  causal=c["causal"], window_size=c["window"], softmax_scale=c["scale"])
    out_ref = attention_reference(q, k, v, **common)
    out_pt = attention_reference(q, k, v, upcast=False, reorder_ops=True, **common)
    dbias = None
    if bias is not None:  # the rule of test_bias_gradient
        g_ref = torch.autograd.grad(out_ref, bias, do, retain_graph=True)[0]
        g_pt = torch.autograd.grad(out_pt, bias, do, retain_graph=True)[0]
        dbias = ((grads[3].float() - g_ref.float()).abs().max().item(), (g_pt.float() - g_ref.float()).abs().max().item())
    before = dict(tolerance.ESCAPES)
    try:
        report = check_fa_tolerance(q, k, v, do, out, out_ref, out_pt, grads=grads[:3])
    finally:
        print(c["id"], dtype, "precondition", pre)
    print(c["id"], dtype, {key: f"{val:.3e}" for key, val in report.items()}, "dbias", dbias)
    print("RATIO", c["group"], c["id"], str(dtype), " ".join(f"{n}={x:.4f}" for n, x in ratios(report, dbias).items()))
    assert tolerance.ESCAPES["ulp"] == before["ulp"] and tolerance.ESCAPES["dv_sum"] == before["dv_sum"], report
    assert report["out_pt"] > 0, "the low-precision oracle is exact: the rule has no scale"
    if dbias is not None:
        assert grads[3].shape == bias.shape and grads[3].dtype == bias.dtype
        assert dbias[0] <= 3 * dbias[1] + 1e-5, dbias
    names = ("out", "dq", "dk", "dv", "dbias")
    for name, g in zip(names, (out,) + tuple(grads)):
        assert torch.isfinite(g).all(), name
    if mask is not None:
        for name, g in zip(names, (out,) + tuple(grads)):
            assert torch.count_nonzero(g[~mask]) == 0, name

    if lse is not None:
        want = lse2_reference(q, k, attn_bias=bias, causal=c["causal"], padding_mask=mask, softmax_scale=c["scale"])
        got = lse[:, :, :sq]
        finite = torch.isfinite(want)
        rows = finite if mask is None else finite & mask[:, None, :]
        assert torch.allclose(got[rows], want[rows], rtol=1e-3, atol=1e-3), (got[rows] - want[rows]).abs().max()
        if mask is None:
            assert torch.all(torch.isneginf(got[~finite]))


# i. decode: caches [2, 512, 2, D], Hq = 8, lengths (512, 200), causal; the staircase ascending over
#    the whole capacity (rows at or past L_b hold the top levels and must stay invisible) or
#    descending over the valid length.  With 4 splits the splits' LSEs differ by more than 30 log2
#    units, so the combine's weights run to 2^-30 and below.
DECODE_LENS = (512, 200)


def dcase(d, sq, nsplit, edges=AL, desc=False, window=(-1, -1), scale=None, stair=True, step=12):
    c = dict(d=d, sq=sq, nsplit=nsplit, edges=edges, desc=desc, window=window, scale=scale, stair=stair, step=step,
             rows="third", lens=DECODE_LENS)
    tag = ["i", f"d{d}", f"sq{sq}", f"splits{nsplit}"]
    if stair:
        tag.append({AL: "al", MID: "mid", WIDE: "wide"}[edges] + ("desc" if desc else "asc"))
    if window != (-1, -1):
        tag.append(f"w{window[0]}")
    if scale is not None:
        tag.append(f"scale{scale}")
    c["id"] = "-".join(tag)
    return c


DECODE_CASES = [dcase(d, sq, 4, e, ds) for d in (64, 128) for sq in (1, 3) for (e, ds) in [(WIDE, False), (MID, True)]]
DECODE_CASES += [dcase(64, 1, 1, WIDE), dcase(64, 3, 1, MID, True), dcase(128, 1, 1, MID, True), dcase(128, 3, 1, WIDE)]
DECODE_CASES += [dcase(128, 1, 4, AL), dcase(64, 3, 1, AL)]
DECODE_CASES += [dcase(64, 3, 4, WIDE, window=(64, -1)), dcase(64, 3, 1, MID, True, window=(64, -1)),
                 dcase(128, 3, 1, WIDE, window=(64, -1)), dcase(128, 3, 4, MID, True, window=(64, -1))]
DECODE_CASES += [dcase(128, 3, n, stair=False, scale=1.0) for n in (1, 4)]
DECODE_CASES += [dcase(64, 3, 4, WIDE, scale=0.03), dcase(128, 3, 1, WIDE, scale=0.03)]
assert len({c["id"] for c in DECODE_CASES}) == len(DECODE_CASES)


def build_decode_inputs(c, dtype, device):
    """q [2, Sq, 8, D] and the caches [2, 512, 2, D] as tests/test_kvcache._data draws them, with the
    staircase of generate_staircase_data planted in column 0."""
    from tests.core import STAIR_A

    b, hq, hkv, cap, d, sq = 2, 8, 2, 512, c["d"], c["sq"]
    torch.manual_seed(0)
    q = torch.empty((b, sq, hq, d), dtype=dtype, device=device).normal_(0.0, 0.5)
    kc = torch.empty((b, cap, hkv, d), dtype=dtype, device=device).normal_(0.0, 0.5)
    vc = torch.empty((b, cap, hkv, d), dtype=dtype, device=device).normal_(0.0, 0.5)
    scale = d ** -0.5 if c["scale"] is None else c["scale"]
    levels = planted = None
    if c["stair"]:
        levels = stair_levels(cap, c["edges"], c["desc"], c["lens"], b, device)
        planted = planted_row_mask(sq, c["rows"], device)
        cc = torch.tensor(c["step"] / (LOG2E * STAIR_A * scale), dtype=dtype, device=device)
        q[:, :, :, 0] = (planted.to(dtype) * STAIR_A)[None, :, None]
        kc[:, :, :, 0] = (levels.to(dtype) * cc)[:, :, None]
    return dict(q=q, k=kc, v=vc, bias=None, levels=levels, planted=planted, scale=scale)


def decode_precondition(c, t):
    if t["levels"] is None:
        return None
    return check_staircase_precondition(scores_log2(t["q"], t["k"], t["scale"]), t["levels"], t["planted"], c["step"], c["lens"])


@DTYPES
@pytest.mark.parametrize("c", DECODE_CASES, ids=[c["id"] for c in DECODE_CASES])
def test_decode(c, dtype):
    """`flash_attn_with_kvcache` by the forward rule and LSE2 (the helpers of tests/test_kvcache.py
    with the scale), and `flash_attn_with_paged_kvcache` (P = 16) bitwise equal to it."""
    from fa2_triton_amd import flash_attn_with_kvcache, flash_attn_with_paged_kvcache
    from tests.test_kvcache import _check, _lens
    from tests.test_kvcache_paged import _pool

    t = build_decode_inputs(c, dtype, "cuda")
    q, kc, vc = t["q"], t["k"], t["v"]
    pre = decode_precondition(c, t)
    kw = dict(cache_seqlens=_lens(c["lens"]), softmax_scale=c["scale"], causal=True, window_size=c["window"],
              num_splits=c["nsplit"], return_lse=True)
    out, lse = flash_attn_with_kvcache(q, kc, vc, **kw)
    print(c["id"], dtype, "precondition", pre)
    ref, pt = _check(q, kc, vc, c["lens"], out, lse, True, c["window"], softmax_scale=c["scale"])
    err, err_pt = (out.float() - ref.float()).abs().max().item(), (pt.float() - ref.float()).abs().max().item()
    print("RATIO", "i", c["id"], str(dtype), f"out={err / (2 * err_pt + 5e-5):.4f}")
    assert err_pt > 0, "the low-precision oracle is exact: the rule has no scale"
    assert torch.isfinite(lse).all()  # every row sees a key
    if c["edges"] == WIDE and c["stair"]:
        # planted row 0 of the full-length sequence: the LSEs of its first and last 128 keys (two of
        # the 4 splits) are more than 30 log2 units apart, and meet in the combine
        s2 = scores_log2(q[:1, :1], kc[:1], t["scale"])[0, :, 0]
        gap = (torch.logsumexp(s2[:, 384:] / LOG2E, -1) - torch.logsumexp(s2[:, :128] / LOG2E, -1)) * LOG2E
        assert gap.min().item() > 30, gap

    kp, vp, table, _ = _pool(kc, vc, 16)
    got = flash_attn_with_paged_kvcache(q, kp, vp, table, **kw)
    assert torch.equal(got[0], out), (got[0].float() - out.float()).abs().max()
    assert torch.equal(got[1], lse)
