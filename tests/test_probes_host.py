"""CPU tests of tests/probes.py: the probes expose what they claim, the fp64 reference agrees with
the oracle, the low-precision oracle itself stays inside the per-element allowance, planted mask and
tile errors are rejected by it -- and two of them are accepted by the whole-tensor rule
(oracle/tolerance.py), which is the gap the probes close.
"""
import pytest
import torch

from oracle.philox import dropout_keep_mask_torch
from oracle.reference import attention_reference
from oracle.tolerance import check_fa_tolerance
from tests.core import generate_test_data
from tests.probes import (KINDS, PROBE_ULPS, build_probe, check_probe, one_hot_blocks, probe_count, probe_reference,
                          visible_mask)

DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
OUTPUT_OF = {"o": "o", "dv": "dv", "dq": "dq", "dk": "dk"}


def _base(b, hq, hkv, sq, sk, d, dtype):
    return tuple(x.detach() for x in generate_test_data(b, hq, hkv, sq, sk, d, dtype, device="cpu"))


# ------------------------------------------------------------------------------------------------
# the fp64 reference against the oracle


def _oracle_window(window, sk):
    """The oracle reads a negative right bound literally when left >= 0; the library (and
    probe_reference) read it as no bound, which for the oracle is right = Sk."""
    left, right = window
    return (left, sk) if left >= 0 and right < 0 else window


REF_CASES = {
    "full": dict(sq=70, sk=133),
    "causal-sq<sk": dict(sq=70, sk=133, causal=True),
    "causal-sq>sk": dict(sq=133, sk=70, causal=True),  # rows without a visible key
    "window-100-30": dict(sq=130, sk=173, window=(100, 30)),
    "window-none-17": dict(sq=70, sk=133, window=(-1, 17)),
    "window-17-none": dict(sq=70, sk=133, window=(17, -1)),
    "window-0-0": dict(sq=70, sk=133, window=(0, 0)),
    "causal-window-63": dict(sq=133, sk=133, causal=True, window=(63, -1)),
    "padded-full": dict(sq=96, sk=96, lens=(96, 50, 7)),
    "padded-causal": dict(sq=96, sk=96, lens=(96, 50, 7), causal=True),
    "padded-window": dict(sq=96, sk=96, lens=(96, 50, 7), window=(20, 5)),
    "keys-padded-causal": dict(sq=3, sk=96, klens=(96, 50, 1), causal=True),  # the decode form
    "bias-1-1": dict(sq=70, sk=133, bias=(1, 1), causal=True),
    "bias-b-hq": dict(sq=70, sk=133, bias=("B", "Hq")),
    "dropout": dict(sq=70, sk=133, dropout=0.17),
    "dropout-causal": dict(sq=70, sk=133, dropout=0.17, causal=True),
}


@pytest.mark.parametrize("name", list(REF_CASES))
def test_reference_agrees_with_the_oracle(name):
    """probe_reference's O, dQ, dK, dV (and dBias) against `attention_reference` and its autograd on
    float64 inputs: with upcast=True (the oracle's fp32 arithmetic) to 1e-5, and with the oracle
    left in fp64 (upcast=False) to 1e-12.  Plain random operands, so every sum has all its terms."""
    c = dict(causal=False, window=(-1, -1), lens=None, klens=None, bias=None, dropout=0.0)
    c.update(REF_CASES[name])
    lens = c["lens"] or c["klens"]
    b, hq, hkv, d, sq, sk = (len(lens) if lens else 2), 4, 2, 24, c["sq"], c["sk"]
    q, k, v, do = (x.double() for x in _base(b, hq, hkv, sq, sk, d, torch.float32))
    qmask = kmask = bias = keep = None
    if lens:
        kmask = torch.arange(sk)[None, :] < torch.tensor(lens)[:, None]
        qmask = kmask if c["lens"] else None
    if c["bias"]:
        bb, bh = (b if c["bias"][0] == "B" else 1), (hq if c["bias"][1] == "Hq" else 1)
        bias = (torch.rand(bb, bh, sq, sk, dtype=torch.float64) * 2 - 1).requires_grad_()
    p, seed = c["dropout"], 4321
    if p:
        keep = dropout_keep_mask_torch(seed, p, b, hq, sq, sk)

    ref = probe_reference(q, k, v, do, qmask, kmask, bias, c["causal"], c["window"], p, seed)
    for upcast, tol in ((True, 1e-5), (False, 1e-12)):
        ql, kl, vl = (x.clone().requires_grad_() for x in (q, k, v))
        out = attention_reference(ql, kl, vl, qmask, kmask, bias, p, keep, c["causal"], _oracle_window(c["window"], sk),
                                  upcast=upcast)
        assert out.dtype == torch.float64
        wrt = (ql, kl, vl) + ((bias,) if bias is not None else ())
        grads = torch.autograd.grad(out, wrt, do)
        got = dict(o=out, dq=grads[0], dk=grads[1], dv=grads[2])
        if bias is not None:
            got["dbias"] = grads[3]
        for key, x in got.items():
            want, m = ref["exposed"][key]
            assert x.shape == want.shape == m.shape, key
            assert torch.isfinite(want).all() and (m >= want.abs() - 1e-15).all(), key
            err = (x - want).abs().max().item()
            assert err <= tol * max(1.0, want.abs().max().item()), (key, upcast, err)
    if lens and c["lens"]:  # padded rows and keys are exact zeros of the reference
        for key in ("o", "dq", "dk", "dv"):
            want, m = ref["exposed"][key]
            assert torch.count_nonzero(want[~kmask]) == 0 and torch.count_nonzero(m[~kmask]) == 0, key


# ------------------------------------------------------------------------------------------------
# the builders, against brute-force loops at a ragged size


def test_one_hot_blocks_brute_force():
    n, heads, d = 70, 2, 59
    hot = one_hot_blocks(n, heads, d, torch.float32, "cpu")
    assert hot.shape == (probe_count(n, d), n, heads, d) == (2, 70, 2, 59)
    for t in range(hot.size(0)):
        for j in range(n):
            for c in range(d):
                assert (hot[t, j, :, c] == (1.0 if j - d * t == c else 0.0)).all()


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_probes_expose_single_elements(causal):
    """At Sq = 70, Sk = 333, D = 59 (a partial last block on both sides), element by element:
    O_t[i, h, c] = P_h[i, D t + c]; dV_t[j, hk, c] = sum_group P_h[D t + c, j];
    dQ_t[i, h, c] = scale dS_h[i, D t + c]; dK_t[j, hk, c] = scale sum_group dS_h[D t + c, j];
    the surplus columns of the last block are exactly zero, and so is M there."""
    b, hq, hkv, sq, sk, d = 2, 4, 2, 70, 333, 59
    g = hq // hkv
    base = _base(b, hq, hkv, sq, sk, d, torch.bfloat16)
    for kind in KINDS:
        q, k, v, do, t_count = build_probe(kind, *base)
        n = sk if kind in ("o", "dq") else sq
        assert t_count == probe_count(n, d) and q.size(0) == b * t_count
        ref = probe_reference(q, k, v, do, causal=causal)
        x, m = ref["exposed"][kind]
        big = ref["P"] if kind in ("o", "dv") else ref["dS"] * ref["scale"]  # [B T, Hq, Sq, Sk]
        for bi in range(b):
            for t in range(t_count):
                r = bi * t_count + t
                for c in range(d):
                    e = d * t + c
                    if e >= n:
                        assert torch.count_nonzero(x[r, :, :, c]) == 0 and torch.count_nonzero(m[r, :, :, c]) == 0
                        continue
                    if kind in ("o", "dq"):
                        want = big[r, :, :, e].transpose(0, 1)  # [Sq, Hq]
                    else:
                        want = big[r, :, e, :].view(hkv, g, sk).sum(1).transpose(0, 1)  # [Sk, Hkv]
                    assert torch.allclose(x[r, :, :, c], want, rtol=1e-12, atol=1e-15), (kind, bi, t, c)  # (fp64 summation order)
        if kind in ("o", "dv"):  # M is the exposed probability itself
            assert torch.equal(x, m)
        if causal:
            assert (ref["P"][~ref["visible"].expand_as(ref["P"])] == 0).all()


# ------------------------------------------------------------------------------------------------
# the low-precision oracle through the probes, honest and mutated


def _bias_of(vis, dtype):
    """A mask as an additive bias of the oracle (0 where visible, -inf elsewhere)."""
    return torch.zeros(vis.shape, dtype=dtype).masked_fill(~vis, float("-inf"))


def _run_oracle(kind, base, dtype, causal=False, window=(-1, -1), key_mask=None, mutant=None):
    """One probe through `attention_reference(upcast=False, reorder_ops=True)` with its gradients by
    autograd, checked against probe_reference of the honest operation.  `mutant(vis, v)` returns
    the visibility and the V rows the mutated run uses for the rows of the second half."""
    q, k, v, do, t_count = build_probe(kind, *base)
    q, k, v = (x.requires_grad_() for x in (q, k, v))
    km = None if key_mask is None else key_mask.repeat_interleave(t_count, 0)
    sq, sk = q.size(1), k.size(1)
    if mutant is None:
        out = attention_reference(q, k, v, key_padding_mask=km, causal=causal, window_size=window, upcast=False,
                                  reorder_ops=True)
    else:
        vis = visible_mask(q.size(0), sq, sk, causal, window, None, km)
        vis_mut, v_mut = mutant(vis, v)
        low = attention_reference(q, k, v, attn_bias=_bias_of(vis, dtype), upcast=False, reorder_ops=True)
        high = attention_reference(q, k, v_mut, attn_bias=_bias_of(vis_mut, dtype), upcast=False, reorder_ops=True)
        out = torch.cat([low[:, : sq // 2], high[:, sq // 2:]], dim=1)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), do)
    ref = probe_reference(q, k, v, do, None, km, None, causal, window)
    x = dict(o=out, dq=dq, dk=dk, dv=dv)[OUTPUT_OF[kind]]
    return check_probe(x, *ref["exposed"][OUTPUT_OF[kind]])


@DTYPES
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("sq,sk,d", [(256, 256, 64), (130, 333, 64)])
def test_low_precision_oracle_stays_inside_the_allowance(sq, sk, d, causal, dtype, record_property):
    base = _base(1, 2, 1, sq, sk, d, dtype)
    for kind in KINDS:
        r = _run_oracle(kind, base, dtype, causal)
        print("ORACLE_RATIO", kind, sq, sk, d, causal, dtype, f"{r['ratio']:.3f}")
        record_property(f"ratio_{kind}", r["ratio"])
        assert r["finite"] and r["nonzero"] == 0 and r["live"] > 0, (kind, r)
        assert r["ratio"] <= PROBE_ULPS, (kind, r)


def _second_half(vis):
    return (torch.arange(vis.size(2)) >= vis.size(2) // 2)[None, None, :, None]


def _diag_of(vis):
    """The last visible key of each row under a causal mask, [B, 1, Sq, 1]."""
    return vis.long().sum(-1, keepdim=True) - 1


def mutant_diag_wide(vis, v):
    j = torch.arange(vis.size(3))[None, None, None, :]
    return vis | (_second_half(vis) & (j == _diag_of(vis) + 1)), v


def mutant_diag_narrow(vis, v):
    j = torch.arange(vis.size(3))[None, None, None, :]
    return vis & ~(_second_half(vis) & (j == _diag_of(vis))), v


def mutant_window_left(vis, v):
    """The band's left edge one key further left (window (64, 0): the first visible key)."""
    first = vis.long().argmax(-1, keepdim=True)
    j = torch.arange(vis.size(3))[None, None, None, :]
    return vis | (_second_half(vis) & (j == first - 1)), v


def mutant_padded_length(vis, v):
    """One key past the valid length is read."""
    j = torch.arange(vis.size(3))[None, None, None, :]
    return vis | (_second_half(vis) & (j == vis.long().sum(-1, keepdim=True))), v


def mutant_v_neighbour(vis, v):
    """Key 200's V row comes from key 136."""
    idx = torch.arange(v.size(1))
    idx[200] = 136
    return vis, v[:, idx]


def mutant_group_dropped(vis, v):
    """Keys 160..167 are skipped."""
    j = torch.arange(vis.size(3))[None, None, None, :]
    return vis & ~(_second_half(vis) & (j >= 160) & (j < 168)), v


MUTANTS = {
    "diagonal-one-key-wide": (mutant_diag_wide, dict(causal=True)),
    "diagonal-one-key-narrow": (mutant_diag_narrow, dict(causal=True)),
    "window-left-edge-off-by-one": (mutant_window_left, dict(window=(64, 0))),
    "padded-length-off-by-one": (mutant_padded_length, dict(key_len=201)),
    "v-from-the-key-64-earlier": (mutant_v_neighbour, dict()),
    "eight-keys-dropped": (mutant_group_dropped, dict()),
}


@DTYPES
@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutants_are_rejected(name, dtype):
    """Each planted error, on the rows of the second half only, is rejected by the checker on the
    probe that exposes P (and reported for the others); the same run without it is accepted."""
    mutant, kw = MUTANTS[name]
    kw = dict(kw)
    sq = sk = 256
    key_len = kw.pop("key_len", None)
    key_mask = None if key_len is None else (torch.arange(sk) < key_len)[None, :]
    base = _base(1, 2, 1, sq, sk, 64, dtype)
    rejected = {}
    for kind in KINDS:
        honest = _run_oracle(kind, base, dtype, key_mask=key_mask, mutant=lambda vis, v: (vis, v), **kw)
        assert honest["ok"], (kind, honest)
        r = _run_oracle(kind, base, dtype, key_mask=key_mask, mutant=mutant, **kw)
        rejected[kind] = not r["ok"]
        print("MUTANT", name, kind, dtype, {key: r[key] for key in ("ratio", "nonzero", "finite")})
    assert rejected["o"], rejected
    assert rejected["dv"], rejected  # P^T: a wrong key or V row shows in dV as well


@pytest.mark.parametrize("mutant", [mutant_diag_wide, mutant_diag_narrow], ids=["wide", "narrow"])
def test_whole_tensor_rule_accepts_the_diagonal_mutants(mutant):
    """The gap: at (1024, 1024, 128), bf16, causal, on the ordinary N(0, 0.5) data, a causal mask one
    key too wide or too narrow on every row >= 768 -- an fp32 forward, rounded once -- passes
    `check_fa_tolerance`, while it changes the output."""
    s, d, dtype = 1024, 128, torch.bfloat16
    q, k, v, _ = _base(1, 1, 1, s, s, d, dtype)
    out_ref = attention_reference(q, k, v, causal=True)
    out_pt = attention_reference(q, k, v, causal=True, upcast=False, reorder_ops=True)
    vis = visible_mask(1, s, s, causal=True)
    rows = (torch.arange(s) >= 768)[None, None, :, None]
    vis_mut, _ = mutant(vis, v)
    vis_mut = torch.where(rows, vis_mut, vis)
    assert int((vis_mut != vis).sum()) in (255, 256)  # one key on each of those rows (the last row has no key to add)
    honest = attention_reference(q.float(), k.float(), v.float(), attn_bias=_bias_of(vis, torch.float32)).to(dtype)
    out = attention_reference(q.float(), k.float(), v.float(), attn_bias=_bias_of(vis_mut, torch.float32)).to(dtype)
    assert not torch.equal(out[:, 768:], honest[:, 768:]) and torch.equal(out[:, :768], honest[:, :768])
    report = check_fa_tolerance(q, k, v, None, out, out_ref, out_pt)  # raises if the rule rejects it
    print("GAP", report)
    assert report["out"] <= 2 * report["out_pt"] + 5e-5


def test_looped_combinations_all_run_and_every_miss_is_reported():
    """tests/test_probes.py runs its combinations as loops inside three cases (`run_all`): every
    combination runs, the case fails if any of them does, and names each one that did."""
    from tests.test_probes import COMBOS, DECODE_COMBOS, DTYPE_IDS, run_all

    assert len(COMBOS) + len(DECODE_COMBOS) == 398 and {c["group"] for c, _ in COMBOS} == set("abcdef")
    seen = []

    def body(c, dtype):
        seen.append((c["id"], dtype))
        assert len(seen) not in (2, 5), "planted"

    with pytest.raises(AssertionError) as err:
        run_all(COMBOS[:6], body)
    assert len(seen) == 6
    for c, dtype in (COMBOS[1], COMBOS[4]):
        assert f"{c['id']}-{DTYPE_IDS[dtype]}: planted" in str(err.value)
    assert "2 of 6" in str(err.value)
    run_all(COMBOS[:3], lambda c, dtype: None)
    with pytest.raises(RuntimeError):  # anything but a missed assertion ends the loop at once
        run_all(COMBOS[:3], lambda c, dtype: (_ for _ in ()).throw(RuntimeError("launch failed")))
