"""Per-element probes (tests/probes.py) through every kernel family on the GPU.

Every training case makes one forward call (the P probe, through O) and three forward + backward
calls (P^T through dV, dS through dQ, dS^T through dK); the T = ceil(S / D) probes of a call are T
replicas of each batch entry inside that one call.  The exposed tensor of each call (and dBias, which
*is* dS, in every backward call of a bias case) goes through `check_probe`: |x - ref| <= 4 u M + floor
per element against the dense fp64 reference, exact zeros wherever the reference is masked (outside
the causal or window region, padded keys and query rows, dropped scores, keys past a cache length),
everything finite, no element excluded.  The derivation of the 4 is in tests/probes.py; the largest
ratio (|x - ref| - floor)+ / (u M) of each tensor of each combination is attached to the test's report.

The 398 combinations (case x dtype) run as loops inside three test cases, as `each` of
tests/test_kvcache_fp8.py does, so the suite grows by three cases and not by the product.  Unlike
`each`, a loop here goes on past a combination that misses its allowance and the case fails at the end
with every miss listed (any other error, a failed launch for one, ends it at once); each combination is
printed, and its figures carry its id in the report.

Families (bf16 and fp16; full and causal unless stated; Hq = 4, Hkv = 2, B = 2 before replication):
  a. D = 128 aligned, no bias: hand-placed (default policy), pipelined forward (PATH_FWD_HP off),
     general dQ and dK/dV (all three off); each again under grid caps 2 and 3 (several units per
     workgroup, state carried across units); MHA, MQA
  b. D = 64 pipelined and general; D = 32, 256, 59 general; unequal K / V sequence strides
  c. padded batches, lengths (256, 150, 70)
  d. sliding window (the local kernels), one padded
  e. bias [1, 1, Sq, Sk] and [B, Hq, Sq, Sk], LDS-staged (16-bit, Sk = 256) and element loads
     (fp32, or Sk = 333), with dBias
  f. dropout p = 0.17: saved keep words, forward only under no_grad, backward regenerating the bits
  g. decode over 16-bit caches (contiguous and paged), forward only, with 64 planted in the probe's
     columns of the cache rows past the length
"""
import pytest
import torch

from tests.core import generate_test_data
from tests.probes import (KINDS, PLANTED, PROBE_ULPS, build_probe, check_probe, one_hot_blocks, probe_count,
                          probe_reference, replicate)

pytestmark = pytest.mark.gpu

DTYPE_LIST = (torch.bfloat16, torch.float16)
DTYPE_IDS = {torch.bfloat16: "bf16", torch.float16: "f16"}
FC = (False, True)
VARLEN = (256, 150, 70)
DROPOUT_P, DROPOUT_SEED = 0.17, 1234
# the forward / backward kernels of a launch, by the per-call path policy (fa2_triton_amd._lib)
PATHS = {"hp": (), "pipe": ("PATH_FWD_HP",), "general": ("PATH_FWD_HP", "PATH_DQ_HP", "PATH_DKDV_HP")}
OUTPUT_INDEX = {"dq": 0, "dk": 1, "dv": 2}


def case(group, sq, sk, d, causal=False, path="hp", cap=0, lens=None, window=(-1, -1), unequal=False, bias=None,
         dropout=None, b=2, hq=4, hkv=2, dtypes=DTYPE_LIST):
    """One row of the tables below.  bias: (batch dim, head dim, dtype name), dtype name "same" or
    "fp32"; dropout: "saved" / "nograd" / "regen"."""
    c = dict(group=group, sq=sq, sk=sk, d=d, causal=causal, path=path, cap=cap, lens=lens, window=window, unequal=unequal,
             bias=bias, dropout=dropout, b=len(lens) if lens else b, hq=hq, hkv=hkv, dtypes=dtypes)
    tag = [group, path, f"d{d}", f"{sq}x{sk}", "causal" if causal else "full"]
    if (hq, hkv) != (4, 2):
        tag.append(f"h{hq}_{hkv}")
    if cap:
        tag.append(f"cap{cap}")
    if lens:
        tag.append("varlen")
    if window != (-1, -1):
        tag.append(f"w{window[0]}_{window[1]}")
    if unequal:
        tag.append("kvstrides")
    if bias:
        tag.append(f"bias{bias[0]}_{bias[1]}_{bias[2]}")
    if dropout:
        tag.append(f"drop_{dropout}")
    c["id"] = "-".join(tag)
    return c


SHAPES = [(256, 256), (192, 320), (130, 333), (1, 239)]

# a. D = 128
CASES_A = [case("a", sq, sk, 128, c, path=p) for p in PATHS for (sq, sk) in SHAPES for c in FC]
CASES_A += [case("a", sq, sk, 128, c, path=p, cap=cap, dtypes=DTYPE_LIST if p != "pipe" else DTYPE_LIST[:1])
            for p in PATHS for (sq, sk) in SHAPES[:2] for cap in (2, 3) for c in FC]
CASES_A += [case("a", 256, 256, 128, c, path=p, hq=hq, hkv=hkv, dtypes=DTYPE_LIST if p == "hp" else DTYPE_LIST[:1])
            for p in ("hp", "general") for (hq, hkv) in ((2, 2), (4, 1)) for c in FC]

# b. other head dims, unequal K / V sequence strides (the general forward)
CASES_B = [case("b", sq, sk, 64, c, path=p) for p in ("pipe", "general") for (sq, sk) in (SHAPES[0], SHAPES[2]) for c in FC]
CASES_B += [case("b", sq, sk, d, c, path="general") for d in (32, 256, 59) for (sq, sk) in (SHAPES[0], SHAPES[2]) for c in FC]
CASES_B += [case("b", sq, sk, 128, c, unequal=True) for (sq, sk) in (SHAPES[0], SHAPES[2]) for c in FC]

# c. padded batches
CASES_C = [case("c", 256, 256, d, c, lens=VARLEN) for d in (64, 128) for c in FC]
CASES_C += [case("c", 256, 256, 128, c, lens=VARLEN, path="general", dtypes=DTYPE_LIST[:1]) for c in FC]

# d. sliding window
WINDOWS = [(False, (64, 0)), (False, (100, 30)), (False, (-1, 17)), (False, (17, -1)), (False, (0, 0)), (True, (63, -1))]
CASES_D = [case("d", sq, sk, d, c, window=w) for d in (64, 128) for (c, w) in WINDOWS for (sq, sk) in SHAPES[:3]]
CASES_D += [case("d", 256, 256, d, False, window=(100, 30), lens=VARLEN) for d in (64, 128)]

# e. bias
CASES_E = [case("e", sq, sk, d, c, bias=(bb, bh, bdt))
           for d in (64, 128) for (bb, bh) in ((1, 1), ("B", "Hq")) for (sq, sk, bdt) in
           ((192, 256, "same"), (192, 256, "fp32"), (130, 333, "same")) for c in FC]

# f. dropout (fp16 on the saved-words path only)
CASES_F = [case("f", sq, sk, d, c, dropout=mode, dtypes=DTYPE_LIST if mode == "saved" else DTYPE_LIST[:1])
           for mode in ("saved", "nograd", "regen") for d in (128, 64) for (sq, sk) in (SHAPES[0], SHAPES[2]) for c in FC]

CASES = CASES_A + CASES_B + CASES_C + CASES_D + CASES_E + CASES_F
assert len({c["id"] for c in CASES}) == len(CASES)
COMBOS = [(c, dt) for c in CASES for dt in c["dtypes"]]


def run_all(combos, body):
    """`body(c, dtype)` for every combination; the AssertionErrors are gathered and raised together."""
    misses = []
    for c, dtype in combos:
        try:
            body(c, dtype)
        except AssertionError as err:
            misses.append(f"{c['id']}-{DTYPE_IDS[dtype]}: {err}")
    assert not misses, f"{len(misses)} of {len(combos)} combinations:\n" + "\n".join(misses)


@pytest.fixture
def policy():
    from fa2_triton_amd import _lib as L

    yield L
    L.set_path_policy(0, 0)


def _report(results, record_property, tag):
    """Print and attach every figure, then assert them all."""
    print("PROBE_RATIO", tag, " ".join(f"{name}={r['ratio']:.3f}" for name, r in results.items()))
    for name, r in results.items():
        record_property(f"ratio_{name}[{tag}]", r["ratio"])
    for name, r in results.items():
        assert r["finite"], f"{name}: not finite"
        assert r["live"] > 0, f"{name}: nothing exposed"
        assert r["nonzero"] == 0, f"{name}: {r['nonzero']} elements that must be exactly 0 are not"
        assert r["ratio"] <= PROBE_ULPS, f"{name}: {r['ratio']:.2f} u M > {PROBE_ULPS} u M at {r['worst']}"


def _attention_case(c, dtype, policy, record_property, monkeypatch):
    from fa2_triton_amd import flash_attn_func

    b, hq, hkv, sq, sk, d = c["b"], c["hq"], c["hkv"], c["sq"], c["sk"], c["d"]
    base = tuple(x.detach() for x in generate_test_data(b, hq, hkv, sq, sk, d, dtype))
    mask0 = bias0 = None
    if c["lens"]:
        mask0 = torch.arange(sk, device="cuda")[None, :] < torch.tensor(c["lens"], device="cuda")[:, None]
    if c["bias"]:
        bb, bh, bdt = c["bias"]
        bb, bh = (b if bb == "B" else 1), (hq if bh == "Hq" else 1)
        bias0 = (torch.rand(bb, bh, sq, sk, device="cuda") * 2 - 1).to(dtype if bdt == "same" else torch.float32)
    p = DROPOUT_P if c["dropout"] else 0.0
    seed = DROPOUT_SEED if c["dropout"] else None
    if c["dropout"] == "regen":  # the keep-mask buffer is refused: the backward draws the bits again
        monkeypatch.setenv("FA2_DROPOUT_MASK_MAX_GB", "0")
    disable = 0
    for name in PATHS[c["path"]]:
        disable |= getattr(policy, name)

    results = {}
    for kind in (("o",) if c["dropout"] == "nograd" else KINDS):
        q, k, v, do, t_count = build_probe(kind, *base)
        mask = replicate(mask0, t_count)
        bias = replicate(bias0, t_count, broadcast=True)
        if c["unequal"]:  # as test_layouts.py::test_kv_unequal_seq_strides: K's sequence stride is twice V's
            wide = torch.zeros(k.size(0), sk, 2 * hkv, d, device="cuda", dtype=dtype)
            wide[:, :, :hkv] = k
            k = wide[:, :, :hkv]
            assert k.stride(1) != v.stride(1)
        grad = c["dropout"] != "nograd"
        if grad:
            q, k, v = (x.requires_grad_() for x in (q, k, v))
            if bias is not None:
                bias = bias.clone().requires_grad_()
        policy.set_path_policy(disable, c["cap"])
        try:
            with torch.enable_grad() if grad else torch.no_grad():
                out = flash_attn_func(q, k, v, mask, bias, p, c["causal"], None, seed, c["window"])
                grads = None
                if kind != "o":
                    grads = torch.autograd.grad(out, (q, k, v) + ((bias,) if bias is not None else ()), do)
            torch.cuda.synchronize()
        finally:
            policy.set_path_policy(0, 0)

        ref = probe_reference(q, k, v, do, mask, mask, bias, c["causal"], c["window"], p, seed)
        x = out if kind == "o" else grads[OUTPUT_INDEX[kind]]
        assert x.dtype == dtype
        results[kind] = check_probe(x, *ref["exposed"][kind])
        if grads is not None and bias is not None:
            assert grads[3].shape == bias.shape and grads[3].dtype == bias.dtype
            # (the one-hot dO of the "dv" probe: delta's allowance with the forward's P rounding, tests/probes.py)
            results[f"dbias_{kind}"] = check_probe(grads[3], *ref["exposed"]["dbias_fwd" if kind == "dv" else "dbias"],
                                                   dtype=dtype)
    _report(results, record_property, f"{c['id']}-{DTYPE_IDS[dtype]}")


def _attention_probes(groups, policy, record_property, monkeypatch):
    def body(c, dtype):
        with monkeypatch.context() as patch:  # (the "regen" environment ends with its combination)
            _attention_case(c, dtype, policy, record_property, patch)

    combos = [(c, dt) for c, dt in COMBOS if c["group"] in groups]
    assert combos
    run_all(combos, body)


def test_attention_probes(policy, record_property, monkeypatch):
    """Families a - d: no bias, no dropout (hand-placed, pipelined, general and local kernels)."""
    _attention_probes("abcd", policy, record_property, monkeypatch)


def test_attention_probes_bias_dropout(policy, record_property, monkeypatch):
    """Families e and f: bias with dBias, dropout three ways."""
    _attention_probes("ef", policy, record_property, monkeypatch)


# g. decode: lengths (1, 200, 333, 512), one batch row each, capacity 512
DECODE_LENS, DECODE_CAP = (1, 200, 333, 512), 512
DECODE_CASES = [dict(api=api, d=d, sq=sq, nsplit=n, window=(-1, -1))
                for api in ("cache", "paged16", "paged64") for d in (64, 128) for sq in (1, 3) for n in (1, 3, 0)]
DECODE_CASES += [dict(api=api, d=d, sq=3, nsplit=3, window=(100, 0)) for api in ("cache", "paged16", "paged64") for d in (64, 128)]
for _c in DECODE_CASES:
    _c["id"] = "-".join(["g", _c["api"], f"d{_c['d']}", f"sq{_c['sq']}", f"splits{_c['nsplit'] or 'auto'}"] +
                        ([f"w{_c['window'][0]}"] if _c["window"] != (-1, -1) else []))
assert len({c["id"] for c in DECODE_CASES}) == len(DECODE_CASES)
DECODE_COMBOS = [(c, dt) for c in DECODE_CASES for dt in DTYPE_LIST]
assert len(COMBOS) + len(DECODE_COMBOS) <= 400


def test_decode_probes(record_property):
    """Family g, every combination of DECODE_COMBOS (_decode_case)."""
    run_all(DECODE_COMBOS, lambda c, dtype: _decode_case(c, dtype, record_property))


def _decode_case(c, dtype, record_property):
    """The P probe through `flash_attn_with_kvcache` / `flash_attn_with_paged_kvcache` (shuffled block
    table): the one-hot V lives in the cache, and holds 64 instead of 1 on the rows past each length,
    so a key read past the length shows as a large element where O must be exactly zero."""
    from fa2_triton_amd import flash_attn_with_kvcache, flash_attn_with_paged_kvcache
    from tests.test_kvcache_paged import _pool

    hq, hkv, d, sq, cap = 4, 2, c["d"], c["sq"], DECODE_CAP
    b, t_count = len(DECODE_LENS), probe_count(cap, d)
    torch.manual_seed(0)
    q = torch.empty((b, sq, hq, d), dtype=dtype, device="cuda").normal_(0.0, 0.5)
    kc = torch.empty((b, cap, hkv, d), dtype=dtype, device="cuda").normal_(0.0, 0.5)
    q, kc = replicate(q, t_count), replicate(kc, t_count)
    lens = replicate(torch.tensor(DECODE_LENS, dtype=torch.int32, device="cuda"), t_count)
    key_mask = torch.arange(cap, device="cuda")[None, :] < lens[:, None]
    vc = one_hot_blocks(cap, hkv, d, dtype, "cuda").repeat(b, 1, 1, 1)
    vc = torch.where(key_mask[:, :, None, None], vc, vc * PLANTED)
    assert vc[~key_mask].max().item() == PLANTED

    kw = dict(cache_seqlens=lens, causal=True, window_size=c["window"], num_splits=c["nsplit"])
    if c["api"] == "cache":
        out = flash_attn_with_kvcache(q, kc, vc, **kw)
    else:
        kp, vp, table, _ = _pool(kc, vc, int(c["api"][5:]))
        out = flash_attn_with_paged_kvcache(q, kp, vp, table, **kw)
    torch.cuda.synchronize()
    assert out.shape == q.shape and out.dtype == dtype

    ref = probe_reference(q, kc, vc, torch.zeros_like(q), None, key_mask, None, True, c["window"])
    want, m = ref["exposed"]["o"]
    past = (torch.arange(d, device="cuda")[None, :] + d * torch.arange(t_count, device="cuda").repeat(b)[:, None]
            >= lens[:, None])  # [B T, D]: the columns of keys at or past the length
    assert torch.count_nonzero(m.transpose(1, 3)[past.nonzero(as_tuple=True)[0], past.nonzero(as_tuple=True)[1]]) == 0
    _report({"o": check_probe(out, want, m)}, record_property, f"{c['id']}-{DTYPE_IDS[dtype]}")
