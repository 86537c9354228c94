"""The unit hand-over of the persistent hand-placed kernels (D = 128) with ONE workgroup walking
every unit.

`set_path_policy(0, grid_cap=1)` launches the forward, dQ and dK/dV with a single workgroup, so
every unit but the first starts from what the previous unit left behind: the next unit's K / V
(forward, dQ) or V rows, step-0 tiles and K fragments (dK/dV) requested before the epilogue, dQ's
next Q / dO fragments in flight in the operand registers across it, delta and LSE2 of the next
unit's rows after it, the dK/dV statement's requests of steps 1 and 2 in its prologue, and each
wave's step classes (masked / unmasked / dead query tiles, computed in closed form per unit).

Two checks per case:
* bitwise equal to the uncapped launch (one unit per workgroup at these sizes, or few);
* the reference's rule against the fp32 oracle (oracle/tolerance.py), since a self-comparison
  cannot see an error both launches share.
The per-element probes of tests/probes.py run under the same cap for the plain and the varlen
case: a tile read from a buffer that is still being staged or refilled moves an element by 100 %.

The shapes are the smallest that reach each path: three 256-row / 256-key blocks (a mirrored pair
plus the lone middle block under a causal mask, both K / V buffer parities in the forward and
dQ); Lq != Lk with partial last blocks (the next unit's O / LSE2 rows past Lq read as zeros,
delta 0); a 40-token sequence in a 512-token batch (units without any tile: range-0 requests); a
whole GQA group per dK/dV block with 1 - 3 steps per head (the steps requested in the statement's
prologue belong to the next q-head); dropout (four dK/dV step buffers, dQ's own next-unit
statement).
"""
import pytest
import torch

from oracle.philox import dropout_keep_mask_torch
from oracle.reference import attention_reference
from oracle.tolerance import check_fa_tolerance
from tests.core import generate_test_data
from tests.probes import KINDS, PROBE_ULPS, build_probe, check_probe, probe_reference, replicate

NAMES = ("out", "dq", "dk", "dv")
BF16, F16 = torch.bfloat16, torch.float16


@pytest.fixture
def policy():
    from fa2_triton_amd import _lib as L

    yield L
    L.set_path_policy(0, 0)


def _fwd_bwd(q, k, v, do, causal, policy, cap, mask=None, dropout_p=0.0, seed=None):
    from fa2_triton_amd import flash_attn_func

    policy.set_path_policy(0, cap)
    try:
        out = flash_attn_func(q, k, v, mask, None, dropout_p, causal, None, seed)
        grads = torch.autograd.grad(out, (q, k, v), do)
        torch.cuda.synchronize()
    finally:
        policy.set_path_policy(0, 0)
    return [t.detach().clone() for t in (out,) + tuple(grads)]


def _check(shape, causal, dtype, policy, lens=None, dropout_p=0.0, seed=None):
    b, hq, hkv, sq, sk = shape
    q, k, v, do = generate_test_data(b, hq, hkv, sq, sk, 128, dtype)
    mask = keep = None
    if lens:
        mask = torch.arange(sk, device="cuda")[None, :] < torch.tensor(lens, device="cuda")[:, None]
    full = _fwd_bwd(q, k, v, do, causal, policy, 0, mask, dropout_p, seed)
    one = _fwd_bwd(q, k, v, do, causal, policy, 1, mask, dropout_p, seed)
    for name, a, c in zip(NAMES, one, full):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, c), f"{name}: one workgroup vs the full grid, max |diff| {(a.float() - c.float()).abs().max().item():.3e}"
    if dropout_p > 0:
        keep = dropout_keep_mask_torch(seed, dropout_p, b, hq, sq, sk, device=q.device)
    common = dict(query_padding_mask=mask, key_padding_mask=mask, dropout_p=dropout_p, dropout_mask=keep, causal=causal)
    out_ref = attention_reference(q, k, v, **common)
    out_pt = attention_reference(q, k, v, upcast=False, reorder_ops=True, **common)
    report = check_fa_tolerance(q, k, v, do, one[0], out_ref, out_pt, grads=one[1:])
    print("HANDOVER", shape, causal, dtype, {n: f"{report[n]:.3e} (pt {report[n + '_pt']:.3e})" for n in NAMES})


# (tag, (b, hq, hkv, sq, sk), causal, dtype, options)
CASES = [("plain-causal-bf16", (1, 3, 3, 768, 768), True, BF16, {}),
         ("plain-full-bf16", (1, 3, 3, 768, 768), False, BF16, {}),
         ("plain-causal-f16", (1, 3, 3, 768, 768), True, F16, {}),
         ("padded-rows", (1, 2, 2, 300, 700), True, BF16, {})]
CASES += [(f"empty-units-{'causal' if c else 'full'}", (2, 2, 2, 512, 512), c, BF16, dict(lens=(512, 40))) for c in (True, False)]
# a whole GQA group per dK/dV block (the q-head split off, as tests/test_hp_paths.py does)
CASES += [(f"q-head-change-{sq}-{'causal' if c else 'full'}", (1, 4, 1, sq, 300), c, BF16, dict(whole_group=True))
          for sq in (32, 64, 96) for c in (True, False)]
CASES += [("dropout", (1, 2, 2, 512, 512), True, BF16, dict(dropout_p=0.1, seed=1234))]

# (tag, b, hq, hkv, s, lens, causal): the plain and the varlen case above
PROBE_CASES = [(f"probe-{name}-{'causal' if c else 'full'}", b, hq, hkv, s, lens, c)
               for (name, b, hq, hkv, s, lens) in (("plain", 1, 3, 3, 768, None), ("varlen", 2, 2, 2, 512, (512, 40)))
               for c in (True, False)]


def _probes(b, hq, hkv, s, lens, causal, policy):
    """Every P (O, dV probes) and dS (dQ, dK probes) element of the capped launch, each against
    the dense fp64 reference within PROBE_ULPS u M; masked and padded elements exactly 0."""
    from fa2_triton_amd import flash_attn_func

    base = tuple(x.detach() for x in generate_test_data(b, hq, hkv, s, s, 128, BF16))
    mask0 = None
    if lens:
        mask0 = torch.arange(s, device="cuda")[None, :] < torch.tensor(lens, device="cuda")[:, None]
    results = {}
    for kind in KINDS:
        q, k, v, do, t_count = build_probe(kind, *base)
        mask = replicate(mask0, t_count)
        q, k, v = (x.requires_grad_() for x in (q, k, v))
        policy.set_path_policy(0, 1)
        try:
            out = flash_attn_func(q, k, v, mask, None, 0.0, causal, None, None)
            grads = torch.autograd.grad(out, (q, k, v), do) if kind != "o" else None
            torch.cuda.synchronize()
        finally:
            policy.set_path_policy(0, 0)
        ref = probe_reference(q, k, v, do, mask, mask, None, causal)
        x = out if kind == "o" else grads[{"dq": 0, "dk": 1, "dv": 2}[kind]]
        results[kind] = check_probe(x, *ref["exposed"][kind])
    print("HANDOVER_PROBE", b, hq, s, lens, causal, " ".join(f"{n}={r['ratio']:.3f}" for n, r in results.items()))
    for name, r in results.items():
        assert r["finite"], f"{name}: not finite"
        assert r["live"] > 0, f"{name}: nothing exposed"
        assert r["nonzero"] == 0, f"{name}: {r['nonzero']} elements that must be exactly 0 are not"
        assert r["ratio"] <= PROBE_ULPS, f"{name}: {r['ratio']:.2f} u M > {PROBE_ULPS} u M at {r['worst']}"


@pytest.mark.gpu
def test_unit_handover(policy, monkeypatch):
    """Every case of CASES and PROBE_CASES in one test (as tests/test_probes.py: the suite grows
    by one case, about five seconds in all); the misses are gathered and raised together."""
    misses = []
    for tag, shape, causal, dtype, opt in CASES:
        opt = dict(opt)
        try:
            with monkeypatch.context() as patch:
                if opt.pop("whole_group", False):
                    patch.setenv("FA2_DKV_SPLIT", "0")
                _check(shape, causal, dtype, policy, **opt)
        except AssertionError as err:
            misses.append(f"{tag}: {err}")
    for tag, b, hq, hkv, s, lens, causal in PROBE_CASES:
        try:
            _probes(b, hq, hkv, s, lens, causal, policy)
        except AssertionError as err:
            misses.append(f"{tag}: {err}")
    assert not misses, f"{len(misses)} of {len(CASES) + len(PROBE_CASES)} cases:\n" + "\n".join(misses)
