"""Per-element probes: inputs that make every probability P[i, j], and every score gradient
dS[i, j], appear alone in one output element, an fp64 reference, and a per-element checker.

Why: the parity tests accept a tensor by its largest absolute error (oracle/tolerance.py).  Under a
causal mask the first rows (one key, |O| ~ 1) set that allowance and the last rows (long key loops,
the diagonal tile, band edges, padded lengths) are where a misplaced key moves O by only |v| / n.
With a one-hot operand the sum collapses to one term, so one wrong key changes its element by 100 %
and a touched masked element is no longer exactly zero.

The probes.  D is the head dim, T(n) = ceil(n / D); the T probes of a case are T replicas of every
batch entry inside ONE call (replica t of entry b is batch row b T + t), equal but for one operand:
  "o"  (P through O)     V[j, :, c]  = 1 iff j - D t == c   =>  O_t[i, h, c]   = P_h[i, D t + c]
  "dv" (P^T through dV)  dO[i, :, c] = 1 iff i - D t == c   =>  dV_t[j, hk, c] = sum_{h in group} P_h[D t + c, j]
  "dq" (dS through dQ)   K[j, :, c]  = 1 iff j - D t == c   =>  dQ_t[i, h, c]  = scale dS_h[i, D t + c]
  "dk" (dS^T through dK) Q[i, :, c]  = 1 iff i - D t == c   =>  dK_t[j, hk, c] = scale sum_{h in group} dS_h[D t + c, j]
(in "dq" / "dk" the scores are scale Q[i, j - D t], resp. scale K[j, i - D t], inside block t and
0 outside: still a legitimate softmax.)

The reference (`probe_reference`) is dense fp64 in plain torch on the device of its inputs, with the
semantics of oracle/reference.py: GQA by contiguous head groups, key padding, causal / window masks
bottom-right aligned against the *valid* lengths, bias added after masking, rows without a visible
key and padded query rows 0, dropout as keep o P / (1 - p) in O and dV and keep o dP / (1 - p) in dP.
One difference, on purpose: a negative window bound is *no bound* (include/fa2_amd.h; the oracle
reads right = -1 with left >= 0 literally, tests/test_window.py::test_negative_right_is_no_bound),
so (left, -1) here is the oracle's (left, Sk).

The allowance (`check_probe`), per element, u the unit roundoff (2^-8 bf16, 2^-11 fp16):
    |x - ref| <= PROBE_ULPS u M + floor,    PROBE_ULPS = 4
  * elements that expose P:  M = sum_group P (with dropout keep P / (1 - p));
  * elements that expose dS: M = scale sum_group P (|dP| + A_i), A_i = sum_c |dO_ic| |O_ic|;
  both are what `probe_reference` returns as the same contraction as the output with every factor
  replaced by its absolute value, which for a one-hot operand is exactly the figures above;
  * floor = 2^-23 for fp16, 0 for bf16;
  * elements with M == 0 must be exactly 0: outside the causal or window region, padded keys or
    query rows, dropped scores, keys past a cache length, the surplus columns of a partial last
    block, rows whose dO is 0 -- every element whose reference is 0 term by term.  (M >= |ref|, so
    M == 0 implies ref == 0.  The converse fails only by cancellation: on a row with a single
    visible key dS = P (dP - delta) is 0 in exact math while M > 0; the kernels form delta from the
    stored O and dP in an MFMA, two fp32 sums in different orders, so what they return there is a
    rounding residue, held to the allowance like every other element and not to an exact 0.)
  * everything is finite; no element is excluded.
Where the 4 comes from (it is not fitted to anything):
  * the kernels round P, or dS, to 16 bits once before its MFMA, round to nearest even
    (csrc/common.h:51, Elem::from_f32 / pack2), and round the result once on store: 2 u;
  * in the backward, delta = rowsum(dO o O) is formed from the stored 16-bit O: at most u A_i inside
    the bracket of dS = P (dP - delta); with the above 3 u M;
  * the fp32 accumulation of a single non-zero term is exact; exp2, the LSE and the normalisation
    contribute parts in 10^-6; the deferred running max keeps P~ <= 2^8, harmless in relative terms;
  * the fp16 floor covers P~ or an output falling into fp16 subnormals: absolute error 2^-25 each,
    with l >= 1;
  * 4 = 3 + one u of margin.
One term the above leaves out, and where it matters: the stored O carries not only its own store
rounding (u |O_ic|) but the forward's rounding of P before the PV MFMA, up to u sum_j P_ij |V_jc|
(fwd_kernel_body.h and its siblings pack P with Elem::pack2 ahead of the MFMA), which is not small
against |O_ic| where the sum P V cancels.  Under a dense random dO the D terms of delta's error add
like a random walk while A_i adds their magnitudes, so the dQ / dK probes (and dBias in their calls)
keep the allowance above as it stands.  Under the one-hot dO of the "dv" probe delta *is* one
element O_ic, A_i = |O_ic| has no such slack, and dBias of that call -- fp32 sums of unrounded dS
(bwd_kernel.h, dbias_kernel: acc += pr * (dpv + ndel)) -- met 177 u M on the MI355X at elements
with a small |O_ic|.  That tensor alone is therefore held to 4 u M~ with A_i replaced by
A~_i = sum_c |dO_ic| sum_j P_ij |V_jc| >= A_i ("dbias_fwd" below): u (A_i + A~_i) <= 2 u A~_i for
delta, one u for the cast to the bias dtype, one of margin.
"""
import math
from typing import Optional, Tuple

import torch
from torch import Tensor

from oracle.philox import dropout_keep_mask_torch

PROBE_ULPS = 4.0  # see the module docstring for the derivation
KINDS = ("o", "dv", "dq", "dk")
PLANTED = 64.0  # decode: the one-hot value of cache rows past the length (exact in bf16 and fp16)


def unit_roundoff(dtype) -> float:
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]


def probe_floor(dtype) -> float:
    return {torch.bfloat16: 0.0, torch.float16: 2.0 ** -23}[dtype]


def probe_count(n: int, d: int) -> int:
    """T(n) = ceil(n / D), at least one call's worth."""
    return max(1, -(-n // d))


def one_hot_blocks(n: int, heads: int, d: int, dtype, device, t_count: Optional[int] = None) -> Tensor:
    """[T, n, heads, D] with [t, j, :, c] = 1 iff j - D t == c, else 0."""
    t_count = probe_count(n, d) if t_count is None else t_count
    j = torch.arange(n, device=device)[None, :, None]
    t = torch.arange(t_count, device=device)[:, None, None]
    c = torch.arange(d, device=device)[None, None, :]
    hot = (j - d * t == c).to(dtype)  # [T, n, D]
    return hot[:, :, None, :].expand(t_count, n, heads, d).contiguous()


def replicate(x: Optional[Tensor], t_count: int, broadcast: bool = False) -> Optional[Tensor]:
    """Every batch entry T times in a row (entry b, replica t -> row b T + t); `broadcast`: a
    leading dimension of 1 (a bias shared by the batch) stays 1."""
    if x is None or (broadcast and x.size(0) == 1):
        return x
    return x.repeat_interleave(t_count, dim=0)


def build_probe(kind: str, q: Tensor, k: Tensor, v: Tensor, do: Tensor):
    """The four operands of probe `kind` from a case's plain (q, k, v, do): every batch entry
    replicated T times, the probed operand replaced.  Returns (q, k, v, do, T), detached."""
    assert kind in KINDS, kind
    b, sq, hq, d = q.shape
    sk, hkv = k.shape[1], k.shape[2]
    t_count = probe_count(sk if kind in ("o", "dq") else sq, d)
    q, k, v, do = (replicate(x.detach(), t_count) for x in (q, k, v, do))
    if kind == "o":
        v = one_hot_blocks(sk, hkv, d, v.dtype, v.device).repeat(b, 1, 1, 1)
    elif kind == "dv":
        do = one_hot_blocks(sq, hq, d, do.dtype, do.device).repeat(b, 1, 1, 1)
    elif kind == "dq":
        k = one_hot_blocks(sk, hkv, d, k.dtype, k.device).repeat(b, 1, 1, 1)
    else:
        q = one_hot_blocks(sq, hq, d, q.dtype, q.device).repeat(b, 1, 1, 1)
    return q, k, v, do, t_count


def visible_mask(b: int, sq: int, sk: int, causal: bool = False, window: Tuple[int, int] = (-1, -1),
                 query_mask: Optional[Tensor] = None, key_mask: Optional[Tensor] = None, device=None) -> Tensor:
    """[B, 1, Sq, Sk] bool, True where query i sees key j: both inside their valid lengths, and
    j in [i + (Lk - Lq) - left, i + (Lk - Lq) + right] with a negative bound no bound and
    causal forcing right = 0."""
    left, right = window
    if causal:
        right = 0
    i = torch.arange(sq, device=device)[None, None, :, None]
    j = torch.arange(sk, device=device)[None, None, None, :]
    lq = torch.full((b,), sq, device=device) if query_mask is None else query_mask.sum(-1)
    lk = torch.full((b,), sk, device=device) if key_mask is None else key_mask.sum(-1)
    lq, lk = lq.view(b, 1, 1, 1), lk.view(b, 1, 1, 1)
    vis = (i < lq) & (j < lk)
    if query_mask is not None:  # (right padding is what the kernels take; any mask works here)
        vis = vis & query_mask[:, None, :, None]
    if key_mask is not None:
        vis = vis & key_mask[:, None, None, :]
    diag = i + lk - lq
    if left >= 0:
        vis = vis & (j >= diag - left)
    if right >= 0:
        vis = vis & (j <= diag + right)
    return vis


def _group_sum(x: Tensor, hkv: int) -> Tensor:
    """[B, S, Hq, D] -> [B, S, Hkv, D], summing each contiguous group of q heads."""
    b, s, hq, d = x.shape
    return x.view(b, s, hkv, hq // hkv, d).sum(3)


def probe_reference(q: Tensor, k: Tensor, v: Tensor, do: Tensor, query_mask: Optional[Tensor] = None,
                    key_mask: Optional[Tensor] = None, bias: Optional[Tensor] = None, causal: bool = False,
                    window: Tuple[int, int] = (-1, -1), dropout_p: float = 0.0, dropout_seed: Optional[int] = None,
                    softmax_scale: Optional[float] = None) -> dict:
    """Dense fp64 attention forward and backward (module docstring for the semantics).  Returns
    P, O, dP, delta, A, dS ([B, Hq, Sq, Sk] or [B, Hq, Sq]; O [B, Sq, Hq, D]), the keep mask, and
    under "exposed" the pairs (ref, M) of every output tensor: "o", "dq", "dk", "dv", and "dbias"
    when there is a bias (dS summed over the bias's broadcast dims, scale 1; "dbias_fwd": the same
    with the forward's P rounding in delta's allowance, for a one-hot dO)."""
    b, sq, hq, d = q.shape
    sk, hkv = k.shape[1], k.shape[2]
    g = hq // hkv
    scale = 1.0 / math.sqrt(d) if softmax_scale is None else float(softmax_scale)
    q64, do64 = q.detach().double(), do.detach().double()
    k64 = torch.repeat_interleave(k.detach().double(), g, dim=2)
    v64 = torch.repeat_interleave(v.detach().double(), g, dim=2)

    vis = visible_mask(b, sq, sk, causal, window, query_mask, key_mask, q.device)
    s = torch.einsum("bqhd,bkhd->bhqk", q64, k64) * scale
    s = s.masked_fill(~vis, float("-inf"))
    if bias is not None:
        s = s + bias.detach().double()
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)  # exp(-inf) = 0 at every masked score
    l = e.sum(-1, keepdim=True)
    p = torch.where(l > 0, e / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(e))

    keep = None
    if dropout_p > 0.0:
        keep = dropout_keep_mask_torch(dropout_seed, dropout_p, b, hq, sq, sk, device=q.device)
    drop = (lambda x: x) if keep is None else (lambda x: x * keep / (1.0 - dropout_p))
    pd = drop(p)
    o = torch.einsum("bhqk,bkhd->bqhd", pd, v64)
    dp = drop(torch.einsum("bqhd,bkhd->bhqk", do64, v64))
    delta = (do64 * o).sum(-1).transpose(1, 2)  # [B, Hq, Sq]
    a = (do64.abs() * o.abs()).sum(-1).transpose(1, 2)
    ds = p * (dp - delta[..., None])
    w = p * (dp.abs() + a[..., None])  # |dS| before any cancellation

    exposed = {
        "o": (o, torch.einsum("bhqk,bkhd->bqhd", pd, v64.abs())),
        "dv": (_group_sum(torch.einsum("bhqk,bqhd->bkhd", pd, do64), hkv),
               _group_sum(torch.einsum("bhqk,bqhd->bkhd", pd, do64.abs()), hkv)),
        "dq": (scale * torch.einsum("bhqk,bkhd->bqhd", ds, k64), scale * torch.einsum("bhqk,bkhd->bqhd", w, k64.abs())),
        "dk": (scale * _group_sum(torch.einsum("bhqk,bqhd->bkhd", ds, q64), hkv),
               scale * _group_sum(torch.einsum("bhqk,bqhd->bkhd", w, q64.abs()), hkv)),
    }
    if bias is not None:
        dims = [i for i in (0, 1) if bias.size(i) == 1 and ds.size(i) != 1]
        a_fwd = (do64.abs() * exposed["o"][1]).sum(-1).transpose(1, 2)  # A~ of the module docstring
        w_fwd = p * (dp.abs() + a_fwd[..., None])
        reduce = (lambda x: x.sum(dims, keepdim=True)) if dims else (lambda x: x)
        exposed["dbias"] = (reduce(ds), reduce(w))
        exposed["dbias_fwd"] = (reduce(ds), reduce(w_fwd))
    return dict(P=p, O=o, dP=dp, delta=delta, A=a, dS=ds, keep=keep, visible=vis, exposed=exposed, scale=scale)


def check_probe(x: Tensor, ref: Tensor, m: Tensor, dtype=None) -> dict:
    """One tensor against its fp64 reference, element by element (module docstring).  Returns
    ratio: the largest (|x - ref| - floor)+ / (u M) over the elements with M > 0; nonzero: how many
    elements that must be exactly 0 (M == 0) are not; finite; worst: the index of the largest ratio;
    ok: finite, nonzero == 0 and ratio <= PROBE_ULPS."""
    dtype = x.dtype if dtype is None else dtype
    u, floor = unit_roundoff(dtype), probe_floor(dtype)
    assert x.shape == ref.shape == m.shape, (x.shape, ref.shape, m.shape)
    x64 = x.detach().double()
    finite = bool(torch.isfinite(x64).all().item())
    zero = m == 0
    assert not (ref[zero] != 0).any(), "M == 0 where the reference is not: M is not an allowance of this tensor"
    nonzero = int(torch.count_nonzero(x64[zero]).item())
    live = ~zero
    ratio, worst = 0.0, None
    if live.any():
        r = ((x64 - ref).abs() - floor).clamp_min(0.0) / (u * torch.where(live, m, torch.ones_like(m)))
        r = torch.where(live, r, torch.zeros_like(r))
        r = torch.nan_to_num(r, nan=float("inf"))
        flat = int(r.argmax().item())
        ratio = float(r.flatten()[flat].item())
        worst = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), r.shape))
    return dict(ratio=ratio, nonzero=nonzero, finite=finite, worst=worst, live=int(live.sum().item()),
                ok=finite and nonzero == 0 and ratio <= PROBE_ULPS)

