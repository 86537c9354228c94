"""Evidence for the strict xfail of tests/test_softmax_range.py (XFAILS): where the dQ error of a
staircase case sits, and whether the kernel's dQ is what exact fp32 math with one 16-bit rounding
of dS (the MFMA operand) over the stored 16-bit O and LSE2 gives.  Needs the GPU.

    python scripts/diag_softmax_range_dq.py c-hp-d59-256x256-causal-al12asc-bf16 [more ids ...]

Per case: the error of the kernel's dQ, of the low-precision oracle's ("pt") and of four exact-math
emulations against the fp32 oracle (whole tensor, column 0, the other columns), and each one's
distance from the kernel's dQ.  The kernel's error is reproduced by the emulation over its own
stored O and disappears with an fp32 O: it is the rounding of O in delta = rowsum(O o dO), times
scale k0 (k0 = 70, the staircase's top level) in the column where sum_j dS_ij cancels."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle.reference import attention_reference, LOG2E
from tests.test_softmax_range import ATTENTION_CASES, build_inputs, PATHS
from fa2_triton_amd import _lib as L, flash_attn_func
from fa2_triton_amd.forward import _flash_attn_forward

want = sys.argv[1:]
for cid in want:
    cid, dtn = cid.rsplit("-", 1)
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16}[dtn]
    c = next(c for c in ATTENTION_CASES if c["id"] == cid)
    t = build_inputs(c, dtype, "cuda")
    q, k, v, do = t["q"], t["k"], t["v"], t["do"]
    dis = 0
    for n in PATHS[c["path"]]:
        dis |= getattr(L, n)
    L.set_path_policy(dis, 0)
    out = flash_attn_func(q, k, v, None, None, 0.0, c["causal"], c["scale"])
    dq = torch.autograd.grad(out, q, do, retain_graph=True)[0].float()
    with torch.no_grad():
        o, lse, _, _ = _flash_attn_forward(q, k, v, None, None, 0.0, c["causal"], c["scale"], None)
    L.set_path_policy(0, 0)
    ref = attention_reference(q, k, v, causal=c["causal"], softmax_scale=c["scale"])
    pt = attention_reference(q, k, v, causal=c["causal"], softmax_scale=c["scale"], upcast=False, reorder_ops=True)
    gr = torch.autograd.grad(ref, q, do)[0].float()
    gp = torch.autograd.grad(pt, q, do)[0].float()
    g = q.size(2) // k.size(2)
    qf, kf, vf, dof = q.detach().float(), k.detach().float().repeat_interleave(g, 2), v.detach().float().repeat_interleave(g, 2), do.float()
    sq, sk, scale = c["sq"], c["sk"], t["scale"]
    s2 = torch.einsum("bqhd,bkhd->bhqk", qf, kf) * (scale * LOG2E)
    if c["causal"]:
        s2 = s2.masked_fill(torch.arange(sk, device="cuda")[None, :] > torch.arange(sq, device="cuda")[:, None] + (sk - sq), float("-inf"))
    dp = torch.einsum("bqhd,bkhd->bhqk", dof, vf)

    def emul(o_used, lse_used, round_ds=True):
        p = torch.exp2(s2 - lse_used[..., None])
        delta = (o_used.float() * dof).sum(-1).permute(0, 2, 1)[..., None]
        ds = p * (dp - delta)
        if round_ds:
            ds = ds.to(dtype).float()
        return (torch.einsum("bhqk,bkhd->bqhd", ds, kf) * scale).to(dtype).float()

    lse_k = lse[:, :, :sq]
    lse_x = torch.logsumexp(s2 / LOG2E, -1) * LOG2E
    variants = {"kernel": dq, "pt": gp,
                "emul(kernel O, kernel LSE, dS 16-bit)": emul(o, lse_k),
                "emul(kernel O, exact LSE, dS 16-bit)": emul(o, lse_x),
                "emul(fp32 O, exact LSE, dS 16-bit)": emul(attention_reference(qf, k.detach().float(), v.detach().float(), causal=c["causal"], softmax_scale=c["scale"]), lse_x),
                "emul(kernel O, kernel LSE, dS fp32)": emul(o, lse_k, False)}
    print("==", cid, dtn, "max|dq_ref|", gr.abs().max().item(), "max |dq_ref col0|", gr[..., 0].abs().max().item())
    for name, x in variants.items():
        e = (x - gr).abs()
        idx = e.flatten().argmax().item()
        pos = []
        for n in reversed(e.shape):
            pos.append(idx % n); idx //= n
        print(f"  {name:42s} err {e.max().item():.3e} at [b,i,h,d]={pos[::-1]}  col0 {e[..., 0].max().item():.3e}  rest {e[..., 1:].max().item():.3e}"
              f"  |x - kernel| col0 {(x - dq)[..., 0].abs().max().item():.3e} rest {(x - dq)[..., 1:].abs().max().item():.3e}")
