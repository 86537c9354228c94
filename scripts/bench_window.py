"""Sliding-window kernels against the full-causal kernels: HIP-event medians of the forward, dQ
and dK/dV launches, one JSON line.

Shape: bf16, D = 128, causal, B = 4, H = 16, S = 8192; window_size = (left, -1) for left in
{256, 1024, 4096}.  Baselines, same shape, full causal: "general" = the hand-placed paths off
(_lib.set_path_policy(7): the pipelined forward and the general dQ / dK-dV the windowed kernels
derive from), "default" = the default policy (the hand-placed kernels).  The variants are timed
in alternation, round after round, so a drift of the machine hits all of them alike.

usage: python scripts/bench_window.py [--rounds N] [--iters N] [--seqlen S] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fa2_triton_amd import _lib as L  # noqa: E402
from fa2_triton_amd.backward import _flash_attn_backward  # noqa: E402
from fa2_triton_amd.forward import _flash_attn_forward  # noqa: E402

LEFTS = (256, 1024, 4096)


def median_ms(fn, iters):
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--seqlen", type=int, default=8192)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_window.py needs a GPU")
    B, H, S, D = args.batch, args.heads, args.seqlen, 128
    torch.manual_seed(0)
    q, k, v = (torch.empty(B, S, H, D, device="cuda", dtype=torch.bfloat16).normal_(0.0, 0.5) for _ in range(3))
    do = torch.randn_like(q)

    # variant -> (path policy, window)
    variants = {"general": (7, (-1, -1)), "default": (0, (-1, -1))}
    variants.update({f"left{w}": (0, (w, -1)) for w in LEFTS})
    state = {}
    for name, (policy, window) in variants.items():
        L.set_path_policy(policy, 0)
        o, lse, scale, _ = _flash_attn_forward(q, k, v, None, None, 0.0, True, None, None, window_size=window)
        state[name] = dict(o=o, lse=lse, scale=scale, delta=torch.empty_like(lse))
    L.set_path_policy(0, 0)

    def run(name, kind):
        policy, window = variants[name]
        st = state[name]
        L.set_path_policy(policy, 0)
        if kind == "fwd":
            _flash_attn_forward(q, k, v, None, None, 0.0, True, None, None, window_size=window)
        else:  # dQ (stage bit 2) writes the delta that dK/dV (bit 1) reads
            _flash_attn_backward(do, q, k, v, None, None, st["o"], st["lse"], 0.0, True, st["scale"], None,
                                 _stages=4 if kind == "dq" else 2, _delta=st["delta"], window_size=window)

    kinds = ("fwd", "dq", "dkdv")
    samples = {n: {kd: [] for kd in kinds} for n in variants}
    for name in variants:  # warm-up: code objects loaded, delta written
        for kd in kinds:
            for _ in range(3):
                run(name, kd)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for kd in kinds:
            for name in variants:
                samples[name][kd].append(median_ms(lambda: run(name, kd), args.iters))
    L.set_path_policy(0, 0)

    def med(xs):
        xs = sorted(xs)
        return xs[len(xs) // 2]

    ms = {n: {kd: round(med(samples[n][kd]), 4) for kd in kinds} for n in variants}
    spread = {n: {kd: round((max(samples[n][kd]) - min(samples[n][kd])) / med(samples[n][kd]), 4) for kd in kinds}
              for n in variants}
    result = {
        "bench": "window", "device": torch.cuda.get_device_name(0), "dtype": "bf16", "causal": True,
        "B": B, "H": H, "S": S, "D": D, "rounds": args.rounds, "iters": args.iters,
        "ms": ms, "round_spread": spread,
        "vs_general": {f"left{w}": {kd: round(ms[f"left{w}"][kd] / ms["general"][kd], 4) for kd in kinds} for w in LEFTS},
        "vs_default": {f"left{w}": {kd: round(ms[f"left{w}"][kd] / ms["default"][kd], 4) for kd in kinds} for w in LEFTS},
    }
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
