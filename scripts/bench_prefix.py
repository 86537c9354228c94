"""Shared-prefix (cascade) decode attention against the paged call over aliased prefix blocks:
HIP-event medians, one JSON line.

Shapes: bf16, D = 128, Hq = 32, Hkv = 8, Sq = 1, page_block_size 64, (B, Lp, L_b) in {(64, 6144, 2048),
(8, 28672, 4096), (64, 1024, 7168), (1, 6144, 2048)}: every sequence is Lp prefix keys, the same for
the whole batch, followed by L_b keys of its own.  One pool holds the prefix blocks once and every
sequence's blocks, scattered by a random permutation.
  "aliased" = flash_attn_with_paged_kvcache(q, pool, table, Lp + L_b), every row of the table naming
              the prefix blocks first: what a caller does without the cascade (the prefix costs no
              memory twice, but every batch row attends to it again);
  "prefix"  = flash_attn_with_prefix_kvcache over the same pool through the two column slices of
              that table, with the split counts the library picks.
The two are timed in alternation, round after round (the method of scripts/bench_decode.py), so a
drift of the machine hits both alike; round_spread (max - min over the rounds' medians, over the
median) of both is the margin of prefix_over_aliased.  max_abs_diff is the largest difference of
the two results (they round differently, so it is not zero).

usage: python scripts/bench_prefix.py [--rounds N] [--iters N] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fa2_triton_amd import _lib as L  # noqa: E402
from fa2_triton_amd import flash_attn_with_paged_kvcache, flash_attn_with_prefix_kvcache  # noqa: E402

SHAPES = ((64, 6144, 2048), (8, 28672, 4096), (64, 1024, 7168), (1, 6144, 2048))
HQ, HKV, D, PAGE = 32, 8, 128, 64


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


def split_counts(batch, lp, lb):
    """(aliased, prefix pass, sequence pass) split counts the library picks for the shapes."""
    lib = L.load()
    a = L.PrefixKvCacheArgs()
    s = a.seq.base
    s.batch, s.heads_q, s.heads_kv, s.seqlen_q, s.capacity, s.head_dim = batch, HQ, HKV, 1, lb, D
    s.dtype, s.window_left, s.window_right = L.FA2_BF16, -1, -1
    a.prefix.base.capacity = lp
    n_p, n_s = ctypes.c_int(), ctypes.c_int()
    L.check(lib.fa2_prefix_kvcache_num_splits(ctypes.byref(a), ctypes.byref(n_p), ctypes.byref(n_s)))
    plain = L.KvCacheArgs()
    ctypes.memmove(ctypes.byref(plain), ctypes.byref(s), ctypes.sizeof(plain))
    plain.capacity = lp + lb
    return lib.fa2_kvcache_num_splits(ctypes.byref(plain)), n_p.value, n_s.value


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_prefix.py needs a GPU")
    torch.manual_seed(0)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    shapes = []
    for batch, lp, lb in SHAPES:
        nb_p, nb_s = lp // PAGE, lb // PAGE
        used = nb_p + batch * nb_s
        q = torch.empty(batch, 1, HQ, D, device="cuda", dtype=torch.bfloat16).normal_(0.0, 0.5)
        kp = torch.empty(used, PAGE, HKV, D, device="cuda", dtype=torch.bfloat16).normal_(0.0, 0.5)
        vp = torch.empty(used, PAGE, HKV, D, device="cuda", dtype=torch.bfloat16).normal_(0.0, 0.5)
        ids = torch.randperm(used, device="cuda").to(torch.int32)
        # row b: the prefix blocks, then the blocks of sequence b
        table = torch.cat((ids[:nb_p].expand(batch, nb_p), ids[nb_p:].reshape(batch, nb_s)), dim=1).contiguous()
        table_p, table_s = table[:1, :nb_p], table[:, nb_p:]
        len_all = torch.full((batch,), lp + lb, dtype=torch.int32, device="cuda")
        len_p = torch.full((1,), lp, dtype=torch.int32, device="cuda")
        len_s = torch.full((batch,), lb, dtype=torch.int32, device="cuda")
        variants = {
            "aliased": lambda: flash_attn_with_paged_kvcache(q, kp, vp, table, len_all, causal=True),
            "prefix": lambda: flash_attn_with_prefix_kvcache(q, kp, vp, kp, vp, prefix_seqlen=len_p, cache_seqlens=len_s,
                                                             prefix_block_table=table_p, block_table=table_s, causal=True),
        }
        samples = {n: [] for n in variants}
        with torch.no_grad():
            for fn in variants.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for name, fn in variants.items():
                    samples[name].append(median_ms(fn, args.iters))
            diff = (variants["prefix"]().float() - variants["aliased"]().float()).abs().max().item()
        ms = {n: med(samples[n]) for n in variants}
        n_all, n_p, n_s = split_counts(batch, lp, lb)
        shapes.append({
            "B": batch, "Lp": lp, "L_b": lb, "prefix_share": round(lp / (lp + lb), 4),
            "num_splits": {"aliased": n_all, "prefix_pass": n_p, "sequence_pass": n_s},
            "ms": {n: round(ms[n], 5) for n in variants},
            "round_spread": {n: round((max(samples[n]) - min(samples[n])) / ms[n], 4) for n in variants},
            "prefix_over_aliased": round(ms["prefix"] / ms["aliased"], 4),
            "max_abs_diff": diff,
        })
        del q, kp, vp, variants
        torch.cuda.empty_cache()
    result = {"bench": "prefix", "device": torch.cuda.get_device_name(0), "dtype": "bf16", "Hq": HQ, "Hkv": HKV, "D": D, "Sq": 1,
              "page_block_size": PAGE, "rounds": args.rounds, "iters": args.iters, "shapes": shapes}
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
