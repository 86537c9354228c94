"""KV-cache decode attention against the training forward on the same shapes: HIP-event medians,
one JSON line.

Shapes: bf16, D = 128, Hq = 32, Hkv = 8, Sq = 1, full-length caches, (B, L) in {(1, 8192),
(1, 131072), (8, 32768), (64, 8192)}.  "kvcache" = flash_attn_with_kvcache(q, k_cache, v_cache)
with the split count the library picks; "baseline" = flash_attn_func(q, k_cache, v_cache) under
no_grad, the kernels a caller had to use before (one workgroup per q-head walking all keys).  The
two are timed in alternation, round after round, so a drift of the machine hits both alike.

Per shape: both times, their ratio, the split count, and the visible K + V bytes / time as a
fraction of the copy bandwidth bench_micro/hbm_copy.hip measures on the same box (--hbm-copy-bin
runs that binary first; --copy-gbps passes a figure).  Shapes whose K + V footprint is under the
256 MiB last-level cache are marked: their figure is a cache figure, not an HBM one.

--page-block-size P [P ...] adds, per shape and per P, a "paged_pP" variant: flash_attn_with_paged_kvcache
over a pool holding the same keys and values in blocks of P rows, placed by a shuffled block table.
It is timed in the same alternation and reported as paged_over_kvcache[P], next to the round spread
of both variants, which is the margin of that ratio.  --page-order identity leaves the blocks in
place (table[b, j] = b * max_blocks + j).  Without --page-block-size the output is unchanged.

--fp8 adds an "fp8" variant: flash_attn_with_fp8_kvcache over e4m3 caches of the same shape (random
bytes of N(0, 1) values, descales 0.5 per (batch, kv head) as device tensors), and with
--page-block-size a "fp8_paged_pP" variant per P over pools placed by the same kind of table.  They
are timed in the same alternation and reported as fp8_over_kvcache (and fp8_paged_over_kvcache[P]),
with fp8_kv_GBps (the fp8 call's K + V bytes, half the 16-bit call's, over its time) and its
fraction of the copy bandwidth; round_spread of both variants is the margin of the ratio.

usage: python scripts/bench_decode.py [--rounds N] [--iters N] [--hbm-copy-bin PATH | --copy-gbps X]
                                      [--page-block-size P [P ...]] [--page-order shuffled|identity] [--fp8]
                                      [--out FILE]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fa2_triton_amd import _lib as L  # noqa: E402
from fa2_triton_amd import (flash_attn_func, flash_attn_with_fp8_kvcache, flash_attn_with_kvcache,  # noqa: E402
                            flash_attn_with_paged_kvcache)

SHAPES = ((1, 8192), (1, 131072), (8, 32768), (64, 8192))
HQ, HKV, D = 32, 8, 128
LLC_BYTES = 256 << 20


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


def measured_copy_gbps(binary):
    """best_copy_GBps of bench_micro/hbm_copy (its last output line), run as a child process."""
    res = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    if res.returncode != 0:
        raise SystemExit(f"{binary} failed: {res.stderr}")
    return float(json.loads(res.stdout.strip().splitlines()[-1])["best_copy_GBps"])


def split_count(batch, cap):
    a = L.KvCacheArgs()
    a.batch, a.heads_q, a.heads_kv, a.seqlen_q, a.capacity, a.head_dim = batch, HQ, HKV, 1, cap, D
    a.dtype, a.window_left, a.window_right = L.FA2_BF16, -1, -1
    return L.load().fa2_kvcache_num_splits(ctypes.byref(a))


def paged_copy(kc, vc, page, order):
    """(k_pool, v_pool, table): the caches [B, cap, Hkv, D] cut into blocks of `page` rows that a
    random permutation scatters over pools of exactly B * cap / page blocks (order "identity":
    left in place, which separates the cost of the lookup from the cost of scattered addresses)."""
    batch, cap, hkv, d = kc.shape
    n = batch * cap // page
    ids = torch.randperm(n, device=kc.device) if order == "shuffled" else torch.arange(n, device=kc.device)
    kp, vp = torch.empty((n, page, hkv, d), dtype=kc.dtype, device=kc.device), torch.empty((n, page, hkv, d), dtype=kc.dtype, device=kc.device)
    kp[ids] = kc.reshape(n, page, hkv, d)
    vp[ids] = vc.reshape(n, page, hkv, d)
    return kp, vp, ids.reshape(batch, cap // page).to(torch.int32)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--hbm-copy-bin", default=None)
    ap.add_argument("--copy-gbps", type=float, default=None)
    ap.add_argument("--page-block-size", type=int, nargs="+", default=[])
    ap.add_argument("--page-order", choices=("shuffled", "identity"), default="shuffled")
    ap.add_argument("--fp8", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    copy_gbps = measured_copy_gbps(args.hbm_copy_bin) if args.hbm_copy_bin else args.copy_gbps
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode.py needs a GPU")
    torch.manual_seed(0)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    shapes = []
    for batch, cap in SHAPES:
        q = torch.empty(batch, 1, HQ, D, device="cuda", dtype=torch.bfloat16).normal_(0.0, 0.5)
        kc = torch.empty(batch, cap, HKV, D, device="cuda", dtype=torch.bfloat16).normal_(0.0, 0.5)
        vc = torch.empty(batch, cap, HKV, D, device="cuda", dtype=torch.bfloat16).normal_(0.0, 0.5)
        variants = {"kvcache": lambda: flash_attn_with_kvcache(q, kc, vc),
                    "baseline": lambda: flash_attn_func(q, kc, vc)}
        for page in args.page_block_size:
            kp, vp, table = paged_copy(kc, vc, page, args.page_order)
            variants[f"paged_p{page}"] = (lambda kp=kp, vp=vp, table=table:
                                          flash_attn_with_paged_kvcache(q, kp, vp, table, cap))
        if args.fp8:
            # byte caches (uint8 for the scatter, viewed as e4m3 for the call) and device descales
            k8 = torch.empty(batch, cap, HKV, D, device="cuda").normal_().to(torch.float8_e4m3fn).view(torch.uint8)
            v8 = torch.empty(batch, cap, HKV, D, device="cuda").normal_().to(torch.float8_e4m3fn).view(torch.uint8)
            kd, vd = torch.full((batch, HKV), 0.5, device="cuda"), torch.full((batch, HKV), 0.5, device="cuda")
            f8 = lambda t: t.view(torch.float8_e4m3fn)
            variants["fp8"] = lambda: flash_attn_with_fp8_kvcache(q, f8(k8), f8(v8), kd, vd)
            for page in args.page_block_size:
                kp8, vp8, table8 = paged_copy(k8, v8, page, args.page_order)
                variants[f"fp8_paged_p{page}"] = (lambda kp=kp8, vp=vp8, table=table8: flash_attn_with_fp8_kvcache(
                    q, f8(kp), f8(vp), kd, vd, block_table=table, cache_seqlens=cap))
        samples = {n: [] for n in variants}
        with torch.no_grad():
            for fn in variants.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for name, fn in variants.items():
                    samples[name].append(median_ms(fn, args.iters))
        ms = {n: med(samples[n]) for n in variants}
        kv_bytes = 2 * batch * cap * HKV * D * 2
        gbps = kv_bytes / (ms["kvcache"] * 1e-3) / 1e9
        if args.page_block_size:
            ref = flash_attn_with_kvcache(q, kc, vc)
            for page in args.page_block_size:
                if not torch.equal(variants[f"paged_p{page}"](), ref):
                    raise SystemExit(f"paged P={page} differs from the contiguous result at B={batch} L={cap}")
        shapes.append({
            "B": batch, "L": cap, "num_splits": split_count(batch, cap),
            "ms": {n: round(ms[n], 5) for n in variants},
            "round_spread": {n: round((max(samples[n]) - min(samples[n])) / ms[n], 4) for n in variants},
            "kvcache_over_baseline": round(ms["kvcache"] / ms["baseline"], 4),
            "kv_bytes": kv_bytes, "fits_last_level_cache": kv_bytes < LLC_BYTES,
            "kv_GBps": round(gbps, 1),
            "frac_of_copy_bandwidth": round(gbps / copy_gbps, 4) if copy_gbps else None,
        })
        if args.fp8:
            ref8 = variants["fp8"]()
            for page in args.page_block_size:
                if not torch.equal(variants[f"fp8_paged_p{page}"](), ref8):
                    raise SystemExit(f"fp8 paged P={page} differs from the contiguous fp8 result at B={batch} L={cap}")
            gbps8 = kv_bytes / 2 / (ms["fp8"] * 1e-3) / 1e9
            shapes[-1].update({
                "fp8_over_kvcache": round(ms["fp8"] / ms["kvcache"], 4), "fp8_kv_bytes": kv_bytes // 2,
                "fp8_fits_last_level_cache": kv_bytes // 2 < LLC_BYTES, "fp8_kv_GBps": round(gbps8, 1),
                "fp8_frac_of_copy_bandwidth": round(gbps8 / copy_gbps, 4) if copy_gbps else None,
            })
            if args.page_block_size:
                shapes[-1]["fp8_paged_over_kvcache"] = {str(p): round(ms[f"fp8_paged_p{p}"] / ms["kvcache"], 4)
                                                        for p in args.page_block_size}
        if args.page_block_size:
            shapes[-1]["paged_over_kvcache"] = {str(p): round(ms[f"paged_p{p}"] / ms["kvcache"], 4)
                                                for p in args.page_block_size}
        del q, kc, vc, variants
        if args.fp8:
            del k8, v8
        torch.cuda.empty_cache()
    result = {"bench": "decode", "device": torch.cuda.get_device_name(0), "dtype": "bf16", "Hq": HQ, "Hkv": HKV, "D": D,
              "Sq": 1, "rounds": args.rounds, "iters": args.iters, "copy_GBps": copy_gbps, "shapes": shapes}
    if args.fp8:
        result["fp8"] = {"cache_dtype": "float8_e4m3fn", "descales": "0.5 per (batch, kv head), device tensors"}
    if args.page_block_size:
        result["page_block_sizes"], result["page_order"] = args.page_block_size, args.page_order
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
