"""Kernel-level paged decode attention: flash_attn_with_kvcache with a block
table (page sizes 16 / 64 / 256, physical pages in a random permutation)
against the contiguous op on the same data, at the shapes of
decode_attn_bench.py. All run in one process, alternating.

  python benchmarks/paged_decode_attn_bench.py [--repeats 7] [--window-ms 5]

One JSON line per shape: per variant the median of --repeats timed windows
with the min..max spread, the paged/contiguous ratio of the medians, and
whether the paged median lies inside the contiguous min..max spread. Before
timing, every paged result is compared bitwise with the contiguous one.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch  # noqa: E402

HEADS = [(32, 32), (32, 8)]      # Llama-2-7B, Llama-3-8B
BATCHES = [1, 8]
CONTEXTS = [128, 2048, 16384]
PAGE_SIZES = [16, 64, 256]
D = 128


def _time_window(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters      # us per call


def _paginate(k, v, ps, gen):
    """Pools holding the pages of k / v [b, cap, hk, d] at permuted physical
    indices, and the table that names them."""
    b, cap, hk, d = k.shape
    w = cap // ps
    perm = torch.randperm(b * w, generator=gen).to(k.device)
    kp = torch.empty(b * w, ps, hk, d, dtype=k.dtype, device=k.device)
    vp = torch.empty_like(kp)
    kp[perm] = k.reshape(b * w, ps, hk, d)
    vp[perm] = v.reshape(b * w, ps, hk, d)
    return kp, vp, perm.view(b, w).to(torch.int32)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--window-ms", type=float, default=5.0,
                   help="target length of one timed window")
    args = p.parse_args()

    from torchacc_amd.ops import flash_attn_with_kvcache
    from torchacc_amd.ops._backend import require_extension
    require_extension()
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)

    for hq, hk in HEADS:
        for b in BATCHES:
            for ctx in CONTEXTS:
                # capacity as in decode_attn_bench.py, rounded up to the
                # largest page so that all layouts share one capacity (the
                # host's split choice depends on it)
                cap = -(-(ctx + 128) // max(PAGE_SIZES)) * max(PAGE_SIZES)
                q = torch.randn(b, 1, hq, D, device="cuda",
                                dtype=torch.bfloat16)
                k = torch.randn(b, cap, hk, D, device="cuda",
                                dtype=torch.bfloat16)
                v = torch.randn_like(k)
                lens = torch.full((b,), ctx, dtype=torch.int32,
                                  device="cuda")

                def contiguous():
                    return flash_attn_with_kvcache(q, k, v,
                                                   cache_seqlens=lens)

                def paged(kp, vp, table):
                    return lambda: flash_attn_with_kvcache(
                        q, kp, vp, cache_seqlens=lens, block_table=table)

                fns = {"contiguous": contiguous}
                for ps in PAGE_SIZES:
                    fns[f"page{ps}"] = paged(*_paginate(k, v, ps, gen))
                want = contiguous()
                for name, fn in fns.items():
                    assert torch.equal(fn(), want), f"{name} differs"
                iters = {}
                for name, fn in fns.items():    # warm, then size the window
                    for _ in range(5):
                        fn()
                    torch.cuda.synchronize()
                    us = _time_window(fn, 20)
                    iters[name] = max(20, int(args.window_ms * 1e3 / us))
                samples = {name: [] for name in fns}
                for _ in range(args.repeats):   # alternate the variants
                    for name, fn in fns.items():
                        samples[name].append(_time_window(fn, iters[name]))
                med = {n: statistics.median(s) for n, s in samples.items()}
                lo, hi = min(samples["contiguous"]), max(samples["contiguous"])
                kv_bytes = 2 * b * ctx * hk * D * 2
                line = {"hq": hq, "hk": hk, "batch": b, "context": ctx,
                        "capacity": cap, "kv_bytes": kv_bytes}
                for name in fns:
                    line[f"{name}_us"] = round(med[name], 2)
                    line[f"{name}_us_min_max"] = [
                        round(min(samples[name]), 2),
                        round(max(samples[name]), 2)]
                for ps in PAGE_SIZES:
                    name = f"page{ps}"
                    line[f"{name}_ratio"] = round(
                        med[name] / med["contiguous"], 3)
                    line[f"{name}_in_contiguous_spread"] = bool(
                        lo <= med[name] <= hi)
                line["contiguous_TBps"] = round(
                    kv_bytes / (med["contiguous"] * 1e-6) / 1e12, 3)
                print(json.dumps(line), flush=True)
                del fns, k, v


if __name__ == "__main__":
    main()
