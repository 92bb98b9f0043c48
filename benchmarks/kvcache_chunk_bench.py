"""Kernel-level chunk attention over a paged KV cache:
flash_attn_chunk_with_kvcache (block table, page 16, physical pages in a
random permutation) against the path it replaces for the same inputs,
``PagedKVCache.gather`` + ``flash_attn_xla`` on the gathered copy (with
``dequantize_kv_fp8`` in between for an fp8 cache). All variants run in one
process, alternating.

  python benchmarks/kvcache_chunk_bench.py [--repeats 7] [--window-ms 5]

One JSON line per shape: per variant the median of --repeats timed windows
with the min..max spread, and the ratio chunk / gather of the medians (< 1:
the new op is faster). Before timing, the two results are compared.
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
# (chunk, context): the context includes the chunk
SHAPES = [(512, 4096), (512, 16384), (8, 4096)]
PAGE = 16
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


def _fill(pool, table, layer, k, v):
    """Write k / v [b, ctx, hk, d] into the pages the table names."""
    b, ctx, hk, d = k.shape
    w = ctx // pool.page_size
    idx = table[:, :w].reshape(-1).long()
    for dst, src in ((pool.k[layer], k), (pool.v[layer], v)):
        src = src.reshape(b * w, pool.page_size, hk, d)
        if pool.fp8:
            dst.view(torch.uint8)[idx] = src.view(torch.uint8)
        else:
            dst[idx] = src


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--window-ms", type=float, default=5.0,
                   help="target length of one timed window")
    args = p.parse_args()

    from torchacc_amd.models.generation import PagedKVCache
    from torchacc_amd.ops import flash_attn_chunk_with_kvcache, flash_attn_xla
    from torchacc_amd.ops._backend import require_extension
    from torchacc_amd.ops.flash_attn import FP8_DTYPE, dequantize_kv_fp8
    require_extension()
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)
    dt = torch.bfloat16

    for hq, hk in HEADS:
        for b in BATCHES:
            for chunk, ctx in SHAPES:
                for fp8 in (False, True):
                    w = ctx // PAGE
                    pool = PagedKVCache([(hk, D)], b, b * w, PAGE, w, dt,
                                        "cuda",
                                        kv_dtype="fp8" if fp8 else None)
                    perm = torch.randperm(b * w, generator=gen)
                    pool.table.copy_(perm.view(b, w).to(torch.int32))
                    pool.lens.fill_(ctx)
                    q = torch.randn(b, chunk, hq, D, device="cuda", dtype=dt)
                    k = torch.randn(b, ctx, hk, D, device="cuda", dtype=dt)
                    v = torch.randn_like(k)
                    scales = {}
                    if fp8:
                        ks = k.float().abs().amax(dim=(0, 1, 3)) / 448.0
                        vs = v.float().abs().amax(dim=(0, 1, 3)) / 448.0
                        pool.k_scale[0].copy_(ks)
                        pool.v_scale[0].copy_(vs)
                        k = (k.float() / ks.view(1, 1, -1, 1)).to(FP8_DTYPE)
                        v = (v.float() / vs.view(1, 1, -1, 1)).to(FP8_DTYPE)
                        scales = {"k_scale": pool.k_scale[0],
                                  "v_scale": pool.v_scale[0]}
                    _fill(pool, pool.table, 0, k, v)

                    def new():
                        return flash_attn_chunk_with_kvcache(
                            q, pool.k[0], pool.v[0], pool.lens,
                            block_table=pool.table, **scales)

                    def old():
                        kc, vc = pool.gather(0, ctx)
                        if fp8:
                            kc = dequantize_kv_fp8(kc, pool.k_scale[0], dt)
                            vc = dequantize_kv_fp8(vc, pool.v_scale[0], dt)
                        return flash_attn_xla(q, kc, vc, causal=True)

                    fns = {"chunk": new, "gather": old}
                    diff = float((new().float() - old().float()).abs().max())
                    assert diff < 5e-2, f"results differ by {diff}"
                    iters = {}
                    for name, fn in fns.items():  # warm, then size the window
                        for _ in range(3):
                            fn()
                        torch.cuda.synchronize()
                        us = _time_window(fn, 5)
                        iters[name] = max(5, int(args.window_ms * 1e3 / us))
                    samples = {name: [] for name in fns}
                    for _ in range(args.repeats):   # alternate the variants
                        for name, fn in fns.items():
                            samples[name].append(
                                _time_window(fn, iters[name]))
                    med = {n: statistics.median(s)
                           for n, s in samples.items()}
                    line = {"hq": hq, "hk": hk, "batch": b, "chunk": chunk,
                            "context": ctx, "kv": "fp8" if fp8 else "bf16",
                            "page": PAGE, "max_abs_diff": round(diff, 5)}
                    for name in fns:
                        line[f"{name}_us"] = round(med[name], 2)
                        line[f"{name}_us_min_max"] = [
                            round(min(samples[name]), 2),
                            round(max(samples[name]), 2)]
                    line["chunk_over_gather"] = round(
                        med["chunk"] / med["gather"], 3)
                    print(json.dumps(line), flush=True)
                    del pool, q, k, v, fns


if __name__ == "__main__":
    main()
