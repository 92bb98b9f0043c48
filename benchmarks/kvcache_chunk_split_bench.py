"""Split-KV in flash_attn_chunk_with_kvcache over a paged KV cache (block
table, page 16, physical pages in a random permutation): the unsplit kernel
(``num_splits=1``), the automatic choice (``num_splits=0``; the count it picks
is printed) and forced counts, all in one process, alternating. Timing
procedure of kvcache_chunk_bench.py.

  python benchmarks/kvcache_chunk_split_bench.py [--repeats 7] [--window-ms 5]
      [--splits 2,4,8,16]

By default the forced counts are the two around the automatic choice (half and
double; 2 and 4 where it is 1). ``--splits`` times the given counts instead,
which is how MQ_MIN_KEYS_PER_SPLIT / MQ_MAX_SPLITS were tuned. For chunk = 1
the decode op (flash_attn_with_kvcache, its own automatic split) runs on the
same cache as one more variant.

One JSON line per shape: per variant the median of --repeats timed windows
with the min..max spread, in microseconds per call. Before timing, every
variant is compared with the unsplit result.
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
CHUNKS = [1, 8, 64, 512]
CONTEXTS = [4096, 16384]         # the context includes the chunk
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


def _around(auto, limit):
    """Two forced counts around the automatic one."""
    if auto == 1:
        return [2, 4]
    lo = auto // 2
    return sorted({lo if lo >= 2 else min(4 * auto, limit),
                   min(2 * auto, limit)} - {auto})


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--window-ms", type=float, default=5.0,
                   help="target length of one timed window")
    p.add_argument("--splits", type=str, default=None,
                   help="comma-separated forced counts to time instead of "
                        "the two around the automatic choice")
    args = p.parse_args()

    from torchacc_amd.models.generation import PagedKVCache
    from torchacc_amd.ops import (flash_attn_chunk_with_kvcache,
                                  flash_attn_with_kvcache)
    from torchacc_amd.ops._backend import require_extension
    from torchacc_amd.ops.flash_attn import FP8_DTYPE
    ext = require_extension()
    _, _, limit = ext.fa_kvcache_mq_split_constants()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)
    dt = torch.bfloat16

    for hq, hk in HEADS:
        for b in BATCHES:
            for chunk in CHUNKS:
                for ctx in CONTEXTS:
                    for fp8 in (False, True):
                        w = ctx // PAGE
                        pool = PagedKVCache([(hk, D)], b, b * w, PAGE, w, dt,
                                            "cuda",
                                            kv_dtype="fp8" if fp8 else None)
                        perm = torch.randperm(b * w, generator=gen)
                        pool.table.copy_(perm.view(b, w).to(torch.int32))
                        pool.lens.fill_(ctx)
                        q = torch.randn(b, chunk, hq, D, device="cuda",
                                        dtype=dt)
                        k = torch.randn(b, ctx, hk, D, device="cuda",
                                        dtype=dt)
                        v = torch.randn_like(k)
                        scales = {}
                        if fp8:
                            ks = k.float().abs().amax(dim=(0, 1, 3)) / 448.0
                            vs = v.float().abs().amax(dim=(0, 1, 3)) / 448.0
                            pool.k_scale[0].copy_(ks)
                            pool.v_scale[0].copy_(vs)
                            k = (k.float() / ks.view(1, 1, -1, 1)).to(
                                FP8_DTYPE)
                            v = (v.float() / vs.view(1, 1, -1, 1)).to(
                                FP8_DTYPE)
                            scales = {"k_scale": pool.k_scale[0],
                                      "v_scale": pool.v_scale[0]}
                        _fill(pool, pool.table, 0, k, v)
                        del k, v

                        def chunk_op(ns):
                            return lambda: flash_attn_chunk_with_kvcache(
                                q, pool.k[0], pool.v[0], pool.lens,
                                block_table=pool.table, num_splits=ns,
                                **scales)

                        auto = ext.fa_kvcache_mq_num_splits(
                            b, hk, chunk * (hq // hk), ctx, cus)
                        forced = ([int(s) for s in args.splits.split(",")]
                                  if args.splits else _around(auto, limit))
                        fns = {"splits_1": chunk_op(1), "auto": chunk_op(0)}
                        for ns in forced:
                            fns[f"splits_{ns}"] = chunk_op(ns)
                        if chunk == 1:
                            fns["decode"] = lambda: flash_attn_with_kvcache(
                                q, pool.k[0], pool.v[0],
                                cache_seqlens=pool.lens,
                                block_table=pool.table, **scales)
                        want = fns["splits_1"]().float()
                        diff = max(float((fn().float() - want).abs().max())
                                   for fn in fns.values())
                        assert diff < 5e-2, f"results differ by {diff}"
                        iters = {}
                        for name, fn in fns.items():  # warm, size the window
                            for _ in range(3):
                                fn()
                            torch.cuda.synchronize()
                            us = _time_window(fn, 5)
                            iters[name] = max(
                                5, int(args.window_ms * 1e3 / us))
                        samples = {name: [] for name in fns}
                        for _ in range(args.repeats):   # alternate
                            for name, fn in fns.items():
                                samples[name].append(
                                    _time_window(fn, iters[name]))
                        line = {"hq": hq, "hk": hk, "batch": b,
                                "chunk": chunk, "context": ctx,
                                "kv": "fp8" if fp8 else "bf16", "page": PAGE,
                                "auto_num_splits": auto,
                                "max_abs_diff": round(diff, 5)}
                        for name in fns:
                            line[f"{name}_us"] = round(
                                statistics.median(samples[name]), 2)
                            line[f"{name}_us_min_max"] = [
                                round(min(samples[name]), 2),
                                round(max(samples[name]), 2)]
                        print(json.dumps(line), flush=True)
                        del pool, q, fns


if __name__ == "__main__":
    main()
