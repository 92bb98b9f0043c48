"""rope_kv_cache_write against the composition it replaces, on a page-16
pool (physical pages in a random permutation), both in one process,
alternating. Timing procedure of kvcache_chunk_split_bench.py.

  python benchmarks/rope_kv_write_bench.py [--repeats 7] [--window-ms 5]

The composition is apply_rotary_pos_emb (two launches) followed by two
index_copy_ calls (16-bit pool) or kv_cache_write_fp8 (fp8 pool): what one
layer of a paged decode or prefill step runs today. Both variants get the
same q / k / v, table rows and slots; before timing, q_rot and both whole
pools are compared bitwise.

One JSON line per shape: per variant the median of --repeats timed windows
with the min..max spread, in microseconds per call (host launch cost
included: at s = 1 both variants are launch-bound).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch  # noqa: E402

HEADS = [(32, 32), (32, 8)]      # Llama-2-7B, Llama-3-8B
SHAPES = [(1, 1), (8, 1), (1, 512)]     # (batch, new tokens per sequence)
CONTEXT = 1024                   # tokens already in the cache
PAGE = 16
D = 128
P = 4096


def _time_window(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters      # us per call


def _bits(t):
    return t.view(torch.uint8 if t.element_size() == 1 else torch.int16)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--window-ms", type=float, default=5.0,
                   help="target length of one timed window")
    args = p.parse_args()

    from torchacc_amd.models.generation import PagedKVCache
    from torchacc_amd.ops import (apply_rotary_pos_emb, kv_cache_write_fp8,
                                  rope_kv_cache_write)
    from torchacc_amd.ops._backend import require_extension
    from torchacc_amd.ops.rope import build_rope_cache
    require_extension()
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)
    dt = torch.bfloat16
    cos, sin = build_rope_cache(P, D, device="cuda")

    for hq, hk in HEADS:
        for b, s in SHAPES:
            for fp8 in (False, True):
                w = (CONTEXT + s + PAGE - 1) // PAGE
                pools = [PagedKVCache([(hk, D)], b, b * w, PAGE, w, dt,
                                      "cuda", kv_dtype="fp8" if fp8 else None)
                         for _ in range(2)]
                perm = torch.randperm(b * w, generator=gen)
                for pool in pools:
                    pool.table.copy_(perm.view(b, w).to(torch.int32))
                    _bits(pool.k[0]).zero_()
                    _bits(pool.v[0]).zero_()
                fused_pool, comp_pool = pools
                q = torch.randn(b, s, hq, D, device="cuda", dtype=dt)
                k = torch.randn(b, s, hk, D, device="cuda", dtype=dt)
                v = torch.randn_like(k)
                if fp8:
                    for pool in pools:
                        pool.k_scale[0].fill_(6.0 / 448.0)
                        pool.v_scale[0].fill_(6.0 / 448.0)
                positions = torch.arange(CONTEXT, CONTEXT + s,
                                         device="cuda").expand(b, s)
                slots = comp_pool.slot_indices(positions)
                flat_pos = positions.reshape(-1).contiguous()
                cos_s = cos[CONTEXT:CONTEXT + s]
                sin_s = sin[CONTEXT:CONTEXT + s]

                def fused():
                    sc = ((fused_pool.k_scale[0], fused_pool.v_scale[0])
                          if fp8 else ())
                    return rope_kv_cache_write(
                        q, k, v, cos, sin, flat_pos, fused_pool.k[0],
                        fused_pool.v[0], slots, *sc)

                def composition():
                    qr, kr = apply_rotary_pos_emb(q, k, cos_s, sin_s)
                    if fp8:
                        kv_cache_write_fp8(kr, v, comp_pool.k[0],
                                           comp_pool.v[0], slots,
                                           comp_pool.k_scale[0],
                                           comp_pool.v_scale[0])
                        return qr
                    for dst, new in ((comp_pool.k[0], kr),
                                     (comp_pool.v[0], v)):
                        dst.view(-1, hk, D).index_copy_(
                            0, slots, new.reshape(-1, hk, D))
                    return qr

                fns = {"fused": fused, "composition": composition}
                assert torch.equal(_bits(fused()), _bits(composition()))
                for a, c in ((fused_pool.k[0], comp_pool.k[0]),
                             (fused_pool.v[0], comp_pool.v[0])):
                    assert torch.equal(_bits(a), _bits(c))
                    assert int(_bits(a).ne(0).sum()) > 0
                iters = {}
                for name, fn in fns.items():    # warm, size the window
                    for _ in range(3):
                        fn()
                    torch.cuda.synchronize()
                    us = _time_window(fn, 5)
                    iters[name] = max(5, int(args.window_ms * 1e3 / us))
                samples = {name: [] for name in fns}
                for _ in range(args.repeats):   # alternate
                    for name, fn in fns.items():
                        samples[name].append(_time_window(fn, iters[name]))
                line = {"hq": hq, "hk": hk, "batch": b, "new_tokens": s,
                        "kv": "fp8" if fp8 else "bf16", "page": PAGE}
                for name in fns:
                    line[f"{name}_us"] = round(
                        statistics.median(samples[name]), 2)
                    line[f"{name}_us_min_max"] = [
                        round(min(samples[name]), 2),
                        round(max(samples[name]), 2)]
                print(json.dumps(line), flush=True)
                del pools, fused_pool, comp_pool, q, k, v, fns


if __name__ == "__main__":
    main()
