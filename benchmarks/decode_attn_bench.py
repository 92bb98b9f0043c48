"""Kernel-level decode attention: flash_attn_with_kvcache (split-KV kernel,
csrc/flash_attn_decode.hip) against the full-tile prefill kernel run at
sq = 1 over the contiguous cache with k_lens, which is what GraphDecoder did
before the decode kernel existed. Both run in one process, alternating.

  python benchmarks/decode_attn_bench.py [--repeats 7] [--window-ms 5]

One JSON line per shape: both times (median of --repeats timed windows, with
the min..max spread), the KV bytes the algorithm must read, and the new
kernel's bytes/s as a share of the HBM peak.
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X HBM3E spec peak

HEADS = [(32, 32), (32, 8)]      # Llama-2-7B, Llama-3-8B
BATCHES = [1, 8]
CONTEXTS = [128, 2048, 16384]
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--window-ms", type=float, default=5.0,
                   help="target length of one timed window")
    args = p.parse_args()

    from torchacc_amd.ops import flash_attn_with_kvcache
    from torchacc_amd.ops._backend import require_extension
    ext = require_extension()
    scale = 1.0 / math.sqrt(D)
    empty = torch.empty(0)
    torch.manual_seed(0)

    for hq, hk in HEADS:
        for b in BATCHES:
            for ctx in CONTEXTS:
                cap = ctx + 128
                q = torch.randn(b, 1, hq, D, device="cuda",
                                dtype=torch.bfloat16)
                k = torch.randn(b, cap, hk, D, device="cuda",
                                dtype=torch.bfloat16)
                v = torch.randn_like(k)
                lens = torch.full((b,), ctx, dtype=torch.int32,
                                  device="cuda")

                def new():
                    return flash_attn_with_kvcache(q, k, v,
                                                   cache_seqlens=lens)

                def old():
                    return ext.fa_forward(q, k, v, scale, True, -1, -1,
                                          empty, lens, empty, 0.0, 0)[0]

                fns = {"new": new, "old": old}
                iters = {}
                for name, fn in fns.items():    # warm, then size the window
                    for _ in range(5):
                        fn()
                    torch.cuda.synchronize()
                    us = _time_window(fn, 20)
                    iters[name] = max(20, int(args.window_ms * 1e3 / us))
                samples = {"new": [], "old": []}
                for _ in range(args.repeats):   # alternate the two
                    for name, fn in fns.items():
                        samples[name].append(_time_window(fn, iters[name]))
                kv_bytes = 2 * b * ctx * hk * D * 2
                med = {n: statistics.median(s) for n, s in samples.items()}
                bps = kv_bytes / (med["new"] * 1e-6)
                print(json.dumps({
                    "hq": hq, "hk": hk, "batch": b, "context": ctx,
                    "capacity": cap,
                    "new_us": round(med["new"], 2),
                    "new_us_min_max": [round(min(samples["new"]), 2),
                                       round(max(samples["new"]), 2)],
                    "old_us": round(med["old"], 2),
                    "old_us_min_max": [round(min(samples["old"]), 2),
                                       round(max(samples["old"]), 2)],
                    "speedup": round(med["old"] / med["new"], 2),
                    "kv_bytes": kv_bytes,
                    "new_TBps": round(bps / 1e12, 3),
                    "hbm_peak_share": round(bps / HBM_PEAK, 3),
                }), flush=True)


if __name__ == "__main__":
    main()
