"""Kernel-level mixed serving steps over a paged KV cache (bf16, d = 128, page
16): flash_attn_varlen_with_kvcache on the packed rows against
flash_attn_chunk_with_kvcache on the same data padded to the longest piece.
Both run in one process, alternating.

  python benchmarks/kvcache_varlen_bench.py [--repeats 7] [--window-ms 5]

Steps: one 64-token prefill piece plus 7 decoding rows, and 8 decoding rows.
One JSON line per shape: per variant the median of --repeats timed windows
with the min..max spread, and the ratio of the medians (< 1: packed is
faster). Before timing, the results are compared on the real rows.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch  # noqa: E402

from kvcache_chunk_bench import _fill, _time_window  # noqa: E402

HEADS = [(32, 8), (32, 32)]
STEPS = {"mixed": [64] + [1] * 7, "decode": [1] * 8}
CONTEXTS = [1024, 8192]
PAGE = 16
D = 128


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--window-ms", type=float, default=5.0,
                   help="target length of one timed window")
    args = p.parse_args()

    from torchacc_amd.models.generation import PagedKVCache
    from torchacc_amd.ops import (flash_attn_chunk_with_kvcache,
                                  flash_attn_varlen_with_kvcache)
    from torchacc_amd.ops._backend import require_extension
    require_extension()
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)
    dt = torch.bfloat16

    for hq, hk in HEADS:
        for step, n in STEPS.items():
            for ctx in CONTEXTS:
                b, T, sq, w = len(n), sum(n), max(n), ctx // PAGE
                pool = PagedKVCache([(hk, D)], b, b * w, PAGE, w, dt, "cuda")
                perm = torch.randperm(b * w, generator=gen)
                pool.table.copy_(perm.view(b, w).to(torch.int32))
                pool.lens.fill_(ctx)
                k = torch.randn(b, ctx, hk, D, device="cuda", dtype=dt)
                _fill(pool, pool.table, 0, k, torch.randn_like(k))
                q = torch.randn(T, hq, D, device="cuda", dtype=dt)
                cu = torch.tensor([0] + torch.tensor(n).cumsum(0).tolist(),
                                  dtype=torch.int32, device="cuda")
                n_dev = torch.tensor(n, dtype=torch.int32, device="cuda")
                qpad = torch.zeros(b, sq, hq, D, device="cuda", dtype=dt)
                for i, ni in enumerate(n):
                    qpad[i, :ni] = q[int(cu[i]):int(cu[i]) + ni]

                def packed():
                    return flash_attn_varlen_with_kvcache(
                        q, pool.k[0], pool.v[0], pool.lens, cu,
                        block_table=pool.table)

                def padded():
                    return flash_attn_chunk_with_kvcache(
                        qpad, pool.k[0], pool.v[0], pool.lens,
                        q_seqlens=n_dev, block_table=pool.table)

                fns = {"packed": packed, "padded": padded}
                ref = torch.cat([padded()[i, :ni] for i, ni in enumerate(n)])
                diff = float((packed().float() - ref.float()).abs().max())
                assert diff < 2e-2, f"results differ by {diff}"
                iters = {}
                for name, fn in fns.items():   # warm, then size the window
                    for _ in range(3):
                        fn()
                    torch.cuda.synchronize()
                    us = _time_window(fn, 5)
                    iters[name] = max(5, int(args.window_ms * 1e3 / us))
                samples = {name: [] for name in fns}
                for _ in range(args.repeats):   # alternate the variants
                    for name, fn in fns.items():
                        samples[name].append(_time_window(fn, iters[name]))
                med = {m: statistics.median(s) for m, s in samples.items()}
                line = {"hq": hq, "hk": hk, "step": step, "rows": T,
                        "padded_rows": b * sq, "context": ctx, "page": PAGE,
                        "max_abs_diff": round(diff, 5)}
                for name in fns:
                    line[f"{name}_us"] = round(med[name], 2)
                    line[f"{name}_us_min_max"] = [
                        round(min(samples[name]), 2),
                        round(max(samples[name]), 2)]
                line["packed_over_padded"] = round(
                    med["packed"] / med["padded"], 3)
                print(json.dumps(line), flush=True)
                del pool, q, k, fns


if __name__ == "__main__":
    main()
