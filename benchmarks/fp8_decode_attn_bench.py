"""Kernel-level fp8 (e4m3fn) KV cache: flash_attn_with_kvcache on fp8 caches,
contiguous and paged at page size 16, against the bf16 op on the same
(dequantised) data, at the shapes of decode_attn_bench.py; and the quantising
cache write against the two index_copy_ calls it replaces. All variants run in
one process, alternating.

  python benchmarks/fp8_decode_attn_bench.py [--repeats 7] [--window-ms 5]

One JSON line per shape: per variant the median of --repeats timed windows
with the min..max spread, and fp8 / bf16 of the medians per layout (0.5 is
the byte ratio). Capacity = context + 128 rounded up to 256, as in
paged_decode_attn_bench.py, so every variant gets the same split count.
Before timing, paged is compared bitwise with contiguous in both dtypes and
fp8 is compared with bf16 (the bf16 caches hold the dequantised codes
exactly, so only the summation arithmetic differs). The last line times the
write op for one decode step of batch 8.
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
PAGE = 16
CAP_ROUND = 256
D = 128
FP8 = torch.float8_e4m3fn


def _time_window(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters      # us per call


def _paginate(t, perm):
    """Pool holding the pages of t [b, cap, hk, d] at the physical indices
    perm (moved as bytes: float8 has no index kernels)."""
    b, cap, hk, d = t.shape
    w = cap // PAGE
    raw = t.view(torch.uint8).view(b * w, PAGE, hk, -1)
    pool = torch.empty_like(raw)
    pool[perm] = raw
    return pool.view(t.dtype).view(b * w, PAGE, hk, d)


def _measure(fns, repeats, window_ms):
    iters = {}
    for name, fn in fns.items():        # warm, then size the window
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        us = _time_window(fn, 20)
        iters[name] = max(20, int(window_ms * 1e3 / us))
    samples = {name: [] for name in fns}
    for _ in range(repeats):            # alternate the variants
        for name, fn in fns.items():
            samples[name].append(_time_window(fn, iters[name]))
    return samples


def _report(line, samples):
    med = {n: statistics.median(s) for n, s in samples.items()}
    for name, s in samples.items():
        line[f"{name}_us"] = round(med[name], 2)
        line[f"{name}_us_min_max"] = [round(min(s), 2), round(max(s), 2)]
    return med


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--window-ms", type=float, default=5.0,
                   help="target length of one timed window")
    args = p.parse_args()

    from torchacc_amd.ops import flash_attn_with_kvcache, kv_cache_write_fp8
    from torchacc_amd.ops._backend import require_extension
    require_extension()
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)

    for hq, hk in HEADS:
        for b in BATCHES:
            for ctx in CONTEXTS:
                cap = -(-(ctx + 128) // CAP_ROUND) * CAP_ROUND
                q = torch.randn(b, 1, hq, D, device="cuda",
                                dtype=torch.bfloat16)
                # power-of-two scales: the bf16 caches hold exactly the
                # values the fp8 codes stand for
                ks = torch.full((hk,), 2.0 ** -6, device="cuda")
                vs = torch.full((hk,), 2.0 ** -5, device="cuda")
                k8 = (torch.randn(b, cap, hk, D, device="cuda") * 64) \
                    .clamp(-448, 448).to(FP8)
                v8 = (torch.randn(b, cap, hk, D, device="cuda") * 32) \
                    .clamp(-448, 448).to(FP8)
                k = (k8.float() * 2.0 ** -6).to(torch.bfloat16)
                v = (v8.float() * 2.0 ** -5).to(torch.bfloat16)
                lens = torch.full((b,), ctx, dtype=torch.int32,
                                  device="cuda")
                perm = torch.randperm(b * cap // PAGE, generator=gen).cuda()
                table = perm.view(b, cap // PAGE).to(torch.int32)
                kp, vp, kp8, vp8 = (_paginate(t, perm)
                                    for t in (k, v, k8, v8))
                sc = dict(k_scale=ks, v_scale=vs)
                fns = {
                    "bf16": lambda: flash_attn_with_kvcache(
                        q, k, v, cache_seqlens=lens),
                    "fp8": lambda: flash_attn_with_kvcache(
                        q, k8, v8, cache_seqlens=lens, **sc),
                    "bf16_page16": lambda: flash_attn_with_kvcache(
                        q, kp, vp, cache_seqlens=lens, block_table=table),
                    "fp8_page16": lambda: flash_attn_with_kvcache(
                        q, kp8, vp8, cache_seqlens=lens, block_table=table,
                        **sc),
                }
                want, want8 = fns["bf16"](), fns["fp8"]()
                assert torch.equal(fns["bf16_page16"](), want)
                assert torch.equal(fns["fp8_page16"](), want8)
                err = float((want8.float() - want.float()).abs().max())
                assert err <= 1.5e-2 * float(want.float().abs().max()), err
                samples = _measure(fns, args.repeats, args.window_ms)
                kv_bytes = 2 * b * ctx * hk * D * 2
                line = {"hq": hq, "hk": hk, "batch": b, "context": ctx,
                        "capacity": cap, "bf16_kv_bytes": kv_bytes}
                med = _report(line, samples)
                line["fp8_over_bf16"] = round(med["fp8"] / med["bf16"], 3)
                line["fp8_over_bf16_page16"] = round(
                    med["fp8_page16"] / med["bf16_page16"], 3)
                line["bf16_TBps"] = round(
                    kv_bytes / (med["bf16"] * 1e-6) / 1e12, 3)
                line["fp8_TBps"] = round(
                    kv_bytes / 2 / (med["fp8"] * 1e-6) / 1e12, 3)
                print(json.dumps(line), flush=True)
                del fns, k, v, k8, v8, kp, vp, kp8, vp8

    # the write of one decode step (batch 8, 8 kv heads) into a contiguous
    # cache: one quantising launch against two index_copy_ calls
    b, hk, cap = 8, 8, 2048
    k = torch.randn(b, 1, hk, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn_like(k)
    kc = torch.empty(b, cap, hk, D, device="cuda", dtype=torch.bfloat16)
    vc = torch.empty_like(kc)
    kc8 = torch.empty(b, cap, hk, D, device="cuda", dtype=FP8)
    vc8 = torch.empty_like(kc8)
    pos = torch.full((1,), 777, device="cuda")
    slots = torch.arange(b, device="cuda") * cap + pos
    ks = torch.full((hk,), 0.02, device="cuda")
    vs = torch.full((hk,), 0.01, device="cuda")

    def copy_bf16():
        kc.index_copy_(1, pos, k)
        vc.index_copy_(1, pos, v)

    fns = {"index_copy_x2_bf16": copy_bf16,
           "kv_cache_write_fp8": lambda: kv_cache_write_fp8(
               k, v, kc8, vc8, slots, ks, vs)}
    line = {"write_op": True, "batch": b, "hk": hk, "d": D}
    med = _report(line, _measure(fns, args.repeats, args.window_ms))
    line["write_over_index_copy"] = round(
        med["kv_cache_write_fp8"] / med["index_copy_x2_bf16"], 3)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
