"""GraphDecoder steady-state ms/token with the split-KV decode attention
against the same step with the full-tile kernel (``FlashAttnFunc`` with
``k_lens`` over the whole cache, the decode step before the decode kernel
existed). One process, one model, batch 1: a GraphDecoder is captured with
each attention call, and the two are timed alternately.

  python benchmarks/decode_graph_ab.py --model llama-2-7b --prompt 2048

ms/token is (time of --new tokens - time of 2 tokens) / (--new - 2), so the
eager prefill that every ``decode`` call starts with is excluded. Prints one
JSON line: median of --repeats with min and max for both.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="llama-2-7b",
                   choices=["llama-2-7b", "llama-3-8b"])
    p.add_argument("--prompt", type=int, default=128)
    p.add_argument("--new", type=int, default=128)
    p.add_argument("--warmup", type=int, default=8)
    p.add_argument("--repeats", type=int, default=5)
    args = p.parse_args()

    from torchacc_amd.models import (LlamaForCausalLM, generation,
                                     llama_2_7b, llama_3_8b)
    from torchacc_amd.ops.flash_attn import FlashAttnFunc

    new_attn = generation.flash_attn_with_kvcache

    def full_tile_attn(q, k, v, cache_seqlens=None, softmax_scale=None,
                       window_size=(-1, -1)):
        o, _ = FlashAttnFunc.apply(q, k, v, 0.0, softmax_scale, True,
                                   window_size, None, False, None,
                                   cache_seqlens)
        return o

    max_len = args.prompt + args.new + args.warmup + 2
    cfg = {"llama-2-7b": llama_2_7b, "llama-3-8b": llama_3_8b}[args.model](
        max_position_embeddings=max(4096, max_len + 2))
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = LlamaForCausalLM(cfg).to(torch.bfloat16).eval()
    ids = torch.randint(0, cfg.vocab_size, (1, args.prompt), device="cuda")

    decs = {}
    try:
        for name, fn in (("split_kv", new_attn),
                         ("full_tile", full_tile_attn)):
            generation.flash_attn_with_kvcache = fn
            dec = generation.GraphDecoder(model, 1, max_len)
            dec.decode(ids, args.warmup)    # warm and capture with `fn`
            torch.cuda.synchronize()
            decs[name] = dec
    finally:
        generation.flash_attn_with_kvcache = new_attn

    def run(dec, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.decode(ids, n)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    ms = {name: [] for name in decs}
    for _ in range(args.repeats):
        for name, dec in decs.items():
            short, long_ = run(dec, 2), run(dec, args.new)
            ms[name].append((long_ - short) / (args.new - 2) * 1e3)
    out = {"model": args.model, "batch": 1, "prompt": args.prompt,
           "new": args.new}
    for name, vals in ms.items():
        out[name + "_ms_per_token"] = round(statistics.median(vals), 4)
        out[name + "_min_max"] = [round(min(vals), 4), round(max(vals), 4)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
