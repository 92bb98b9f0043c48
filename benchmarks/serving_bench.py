"""Continuous batching against one request at a time.

16 requests with prompt lengths spread over 16..1024 and 64 new tokens each
(greedy) run through ``ContinuousBatcher(max_batch=8)`` and, one after the
other, through ``generate(page_size=16)`` on the same model: Llama-2-7B
shapes, random weights, bf16, pages of 16 tokens.

  python benchmarks/serving_bench.py [--layers 32] [--repeats 3]

Both variants are warmed with a short request first and then alternate
--repeats times in one process; wall-clock time between device
synchronisations, prefill included. One JSON line: generated tokens/s of both
(median, with min..max), and how many of the generated tokens agree (random
weights give near-ties, so bf16 paths that round differently may part ways;
the number is reported, not asserted).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch  # noqa: E402

REQUESTS = 16
NEW = 64
PAGE = 16
MAX_BATCH = 8


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--layers", type=int, default=32)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--prefill-chunk", type=int, default=64)
    args = p.parse_args()

    from torchacc_amd.models import (ContinuousBatcher, LlamaForCausalLM,
                                     llama_2_7b)
    from torchacc_amd.ops._backend import require_extension
    require_extension()
    torch.manual_seed(0)
    cfg = llama_2_7b()
    cfg.num_hidden_layers = args.layers
    with torch.device("cuda"):
        model = LlamaForCausalLM(cfg).to(torch.bfloat16).eval()
    gen = torch.Generator().manual_seed(0)
    lens = [int(x) for x in torch.linspace(16, 1024, REQUESTS).round()]
    order = torch.randperm(REQUESTS, generator=gen).tolist()
    prompts = [torch.randint(0, cfg.vocab_size, (lens[i],), generator=gen)
               for i in order]
    max_len = max(lens) + NEW
    pages = sum((n + NEW + PAGE - 1) // PAGE for n in lens)

    def engine(reqs):
        eng = ContinuousBatcher(model, MAX_BATCH, pages, PAGE, max_len,
                                prefill_chunk=args.prefill_chunk)
        rids = [eng.add(r, NEW) for r in reqs]
        outs = eng.run()
        return [outs[r] for r in rids]

    def one_by_one(reqs):
        return [model.generate(r[None].cuda(), max_new_tokens=NEW,
                               page_size=PAGE)[0].cpu() for r in reqs]

    fns = {"engine": engine, "generate": one_by_one}
    for fn in fns.values():
        fn(prompts[:1])
    torch.cuda.synchronize()
    samples = {name: [] for name in fns}
    outs = {}
    for _ in range(args.repeats):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[name] = fn(prompts)
            torch.cuda.synchronize()
            samples[name].append(REQUESTS * NEW
                                 / (time.perf_counter() - t0))
    agree = sum(int((a[-NEW:] == b[-NEW:]).sum())
                for a, b in zip(outs["engine"], outs["generate"]))
    line = {"model": "llama-2-7b", "layers": args.layers, "requests": REQUESTS,
            "prompt_lens": "16..1024", "new_tokens": NEW, "page": PAGE,
            "max_batch": MAX_BATCH, "prefill_chunk": args.prefill_chunk,
            "tokens_agree": f"{agree}/{REQUESTS * NEW}"}
    for name in fns:
        line[f"{name}_tok_s"] = round(statistics.median(samples[name]), 1)
        line[f"{name}_tok_s_min_max"] = [round(min(samples[name]), 1),
                                         round(max(samples[name]), 1)]
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
