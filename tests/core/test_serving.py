"""ContinuousBatcher on the GPU (bf16, 16-bit and fp8 pages) against the
plain forward without a cache.

Reference: ``model(full_ids)`` on each request's final sequence; the logits
of interest are those at the positions that produced the generated tokens.
Bound: the error of the path that existed before the engine,
``generate(page_size=16, prefill_chunk=32)`` (fp8 likewise), driven through
``_forward_step`` on the same sequences, against the same reference; the
engine may be off by at most twice that plus 1e-3 (it takes the chunk op for
the first piece of a prompt where that path takes the full-tile kernel: a
different, equally rounded path). Measured figures:
profiles/r12_ragged_serving.md."""
import pytest
import torch

from torchacc_amd.models import (ContinuousBatcher, LlamaConfig,
                                 LlamaForCausalLM)
from torchacc_amd.models import generation

pytestmark = pytest.mark.gpu

PROMPT_LENS = (5, 60, 33, 17)
NEW = 12
MAX_BATCH, NUM_PAGES, PAGE, MAX_LEN, CHUNK = 3, 10, 16, 80, 32
# model seed and one prompt seed per request (see _setup)
MODEL_SEED = 0
PROMPT_SEEDS = (22983, 2312, 261, 658)


def _setup():
    """The 2-layer Llama of test_generation_end_to_end, initialised on the
    host (so the weights do not depend on the device's generator) and the
    four prompts. The prompt seeds were chosen by looking at the reference
    alone (its fp32 evaluation on the host, greedy continuation by
    ``generate``): per request the first seed, counting from 0, whose 12
    generated positions all have a top-1 - top-2 reference logit gap above
    0.5. Twice the fp8 bound is 0.35 to 0.42 (it moves with the prompts) and
    twice the 16-bit bound about 0.10, so the condition on exempt positions
    can hold for both."""
    torch.manual_seed(MODEL_SEED)
    cfg = LlamaConfig(vocab_size=1024, hidden_size=1024,
                      intermediate_size=2048, num_hidden_layers=2,
                      num_attention_heads=8, num_key_value_heads=2,
                      max_position_embeddings=256)
    model = LlamaForCausalLM(cfg).cuda().to(torch.bfloat16).eval()
    prompts = [torch.randint(0, 1024, (n,),
                             generator=torch.Generator().manual_seed(s))
               for n, s in zip(PROMPT_LENS, PROMPT_SEEDS)]
    return model, prompts


def _calibrated_scales(model, prompt):
    """kv_scales as generate calibrates them from one prompt."""
    pool = generation.PagedKVCache.for_model(model, 1, 8, PAGE, MAX_LEN,
                                             kv_dtype="fp8")
    model.generate(prompt[None].cuda(), max_new_tokens=1, kv_pool=pool)
    return [(k.clone(), v.clone())
            for k, v in zip(pool.k_scale, pool.v_scale)]


def _run_engine(model, prompts, **kw):
    """-> ({rid: tokens}, {rid: fp32 logits [NEW, vocab]}, engine)."""
    eng = ContinuousBatcher(model, MAX_BATCH, NUM_PAGES, PAGE, MAX_LEN,
                            prefill_chunk=CHUNK, **kw)
    rids = [eng.add(p, NEW) for p in prompts]
    rows = {rid: [] for rid in rids}
    toks = {rid: [] for rid in rids}
    while not eng.idle():
        events, logits = eng.step(return_logits=True)
        assert logits.dtype == torch.float32
        assert logits.shape == (len(events), 1024)
        for (rid, t, _), row in zip(events, logits):
            rows[rid].append(row)
            toks[rid].append(t)
    outs = eng.run()
    for rid, p in zip(rids, prompts):
        assert outs[rid].tolist() == p.tolist() + toks[rid]
    return outs, {rid: torch.stack(r) for rid, r in rows.items()}, eng


@torch.no_grad()
def _reference_logits(model, full, n_prompt):
    """Plain forward: logits at the positions that produced each new token."""
    return model(full[None].cuda())[0, n_prompt - 1:-1].float()


@torch.no_grad()
def _parent_logits(model, full, n_prompt, kv_scales=None):
    """The pre-engine path on the same sequence: paged cache, prompt in
    pieces of CHUNK, then one token per step, through _forward_step."""
    fp8 = kv_scales is not None
    pool = generation.PagedKVCache.for_model(
        model, 1, 8, PAGE, MAX_LEN, kv_dtype="fp8" if fp8 else None)
    if fp8:
        generation._configure_scales(pool, kv_scales, 2.0)
    ids = full[None].cuda()
    out = []
    for pos in range(0, n_prompt, CHUNK):
        logits = generation._step(model, ids[:, pos:min(pos + CHUNK,
                                                        n_prompt)],
                                  pool, pos)
    out.append(logits[0].float())
    for pos in range(n_prompt, len(full) - 1):
        out.append(generation._step(model, ids[:, pos:pos + 1], pool,
                                    pos)[0].float())
    pool.free(0)
    return torch.stack(out)


@pytest.fixture(scope="module", params=["kv16", "kvfp8"])
def run(request):
    """One engine run (and a repeat), the reference and the pre-engine path,
    computed once per cache dtype and shared by the tests below."""
    kv = request.param
    model, prompts = _setup()
    kw = {}
    if kv == "kvfp8":
        kw = {"kv_dtype": "fp8",
              "kv_scales": _calibrated_scales(model, prompts[1])}
    outs, logits, eng = _run_engine(model, prompts, **kw)
    outs2, _, eng2 = _run_engine(model, prompts, **kw)
    parent_err = engine_err = 0.0
    per_request = []
    for rid, p in enumerate(prompts):
        full = outs[rid]
        ref = _reference_logits(model, full, len(p))
        par = _parent_logits(model, full, len(p), kw.get("kv_scales"))
        assert ref.shape == par.shape == logits[rid].shape == (NEW, 1024)
        parent_err = max(parent_err, float((par - ref).abs().max()))
        engine_err = max(engine_err,
                         float((logits[rid].cuda() - ref).abs().max()))
        per_request.append((full[len(p):].cuda(), ref))
    bound = 2.0 * parent_err + 1e-3
    print(f"\n{kv}: parent max |dlogit| {parent_err:.5f}  bound {bound:.5f}  "
          f"engine max |dlogit| {engine_err:.5f}")
    return {"kv": kv, "outs": outs, "outs2": outs2, "engines": (eng, eng2),
            "bound": bound, "engine_err": engine_err,
            "per_request": per_request}


def test_logits_within_bound(run):
    """Measured (max |dlogit|): 16-bit pages, pre-engine path 0.0234, bound
    0.0479, engine 0.0176; fp8 pages, pre-engine path 0.0859, bound 0.1729,
    engine 0.1211."""
    assert run["engine_err"] <= run["bound"], (run["engine_err"],
                                               run["bound"])


def test_tokens_match_reference(run):
    """Tokens equal the reference argmax wherever its top-1 - top-2 gap
    exceeds twice the bound, and at most 10 % of the positions may be exempt
    on that ground.

    Measured: no position is exempt (0 of 48) and all 48 tokens are the
    reference argmax, with 16-bit and with fp8 pages: twice the bound is
    0.096 and 0.346, and the prompts were chosen for reference gaps above
    0.5 (see _setup). With prompts drawn without that choice (seeds 0..3)
    22 of 48 (16-bit) and 46 of 48 (fp8) reference gaps lie within twice the
    bound: the fp8 error of the existing path, about 0.1, is of the order of
    this model's typical logit gaps."""
    exempt = wrong = 0
    for got, ref in run["per_request"]:
        top = ref.topk(2, dim=-1)
        clear = (top.values[:, 0] - top.values[:, 1]) > 2.0 * run["bound"]
        exempt += int((~clear).sum())
        wrong += int((got[clear] != top.indices[clear, 0]).sum())
    total = NEW * len(PROMPT_LENS)
    print(f"\n{run['kv']}: {exempt} of {total} positions within 2 x bound of "
          f"a tie, {wrong} clear positions differ")
    assert wrong == 0
    assert exempt <= total // 10, (exempt, total)


def test_deterministic(run):
    for rid, out in run["outs"].items():
        assert out.shape == (PROMPT_LENS[rid] + NEW,)
        assert torch.equal(out, run["outs2"][rid])


def test_page_accounting(run):
    for eng in run["engines"]:
        assert len(eng.pool.free_pages) == NUM_PAGES
        assert eng.pool.owned == [0] * MAX_BATCH
        assert int(eng.pool.table.abs().sum()) == 0
        assert eng.idle()
