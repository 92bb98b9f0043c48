"""ContinuousBatcher on the CPU reference paths (fp32 tiny models): tokens
equal per-request generate, rows and pages are recycled, admission checks."""
import pytest
import torch

from torchacc_amd.models import (ContinuousBatcher, LlamaForCausalLM,
                                 Qwen2ForCausalLM, llama_tiny, qwen2_tiny)
from torchacc_amd.models import serving

PROMPT_LENS = (3, 12, 7, 20, 1)
NEW_TOKENS = (6, 2, 9, 4, 5)
# 2 pages of 16: request 3 (24 tokens) needs the whole pool, so it waits at
# the head of the queue until both rows have drained, request 4 behind it
NUM_PAGES, PAGE, MAX_LEN, MAX_BATCH, CHUNK = 2, 16, 32, 2, 8


def _model(family):
    torch.manual_seed(0)
    if family == "llama":
        return LlamaForCausalLM(llama_tiny()).eval()
    return Qwen2ForCausalLM(qwen2_tiny()).eval()


def _prompts():
    g = torch.Generator().manual_seed(1)
    return [torch.randint(0, 1024, (n,), generator=g) for n in PROMPT_LENS]


def _engine(model, **kw):
    return ContinuousBatcher(model, MAX_BATCH, NUM_PAGES, PAGE, MAX_LEN,
                             prefill_chunk=CHUNK, **kw)


def _assert_all_pages_back(eng):
    assert len(eng.pool.free_pages) == NUM_PAGES
    assert sorted(eng.pool.free_pages) == list(range(NUM_PAGES))
    assert eng.pool.owned == [0] * eng.max_batch
    assert int(eng.pool.table.abs().sum()) == 0
    assert int(eng.pool.table_host.abs().sum()) == 0


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_run_matches_generate(family):
    """Every request gets exactly the tokens of generate on it alone (the
    precedent: test_generate_matches_naive_decode demands token equality
    between two fp32 paths of these models; at seed 0 / 1 the smallest
    top-1 - top-2 logit gap of the reference over all generated positions is
    6e-3, far above fp32 rounding)."""
    model = _model(family)
    prompts = _prompts()
    eng = _engine(model)
    rids = [eng.add(p, n) for p, n in zip(prompts, NEW_TOKENS)]
    assert rids == list(range(5))
    outs = eng.run()
    assert sorted(outs) == rids
    for rid, p, n in zip(rids, prompts, NEW_TOKENS):
        want = model.generate(p[None], max_new_tokens=n)[0]
        assert outs[rid].shape == (len(p) + n,)
        assert torch.equal(outs[rid], want), (rid, outs[rid], want)
    _assert_all_pages_back(eng)
    assert eng.idle() and eng.run() == {}


def test_fifo_admission_and_head_of_line_blocking():
    model = _model("llama")
    eng = _engine(model)
    for p, n in zip(_prompts(), NEW_TOKENS):
        eng.add(p, n)
    eng.step()
    assert [r.rid for r in eng.rows] == [0, 1]
    started = {}
    for i in range(200):
        if eng.idle():
            break
        eng.step()
        for r in eng.rows:
            if r is not None:
                started.setdefault(r.rid, i)
    assert eng.idle()
    # request 1 ends first (2 tokens) and request 2 takes its row; request 3
    # needs both pages and starts only after 0 and 2 are gone; 4 follows it
    assert started[2] < started[3] <= started[4]
    assert sorted(started) == [0, 1, 2, 3, 4]


def test_eos_finishes_and_row_is_reused():
    model = _model("llama")
    prompts = _prompts()
    full = model.generate(prompts[2][None], max_new_tokens=9)[0]
    eos = int(full[7 + 2])   # force the 3rd generated token to be "eos"
    assert eos not in full[7:7 + 2].tolist()
    eng = ContinuousBatcher(model, 1, NUM_PAGES, PAGE, MAX_LEN,
                            prefill_chunk=CHUNK)
    a = eng.add(prompts[2], 9, eos_token_id=eos)
    b = eng.add(prompts[0], 6)
    events = []
    while not eng.idle():
        events += eng.step()
    got_a = [(t, f) for rid, t, f in events if rid == a]
    assert [t for t, _ in got_a] == full[7:7 + 3].tolist()
    assert [f for _, f in got_a] == [False, False, True]
    # the single row went to the waiting request right after
    first_b = next(i for i, e in enumerate(events) if e[0] == b)
    assert all(e[0] == a for e in events[:first_b])
    assert all(e[0] == b for e in events[first_b:])
    outs = eng.run()
    assert torch.equal(outs[a], full[:7 + 3])
    assert torch.equal(outs[b],
                       model.generate(prompts[0][None], max_new_tokens=6)[0])
    _assert_all_pages_back(eng)


def test_add_rejects_what_can_never_fit():
    model = _model("llama")
    eng = _engine(model)
    with pytest.raises(ValueError, match="pages"):
        eng.add(torch.zeros(30, dtype=torch.long), 3)     # 33 > 2 pages
    wide = ContinuousBatcher(model, 1, 1, PAGE, 64)       # table 4, pool 1
    with pytest.raises(ValueError, match="pages"):
        wide.add(torch.zeros(10, dtype=torch.long), 7)
    big = ContinuousBatcher(model, 1, 64, PAGE, 1024)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        big.add(torch.zeros(500, dtype=torch.long), 13)   # 513 > 512
    with pytest.raises(ValueError, match="at least one token"):
        eng.add(torch.zeros(0, dtype=torch.long), 3)
    assert eng.idle() and wide.idle() and big.idle()
    eng.add(torch.zeros(29, dtype=torch.long), 3)         # 32: just fits


def test_fp8_needs_scales():
    model = _model("llama")
    with pytest.raises(ValueError, match="shared by every request"):
        _engine(model, kv_dtype="fp8")
    with pytest.raises(ValueError, match="fp8 KV cache only"):
        _engine(model, kv_scales=[(1.0, 1.0)] * len(model.layers))
    eng = _engine(model, kv_dtype="fp8",
                  kv_scales=[(0.05, 0.05)] * len(model.layers))
    rid = eng.add(_prompts()[1], 3)
    out = eng.run()[rid]
    assert out.shape == (15,)
    _assert_all_pages_back(eng)


def test_attention_op_per_step(monkeypatch):
    """All rows decoding -> the decode op; any prefill piece or idle row ->
    the chunk op."""
    calls = []
    real_decode = serving.flash_attn_with_kvcache
    real_chunk = serving.flash_attn_chunk_with_kvcache

    def decode(*a, **kw):
        calls.append("decode")
        assert a[0].shape[1] == 1 and kw["block_table"] is not None
        return real_decode(*a, **kw)

    def chunk(*a, **kw):
        calls.append("chunk")
        return real_chunk(*a, **kw)

    monkeypatch.setattr(serving, "flash_attn_with_kvcache", decode)
    monkeypatch.setattr(serving, "flash_attn_chunk_with_kvcache", chunk)
    model = _model("llama")
    layers = len(model.layers)
    prompts = _prompts()
    eng = _engine(model)
    eng.add(prompts[1], 4)      # 12 tokens: pieces of 8 and 4
    eng.add(prompts[0], 2)      # 3 tokens: one piece
    want = [
        "chunk",    # 8 | 3: both prefill; row 1 yields its first token
        "chunk",    # 4 | 1: prefill piece next to a decoding row; row 1 ends
        "chunk",    # 1 | idle: a decoding row next to an idle one
    ]
    for kind in want:
        calls.clear()
        eng.step()
        assert calls == [kind] * layers, calls
    assert eng.rows[1] is None and eng.rows[0] is not None
    eng.add(prompts[4], 5)      # 1 token: its prefill piece has n = 1
    for _ in range(2):          # 1 | 1 twice: every row holds one token
        calls.clear()
        eng.step()
        assert calls == ["decode"] * layers, calls
    assert eng.rows[0] is None  # 4 tokens done
    calls.clear()
    eng.step()
    assert calls == ["chunk"] * layers, calls
    eng.run()
    _assert_all_pages_back(eng)
