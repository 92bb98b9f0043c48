"""GPU numerics of flash_attn_with_kvcache (split-KV decode kernel).

Inputs are quantised to the kernel dtype BEFORE the fp32 reference (the op's
CPU path) is computed, so the error measured is the kernel's own.

Bounds: out  max|got - ref| <= 1.5e-2 * max|ref|
        lse  max|got - ref| <= 1e-2
A CPU emulation of bf16 rounding in such a kernel gives 0.002-0.004 on the
output scale at contexts 63..4097, while losing ONE visible key costs
>= 0.035 and a 64-key tile >= 0.2, so the relative bound separates the two
(the absolute 2.5e-2 of the prefill tests would not at |ref| ~ 0.1-0.8).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

OUT_REL = 1.5e-2
LSE_ABS = 1e-2
BF16, FP16 = torch.bfloat16, torch.float16


def _op():
    from torchacc_amd.ops import flash_attn_with_kvcache
    return flash_attn_with_kvcache


def _make(b, cap, hq, hk, d, dtype, seed=0):
    """CPU tensors already rounded to `dtype`, held in fp32."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, 1, hq, d, generator=g).to(dtype).float()
    k = torch.randn(b, cap, hk, d, generator=g).to(dtype).float()
    v = torch.randn(b, cap, hk, d, generator=g).to(dtype).float()
    return q, k, v


def _gpu(t, dtype):
    return t.to("cuda", dtype)


def _lens(vals):
    return torch.tensor(vals, dtype=torch.int32)


def _check(out, lse, ref, ref_lse, tag=""):
    out = out.float().cpu()
    lse = lse.float().cpu()
    assert out.shape == ref.shape and lse.shape == ref_lse.shape
    assert bool(torch.isfinite(out).all()), "non-finite output"
    err = float((out - ref).abs().max())
    bound = OUT_REL * float(ref.abs().max())
    empty = torch.isinf(ref_lse)
    got_empty = torch.isinf(lse) & (lse < 0)
    lerr = 0.0
    if bool((~empty).any()):
        lerr = float((lse - ref_lse)[~empty].abs().max())
    print(f"{tag} out err {err:.3e} (bound {bound:.3e})  lse err {lerr:.3e}")
    assert torch.equal(got_empty, empty), "lse = -inf rows differ"
    assert err <= bound, (err, bound)
    assert lerr <= LSE_ABS, lerr


def _run_case(klens, heads, d, dtype, ns, wl=-1, cap=1024, poison=False):
    hq, hk = heads
    fn = _op()
    q, k, v = _make(len(klens), cap, hq, hk, d, dtype)
    lens = _lens(klens)
    ref, ref_lse = fn(q, k, v, cache_seqlens=lens, window_size=(wl, -1),
                      return_lse=True)
    if poison:  # what torch.empty may leave in never-written slots
        k, v = k.clone(), v.clone()
        for i, n in enumerate(klens):
            lo = max(0, n - 1 - wl) if wl >= 0 else 0
            for t in (k, v):
                t[i, n:] = float("nan")
                t[i, :lo] = float("nan")
    out, lse = fn(_gpu(q, dtype), _gpu(k, dtype), _gpu(v, dtype),
                  cache_seqlens=lens.cuda(), window_size=(wl, -1),
                  num_splits=ns, return_lse=True)
    assert out.dtype == dtype and lse.dtype == torch.float32
    _check(out, lse, ref, ref_lse, f"{klens} {heads} d{d} ns{ns} wl{wl}")
    return out, lse


KLENS = [[1, 1], [63, 64], [65, 128], [257, 1000], [1024, 0]]

# every boundary length set with one split and with five (five divides
# nothing and leaves empty splits at short lengths), then each remaining
# value of heads / head dim / dtype / num_splits at least once
GRID = [(kl, (8, 2), 128, BF16, ns) for kl in KLENS for ns in (1, 5)] + [
    ([257, 1000], (4, 4), 64, BF16, 2),
    ([257, 1000], (28, 4), 128, FP16, 0),
    ([65, 128], (32, 2), 64, FP16, 5),
    ([257, 1000], (32, 2), 128, BF16, 0),
    ([63, 64], (28, 4), 64, BF16, 1),
    ([1024, 0], (4, 4), 128, FP16, 2),
    ([257, 1000], (8, 1), 128, BF16, 5),
]


@pytest.mark.parametrize("klens,heads,d,dtype,ns", GRID)
def test_parity_grid(klens, heads, d, dtype, ns):
    _run_case(klens, heads, d, dtype, ns)


def test_strided_cache_no_lens():
    fn = _op()
    q, big_k, big_v = _make(3, 512, 8, 2, 128, BF16, seed=1)
    ref, ref_lse = fn(q, big_k[:, :200], big_v[:, :200], return_lse=True)
    gk, gv = _gpu(big_k, BF16)[:, :200], _gpu(big_v, BF16)[:, :200]
    assert not gk.is_contiguous() and not gv.is_contiguous()
    for ns in (1, 3):
        out, lse = fn(_gpu(q, BF16), gk, gv, num_splits=ns, return_lse=True)
        _check(out, lse, ref, ref_lse, f"strided ns{ns}")


@pytest.mark.parametrize("ns", [1, 5])
@pytest.mark.parametrize("wl", [-1, 100])
def test_uninitialised_slots_cannot_matter(ns, wl):
    """Every slot outside [lo, k_lens) is NaN in K and V: the output must be
    finite and as accurate as on a clean cache (loads are predicated, not
    multiplied by p = 0)."""
    _run_case([257, 1000], (8, 2), 128, BF16, ns, wl=wl, poison=True)


@pytest.mark.parametrize("ns", [1, 5])
@pytest.mark.parametrize("wl", [0, 16, 100])
def test_window(wl, ns):
    klens = [65, 300]
    out, _ = _run_case(klens, (8, 2), 128, BF16, ns, wl=wl)
    if wl == 0:
        # one visible key: p = 1, out is V's last visible row, exactly
        _, _, v = _make(2, 1024, 8, 2, 128, BF16)
        for i, n in enumerate(klens):
            want = v[i, n - 1].repeat_interleave(4, dim=0)   # [hq, d]
            assert torch.equal(out[i, 0].float().cpu(), want)


def test_split_invariance_and_determinism():
    fn = _op()
    q, k, v = _make(2, 1024, 8, 2, 128, BF16)
    gq, gk, gv = (_gpu(t, BF16) for t in (q, k, v))
    lens = _lens([257, 1000]).cuda()
    res = {}
    for ns in (1, 5):
        a = fn(gq, gk, gv, cache_seqlens=lens, num_splits=ns,
               return_lse=True)
        b = fn(gq, gk, gv, cache_seqlens=lens, num_splits=ns,
               return_lse=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        res[ns] = a
    o1, o5 = res[1][0].float(), res[5][0].float()
    assert float((o1 - o5).abs().max()) <= OUT_REL * float(o1.abs().max())
    assert float((res[1][1] - res[5][1]).abs().max()) <= LSE_ABS


@pytest.mark.parametrize("heads", [(4, 4), (8, 2)])
def test_against_full_tile_kernel(heads):
    """Same numbers as the prefill kernel run at sq = 1 over the contiguous
    cache with k_lens (the decode path before this kernel existed)."""
    from torchacc_amd.ops._backend import require_extension
    ext = require_extension()
    fn = _op()
    hq, hk = heads
    q, k, v = _make(2, 1024, hq, hk, 128, BF16)
    gq, gk, gv = (_gpu(t, BF16) for t in (q, k, v))
    lens = _lens([257, 1000]).cuda()
    e = torch.empty(0)
    old, old_lse = ext.fa_forward(gq, gk, gv, 1.0 / math.sqrt(128), True,
                                  -1, -1, e, lens, e, 0.0, 0)
    new, new_lse = fn(gq, gk, gv, cache_seqlens=lens, return_lse=True)
    _check(new, new_lse, old.float().cpu(), old_lse.cpu(), f"vs old {heads}")


def test_graph_capture_follows_device_lengths():
    fn = _op()
    q, k, v = _make(2, 1024, 8, 2, 128, BF16)
    gq, gk, gv = (_gpu(t, BF16) for t in (q, k, v))
    lens = _lens([40, 70]).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(gq, gk, gv, cache_seqlens=lens, num_splits=5)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = fn(gq, gk, gv, cache_seqlens=lens, num_splits=5,
                      return_lse=True)

    def replay_and_check(tag):
        graph.replay()
        eager, eager_lse = fn(gq, gk, gv, cache_seqlens=lens, num_splits=5,
                              return_lse=True)
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(lse, eager_lse)
        ref, ref_lse = fn(gq.float().cpu(), gk.float().cpu(),
                          gv.float().cpu(), cache_seqlens=lens.cpu(),
                          return_lse=True)
        _check(out, lse, ref, ref_lse, tag)

    replay_and_check("graph [40, 70]")
    # append one token per sequence in place, as a decode step does
    g = torch.Generator().manual_seed(7)
    for i, n in enumerate((40, 70)):
        gk[i, n] = torch.randn(2, 128, generator=g).to("cuda", BF16)
        gv[i, n] = torch.randn(2, 128, generator=g).to("cuda", BF16)
    lens.add_(1)
    replay_and_check("graph [41, 71]")
    # a jump across several tiles and splits: only the device length changed
    lens.copy_(_lens([200, 300]))
    replay_and_check("graph [200, 300]")


def test_batch_stride_past_2_31_elements():
    """The caches are views whose second batch lies more than 2^31 elements
    into the buffer: offsets must be computed in 64 bits."""
    fn = _op()
    cap, hk, d = 96, 2, 128
    q, k, v = _make(2, cap, 8, hk, d, BF16, seed=3)
    stride_b = 2 ** 31 + 8 * hk * d
    n = cap * hk * d
    buf = torch.empty(stride_b + 2 * n, dtype=BF16, device="cuda")
    gk = buf.as_strided((2, cap, hk, d), (stride_b, hk * d, d, 1), 0)
    gv = buf.as_strided((2, cap, hk, d), (stride_b, hk * d, d, 1), n)
    gk.copy_(k)
    gv.copy_(v)
    lens = _lens([96, 77])
    ref, ref_lse = fn(q, k, v, cache_seqlens=lens, return_lse=True)
    out, lse = fn(_gpu(q, BF16), gk, gv, cache_seqlens=lens.cuda(),
                  return_lse=True)
    _check(out, lse, ref, ref_lse, "2^31 stride")


@pytest.mark.parametrize("dtype,d", [(torch.float32, 64), (BF16, 96)])
def test_uncovered_inputs_take_the_fixed_length_path(dtype, d):
    """fp32 and padded head dims are not silently computed on the CPU: they
    run the fixed-length GPU attention with the same visibility rule."""
    fn = _op()
    q, k, v = _make(3, 64, 4, 2, d, dtype, seed=4)
    lens = _lens([5, 0, 33])
    ref, ref_lse = fn(q, k, v, cache_seqlens=lens, window_size=(8, -1),
                      return_lse=True)
    out, lse = fn(_gpu(q, dtype), _gpu(k, dtype), _gpu(v, dtype),
                  cache_seqlens=lens.cuda(), window_size=(8, -1),
                  return_lse=True)
    assert out.is_cuda and out.dtype == dtype
    _check(out, lse, ref, ref_lse, f"fallback {dtype} d{d}")


@pytest.mark.parametrize("dtype,d", [(torch.float32, 64), (BF16, 32)])
def test_uncovered_inputs_capture_with_device_lengths(dtype, d):
    """Without a window the uncovered inputs run one batched call that never
    reads the lengths on the host: it captures into a graph, follows the
    device lengths on replay, and ignores NaN past them."""
    fn = _op()
    q, k, v = _make(3, 64, 4, 2, d, dtype, seed=5)
    gq = _gpu(q, dtype)
    gk, gv = _gpu(k, dtype), _gpu(v, dtype)
    lens = _lens([5, 0, 33]).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(gq, gk, gv, cache_seqlens=lens)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = fn(gq, gk, gv, cache_seqlens=lens, return_lse=True)
    for vals in ([5, 0, 33], [64, 17, 0]):
        lens.copy_(_lens(vals))
        ref, ref_lse = fn(q, k, v, cache_seqlens=_lens(vals),
                          return_lse=True)
        for i, n in enumerate(vals):       # poison what must not be read
            gk[i, n:] = float("nan")
            gv[i, n:] = float("nan")
        graph.replay()
        torch.cuda.synchronize()
        _check(out, lse, ref, ref_lse, f"fallback graph {dtype} d{d} {vals}")
        gk.copy_(k)
        gv.copy_(v)


def test_graph_decoder_with_uncovered_head_dim():
    """head_dim 32 is outside the decode kernel: GraphDecoder must still
    capture (padded fixed-length attention, device lengths) and agree with
    the eager loop."""
    from torchacc_amd.models import LlamaConfig, LlamaForCausalLM
    from torchacc_amd.models.generation import GraphDecoder
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=1024, hidden_size=256,
                      intermediate_size=512, num_hidden_layers=2,
                      num_attention_heads=8, num_key_value_heads=2,
                      max_position_embeddings=128)
    with torch.device("cuda"):
        model = LlamaForCausalLM(cfg).to(torch.bfloat16).eval()
    assert model.layers[0].self_attn.head_dim == 32
    ids = torch.randint(0, 1024, (2, 20), device="cuda")
    eager = model.generate(ids, max_new_tokens=12)
    dec = GraphDecoder(model, 2, 64)
    got = dec.decode(ids, 12)
    torch.cuda.synchronize()
    agree = (got[:, 20:] == eager[:, 20:]).float().mean()
    assert agree > 0.9, (float(agree), got[:, 20:], eager[:, 20:])
    got2 = dec.decode(ids, 12)
    torch.cuda.synchronize()
    assert torch.equal(got2, got)


def test_int64_lens_and_argument_errors():
    fn = _op()
    q, k, v = _make(2, 128, 8, 2, 64, BF16)
    gq, gk, gv = (_gpu(t, BF16) for t in (q, k, v))
    a = fn(gq, gk, gv, cache_seqlens=_lens([5, 100]).cuda())
    b = fn(gq, gk, gv, cache_seqlens=torch.tensor([5, 100]).cuda())
    assert torch.equal(a, b)
    with pytest.raises(AssertionError):
        fn(torch.cat([gq, gq], 1), gk, gv)
    with pytest.raises(AssertionError):       # lens on the wrong device
        fn(gq, gk, gv, cache_seqlens=_lens([5, 100]))
    wide = torch.zeros(2, 128, 2, 128, dtype=BF16, device="cuda")
    with pytest.raises(RuntimeError):         # [heads][d] not dense
        fn(gq, wide[..., :64], wide[..., :64])


def test_generation_end_to_end(monkeypatch):
    """Eager generate and the captured GraphDecoder both decode through the
    new op (context crosses 64 while decoding) and agree on the tokens."""
    from torchacc_amd.models import LlamaConfig, LlamaForCausalLM
    from torchacc_amd.models import generation
    calls = []
    real = generation.flash_attn_with_kvcache

    def counted(*a, **kw):
        calls.append(a[1].shape[1])
        return real(*a, **kw)

    monkeypatch.setattr(generation, "flash_attn_with_kvcache", counted)
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=1024, hidden_size=1024,
                      intermediate_size=2048, num_hidden_layers=2,
                      num_attention_heads=8, num_key_value_heads=2,
                      max_position_embeddings=256)
    with torch.device("cuda"):
        model = LlamaForCausalLM(cfg).to(torch.bfloat16).eval()
    ids = torch.randint(0, 1024, (2, 60), device="cuda")
    eager = model.generate(ids, max_new_tokens=12)
    # the prompt's last position yields token 1; 11 decode steps x 2 layers
    assert len(calls) == 11 * 2, calls
    assert calls[0] == 61 and calls[-1] == 71, calls
    calls.clear()
    dec = generation.GraphDecoder(model, 2, 128)
    got = dec.decode(ids, 12)
    torch.cuda.synchronize()
    # two warm-up steps and the captured one, 2 layers each, full-cache view
    assert len(calls) == 3 * 2 and set(calls) == {128}, calls
    assert got.shape == eager.shape
    agree = (got[:, 60:] == eager[:, 60:]).float().mean()
    assert agree > 0.9, (float(agree), got[:, 60:], eager[:, 60:])
    calls.clear()
    got2 = dec.decode(ids, 12)
    torch.cuda.synchronize()
    assert calls == [] and torch.equal(got2, got)
