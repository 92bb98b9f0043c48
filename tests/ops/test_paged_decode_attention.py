"""GPU numerics of flash_attn_with_kvcache with a block table (paged variant
of the split-KV decode kernel).

The main check is exact: the paged kernel keeps the contiguous kernel's
key-to-lane mapping, tile loop, split chunks and arithmetic order and changes
the address computation only, so on a pool cut from a contiguous cache its
out and lse are bitwise the contiguous op's at the same num_splits. On top of
that every case meets the bounds of test_decode_attention.py against the
fp32 reference on inputs quantised to the kernel dtype first:
        out  max|got - ref| <= 1.5e-2 * max|ref|
        lse  max|got - ref| <= 1e-2

No test uses an out-of-range page index: the kernel's clamp is there so that
a bad table cannot read out of bounds, and is not provoked here.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

OUT_REL = 1.5e-2
LSE_ABS = 1e-2
BF16, FP16 = torch.bfloat16, torch.float16
CAP = 1024
NAN = float("nan")


def _op():
    from torchacc_amd.ops import flash_attn_with_kvcache
    return flash_attn_with_kvcache


@functools.lru_cache(maxsize=None)
def _make(b, cap, hq, hk, d, dtype, seed=0):
    """CPU tensors already rounded to `dtype`, held in fp32. Shared between
    tests: never modified in place."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, 1, hq, d, generator=g).to(dtype).float()
    k = torch.randn(b, cap, hk, d, generator=g).to(dtype).float()
    v = torch.randn(b, cap, hk, d, generator=g).to(dtype).float()
    return q, k, v


@functools.lru_cache(maxsize=None)
def _reference(klens, b, cap, hq, hk, d, dtype, wl, seed=0):
    q, k, v = _make(b, cap, hq, hk, d, dtype, seed)
    return _op()(q, k, v, cache_seqlens=_lens(klens), window_size=(wl, -1),
                 return_lse=True)


def _lens(vals):
    return torch.tensor(vals, dtype=torch.int32)


def _paginate(k, v, ps, extra=1, seed=1):
    """Cut contiguous [b, cap, hk, d] caches (any device) into pages placed
    at permuted physical indices. Returns the pools, the int32 table and the
    indices of `extra` spare pages that no table entry names (zero-filled)."""
    b, cap, hk, d = k.shape
    w = cap // ps
    assert w * ps == cap
    n = b * w + extra
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    table = perm[:b * w].view(b, w).to(torch.int32)
    idx = table.reshape(-1).long().to(k.device)
    kp = torch.zeros(n, ps, hk, d, dtype=k.dtype, device=k.device)
    vp = torch.zeros(n, ps, hk, d, dtype=v.dtype, device=v.device)
    kp[idx] = k.reshape(b * w, ps, hk, d)
    vp[idx] = v.reshape(b * w, ps, hk, d)
    return kp, vp, table.to(k.device), perm[b * w:].tolist()


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


def _same(a, b, tag):
    assert torch.equal(a[0], b[0]), f"{tag}: out differs bitwise"
    assert torch.equal(a[1], b[1]), f"{tag}: lse differs bitwise"


def _run_case(klens, heads, d, dtype, ns, ps, wl=-1, cap=CAP):
    """Paged op on a permuted pool vs the contiguous op on the cache the pool
    was cut from (bitwise), and vs the fp32 reference (tolerance)."""
    hq, hk = heads
    b = len(klens)
    fn = _op()
    q, k, v = _make(b, cap, hq, hk, d, dtype)
    gq, gk, gv = (t.to("cuda", dtype) for t in (q, k, v))
    lens = _lens(klens).cuda()
    kp, vp, table, _ = _paginate(gk, gv, ps)
    want = fn(gq, gk, gv, cache_seqlens=lens, window_size=(wl, -1),
              num_splits=ns, return_lse=True)
    got = fn(gq, kp, vp, cache_seqlens=lens, window_size=(wl, -1),
             num_splits=ns, return_lse=True, block_table=table)
    assert got[0].dtype == dtype and got[1].dtype == torch.float32
    tag = f"{klens} {heads} d{d} ns{ns} ps{ps} wl{wl}"
    _same(got, want, tag)
    _check(*got, *_reference(tuple(klens), b, cap, hq, hk, d, dtype, wl), tag)
    return got


KLENS = [[1, 1], [15, 16], [17, 32], [63, 64], [65, 128], [257, 1000],
         [1024, 0]]

# page 16: with d = 128 a wave row of 16 key slots is exactly one page, with
# d = 64 one 32-slot load straddles two pages. Every boundary length set with
# one split and with five, then the host's own choice; then each remaining
# value of heads / dtype / page size once.
GRID = [(kl, (8, 2), d, BF16, ns, 16)
        for d in (128, 64) for kl in KLENS for ns in (1, 5)] + [
    ([257, 1000], (8, 2), 128, BF16, 0, 16),
    ([257, 1000], (8, 2), 64, BF16, 0, 16),
    ([257, 1000], (4, 4), 64, BF16, 5, 16),
    ([257, 1000], (28, 4), 128, BF16, 5, 16),
    ([65, 128], (32, 2), 64, BF16, 5, 16),
    ([257, 1000], (32, 2), 128, BF16, 0, 16),
    ([257, 1000], (8, 1), 128, BF16, 5, 16),
    ([257, 1000], (28, 4), 128, FP16, 0, 16),
    ([63, 64], (4, 4), 64, FP16, 1, 16),
    ([257, 1000], (8, 2), 128, BF16, 5, 64),
    ([65, 128], (8, 2), 64, BF16, 1, 64),
    ([257, 1000], (8, 2), 128, BF16, 5, 256),
    ([257, 1000], (4, 4), 64, FP16, 0, 256),
]


@pytest.mark.parametrize("klens,heads,d,dtype,ns,ps", GRID)
def test_bitwise_equal_to_contiguous(klens, heads, d, dtype, ns, ps):
    _run_case(klens, heads, d, dtype, ns, ps)


@pytest.mark.parametrize("ns", [1, 5])
@pytest.mark.parametrize("wl", [0, 16, 100])
def test_window(wl, ns):
    """lo = 64, 48, 0 and 299, 283, 199: not page- or tile-aligned."""
    klens = [65, 300]
    out, _ = _run_case(klens, (8, 2), 128, BF16, ns, 16, wl=wl)
    if wl == 0:
        # one visible key: p = 1, out is V's last visible row, exactly
        _, _, v = _make(2, CAP, 8, 2, 128, BF16)
        for i, n in enumerate(klens):
            want = v[i, n - 1].repeat_interleave(4, dim=0)   # [hq, d]
            assert torch.equal(out[i, 0].float().cpu(), want)


def test_shared_prefix_pages():
    """Two table rows name the same physical pages for their first three
    logical pages."""
    fn = _op()
    q, k, v = _make(2, 256, 8, 2, 128, BF16, seed=2)
    k, v = k.clone(), v.clone()
    k[1, :48], v[1, :48] = k[0, :48], v[0, :48]
    gq, gk, gv = (t.to("cuda", BF16) for t in (q, k, v))
    lens = _lens([50, 200]).cuda()
    kp, vp, table, _ = _paginate(gk, gv, 16)
    table[1, :3] = table[0, :3]
    ref = fn(q, k, v, cache_seqlens=lens.cpu(), return_lse=True)
    for ns in (1, 5):
        want = fn(gq, gk, gv, cache_seqlens=lens, num_splits=ns,
                  return_lse=True)
        got = fn(gq, kp, vp, cache_seqlens=lens, num_splits=ns,
                 return_lse=True, block_table=table)
        _same(got, want, f"shared prefix ns{ns}")
        _check(*got, *ref, f"shared prefix ns{ns}")


@pytest.mark.parametrize("ns", [1, 5])
@pytest.mark.parametrize("wl", [-1, 100])
def test_poisoned_slots_and_pages_cannot_matter(ns, wl):
    """Every slot outside [lo, len) is NaN (the tail of the last live page,
    the head of the window's first page, whole pages before and after),
    whole unreferenced pages are NaN, and every unused table entry points at
    a valid all-NaN page. The output is finite and bitwise the clean run's:
    loads are predicated, not multiplied by p = 0."""
    fn = _op()
    klens, ps = [257, 1000], 16
    q, k, v = _make(2, CAP, 8, 2, 128, BF16)
    gq = q.to("cuda", BF16)
    lens = _lens(klens).cuda()
    clean = _run_case(klens, (8, 2), 128, BF16, ns, ps, wl=wl)
    k, v = k.clone(), v.clone()
    for i, n in enumerate(klens):
        lo = max(0, n - 1 - wl) if wl >= 0 else 0
        for t in (k, v):
            t[i, n:] = NAN
            t[i, :lo] = NAN
    kp, vp, table, spare = _paginate(k.to("cuda", BF16), v.to("cuda", BF16),
                                     ps, extra=3)
    for t in (kp, vp):
        t[spare] = NAN
    for i, n in enumerate(klens):
        table[i, (n + ps - 1) // ps:] = spare[i]
    got = fn(gq, kp, vp, cache_seqlens=lens, window_size=(wl, -1),
             num_splits=ns, return_lse=True, block_table=table)
    assert bool(torch.isfinite(got[0]).all())
    _same(got, clean, f"poison ns{ns} wl{wl}")


def test_strided_pool():
    """Pools that are strided views: K with a page stride larger than
    page_size * hk * d, V with a larger slot stride as well."""
    fn = _op()
    hk, d, ps = 2, 128, 16
    q, k, v = _make(2, 256, 8, hk, d, BF16, seed=3)
    gq, gk, gv = (t.to("cuda", BF16) for t in (q, k, v))
    kp, vp, table, _ = _paginate(gk, gv, ps)
    n = kp.shape[0]
    row = hk * d
    kbuf = torch.full((n, ps * row + 8 * row), NAN, dtype=BF16, device="cuda")
    ks = kbuf.as_strided((n, ps, hk, d), (kbuf.stride(0), row, d, 1))
    vbuf = torch.full((n, ps * (row + 8) + 64), NAN, dtype=BF16,
                      device="cuda")
    vs = vbuf.as_strided((n, ps, hk, d), (vbuf.stride(0), row + 8, d, 1))
    ks.copy_(kp)
    vs.copy_(vp)
    assert not ks.is_contiguous() and not vs.is_contiguous()
    lens = _lens([77, 256]).cuda()
    ref = fn(q, k, v, cache_seqlens=lens.cpu(), return_lse=True)
    for ns in (1, 3):
        want = fn(gq, gk, gv, cache_seqlens=lens, num_splits=ns,
                  return_lse=True)
        got = fn(gq, ks, vs, cache_seqlens=lens, num_splits=ns,
                 return_lse=True, block_table=table)
        _same(got, want, f"strided pool ns{ns}")
        _check(*got, *ref, f"strided pool ns{ns}")


def test_page_stride_past_2_31_elements():
    """The pools are views whose second page lies more than 2^31 elements
    from the first: page offsets must be computed in 64 bits."""
    fn = _op()
    hk, d, ps = 2, 128, 64
    q, k, v = _make(2, 2 * ps, 8, hk, d, BF16, seed=4)
    stride_p = 2 ** 31 + 8 * hk * d
    n = ps * hk * d
    buf = torch.empty(stride_p + 2 * n, dtype=BF16, device="cuda")
    kp = buf.as_strided((2, ps, hk, d), (stride_p, hk * d, d, 1), 0)
    vp = buf.as_strided((2, ps, hk, d), (stride_p, hk * d, d, 1), n)
    # sequence 0 holds pages (1, 0), sequence 1 only page 1: fill the pools
    # from sequence 0 and read sequence 1 through the shared page
    table = torch.tensor([[1, 0], [1, 0]], dtype=torch.int32, device="cuda")
    for pool, src in ((kp, k), (vp, v)):
        pool[1].copy_(src[0, :ps])
        pool[0].copy_(src[0, ps:])
    kc = torch.stack([k[0], k[0]])
    vc = torch.stack([v[0], v[0]])
    lens = _lens([2 * ps - 5, 40])
    ref = fn(q, kc, vc, cache_seqlens=lens, return_lse=True)
    gq = q.to("cuda", BF16)
    want = fn(gq, kc.to("cuda", BF16), vc.to("cuda", BF16),
              cache_seqlens=lens.cuda(), return_lse=True)
    got = fn(gq, kp, vp, cache_seqlens=lens.cuda(), return_lse=True,
             block_table=table)
    _same(got, want, "2^31 page stride")
    _check(*got, *ref, "2^31 page stride")


def test_determinism():
    fn = _op()
    q, k, v = _make(2, CAP, 8, 2, 128, BF16)
    gq, gk, gv = (t.to("cuda", BF16) for t in (q, k, v))
    kp, vp, table, _ = _paginate(gk, gv, 16)
    lens = _lens([257, 1000]).cuda()
    for ns in (1, 5, 0):
        a = fn(gq, kp, vp, cache_seqlens=lens, num_splits=ns,
               return_lse=True, block_table=table)
        b = fn(gq, kp, vp, cache_seqlens=lens, num_splits=ns,
               return_lse=True, block_table=table)
        _same(a, b, f"determinism ns{ns}")


def test_graph_capture_follows_device_lengths_and_table():
    fn = _op()
    q, k, v = _make(2, CAP, 8, 2, 128, BF16)
    gq, gk, gv = (t.to("cuda", BF16) for t in (q, k, v))
    kp, vp, table, _ = _paginate(gk, gv, 16)
    lens = _lens([40, 70]).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(gq, kp, vp, cache_seqlens=lens, num_splits=5, block_table=table)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = fn(gq, kp, vp, cache_seqlens=lens, num_splits=5,
                      return_lse=True, block_table=table)

    def replay_and_check(tag):
        graph.replay()
        eager = fn(gq, kp, vp, cache_seqlens=lens, num_splits=5,
                   return_lse=True, block_table=table)
        torch.cuda.synchronize()
        _same((out, lse), eager, tag)
        ref = fn(gq.float().cpu(), gk.float().cpu(), gv.float().cpu(),
                 cache_seqlens=lens.cpu(), return_lse=True)
        _check(out, lse, *ref, tag)

    replay_and_check("graph [40, 70]")
    # append one token per sequence in place, as a decode step does
    g = torch.Generator().manual_seed(7)
    for i, n in enumerate((40, 70)):
        for cache, pool in ((gk, kp), (gv, vp)):
            new = torch.randn(2, 128, generator=g).to("cuda", BF16)
            cache[i, n] = new
            pool[int(table[i, n // 16]), n % 16] = new
    lens.add_(1)
    replay_and_check("graph [41, 71]")
    # longer lengths AND another page assignment, data moved accordingly:
    # only device buffers changed
    kp2, vp2, table2, _ = _paginate(gk, gv, 16, seed=9)
    assert not torch.equal(table2, table)
    kp.copy_(kp2)
    vp.copy_(vp2)
    table.copy_(table2)
    lens.copy_(_lens([200, 300]))
    replay_and_check("graph [200, 300], new table")


@pytest.mark.parametrize("dtype,d,ps", [(torch.float32, 64, 16),
                                        (BF16, 96, 16), (BF16, 128, 24)])
def test_uncovered_inputs_stay_on_the_gpu(dtype, d, ps):
    """fp32, head dims other than 64/128 and page sizes that are no power
    of two >= 16 gather the pages on the device and run the fixed-length
    GPU attention with the same visibility rule."""
    fn = _op()
    q, k, v = _make(3, 48, 4, 2, d, dtype, seed=5)
    lens = _lens([5, 0, 33])
    ref = fn(q, k, v, cache_seqlens=lens, return_lse=True)
    kp, vp, table, _ = _paginate(k.to("cuda", dtype), v.to("cuda", dtype), ps)
    out, lse = fn(q.to("cuda", dtype), kp, vp, cache_seqlens=lens.cuda(),
                  return_lse=True, block_table=table)
    assert out.is_cuda and lse.is_cuda and out.dtype == dtype
    _check(out, lse, *ref, f"paged fallback {dtype} d{d} ps{ps}")


def test_generation_end_to_end(monkeypatch):
    """generate(page_size=16) and GraphDecoder(page_size=16) return exactly
    the tokens of the contiguous paths: at these capacities (< 512) the host
    picks one split in both layouts and the key ranges start at 0 in both,
    so the attention outputs are bitwise equal."""
    from torchacc_amd.models import LlamaConfig, LlamaForCausalLM
    from torchacc_amd.models import generation
    calls = []
    real = generation.flash_attn_with_kvcache

    def counted(*a, **kw):
        calls.append(kw.get("block_table") is not None)
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
    assert calls == [False] * (11 * 2), calls
    calls.clear()
    paged = model.generate(ids, max_new_tokens=12, page_size=16)
    # 11 decode steps x 2 layers, all through the block table
    assert calls == [True] * (11 * 2), calls
    assert torch.equal(paged, eager), (paged[:, 60:], eager[:, 60:])

    # a pool sized for ONE batch serves two calls: pages come back
    pool = generation.PagedKVCache.for_model(model, 2, 2 * 5, 16, 72)
    for _ in range(2):
        again = model.generate(ids, max_new_tokens=12, kv_pool=pool)
        assert torch.equal(again, eager)
        assert len(pool.free_pages) == 10

    want = generation.GraphDecoder(model, 2, 128).decode(ids, 12)
    calls.clear()
    dec = generation.GraphDecoder(model, 2, 128, page_size=16)
    got = dec.decode(ids, 12)
    torch.cuda.synchronize()
    # two warm-up steps and the captured one, 2 layers each
    assert calls == [True] * (3 * 2), calls
    assert torch.equal(got, want), (got[:, 60:], want[:, 60:])
    # another page assignment: free everything, re-reserve in reversed
    # order (the two sequences swap their pages); the captured graph reads
    # the new table at replay
    calls.clear()
    before = dec.paged.table.clone()
    for i in reversed(range(2)):
        dec.paged.free(i)
    for i in reversed(range(2)):
        dec.paged.reserve(i, 128)
    assert not torch.equal(dec.paged.table, before)
    got2 = dec.decode(ids, 12)
    torch.cuda.synchronize()
    assert calls == [] and torch.equal(got2, got)
