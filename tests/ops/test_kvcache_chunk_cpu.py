"""flash_attn_chunk_with_kvcache on the CPU: the fp32 composite (_ref_chunk)
against an explicit per-row softmax, its agreement with the decode op and the
fixed-length reference where they overlap, paged / fp8 / ragged / windowed
inputs against the contiguous result, NaN poison in every invisible slot,
argument checks, and generate(prefill_chunk=k) on the tiny models."""
import math

import pytest
import torch

from torchacc_amd.ops import (flash_attn_chunk_with_kvcache,
                              flash_attn_with_kvcache)
from torchacc_amd.ops.flash_attn import (FP8_DTYPE, _gather_pages,
                                         _ref_attention, _ref_chunk,
                                         dequantize_kv_fp8)

FN = flash_attn_chunk_with_kvcache
TOL = 2e-6     # fp32 composites that differ in summation order only


def _make(b, sq, cap, hq, hk, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, sq, hq, d, generator=g)
    k = torch.randn(b, cap, hk, d, generator=g)
    v = torch.randn(b, cap, hk, d, generator=g)
    return q, k, v


def _i32(vals):
    return torch.tensor(vals, dtype=torch.int32)


def _visible(L, n, j, wl, cap, sq):
    """Keys row j of a sequence sees, by the rule of the issue."""
    L = min(max(L, 0), cap)
    n = min(max(n, 0), sq)
    p = L - n + j
    if j >= n or p < 0:
        return []
    lo = max(0, p - wl) if wl >= 0 else 0
    return [t for t in range(lo, p + 1) if t < L]


def _loop(q, k, v, lens, qlens, scale, wl):
    """Explicit softmax per sequence, head and row, in fp64."""
    b, sq, hq, d = q.shape
    cap, hk = k.shape[1], k.shape[2]
    rep = hq // hk
    out = torch.zeros(b, sq, hq, d, dtype=torch.float64)
    lse = torch.full((b, hq, sq), float("-inf"), dtype=torch.float64)
    for i in range(b):
        n = sq if qlens is None else int(qlens[i])
        for j in range(sq):
            keys = _visible(int(lens[i]), n, j, wl, cap, sq)
            if not keys:
                continue
            for h in range(hq):
                kk = k[i, keys, h // rep].double()
                vv = v[i, keys, h // rep].double()
                s = (kk @ q[i, j, h].double()) * scale
                m = s.max()
                e = torch.exp(s - m)
                lse[i, h, j] = m + torch.log(e.sum())
                out[i, j, h] = (e / e.sum()) @ vv
    return out, lse


def _close(got, want, tol=TOL):
    out, lse = got
    wout, wlse = want
    assert out.shape == wout.shape and lse.shape == wlse.shape
    empty = torch.isinf(wlse)
    assert torch.equal(torch.isinf(lse) & (lse < 0), empty)
    assert bool(torch.isfinite(out).all())
    assert float((out.double() - wout.double()).abs().max()) <= tol
    if bool((~empty).any()):
        assert float((lse.double() - wlse.double())[~empty].abs().max()) <= tol


CASES = [
    # lens, q_seqlens, wl
    ([40, 64, 17], None, -1),
    ([40, 64, 17], [5, 0, 3], -1),            # ragged, n = 0
    ([0, 3, 64], [5, 5, 1], -1),              # L = 0, L < n, n = 1
    ([40, 64, 17], None, 0),
    ([40, 64, 9], [5, 2, 4], 7),
    ([70, -3, 64], [9, 5, -1], 3),            # clamped lengths
]


@pytest.mark.parametrize("lens,qlens,wl", CASES)
@pytest.mark.parametrize("heads", [(4, 4), (6, 2)])
def test_ref_chunk_against_explicit_softmax(lens, qlens, wl, heads):
    hq, hk = heads
    q, k, v = _make(3, 5, 64, hq, hk, 16)
    scale = 0.3
    ql = None if qlens is None else _i32(qlens)
    got = _ref_chunk(q, k, v, _i32(lens), ql, scale, wl)
    want = _loop(q, k, v, lens, qlens, scale, wl)
    _close(got, want)
    # the public op on CPU tensors is that composite
    pub = FN(q, k, v, _i32(lens), q_seqlens=ql, softmax_scale=scale,
             window_size=(wl, -1), return_lse=True)
    assert torch.equal(pub[0], got[0]) and torch.equal(pub[1], got[1])
    assert torch.equal(FN(q, k, v, _i32(lens), q_seqlens=ql,
                          softmax_scale=scale, window_size=(wl, -1)), got[0])


@pytest.mark.parametrize("wl", [-1, 0, 9])
def test_single_query_equals_decode_op(wl):
    q, k, v = _make(3, 1, 64, 8, 2, 16, seed=1)
    lens = _i32([40, 0, 64])
    want = flash_attn_with_kvcache(q, k, v, cache_seqlens=lens,
                                   window_size=(wl, -1), return_lse=True)
    got = FN(q, k, v, lens, window_size=(wl, -1), return_lse=True)
    _close(got, want)


@pytest.mark.parametrize("wl", [-1, 5])
def test_full_cache_equals_fixed_length_causal(wl):
    b, sq, cap = 2, 7, 32
    q, k, v = _make(b, sq, cap, 6, 2, 16, seed=2)
    scale = 1.0 / math.sqrt(16)
    want = _ref_attention(q, k, v, scale, True, (wl, -1))
    got = FN(q, k, v, _i32([cap] * b), window_size=(wl, -1), return_lse=True)
    _close(got, want)


@pytest.mark.parametrize("wl", [-1, 6])
def test_ragged_rows_agree_with_each_sequence_alone(wl):
    """Sequence i of a ragged batch equals the op on q[i, :n] alone against
    its own cache; the rows past n are zero with lse = -inf."""
    b, sq, cap = 4, 6, 48
    q, k, v = _make(b, sq, cap, 4, 2, 16, seed=3)
    lens, qlens = [30, 48, 0, 2], [6, 1, 3, 5]     # L = 0 and L < n included
    out, lse = FN(q, k, v, _i32(lens), q_seqlens=_i32(qlens),
                  window_size=(wl, -1), return_lse=True)
    for i, (L, n) in enumerate(zip(lens, qlens)):
        o1, l1 = FN(q[i:i + 1, :n], k[i:i + 1], v[i:i + 1], _i32([L]),
                    window_size=(wl, -1), return_lse=True)
        _close((out[i:i + 1, :n], lse[i:i + 1, :, :n]), (o1, l1))
        assert bool((out[i, n:] == 0).all())
        assert bool(torch.isinf(lse[i, :, n:]).all())
        dead = max(0, n - L)                        # rows with p < 0
        assert bool((out[i, :dead] == 0).all())
        assert bool(torch.isinf(lse[i, :, :dead]).all())


def _paginate(k, v, ps, seed=0, extra=3):
    """Pools with the pages of k / v at permuted indices (plus `extra` unused
    pages) and the table naming them."""
    b, cap, hk, d = k.shape
    w = cap // ps
    n = b * w + extra
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    used = perm[:b * w]
    kp = torch.zeros(n, ps, hk, d, dtype=k.dtype)
    vp = torch.zeros_like(kp)
    kp[used] = k.reshape(b * w, ps, hk, d)
    vp[used] = v.reshape(b * w, ps, hk, d)
    return kp, vp, used.view(b, w).to(torch.int32), perm[b * w:]


@pytest.mark.parametrize("ps", [4, 16])
@pytest.mark.parametrize("wl", [-1, 6])
def test_paged_equals_gathered(ps, wl):
    q, k, v = _make(3, 5, 64, 4, 2, 16, seed=4)
    lens, qlens = _i32([40, 64, 3]), _i32([5, 2, 4])
    want = FN(q, k, v, lens, q_seqlens=qlens, window_size=(wl, -1),
              return_lse=True)
    kp, vp, table, _ = _paginate(k, v, ps)
    assert torch.equal(_gather_pages(kp, table), k)
    for tab in (table, table.long()):
        got = FN(q, kp, vp, lens, q_seqlens=qlens, window_size=(wl, -1),
                 return_lse=True, block_table=tab)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def _quant(x, scale):
    y = x * (1.0 / scale).view(1, 1, -1, 1)
    return y.clamp(-448.0, 448.0).to(FP8_DTYPE)


@pytest.mark.parametrize("paged", [False, True])
def test_fp8_equals_dequantised(paged):
    q, k, v = _make(2, 5, 32, 4, 2, 16, seed=5)
    ks, vs = torch.tensor([0.02, 0.05]), torch.tensor([0.03, 0.01])
    k8, v8 = _quant(k, ks), _quant(v, vs)
    lens, qlens = _i32([32, 11]), _i32([5, 3])
    want = FN(q, dequantize_kv_fp8(k8, ks), dequantize_kv_fp8(v8, vs), lens,
              q_seqlens=qlens, return_lse=True)
    if paged:
        kp, vp, table, _ = _paginate(k8.view(torch.uint8),
                                     v8.view(torch.uint8), 8)
        got = FN(q, kp.view(FP8_DTYPE), vp.view(FP8_DTYPE), lens,
                 q_seqlens=qlens, return_lse=True, block_table=table,
                 k_scale=ks, v_scale=vs)
    else:
        got = FN(q, k8, v8, lens, q_seqlens=qlens, return_lse=True,
                 k_scale=ks, v_scale=vs)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("wl", [-1, 6])
def test_nan_in_invisible_slots_and_unused_pages(wl):
    b, sq, cap, ps = 3, 5, 64, 16
    q, k, v = _make(b, sq, cap, 4, 2, 16, seed=6)
    lens, qlens = [40, 64, 3], [5, 2, 4]
    want = FN(q, k, v, _i32(lens), q_seqlens=_i32(qlens),
              window_size=(wl, -1), return_lse=True)
    kn, vn = k.clone(), v.clone()
    for i in range(b):
        seen = set()
        for j in range(sq):
            seen.update(_visible(lens[i], qlens[i], j, wl, cap, sq))
        hidden = [t for t in range(cap) if t not in seen]
        kn[i, hidden] = float("nan")
        vn[i, hidden] = float("nan")
    got = FN(q, kn, vn, _i32(lens), q_seqlens=_i32(qlens),
             window_size=(wl, -1), return_lse=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    kp, vp, table, unused = _paginate(kn, vn, ps)
    kp[unused] = float("nan")
    vp[unused] = float("nan")
    for i in range(b):      # entries past the live pages: out of range
        table[i, -(-lens[i] // ps):] = 10 ** 6
    got = FN(q, kp, vp, _i32(lens), q_seqlens=_i32(qlens),
             window_size=(wl, -1), return_lse=True, block_table=table)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_argument_checks():
    q, k, v = _make(2, 3, 16, 4, 2, 16)
    lens = _i32([5, 9])
    with pytest.raises((AssertionError, TypeError)):
        FN(q, k, v)                                       # lens are required
    with pytest.raises(AssertionError):
        FN(q, k, v, None)
    with pytest.raises(AssertionError):
        FN(q, k, v, lens.float())
    with pytest.raises(AssertionError):
        FN(q, k, v, _i32([5, 9, 1]))
    with pytest.raises(AssertionError):
        FN(q, k, v, lens, q_seqlens=_i32([1]))
    with pytest.raises(AssertionError):
        FN(q, k, v, lens, q_seqlens=torch.tensor([1.0, 2.0]))
    with pytest.raises(AssertionError):
        FN(q[:, :0], k, v, lens)                          # sq >= 1
    with pytest.raises(AssertionError):
        FN(q[:, :, :3], k, v, lens)                       # h_k | h_q
    with pytest.raises(AssertionError):
        FN(q, k, v[:, :8], lens)
    with pytest.raises(AssertionError):
        FN(q, k.half(), v.half(), lens)
    with pytest.raises(AssertionError):
        FN(q, k, v, lens, k_scale=torch.ones(2), v_scale=torch.ones(2))
    k8, v8 = k.to(FP8_DTYPE), v.to(FP8_DTYPE)
    with pytest.raises(AssertionError):
        FN(q, k8, v8, lens)                               # scales required
    with pytest.raises(AssertionError):
        FN(q, k8, v8, lens, k_scale=torch.ones(3), v_scale=torch.ones(2))
    with pytest.raises(AssertionError):
        FN(q, k, v, lens, block_table=torch.zeros(3, 1, dtype=torch.int32))
    with pytest.raises(AssertionError):
        FN(q, k, v, lens, block_table=torch.zeros(2, 1))
    with pytest.raises(RuntimeError):
        FN(q.clone().requires_grad_(), k, v, lens)
    with torch.no_grad():
        FN(q.clone().requires_grad_(), k, v, lens)


# ---- generate(prefill_chunk=k) ----------------------------------------------
# Seed 0 was picked on the CPU: with it the unchunked fp32 reference of either
# tiny model has no top-2 logit gap below 1e-3 at the prefill position or at
# any of the 6 decode steps (asserted below), so greedy tokens cannot flip on
# the <= 1e-4 differences chunking causes.
SEED = 0
PROMPT, NEW = 11, 6


def _tiny(family):
    torch.manual_seed(SEED)
    if family == "llama":
        from torchacc_amd.models import LlamaForCausalLM, llama_tiny
        model = LlamaForCausalLM(llama_tiny())
    else:
        from torchacc_amd.models import Qwen2ForCausalLM, qwen2_tiny
        model = Qwen2ForCausalLM(qwen2_tiny())
    ids = torch.randint(0, 1024, (2, PROMPT))
    return model.eval(), ids


def _prefill_logits(model, ids, page_size, chunk):
    from torchacc_amd.models import generation as G
    b, s = ids.shape
    if page_size is None:
        p = next(model.parameters())
        caches = [G.LayerKV(b, s, layer.self_attn.num_kv_heads,
                            layer.self_attn.head_dim, p.dtype, p.device)
                  for layer in model.layers]
    else:
        pages = -(-s // page_size)
        caches = G.PagedKVCache.for_model(model, b, b * pages, page_size, s)
    with torch.no_grad():
        return G._prefill(model, ids, caches, chunk)


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_seed_has_no_near_ties(family):
    model, ids = _tiny(family)
    out = ids
    with torch.no_grad():
        for _ in range(NEW + 1):
            top = model(out)[:, -1].float().topk(2, dim=-1).values
            assert float((top[:, 0] - top[:, 1]).min()) >= 1e-3
            out = torch.cat([out, model(out)[:, -1].argmax(-1, keepdim=True)],
                            dim=1)


@pytest.mark.parametrize("chunk", [1, 5, PROMPT])
@pytest.mark.parametrize("page_size", [None, 4])
@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_generate_prefill_chunk(family, page_size, chunk):
    model, ids = _tiny(family)
    want_logits = _prefill_logits(model, ids, page_size, None)
    got_logits = _prefill_logits(model, ids, page_size, chunk)
    assert float((got_logits - want_logits).abs().max()) <= 1e-4
    want = model.generate(ids, max_new_tokens=NEW, page_size=page_size)
    got = model.generate(ids, max_new_tokens=NEW, page_size=page_size,
                         prefill_chunk=chunk)
    assert torch.equal(got, want)


def test_generate_prefill_chunk_fp8_runs_the_op(monkeypatch):
    """Contiguous and paged fp8 caches take later chunks through the new op
    (not a dequantised / gathered copy) and still produce tokens."""
    from torchacc_amd.models import generation as G
    model, ids = _tiny("llama")
    calls = []
    real = G.flash_attn_chunk_with_kvcache

    def counted(*a, **kw):
        calls.append(a[0].shape[1])
        return real(*a, **kw)

    def no_gather(*a, **kw):
        raise AssertionError("PagedKVCache.gather must not be called")

    monkeypatch.setattr(G, "flash_attn_chunk_with_kvcache", counted)
    monkeypatch.setattr(G.PagedKVCache, "gather", no_gather)
    layers = len(model.layers)
    for page_size in (None, 4):
        calls.clear()
        out = model.generate(ids, max_new_tokens=2, page_size=page_size,
                             kv_dtype="fp8", prefill_chunk=4)
        assert out.shape == (2, PROMPT + 2)
        # 11 tokens = 4 + 4 + 3: two later chunks per layer
        assert calls == [4] * layers + [3] * layers, calls
    with pytest.raises(AssertionError):
        model.generate(ids, max_new_tokens=2, prefill_chunk=0)
