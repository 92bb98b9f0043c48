"""fp8 (e4m3fn) KV cache on the CPU reference path: the quantising write op,
the decode op on fp8 caches (contiguous and paged), the argument checks, and
generate(kv_dtype="fp8") on a tiny model."""
import pytest
import torch

FP8 = torch.float8_e4m3fn


def _ops():
    from torchacc_amd.ops import flash_attn_with_kvcache, kv_cache_write_fp8
    return flash_attn_with_kvcache, kv_cache_write_fp8


def _codes(x, scale):
    """The specified quantisation: fp32 reciprocal, fp32 product, clamp,
    round to nearest even."""
    inv = (1.0 / scale.float()).view(1, 1, -1, 1)
    return (x.float() * inv).clamp(-448, 448).to(FP8)


def _bytes(t):
    return t.view(torch.uint8)


def _special_rows(hk, d):
    """Saturating values, e4m3 ties (17, 18, 19 lie between 16, 18, 20 at a
    spacing of 2: 17 -> 16, 19 -> 20 by ties-to-even), the largest finite
    value and its neighbours, and magnitudes around and below the smallest
    subnormal 2^-9 (half of it ties to zero)."""
    vals = [1000.0, -1000.0, 448.0, -448.0, 449.0, 464.0, 17.0, 18.0, 19.0,
            -17.0, -19.0, 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -10,
            2.0 ** -11, -2.0 ** -12, 1e-8, 0.0, 0.3, -5.7]
    row = torch.tensor(vals).repeat((hk * d + len(vals) - 1) // len(vals))
    return row[:hk * d].view(hk, d)


def test_write_codes_are_the_specified_rounding():
    _, write = _ops()
    b, s, hk, d, n0, n1 = 2, 3, 2, 24, 4, 8
    g = torch.Generator().manual_seed(0)
    k = (torch.randn(b, s, hk, d, generator=g) * 40).to(torch.bfloat16)
    v = (torch.randn(b, s, hk, d, generator=g) * 3).to(torch.bfloat16)
    k[0, 0] = _special_rows(hk, d).to(torch.bfloat16)
    v[1, 2] = _special_rows(hk, d).to(torch.bfloat16)
    ks = torch.tensor([0.5, 4.0])
    vs = torch.tensor([2.0, 0.125])
    poison = 0x5a
    kc = torch.full((n0, n1, hk, d), poison, dtype=torch.uint8).view(FP8)
    vc = torch.full((n0, n1, hk, d), poison, dtype=torch.uint8).view(FP8)
    slots = torch.tensor([9, 31, 0, 17, 3, 22])          # permuted, unique
    write(k, v, kc, vc, slots, ks, vs)
    for x, cache, scale in ((k, kc, ks), (v, vc, vs)):
        want = _bytes(_codes(x, scale)).reshape(b * s, hk, d)
        flat = _bytes(cache).reshape(n0 * n1, hk, d)
        assert torch.equal(flat[slots], want)
        # no finite input becomes the NaN code
        assert not bool(((flat[slots] & 0x7f) == 0x7f).any())
        # only the named slots changed
        rest = torch.ones(n0 * n1, dtype=torch.bool)
        rest[slots] = False
        assert bool((flat[rest] == poison).all())
    # spot checks of the rounding itself (scale 0.5 on head 0: x * 2)
    got = kc.view(-1, hk, d)[9, 0].float()
    assert got[0] == 448 and got[1] == -448          # +-1000 * 2 saturate
    sk = _codes(torch.tensor([17.0, 18.0, 19.0]).view(1, 1, 1, 3),
                torch.ones(1)).float().flatten().tolist()
    assert sk == [16.0, 18.0, 20.0]


def test_write_int32_slots_and_strided_pool():
    _, write = _ops()
    b, s, hk, d, n0, n1 = 1, 4, 2, 16, 3, 4
    g = torch.Generator().manual_seed(1)
    k = torch.randn(b, s, hk, d, generator=g).to(torch.float16)
    v = torch.randn(b, s, hk, d, generator=g).to(torch.float16)
    sc = torch.tensor([0.25, 1.0])
    buf = torch.zeros(2, n0, n1 + 2, hk, d, dtype=torch.uint8).view(FP8)
    kc, vc = buf[0, :, :n1], buf[1, :, :n1]
    assert not kc.is_contiguous()
    slots = torch.tensor([11, 2, 5, 8], dtype=torch.int32)
    write(k, v, kc, vc, slots, sc, sc)
    for x, cache in ((k, kc), (v, vc)):
        want = _bytes(_codes(x, sc)).reshape(s, hk, d)
        for i, t in enumerate(slots.tolist()):
            assert torch.equal(_bytes(cache)[t // n1, t % n1], want[i])
    # the padding slots of the strided buffer stay untouched
    assert bool((_bytes(buf)[:, :, n1:] == 0).all())


def _paginate(k, v, ps, extra=1, seed=1):
    b, cap, hk, d = k.shape
    w = cap // ps
    n = b * w + extra
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    table = perm[:b * w].view(b, w).to(torch.int32)
    idx = table.reshape(-1).long()
    kp = torch.zeros(n, ps, hk, d, dtype=torch.uint8)
    vp = torch.zeros(n, ps, hk, d, dtype=torch.uint8)
    kp[idx] = _bytes(k).reshape(b * w, ps, hk, d)
    vp[idx] = _bytes(v).reshape(b * w, ps, hk, d)
    return kp.view(FP8), vp.view(FP8), table


@pytest.mark.parametrize("wl", [-1, 7])
def test_decode_equals_reference_on_dequantised_cache(wl):
    from torchacc_amd.ops.flash_attn import _ref_decode
    fn, _ = _ops()
    b, cap, hq, hk, d = 3, 48, 4, 2, 32
    g = torch.Generator().manual_seed(2)
    q = torch.randn(b, 1, hq, d, generator=g)
    ks = torch.tensor([0.013, 0.021])
    vs = torch.tensor([0.017, 0.009])
    k8 = _codes(torch.randn(b, cap, hk, d, generator=g), ks)
    v8 = _codes(torch.randn(b, cap, hk, d, generator=g), vs)
    lens = torch.tensor([5, 0, 33], dtype=torch.int32)
    want = _ref_decode(q, k8.float() * ks.view(1, 1, -1, 1),
                       v8.float() * vs.view(1, 1, -1, 1), lens, d ** -0.5,
                       wl)
    got = fn(q, k8, v8, cache_seqlens=lens, window_size=(wl, -1),
             return_lse=True, k_scale=ks, v_scale=vs)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert bool((got[0][1] == 0).all()) and bool(torch.isinf(got[1][1]).all())
    kp, vp, table = _paginate(k8, v8, 16)
    paged = fn(q, kp, vp, cache_seqlens=lens, window_size=(wl, -1),
               return_lse=True, block_table=table, k_scale=ks, v_scale=vs)
    assert torch.equal(paged[0], want[0]) and torch.equal(paged[1], want[1])


def test_argument_checks():
    fn, write = _ops()
    b, cap, hq, hk, d = 1, 16, 4, 2, 32
    q = torch.randn(b, 1, hq, d)
    k8 = torch.zeros(b, cap, hk, d, dtype=torch.uint8).view(FP8)
    ok = torch.ones(hk)
    fn(q, k8, k8, k_scale=ok, v_scale=ok)
    bad = [dict(), dict(k_scale=ok), dict(v_scale=ok),
           dict(k_scale=torch.ones(hk + 1), v_scale=ok),
           dict(k_scale=ok, v_scale=torch.ones(hk, 1)),
           dict(k_scale=ok.double(), v_scale=ok),
           dict(k_scale=ok, v_scale=ok.to(torch.bfloat16)),
           dict(k_scale=1.0, v_scale=ok)]
    for kw in bad:
        with pytest.raises((AssertionError, ValueError, TypeError)):
            fn(q, k8, k8, **kw)
    # scales with caches of q's dtype, and mixed cache dtypes
    kf = torch.zeros(b, cap, hk, d)
    with pytest.raises((AssertionError, ValueError)):
        fn(q, kf, kf, k_scale=ok, v_scale=ok)
    with pytest.raises((AssertionError, ValueError)):
        fn(q, k8, kf, k_scale=ok, v_scale=ok)
    x = torch.randn(b, 1, hk, d).to(torch.bfloat16)
    slots = torch.zeros(1, dtype=torch.int64)
    write(x, x, k8, k8.clone(), slots, ok, ok)
    with pytest.raises((AssertionError, ValueError)):
        write(x, x, k8, k8, slots, torch.ones(hk + 1), ok)
    with pytest.raises((AssertionError, ValueError)):
        write(x, x, kf, kf, slots, ok, ok)


def _tiny_llama():
    from torchacc_amd.models import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=128, hidden_size=64, intermediate_size=128,
                      num_hidden_layers=2, num_attention_heads=8,
                      num_key_value_heads=2, max_position_embeddings=256)
    return LlamaForCausalLM(cfg).eval()


def test_generate_fp8():
    from torchacc_amd.models import generation
    model = _tiny_llama()
    ids = torch.randint(0, 128, (2, 21),
                        generator=torch.Generator().manual_seed(3))
    base = model.generate(ids, max_new_tokens=6)
    cont = model.generate(ids, max_new_tokens=6, kv_dtype="fp8")
    paged = model.generate(ids, max_new_tokens=6, kv_dtype="fp8",
                           page_size=16)
    assert cont.shape == base.shape
    assert torch.equal(cont, paged)
    # prefill never reads the cache
    assert torch.equal(cont[:, :22], base[:, :22])

    # a caller-owned fp8 pool decides the dtype; its pages come back
    pool = generation.PagedKVCache.for_model(model, 2, 2 * 2, 16, 27,
                                             kv_dtype="fp8")
    assert pool.k[0].dtype == FP8 and pool.k_scale[0].dtype == torch.float32
    assert pool.k_scale[1].shape == (2,)
    for _ in range(2):
        again = model.generate(ids, max_new_tokens=6, kv_pool=pool)
        assert torch.equal(again, cont)
        assert len(pool.free_pages) == 4
    # the prefill calibration wrote the scale buffers in place
    assert not torch.equal(pool.k_scale[0], torch.ones(2))
    same = model.generate(ids, max_new_tokens=6, kv_pool=pool,
                          kv_dtype="fp8")
    assert torch.equal(same, cont)

    plain = generation.PagedKVCache.for_model(model, 2, 2 * 2, 16, 27)
    with pytest.raises(ValueError):
        model.generate(ids, max_new_tokens=6, kv_pool=plain, kv_dtype="fp8")
    assert all(n == 0 for n in plain.owned)
    with pytest.raises(ValueError):
        model.generate(ids, max_new_tokens=6, kv_scales=[(1.0, 1.0)] * 2)
    with pytest.raises(ValueError):
        model.generate(ids, max_new_tokens=6, kv_dtype="int4")


def test_generate_fp8_given_scales_are_kept():
    from torchacc_amd.models import generation
    model = _tiny_llama()
    ids = torch.randint(0, 128, (1, 9),
                        generator=torch.Generator().manual_seed(4))
    pool = generation.PagedKVCache.for_model(model, 1, 2, 16, 16,
                                             kv_dtype="fp8")
    scales = [(torch.tensor([0.05, 0.07]), 0.03), (0.04, 0.02)]
    out = model.generate(ids, max_new_tokens=4, kv_pool=pool,
                         kv_scales=scales)
    assert out.shape == (1, 13)
    assert torch.equal(pool.k_scale[0], torch.tensor([0.05, 0.07]))
    assert torch.equal(pool.v_scale[0], torch.full((2,), 0.03))
    assert torch.equal(pool.k_scale[1], torch.full((2,), 0.04))


def test_layerkv_fp8_write_matches_op_and_dequantised_multi_token_step():
    """LayerKV(kv_dtype="fp8") computes batch * cap + pos slots; several new
    tokens against a non-empty fp8 cache attend a dequantised copy."""
    from torchacc_amd.models.generation import LayerKV
    b, cap, hk, d = 2, 8, 2, 16
    c = LayerKV(b, cap, hk, d, torch.float32, "cpu", kv_dtype="fp8")
    assert c.k.dtype == FP8 and torch.equal(c.k_scale, torch.ones(hk))
    _bytes(c.k).fill_(0x7f)
    c.k_scale.copy_(torch.tensor([0.5, 0.25]))
    g = torch.Generator().manual_seed(5)
    k = torch.randn(b, 3, hk, d, generator=g)
    c.append(k, k)
    assert c.len == 3
    assert torch.equal(_bytes(c.k[:, :3]), _bytes(_codes(k, c.k_scale)))
    assert bool((_bytes(c.k[:, 3:]) == 0x7f).all())
