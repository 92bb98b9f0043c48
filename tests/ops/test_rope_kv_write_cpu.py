"""rope_kv_cache_write: the torch reference path against explicit per-token
arithmetic, and the front end's argument checks (no GPU needed)."""
import pytest
import torch

from torchacc_amd.ops import kv_cache_write_fp8, rope_kv_cache_write
from torchacc_amd.ops.rope import build_rope_cache

FP8 = torch.float8_e4m3fn
B, S, D, P = 3, 5, 64, 40
N0, N1 = 4, 8
STARTS = (0, 7, 31)     # every row starts elsewhere; row 2 runs to 35 < P


def _case(hq, hk, idx_dtype, dtype=torch.float32):
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, S, hq, D, generator=g).to(dtype)
    k = torch.randn(B, S, hk, D, generator=g).to(dtype)
    v = torch.randn(B, S, hk, D, generator=g).to(dtype)
    cos, sin = build_rope_cache(P, D)
    pos = torch.tensor([[p0 + j for j in range(S)] for p0 in STARTS])
    pos[0, 4] = -1          # padding
    pos[1, 0] = P + 3       # past the table: padding too
    slots = torch.randperm(N0 * N1, generator=g)[:B * S].view(B, S)
    slots[1, 2] = -1        # real token, nothing written
    slots[2, 3] = N0 * N1   # likewise
    return (q, k, v, cos, sin, pos.reshape(-1).to(idx_dtype),
            slots.reshape(-1).to(idx_dtype))


def _rot(x, c, s):
    """One token [h, d] rotated by table row (c, s) [d / 2]."""
    d2 = x.shape[-1] // 2
    x1, x2 = x[:, :d2].float(), x[:, d2:].float()
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).to(x.dtype)


def _pattern(hk, dtype=torch.float32):
    n = N0 * N1 * hk * D
    return ((torch.arange(n) % 251).float() - 125.0).view(N0, N1, hk,
                                                          D).to(dtype)


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("hq,hk", [(4, 1), (2, 2)])
def test_reference_matches_per_token_arithmetic(hq, hk, idx_dtype):
    q, k, v, cos, sin, pos, slots = _case(hq, hk, idx_dtype)
    k_cache, v_cache = _pattern(hk), -_pattern(hk)
    want_k, want_v = k_cache.clone(), v_cache.clone()
    want_q = torch.zeros_like(q)
    padding = []
    for t in range(B * S):
        bi, si = divmod(t, S)
        p, slot = int(pos[t]), int(slots[t])
        if p < 0 or p >= P:
            padding.append((bi, si))
            continue
        want_q[bi, si] = _rot(q[bi, si], cos[p], sin[p])
        if 0 <= slot < N0 * N1:
            want_k[slot // N1, slot % N1] = _rot(k[bi, si], cos[p], sin[p])
            want_v[slot // N1, slot % N1] = v[bi, si]
    assert padding == [(0, 4), (1, 0)]
    got_q = rope_kv_cache_write(q, k, v, cos, sin, pos, k_cache, v_cache,
                                slots)
    assert got_q.shape == q.shape and got_q.dtype == q.dtype
    assert torch.equal(got_q, want_q)
    for bi, si in padding:
        assert got_q[bi, si].abs().max() == 0
    # the named slots hold the new rows, every other slot its pattern
    assert torch.equal(k_cache, want_k) and torch.equal(v_cache, want_v)
    named = torch.zeros(N0 * N1, dtype=torch.bool)
    for t in range(B * S):
        if 0 <= int(pos[t]) < P and 0 <= int(slots[t]) < N0 * N1:
            named[int(slots[t])] = True
    assert int(named.sum()) == B * S - 4
    rest = ~named.view(N0, N1)
    assert torch.equal(k_cache[rest], _pattern(hk)[rest])
    assert torch.equal(v_cache[rest], -_pattern(hk)[rest])


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("hq,hk", [(4, 1), (2, 2)])
def test_fp8_is_round_to_bf16_then_quantise(hq, hk, idx_dtype):
    q, k, v, cos, sin, pos, slots = _case(hq, hk, idx_dtype, torch.bfloat16)
    k_scale = torch.linspace(0.01, 0.02, hk)
    v_scale = torch.linspace(0.015, 0.03, hk)
    fill = torch.full((N0, N1, hk, D), 0x5A, dtype=torch.uint8)
    k_cache, v_cache = fill.clone().view(FP8), fill.clone().view(FP8)
    want_k, want_v = fill.clone().view(FP8), fill.clone().view(FP8)
    # rotated K rounded to bf16 first, then the write op's own reference;
    # padding tokens write nothing: give them an out-of-range slot there
    k_rot = torch.zeros_like(k)
    for t in range(B * S):
        bi, si = divmod(t, S)
        p = int(pos[t])
        if 0 <= p < P:
            k_rot[bi, si] = _rot(k[bi, si], cos[p], sin[p])
    real = (pos >= 0) & (pos < P)
    kv_cache_write_fp8(k_rot, v, want_k, want_v,
                       torch.where(real, slots, torch.full_like(slots, -1)),
                       k_scale, v_scale)
    got_q = rope_kv_cache_write(q, k, v, cos, sin, pos, k_cache, v_cache,
                                slots, k_scale=k_scale, v_scale=v_scale)
    assert got_q.dtype == torch.bfloat16
    assert got_q[0, 4].abs().max() == 0 and got_q[1, 0].abs().max() == 0
    assert torch.equal(k_cache.view(torch.uint8), want_k.view(torch.uint8))
    assert torch.equal(v_cache.view(torch.uint8), want_v.view(torch.uint8))
    assert not torch.equal(k_cache.view(torch.uint8), fill)


def test_argument_checks():
    q, k, v, cos, sin, pos, slots = _case(2, 2, torch.int64, torch.bfloat16)
    kc = torch.zeros(N0, N1, 2, D, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    k8, v8 = kc.to(FP8), vc.to(FP8)
    sc = torch.ones(2)
    with pytest.raises(ValueError, match="float8_e4m3fn caches only"):
        rope_kv_cache_write(q, k, v, cos, sin, pos, kc, vc, slots,
                            k_scale=sc, v_scale=sc)
    with pytest.raises(ValueError, match="need k_scale and v_scale"):
        rope_kv_cache_write(q, k, v, cos, sin, pos, k8, v8, slots)
    with pytest.raises(ValueError, match="slots must be"):
        rope_kv_cache_write(q, k, v, cos, sin, pos, kc, vc, slots[:-1])
    with pytest.raises(ValueError, match="positions must be"):
        rope_kv_cache_write(q, k, v, cos, sin, pos.float(), kc, vc, slots)
    with pytest.raises(ValueError, match="slots must live on q's device"):
        rope_kv_cache_write(q, k, v, cos, sin, pos, kc, vc,
                            slots.to("meta"))
    with pytest.raises(ValueError, match="k_cache must live on q's device"):
        rope_kv_cache_write(q, k, v, cos, sin, pos, kc.to("meta"), vc, slots)
    with pytest.raises(ValueError, match="P >= 1"):
        rope_kv_cache_write(q, k, v, cos[:0], sin[:0], pos, kc, vc, slots)
    with pytest.raises(ValueError, match="caches must have k's dtype"):
        rope_kv_cache_write(q, k, v, cos, sin, pos, kc.float(), vc.float(),
                            slots)
    with pytest.raises(ValueError, match="multiple of 16"):
        rope_kv_cache_write(q[..., :24], k[..., :24], v[..., :24],
                            cos[:, :12], sin[:, :12], pos, kc[..., :24],
                            vc[..., :24], slots)
    # nothing was written by the rejected calls
    assert kc.abs().max() == 0 and vc.abs().max() == 0
