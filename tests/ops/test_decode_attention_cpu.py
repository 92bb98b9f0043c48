"""CPU path of flash_attn_with_kvcache against a hand-written per-batch
softmax(q K^T) V on the visible slice (fp32, atol 1e-5), plus the argument
checks."""
import math

import pytest
import torch

from torchacc_amd.ops import flash_attn_with_kvcache

ATOL = 1e-5


def _by_hand(q, k, v, lens, wl):
    """Per batch, per head: plain softmax over keys [lo, len)."""
    b, _, hq, d = q.shape
    hk = k.shape[2]
    rep = hq // hk
    out = torch.zeros(b, 1, hq, d)
    lse = torch.full((b, hq, 1), float("-inf"))
    for i in range(b):
        n = int(lens[i])
        if n == 0:
            continue
        lo = max(0, n - 1 - wl) if wl >= 0 else 0
        for h in range(hq):
            ks = k[i, lo:n, h // rep]                  # [n-lo, d]
            vs = v[i, lo:n, h // rep]
            s = (ks @ q[i, 0, h]) / math.sqrt(d)
            lse[i, h, 0] = torch.logsumexp(s, 0)
            out[i, 0, h] = torch.softmax(s, 0) @ vs
    return out, lse


def _inputs(b, cap, hq, hk, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, 1, hq, d, generator=g)
    k = torch.randn(b, cap, hk, d, generator=g)
    v = torch.randn(b, cap, hk, d, generator=g)
    return q, k, v


@pytest.mark.parametrize("window", [(-1, -1), (16, -1)])
@pytest.mark.parametrize("lens_dtype", [torch.int32, torch.int64])
def test_lens_gqa_window(window, lens_dtype):
    q, k, v = _inputs(3, 64, 8, 2, 32)
    lens = torch.tensor([1, 37, 64], dtype=lens_dtype)
    out, lse = flash_attn_with_kvcache(q, k, v, cache_seqlens=lens,
                                       window_size=window, return_lse=True)
    ref, ref_lse = _by_hand(q, k, v, lens, window[0])
    assert out.shape == (3, 1, 8, 32) and lse.shape == (3, 8, 1)
    assert lse.dtype == torch.float32
    torch.testing.assert_close(out, ref, atol=ATOL, rtol=0)
    torch.testing.assert_close(lse, ref_lse, atol=ATOL, rtol=0)


def test_strided_cache_without_lens():
    q, big_k, big_v = _inputs(3, 64, 8, 2, 32, seed=1)
    k, v = big_k[:, :40], big_v[:, :40]
    assert not k.is_contiguous() and not v.is_contiguous()
    out, lse = flash_attn_with_kvcache(q, k, v, return_lse=True)
    ref, ref_lse = _by_hand(q, k, v, [40, 40, 40], -1)
    torch.testing.assert_close(out, ref, atol=ATOL, rtol=0)
    torch.testing.assert_close(lse, ref_lse, atol=ATOL, rtol=0)
    # plain return is the output alone
    assert torch.equal(flash_attn_with_kvcache(q, k, v), out)


def test_empty_sequence_gives_zeros_and_minus_inf():
    q, k, v = _inputs(3, 64, 8, 2, 32, seed=2)
    lens = torch.tensor([0, 5, 0], dtype=torch.int32)
    out, lse = flash_attn_with_kvcache(q, k, v, cache_seqlens=lens,
                                       return_lse=True)
    ref, ref_lse = _by_hand(q, k, v, lens, -1)
    assert torch.equal(out[0], torch.zeros_like(out[0]))
    assert torch.equal(out[2], torch.zeros_like(out[2]))
    assert bool((lse[0] == float("-inf")).all())
    assert bool((lse[2] == float("-inf")).all())
    torch.testing.assert_close(out, ref, atol=ATOL, rtol=0)
    torch.testing.assert_close(lse[1], ref_lse[1], atol=ATOL, rtol=0)


def test_invisible_slots_cannot_matter():
    q, k, v = _inputs(2, 64, 4, 2, 32, seed=3)
    lens = torch.tensor([20, 50], dtype=torch.int32)
    ref, ref_lse = _by_hand(q, k, v, lens, 16)
    k, v = k.clone(), v.clone()
    for i, n in enumerate(lens.tolist()):
        for t in (k, v):
            t[i, n:] = float("nan")
            t[i, :max(0, n - 1 - 16)] = float("nan")
    out, lse = flash_attn_with_kvcache(q, k, v, cache_seqlens=lens,
                                       window_size=(16, -1), return_lse=True)
    torch.testing.assert_close(out, ref, atol=ATOL, rtol=0)
    torch.testing.assert_close(lse, ref_lse, atol=ATOL, rtol=0)


def test_more_than_one_query_raises():
    q, k, v = _inputs(2, 16, 4, 2, 32)
    with pytest.raises(AssertionError):
        flash_attn_with_kvcache(torch.cat([q, q], dim=1), k, v)


def test_bad_arguments_raise():
    q, k, v = _inputs(2, 16, 4, 2, 32)
    with pytest.raises(AssertionError):      # hk does not divide hq
        flash_attn_with_kvcache(q[:, :, :3], k, v)
    with pytest.raises(AssertionError):      # lens dtype
        flash_attn_with_kvcache(q, k, v, cache_seqlens=torch.ones(2))
    with pytest.raises(AssertionError):      # lens shape
        flash_attn_with_kvcache(
            q, k, v, cache_seqlens=torch.ones(3, dtype=torch.int32))
    with pytest.raises(AssertionError):      # dtype mismatch
        flash_attn_with_kvcache(q, k.double(), v.double())


def test_requires_grad_raises_under_grad_mode():
    q, k, v = _inputs(2, 16, 4, 2, 32)
    q.requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference only"):
        flash_attn_with_kvcache(q, k, v)
    with torch.no_grad():
        flash_attn_with_kvcache(q, k, v)     # fine without grad mode
