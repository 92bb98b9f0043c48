"""flash_attn_with_kvcache and flash_attn_chunk_with_kvcache share one
argument front end: both refuse the same invalid inputs with an
AssertionError, before any arithmetic (CPU tensors, no extension)."""
import pytest
import torch

from torchacc_amd.ops import (flash_attn_chunk_with_kvcache,
                              flash_attn_with_kvcache)

FP8 = torch.float8_e4m3fn
B, HQ, HK, D, PS, W = 2, 4, 2, 16, 4, 3


def _decode(q, k, v, lens, **kw):
    return flash_attn_with_kvcache(q[:, :1], k, v, cache_seqlens=lens, **kw)


def _chunk(q, k, v, lens, **kw):
    return flash_attn_chunk_with_kvcache(q, k, v, lens, **kw)


def _inputs(fp8=False):
    g = torch.Generator().manual_seed(0)
    q = torch.randn(B, 2, HQ, D, generator=g)
    k = torch.randn(B, PS * W, HK, D, generator=g)
    v = torch.randn(B, PS * W, HK, D, generator=g)
    if fp8:
        k, v = k.to(FP8), v.to(FP8)
    return q, k, v, torch.tensor([5, 9], dtype=torch.int32)


def _pools(k, v):
    return (k.reshape(B * W, PS, HK, D), v.reshape(B * W, PS, HK, D),
            torch.arange(B * W, dtype=torch.int32).view(B, W))


@pytest.mark.parametrize("op", [_decode, _chunk])
def test_valid_inputs_pass(op):
    q, k, v, lens = _inputs()
    kp, vp, table = _pools(k, v)
    want = op(q, k, v, lens)
    assert torch.equal(op(q, kp, vp, lens, block_table=table), want)
    q, k8, v8, lens = _inputs(fp8=True)
    s = torch.full((HK,), 0.5)
    op(q, k8, v8, lens, k_scale=s, v_scale=s)


@pytest.mark.parametrize("op", [_decode, _chunk])
def test_both_ops_refuse_the_same_inputs(op):
    q, k, v, lens = _inputs()
    kp, vp, table = _pools(k, v)
    with pytest.raises(AssertionError, match="requires cache_seqlens"):
        op(q, kp, vp, None, block_table=table)
    with pytest.raises(AssertionError):     # table with the wrong batch
        op(q, kp, vp, lens, block_table=table[:1])
    with pytest.raises(AssertionError):     # table of a non-integer dtype
        op(q, kp, vp, lens, block_table=table.float())
    _, k8, v8, _ = _inputs(fp8=True)
    s = torch.full((HK,), 0.5)
    with pytest.raises(AssertionError):     # fp8 caches without scales
        op(q, k8, v8, lens)
    with pytest.raises(AssertionError):     # scales with 16-bit caches
        op(q, k, v, lens, k_scale=s, v_scale=s)
    with pytest.raises(AssertionError):     # a scale of the wrong shape
        op(q, k8, v8, lens, k_scale=s, v_scale=torch.full((HK + 1,), 0.5))
