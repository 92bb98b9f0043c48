"""flash_attn_chunk_with_kvcache(num_splits=) on the CPU: the fp32 composite
validates the argument and ignores it."""
import pytest
import torch

from torchacc_amd.ops import flash_attn_chunk_with_kvcache as FN


def _inputs(paged):
    g = torch.Generator().manual_seed(0)
    b, sq, cap, hq, hk, d = 3, 5, 64, 4, 2, 32
    q = torch.randn(b, sq, hq, d, generator=g)
    k = torch.randn(b, cap, hk, d, generator=g)
    v = torch.randn(b, cap, hk, d, generator=g)
    lens = torch.tensor([5, 0, 33], dtype=torch.int32)
    kw = {"q_seqlens": torch.tensor([5, 2, 3], dtype=torch.int32),
          "window_size": (8, -1), "return_lse": True}
    if paged:
        ps, w = 8, cap // 8
        perm = torch.randperm(b * w, generator=g)
        pool_k = torch.empty(b * w, ps, hk, d)
        pool_v = torch.empty(b * w, ps, hk, d)
        pool_k[perm] = k.reshape(b * w, ps, hk, d)
        pool_v[perm] = v.reshape(b * w, ps, hk, d)
        k, v = pool_k, pool_v
        kw["block_table"] = perm.view(b, w).to(torch.int32)
    return (q, k, v, lens), kw


@pytest.mark.parametrize("paged", [False, True])
def test_num_splits_is_ignored_on_the_cpu(paged):
    args, kw = _inputs(paged)
    want = FN(*args, **kw)
    for ns in (0, 1, 5):
        got = FN(*args, num_splits=ns, **kw)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_num_splits_is_the_last_parameter():
    """Positional callers of the earlier signature are unaffected."""
    import inspect
    names = list(inspect.signature(FN).parameters)
    assert names[-1] == "num_splits"
    assert inspect.signature(FN).parameters["num_splits"].default == 0


@pytest.mark.parametrize("bad", [-1, -7, 1.0, "2", None, True])
def test_bad_num_splits_raises(bad):
    args, kw = _inputs(False)
    with pytest.raises((AssertionError, TypeError)):
        FN(*args, num_splits=bad, **kw)
