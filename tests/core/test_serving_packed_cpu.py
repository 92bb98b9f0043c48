"""ContinuousBatcher(packed=True) on the CPU reference paths (fp32, the setup
of test_serving_cpu.py): exactly the tokens of the padded engine, every page
back afterwards, and the packed op on every step that is not all-decode."""
import pytest
import torch

from torchacc_amd.models import serving
from tests.core.test_serving_cpu import (NEW_TOKENS, _assert_all_pages_back,
                                         _engine, _model, _prompts)


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_packed_tokens_equal_padded(family, monkeypatch):
    model = _model(family)
    calls = []
    for name in ("flash_attn_with_kvcache", "flash_attn_chunk_with_kvcache",
                 "flash_attn_varlen_with_kvcache"):
        def counted(*a, _real=getattr(serving, name), _name=name, **kw):
            calls.append(_name)
            return _real(*a, **kw)
        monkeypatch.setattr(serving, name, counted)
    outs = []
    for packed in (False, True):
        calls.clear()
        eng = _engine(model, packed=packed)
        rids = [eng.add(p, n) for p, n in zip(_prompts(), NEW_TOKENS)]
        outs.append(eng.run())
        assert sorted(outs[-1]) == rids
        _assert_all_pages_back(eng)
        kinds = set(calls)
        assert "flash_attn_with_kvcache" in kinds
        assert ("flash_attn_varlen_with_kvcache" in kinds) == packed
        assert ("flash_attn_chunk_with_kvcache" in kinds) != packed
    for rid in outs[0]:
        assert torch.equal(outs[0][rid], outs[1][rid]), rid
