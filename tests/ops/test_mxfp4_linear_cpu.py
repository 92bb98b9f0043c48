"""MXFP4 quantiser, CPU formula and model swap (ops/linear_mxfp4.py); no GPU."""
import pytest
import torch
import torch.nn as nn

from torchacc_amd import models
from torchacc_amd.ops import (Mxfp4Linear, Mxfp4SwiGLUMLP,
                              dequantize_weight_mxfp4, mxfp4_linear,
                              mxfp4_swiglu_linear, quantize_model_mxfp4,
                              quantize_weight_mxfp4)


def _random_codes(n, k, lo, hi, seed=0):
    """Random codes whose every group holds a +-4 or +-6, random scale bytes."""
    g = torch.Generator().manual_seed(seed)
    el = torch.randint(0, 16, (n, k // 32, 32), generator=g, dtype=torch.uint8)
    top = torch.tensor([6, 7, 14, 15], dtype=torch.uint8)
    el[..., 5] = top[torch.randint(0, 4, (n, k // 32), generator=g)]
    el = el.reshape(n, k // 2, 2)
    codes = el[..., 0] | (el[..., 1] << 4)
    scales = torch.randint(lo, hi + 1, (n, k // 32), generator=g,
                           dtype=torch.uint8)
    return codes, scales


def test_quantiser_reproduces_representable_weights():
    # every scale byte the bf16 contract allows: 1 (2^-126) .. 252 (2^125)
    codes, scales = _random_codes(24, 256, 1, 252)
    w = dequantize_weight_mxfp4(codes, scales, torch.float32)
    c2, s2 = quantize_weight_mxfp4(w)
    assert c2.dtype == torch.uint8 and s2.dtype == torch.uint8
    assert torch.equal(s2, scales)
    assert torch.equal(dequantize_weight_mxfp4(c2, s2, torch.float32), w)


def test_quantiser_edge_cases():
    w = torch.zeros(2, 64)
    # group (0, 1): amax 4 -> exponent 0; midpoints between grid neighbours
    # round to the one with mantissa bit 0, and values beyond 6 saturate
    mids = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -2.5,
                         -5.0, 4.0])
    w[0, 32:32 + len(mids)] = mids
    w[1, 0:3] = torch.tensor([7.9, -7.9, 1e-45])   # amax in [4, 8): exponent 0
    w[1, 32] = 1e-45                                # below 2^-126: byte 1
    codes, scales = quantize_weight_mxfp4(w)
    assert scales.tolist() == [[127, 127], [127, 1]]
    assert int(codes[0, :16].max()) == 0            # all-zero group
    deq = dequantize_weight_mxfp4(codes, scales, torch.float32)
    want = torch.tensor([0., 1., 1., 2., 2., 4., 4., -0., -2., -4., 4.])
    assert torch.equal(deq[0, 32:32 + len(mids)], want)
    assert deq[1, :3].tolist() == [6.0, -6.0, 0.0]
    assert float(deq[1, 32:].abs().max()) == 0.0
    with pytest.raises(ValueError, match="multiple of 32"):
        quantize_weight_mxfp4(torch.zeros(4, 48))
    with pytest.raises(ValueError, match="non-finite"):
        quantize_weight_mxfp4(torch.full((1, 32), float("inf")))


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_cpu_ops_match_dequantised_matmul(bias):
    g = torch.Generator().manual_seed(1)
    cg, sg = _random_codes(40, 96, 120, 130, seed=1)
    cu, su = _random_codes(40, 96, 120, 130, seed=2)
    x = torch.randn(3, 5, 96, generator=g)
    bg = torch.randn(40, generator=g) if bias else None
    bu = torch.randn(40, generator=g) if bias else None
    wg = dequantize_weight_mxfp4(cg, sg, torch.float32)
    wu = dequantize_weight_mxfp4(cu, su, torch.float32)
    gate, up = x @ wg.t(), x @ wu.t()
    if bias:
        gate, up = gate + bg, up + bu
    assert torch.allclose(mxfp4_linear(x, cg, sg, bg), gate, rtol=1e-6,
                          atol=1e-6)
    got = mxfp4_swiglu_linear(x, cg, sg, cu, su, bg, bu)
    want = torch.nn.functional.silu(gate) * up
    assert got.shape == (3, 5, 40)
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-5)
    with pytest.raises(RuntimeError, match="inference-only"):
        mxfp4_linear(x.clone().requires_grad_(), cg, sg, bg)
    with pytest.raises(ValueError, match="multiple of 32"):
        mxfp4_linear(x[..., :48], cg, sg, bg)


def test_quantize_model_swaps_modules_and_keeps_uint8():
    torch.manual_seed(0)
    cfg = models.llama_tiny(intermediate_size=704, num_hidden_layers=1)
    plain = models.LlamaForCausalLM(cfg).eval()
    before = [(n, type(m)) for n, m in plain.named_modules()]
    model = quantize_model_mxfp4(models.LlamaForCausalLM(cfg).eval(),
                                 include_lm_head=True)
    # the unquantised model's tree is what it was before anything was swapped
    assert [(n, type(m)) for n, m in plain.named_modules()] == before
    assert not any(isinstance(m, (Mxfp4Linear, Mxfp4SwiGLUMLP))
                   for m in plain.modules())
    layer = model.layers[0]
    assert isinstance(layer.mlp, Mxfp4SwiGLUMLP)
    assert isinstance(layer.mlp.down_proj, Mxfp4Linear)
    assert isinstance(layer.self_attn.q_proj, Mxfp4Linear)
    assert isinstance(model.lm_head, Mxfp4Linear)
    assert not any(type(m) is nn.Linear for m in model.layers.modules())
    model = model.to(torch.float16)
    uint8 = [b.dtype for n, b in model.named_buffers()
             if n.endswith(("codes", "scales"))]
    assert len(uint8) == 2 * 4 + 2 * 3 + 2 and set(uint8) == {torch.uint8}
    with torch.no_grad():
        logits = model.float()(torch.randint(0, 1024, (1, 6)))
    assert bool(torch.isfinite(logits).all())


def test_quantize_model_names_the_layer_with_bad_in_features():
    model = models.LlamaForCausalLM(models.llama_tiny(num_hidden_layers=1))
    with pytest.raises(ValueError, match=r"layers\.0\.mlp\.down_proj.*688"):
        quantize_model_mxfp4(model)
    # nothing was swapped
    assert not any(isinstance(m, Mxfp4Linear) for m in model.modules())
