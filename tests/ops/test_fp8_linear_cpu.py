"""fp8 weight quantiser, Fp8Linear and quantize_model_fp8 on the CPU."""
import pytest
import torch
import torch.nn as nn

from torchacc_amd.ops import (Fp8Linear, fp8_linear, quantize_model_fp8,
                              quantize_weight_fp8)
from torchacc_amd.ops.linear import TunedLinear


def test_quantiser_round_trip():
    torch.manual_seed(0)
    # magnitudes over many binades, so that subnormal codes are hit too
    w = torch.randn(48, 256) * torch.exp2(torch.randint(-12, 3, (48, 256)))
    w[5] = 0
    w8, scale = quantize_weight_fp8(w.to(torch.bfloat16))
    w = w.to(torch.bfloat16).float()
    assert w8.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32
    assert scale[5] == 1 and bool((w8[5].float() == 0).all())
    assert float(w8.float().abs().max()) == 448
    deq = w8.float() * scale[:, None]
    assert bool(torch.isfinite(deq).all())
    # three mantissa bits: half an ulp is 2^-4 relative; the subnormal step
    # is 2^-9, half of it 2^-10, in units of the scale
    bound = 2.0 ** -4 * w.abs() + 2.0 ** -10 * scale[:, None]
    assert bool(((w - deq).abs() <= bound).all())


@pytest.mark.parametrize("bias", [False, True])
def test_cpu_path_is_the_formula(bias):
    torch.manual_seed(1)
    lin = nn.Linear(64, 24, bias=bias)
    q = Fp8Linear.from_linear(lin)
    x = torch.randn(3, 5, 64).to(torch.bfloat16)
    want = (x.float() @ q.weight_fp8.float().t()) * q.weight_scale
    if bias:
        want = want + lin.bias.float()
    with torch.no_grad():
        got = q(x)
    assert got.shape == (3, 5, 24) and got.dtype == torch.bfloat16
    assert torch.equal(got, want.to(torch.bfloat16))
    assert torch.equal(got, fp8_linear(x, q.weight_fp8, q.weight_scale,
                                       q.bias))


def test_grad_enabled_input_raises():
    q = Fp8Linear.from_linear(nn.Linear(32, 16))
    with pytest.raises(RuntimeError, match="inference-only"):
        q(torch.randn(2, 32, requires_grad=True))
    q(torch.randn(2, 32))       # grad mode on, nothing requires grad: fine


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_quantize_model_swaps_the_intended_modules(family):
    from torchacc_amd import models
    torch.manual_seed(0)
    if family == "llama":
        model = models.LlamaForCausalLM(
            models.llama_tiny(tie_word_embeddings=True))
    else:
        model = models.Qwen2ForCausalLM(
            models.qwen2_tiny(tie_word_embeddings=True))
    model.eval()
    embed = model.embed_tokens.weight.detach().clone()
    quantize_model_fp8(model)
    assert type(model.lm_head) is nn.Linear
    assert model.lm_head.weight is model.embed_tokens.weight
    left = [n for n, m in model.layers.named_modules()
            if isinstance(m, (nn.Linear, TunedLinear))]
    swapped = [n for n, m in model.layers.named_modules()
               if isinstance(m, Fp8Linear)]
    assert left == [] and len(swapped) == 7 * len(model.layers)
    has_bias = model.layers[0].self_attn.q_proj.bias is not None
    assert has_bias == (family == "qwen2")

    quantize_model_fp8(model, include_lm_head=True)   # layers: already done
    assert isinstance(model.lm_head, Fp8Linear)
    assert torch.equal(model.embed_tokens.weight, embed)

    # dtype sweeps leave codes and scales alone; state_dict round trip
    model.to(torch.bfloat16).float()
    q = model.layers[0].mlp.down_proj
    assert q.weight_fp8.dtype == torch.float8_e4m3fn
    assert q.weight_scale.dtype == torch.float32
    ids = torch.randint(0, 1024, (1, 6))
    want = model.generate(ids, max_new_tokens=4)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    for buf in q.buffers():
        buf.zero_()
    model.load_state_dict(sd)
    assert torch.equal(model.generate(ids, max_new_tokens=4), want)
