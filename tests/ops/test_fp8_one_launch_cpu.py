"""fp8_swiglu_linear, Fp8SwiGLUMLP and quantize_model_fp8(one_launch=True) on
the CPU."""
import pytest
import torch
import torch.nn as nn

from torchacc_amd.ops import (Fp8Linear, Fp8SwiGLUMLP, fp8_swiglu_linear,
                              quantize_model_fp8, quantize_weight_fp8)


@pytest.mark.parametrize("bias", [False, True])
def test_cpu_path_is_the_formula(bias):
    torch.manual_seed(1)
    wg8, sg = quantize_weight_fp8(torch.randn(24, 64))
    wu8, su = quantize_weight_fp8(torch.randn(24, 64))
    bg, bu = (torch.randn(2, 24).to(torch.bfloat16) if bias else (None, None))
    x = torch.randn(3, 5, 64).to(torch.bfloat16)
    got = fp8_swiglu_linear(x, wg8, sg, wu8, su, bg, bu)
    assert got.shape == (3, 5, 24) and got.dtype == torch.bfloat16
    g = x.double() @ (wg8.double() * sg.double()[:, None]).t()
    u = x.double() @ (wu8.double() * su.double()[:, None]).t()
    if bias:
        g, u = g + bg.double(), u + bu.double()
    ref = g * torch.sigmoid(g) * u
    # bf16 output rounding (2^-9) with room for the fp32 arithmetic, plus the
    # fp32 error of g and u (K = 64 terms of size <= amax) pushed through
    amax = max(float(g.abs().max()), float(u.abs().max()), 1.0)
    bound = 2.0 ** -8 * ref.abs() + 64 * 2.0 ** -23 * amax * amax
    assert bool(((got.double() - ref).abs() <= bound).all())


def test_grad_enabled_input_raises():
    wg8, sg = quantize_weight_fp8(torch.randn(16, 32))
    with pytest.raises(RuntimeError, match="inference-only"):
        fp8_swiglu_linear(torch.randn(2, 32, requires_grad=True),
                          wg8, sg, wg8, sg)
    fp8_swiglu_linear(torch.randn(2, 32), wg8, sg, wg8, sg)


def _tree(model):
    return [(n, type(m).__name__) for n, m in model.named_modules()]


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_one_launch_swaps_the_mlp_and_the_default_does_not(family):
    from torchacc_amd import models
    cls, cfg = ((models.LlamaForCausalLM, models.llama_tiny)
                if family == "llama"
                else (models.Qwen2ForCausalLM, models.qwen2_tiny))

    def fresh():
        torch.manual_seed(0)
        return cls(cfg()).eval()

    plain = quantize_model_fp8(fresh())
    assert not any(isinstance(m, Fp8SwiGLUMLP) for m in plain.modules())
    lins = [m for m in plain.layers.modules() if isinstance(m, Fp8Linear)]
    assert len(lins) == 7 * len(plain.layers)
    assert not any(m.one_launch for m in lins)
    assert _tree(plain) == _tree(quantize_model_fp8(fresh(),
                                                    one_launch=False))

    model = quantize_model_fp8(fresh(), one_launch=True)
    for layer in model.layers:
        assert isinstance(layer.mlp, Fp8SwiGLUMLP)
    lins = [m for m in model.layers.modules() if isinstance(m, Fp8Linear)]
    assert len(lins) == 5 * len(model.layers)       # q, k, v, o, down
    assert all(m.one_launch for m in lins)
    # same codes, same CPU formula up to the 16-bit rounding of gate and up
    ids = torch.randint(0, 1024, (1, 6))
    with torch.no_grad():
        x = torch.randn(2, 3, model.layers[0].mlp.gate_fp8.shape[1])
        assert torch.allclose(model.layers[0].mlp(x), plain.layers[0].mlp(x),
                              rtol=1e-4, atol=1e-5)

    # dtype sweeps leave codes and scales alone; state_dict round trip
    model.to(torch.bfloat16).float()
    mlp = model.layers[0].mlp
    assert mlp.gate_fp8.dtype == mlp.up_fp8.dtype == torch.float8_e4m3fn
    assert mlp.gate_scale.dtype == mlp.up_scale.dtype == torch.float32
    want = model.generate(ids, max_new_tokens=4)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    for buf in mlp.buffers():
        buf.zero_()
    model.load_state_dict(sd)
    assert torch.equal(model.generate(ids, max_new_tokens=4), want)


def test_from_mlp_takes_plain_linears():
    class MLP(nn.Module):
        def __init__(self):
            super().__init__()
            self.gate_proj = nn.Linear(32, 48, bias=True)
            self.up_proj = nn.Linear(32, 48, bias=True)
            self.down_proj = nn.Linear(48, 32, bias=False)

    torch.manual_seed(2)
    q = Fp8SwiGLUMLP.from_mlp(MLP())
    assert q.gate_bias is not None and q.down_proj.one_launch
    with torch.no_grad():
        assert q(torch.randn(4, 32)).shape == (4, 32)
