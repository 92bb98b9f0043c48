"""One-launch fp8 projections (fp8_wide_kernel in csrc/fp8_linear.hip): the
fused gate/up SwiGLU epilogue and the plain one against float64, their bitwise
properties, and models quantised with one_launch=True through decode."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

# (M, I, K): one tile and one load; a predicated tail and one that is no
# multiple of 4 (scalar stores), both with ragged K; MT = 2 and MT = 4; several
# steps per wave with a tail tile, and many workgroups.
SWIGLU_SHAPES = [(1, 16, 16), (5, 40, 1040), (5, 18, 1040), (17, 16, 1040),
                 (33, 688, 16), (64, 40, 4096), (1, 688, 4096)]
PLAIN_SHAPES = [(1, 16, 16), (5, 18, 1040), (17, 40, 4096), (64, 1024, 1040)]


def _problem(m, n, k, dtype, bias, seed=0):
    g = torch.Generator().manual_seed(seed)
    # uniform over every finite e4m3 code: +-448, subnormals and zeros included
    codes = torch.randint(0, 256, (n, k), generator=g, dtype=torch.int16)
    codes[(codes & 0x7F) == 0x7F] = 0x7E
    w8 = codes.to(torch.uint8).view(torch.float8_e4m3fn)
    scale = (0.5 + torch.rand(n, generator=g)) / 300.0
    x = torch.randn(m, k, generator=g).to(dtype)
    b = torch.randn(n, generator=g).to(dtype) if bias else None
    return x, w8, scale, b


def _cuda(*ts):
    return [None if t is None else t.cuda() for t in ts]


def _eps(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -10


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                         ids=["bf16", "fp16"])
@pytest.mark.parametrize("m,n,k", SWIGLU_SHAPES)
def test_fp8_swiglu_linear_matches_float64(m, n, k, dtype, bias):
    from torchacc_amd.ops import fp8_swiglu_linear
    x, wg8, sg, bg = _problem(m, n, k, dtype, bias)
    _, wu8, su, bu = _problem(m, n, k, dtype, bias, seed=1)
    got = fp8_swiglu_linear(*_cuda(x, wg8, sg, wu8, su, bg, bu))
    assert got.dtype == dtype and got.shape == (m, n)
    xd = x.double()
    wg = wg8.double() * sg.double()[:, None]
    wu = wu8.double() * su.double()[:, None]
    g, u = xd @ wg.t(), xd @ wu.t()
    if bias:
        g, u = g + bg.double(), u + bu.double()
    silu = g * torch.sigmoid(g)
    ref = silu * u
    # worst-case fp32 summation error of either product (K * 2^-24, K <= 4096)
    # pushed through silu (|silu'| <= 1.1) and the product, plus the output
    # rounding and the fp32 epilogue in eps
    eg = 2.0 ** -12 * (xd.abs() @ wg.abs().t())
    eu = 2.0 ** -12 * (xd.abs() @ wu.abs().t())
    bound = (_eps(dtype) * ref.abs() + 1.1 * eg * (u.abs() + eu)
             + silu.abs() * eu)
    err = (got.cpu().double() - ref).abs()
    print(f"max err/bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("waves,tiles", [(4, 1), (4, 2), (8, 1), (8, 2)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                         ids=["bf16", "fp16"])
@pytest.mark.parametrize("m,n,k", PLAIN_SHAPES)
def test_fp8_linear_wide_matches_float64(m, n, k, dtype, waves, tiles):
    from torchacc_amd.ops._backend import require_extension
    x, w8, scale, b = _problem(m, n, k, dtype, True)
    got = require_extension().fp8_linear_wide(*_cuda(x, w8, scale, b),
                                              waves, tiles)
    assert got.dtype == dtype and got.shape == (m, n)
    wdeq = w8.double() * scale.double()[:, None]
    ref = x.double() @ wdeq.t() + b.double()
    bound = (_eps(dtype) * ref.abs()
             + 2.0 ** -12 * (x.double().abs() @ wdeq.abs().t()))
    err = (got.cpu().double() - ref).abs()
    print(f"max err/bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("op", ["plain", "swiglu"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                         ids=["bf16", "fp16"])
def test_one_launch_deterministic_and_batch_invariant(dtype, op):
    from torchacc_amd.ops import fp8_linear, fp8_swiglu_linear
    x, w8, scale, b = _cuda(*_problem(64, 40, 4096, dtype, True, seed=1))
    _, wu8, su, bu = _cuda(*_problem(64, 40, 4096, dtype, True, seed=2))

    def f(x):
        if op == "plain":
            return fp8_linear(x, w8, scale, b, one_launch=True)
        return fp8_swiglu_linear(x, w8, scale, wu8, su, b, bu)

    row = x[40:41]
    y64 = f(x)
    assert torch.equal(y64, f(x))
    y1 = f(row)                                    # MT = 1
    y5 = f(torch.cat([x[:3], row, x[7:8]]))
    assert torch.equal(y1[0], y5[3])
    assert torch.equal(y1[0], y64[40])             # MT = 4


def _models(family, **quant_kw):
    """The same tiny model as (GPU bf16, CPU fp32): quantize_model_fp8 with
    quant_kw, or with none given the 16-bit weights."""
    from torchacc_amd import models
    from torchacc_amd.ops import quantize_model_fp8
    torch.manual_seed(0)
    if family == "llama":
        model = models.LlamaForCausalLM(models.llama_tiny())
    else:
        model = models.Qwen2ForCausalLM(models.qwen2_tiny())
    model = model.eval().to(torch.bfloat16)
    if quant_kw:
        model = quantize_model_fp8(model, **quant_kw)
    return copy.deepcopy(model).cuda(), model.float()


ONE_LAUNCH = dict(include_lm_head=True, one_launch=True)


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_one_launch_model_graph_decode_equals_eager(family):
    from torchacc_amd.models.generation import GraphDecoder
    from torchacc_amd.ops import Fp8SwiGLUMLP
    gpu, _ = _models(family, **ONE_LAUNCH)
    assert isinstance(gpu.layers[0].mlp, Fp8SwiGLUMLP)
    ids = torch.randint(0, 1024, (2, 12), device="cuda")
    want = gpu.generate(ids, max_new_tokens=8)
    got = GraphDecoder(gpu, b=2, max_len=32).decode(ids, 8)
    assert torch.equal(got, want), (got[:, 12:], want[:, 12:])


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_one_launch_model_decode_logits_match_cpu(family):
    """One decode step (after a 12-token prefill) on the GPU against the fp32
    CPU run of the same weights: the one_launch fp8 model may be off by at
    most twice what the 16-bit model is, measured here on the same prompt."""
    from torchacc_amd.models.generation import LayerKV, _forward_step
    ids = torch.randint(0, 1024, (2, 13),
                        generator=torch.Generator().manual_seed(3))

    def decode_logits(model, ids):
        p = next(model.parameters())
        caches = [LayerKV(2, 16, layer.self_attn.num_kv_heads,
                          layer.self_attn.head_dim, p.dtype, p.device)
                  for layer in model.layers]
        with torch.no_grad():
            _forward_step(model, ids[:, :-1], caches, 0)
            return _forward_step(model, ids[:, -1:], caches, 12).float().cpu()

    def gpu_vs_cpu(**quant_kw):
        gpu, cpu = _models(family, **quant_kw)
        return float((decode_logits(gpu, ids.cuda())
                      - decode_logits(cpu, ids)).abs().max())

    err16, err8 = gpu_vs_cpu(), gpu_vs_cpu(**ONE_LAUNCH)
    print(f"{family}: 16-bit logit err {err16:.5f}, one-launch fp8 {err8:.5f}")
    assert err8 <= 2 * err16
