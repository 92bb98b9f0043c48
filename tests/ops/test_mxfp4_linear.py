"""MXFP4 weight-only linear kernels (csrc/mxfp4_linear.hip) against float64:
the plain and the fused gate/up SwiGLU epilogue, their bitwise properties, the
dequantise kernel, and models quantised with quantize_model_mxfp4 through
decode."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

E2M1 = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6,
                     -0., -.5, -1, -1.5, -2, -3, -4, -6], dtype=torch.float64)

# (M, N, K): one group and one tile; many workgroups; ragged last step with a
# channel tail, and with N % 4 != 0 (scalar stores); MT = 2; fewer steps than
# waves at MT = 4; MT = 4 with several steps per wave, and with a ragged one;
# one full step over many workgroups; long K.
SHAPES = [(1, 16, 32), (1, 1024, 4096), (5, 40, 1056), (5, 18, 1056),
          (17, 16, 288), (33, 1024, 32), (64, 40, 4096), (64, 16, 1056),
          (16, 4096, 256), (16, 64, 11008)]
SWIGLU_SHAPES = [(1, 16, 32), (5, 18, 1056), (17, 16, 288), (64, 40, 4096)]
FORCED = (5, 40, 1056)      # ragged K, channel tail, two steps on the last wave
INSTANCES = [(4, 1), (8, 1), (4, 2), (8, 2), (4, 4)]
SWIGLU_INSTANCES = [(4, 2), (8, 2), (4, 4)]


def _problem(m, n, k, dtype, bias, seed=0, lo=117, hi=129):
    """codes uniform over all 256 bytes, scale bytes uniform in lo..hi."""
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 256, (n, k // 2), generator=g, dtype=torch.uint8)
    scales = torch.randint(lo, hi + 1, (n, k // 32), generator=g,
                           dtype=torch.uint8)
    x = torch.randn(m, k, generator=g).to(dtype)
    b = torch.randn(n, generator=g).to(dtype) if bias else None
    return x, codes, scales, b


def _deq(codes, scales):
    """float64 [N, K] from the 16-entry table; byte 0 reads as 2^-126."""
    n, kb = codes.shape
    idx = torch.stack([codes & 0xF, codes >> 4], dim=2).long()
    sc = 2.0 ** (scales.clamp(min=1).double() - 127)
    return (E2M1[idx].reshape(n, -1, 32) * sc[..., None]).reshape(n, 2 * kb)


def _cuda(*ts):
    return [None if t is None else t.cuda() for t in ts]


def _eps(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -10


def _check_plain(m, n, k, dtype, bias, waves=0, tiles=0, **kw):
    from torchacc_amd.ops._backend import require_extension
    x, codes, scales, b = _problem(m, n, k, dtype, bias, **kw)
    got = require_extension().mxfp4_linear(*_cuda(x, codes, scales, b),
                                           waves, tiles)
    assert got.dtype == dtype and got.shape == (m, n)
    deq = _deq(codes, scales)
    ref = x.double() @ deq.t()
    if bias:
        ref = ref + b.double()
    # half an ulp of output rounding, doubled for the bias add, plus
    # worst-case fp32 summation of K terms in any order
    bound = (_eps(dtype) * ref.abs()
             + k * 2.0 ** -24 * (x.double().abs() @ deq.abs().t()))
    err = (got.cpu().double() - ref).abs()
    print(f"max err/bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                         ids=["bf16", "fp16"])
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_mxfp4_linear_matches_float64(m, n, k, dtype, bias):
    _check_plain(m, n, k, dtype, bias)


@pytest.mark.parametrize("waves,tiles", INSTANCES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                         ids=["bf16", "fp16"])
def test_mxfp4_linear_every_instance(dtype, waves, tiles):
    _check_plain(*FORCED, dtype, True, waves, tiles)


def test_mxfp4_linear_lowest_scale_bytes_bf16():
    """Scale bytes 0..129: 1 (2^-126) is the lowest allowed, and 0 reads as 1."""
    _check_plain(*FORCED, torch.bfloat16, True, seed=3, lo=0, hi=129)


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                         ids=["bf16", "fp16"])
@pytest.mark.parametrize(
    "m,n,k,waves,tiles",
    [s + (0, 0) for s in SWIGLU_SHAPES] + [FORCED + i for i in SWIGLU_INSTANCES])
def test_mxfp4_swiglu_linear_matches_float64(m, n, k, waves, tiles, dtype,
                                             bias):
    from torchacc_amd.ops._backend import require_extension
    # scale bytes 2^-6 .. 2^-2: the PRODUCT of two pre-activations has to stay
    # finite in fp16 at K = 4096 and clear of fp16's subnormals (whose rounding
    # error is absolute, not eps * |ref|) at K = 32
    x, cg, sg, bg = _problem(m, n, k, dtype, bias, lo=121, hi=125)
    _, cu, su, bu = _problem(m, n, k, dtype, bias, seed=1, lo=121, hi=125)
    got = require_extension().mxfp4_swiglu_linear(
        *_cuda(x, cg, sg, cu, su, bg, bu), waves, tiles)
    assert got.dtype == dtype and got.shape == (m, n)
    xd, wg, wu = x.double(), _deq(cg, sg), _deq(cu, su)
    g, u = xd @ wg.t(), xd @ wu.t()
    if bias:
        g, u = g + bg.double(), u + bu.double()
    silu = g * torch.sigmoid(g)
    ref = silu * u
    # worst-case fp32 summation error of either product (K * 2^-24) pushed
    # through silu (|silu'| <= 1.1) and the product, plus the output rounding
    # and the fp32 epilogue in eps. The dequantised weights are exact, so
    # there is no scale term.
    eg = k * 2.0 ** -24 * (xd.abs() @ wg.abs().t())
    eu = k * 2.0 ** -24 * (xd.abs() @ wu.abs().t())
    bound = (_eps(dtype) * ref.abs() + 1.1 * eg * (u.abs() + eu)
             + silu.abs() * eu)
    err = (got.cpu().double() - ref).abs()
    print(f"max err/bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("op", ["plain", "swiglu"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                         ids=["bf16", "fp16"])
def test_mxfp4_deterministic_and_batch_invariant(dtype, op):
    from torchacc_amd.ops import mxfp4_linear, mxfp4_swiglu_linear
    x, cg, sg, bg = _cuda(*_problem(64, 40, 4096, dtype, True, seed=1, hi=125))
    _, cu, su, bu = _cuda(*_problem(64, 40, 4096, dtype, True, seed=2, hi=125))

    def f(x):
        if op == "plain":
            return mxfp4_linear(x, cg, sg, bg)
        return mxfp4_swiglu_linear(x, cg, sg, cu, su, bg, bu)

    row = x[40:41]
    y64 = f(x)
    assert torch.equal(y64, f(x))
    y1 = f(row)                                    # MT = 1
    y5 = f(torch.cat([x[:3], row, x[7:8]]))
    assert torch.equal(y1[0], y5[3])
    assert torch.equal(y1[0], y64[40])             # MT = 4


@pytest.mark.parametrize("dtype,lo,hi", [(torch.bfloat16, 0, 252),
                                         (torch.float16, 113, 139)],
                         ids=["bf16", "fp16"])
def test_mxfp4_dequantize_equals_cpu_table(dtype, lo, hi):
    """Exact conversion over each dtype's whole contract range of scale bytes
    (byte 0 reads as 1), so GPU and CPU must agree bit for bit."""
    from torchacc_amd.ops import dequantize_weight_mxfp4
    _, codes, scales, _ = _problem(1, 37, 1056, dtype, False, lo=lo, hi=hi)
    want = dequantize_weight_mxfp4(codes, scales, dtype)
    assert torch.equal(want.double(), _deq(codes, scales))     # exact in dtype
    got = dequantize_weight_mxfp4(codes.cuda(), scales.cuda(), dtype)
    assert got.dtype == dtype
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


def _models(family):
    """The same tiny model, its linear weights snapped to MXFP4 values, as
    (quantised GPU bf16, quantised CPU fp32, 16-bit GPU bf16, 16-bit CPU
    fp32). The snapped weights are exact in bf16 and re-quantise to
    themselves, so all four hold the same weight values."""
    from torchacc_amd import models
    from torchacc_amd.models.qwen2 import Qwen2Config
    from torchacc_amd.ops import (dequantize_weight_mxfp4,
                                  quantize_model_mxfp4, quantize_weight_mxfp4)
    from torchacc_amd.ops.linear import TunedLinear
    torch.manual_seed(0)
    if family == "llama":
        model = models.LlamaForCausalLM(
            models.llama_tiny(intermediate_size=704))
    else:
        model = models.Qwen2ForCausalLM(Qwen2Config(
            vocab_size=1024, hidden_size=256, intermediate_size=704,
            num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2,
            max_position_embeddings=512))
    model = model.eval().to(torch.bfloat16)
    for mod in list(model.layers.modules()) + [model.lm_head]:
        if type(mod) in (torch.nn.Linear, TunedLinear):
            mod.weight.data.copy_(dequantize_weight_mxfp4(
                *quantize_weight_mxfp4(mod.weight), torch.bfloat16))
    quant = quantize_model_mxfp4(copy.deepcopy(model), include_lm_head=True)
    return (copy.deepcopy(quant).cuda(), quant.float(),
            copy.deepcopy(model).cuda(), model.float())


@pytest.fixture(scope="module", params=["llama", "qwen2"])
def family_models(request):
    return request.param, _models(request.param)


def test_mxfp4_model_graph_decode_equals_eager(family_models):
    from torchacc_amd.models.generation import GraphDecoder
    from torchacc_amd.ops import Mxfp4Linear, Mxfp4SwiGLUMLP
    gpu = family_models[1][0]
    assert isinstance(gpu.layers[0].mlp, Mxfp4SwiGLUMLP)
    assert isinstance(gpu.lm_head, Mxfp4Linear)
    ids = torch.randint(0, 1024, (2, 12), device="cuda")
    want = gpu.generate(ids, max_new_tokens=8)
    got = GraphDecoder(gpu, b=2, max_len=32).decode(ids, 8)
    assert torch.equal(got, want), (got[:, 12:], want[:, 12:])


def test_mxfp4_model_decode_logits_match_cpu(family_models):
    """One decode step (after a 12-token prefill) on the GPU in bf16 against
    the fp32 CPU run of the same codes and scales: the MXFP4 model may be off
    by at most twice what plain 16-bit linears holding the same (dequantised)
    weights are, measured here on the same prompt."""
    from torchacc_amd.models.generation import LayerKV, _forward_step
    family, (q_gpu, q_cpu, w_gpu, w_cpu) = family_models
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

    def gpu_vs_cpu(gpu, cpu):
        return float((decode_logits(gpu, ids.cuda())
                      - decode_logits(cpu, ids)).abs().max())

    err16, err4 = gpu_vs_cpu(w_gpu, w_cpu), gpu_vs_cpu(q_gpu, q_cpu)
    print(f"{family}: 16-bit logit err {err16:.5f}, mxfp4 {err4:.5f}")
    assert err4 <= 2 * err16
