"""Tiled MXFP4-weight GEMM (mxfp4_gemm / mxfp4_swiglu_gemm in
csrc/mxfp4_linear.hip, M > 64) against float64, its forced K splits, the
routing of ops.mxfp4_linear / mxfp4_swiglu_linear by row count, and model
prefills that run on it."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

E2M1 = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6,
                     -0., -.5, -1, -1.5, -2, -3, -4, -6], dtype=torch.float64)

# (M, N, K), tiles of 128 x 128, BK = 64, three stage buffers: one partial
# tile whose ragged step is the only step; exactly one tile and one step;
# partial second tiles on both axes, two steps and a ragged one; N % 4 != 0
# (scalar stores), 33 scale bytes per row (unaligned rows), 16 steps and a
# ragged one, every stage buffer wraps; three row tiles, three steps;
# automatic split-K; split-K with partial tiles; M below one MFMA tile.
SHAPES = [(65, 16, 32), (128, 128, 64), (129, 136, 160), (70, 18, 1056),
          (257, 40, 192), (128, 1024, 4096), (200, 264, 4096), (1, 128, 128)]
# (M, I, K, num_splits): 0 = automatic
SWIGLU_CASES = [(65, 16, 32, 0), (70, 18, 1056, 0), (129, 72, 4096, 0),
                (129, 72, 4096, 1), (129, 72, 4096, 4)]


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


def _check_plain(got, x, codes, scales, b):
    """The skinny kernel's bound: half an ulp of output rounding, doubled for
    the bias add, plus worst-case fp32 summation of K terms in any order. The
    conversion is exact, so there is no scale term."""
    k = x.shape[1]
    assert got.dtype == x.dtype and got.shape == (x.shape[0], codes.shape[0])
    deq = _deq(codes, scales)
    ref = x.double() @ deq.t()
    if b is not None:
        ref = ref + b.double()
    bound = (_eps(x.dtype) * ref.abs()
             + k * 2.0 ** -24 * (x.double().abs() @ deq.abs().t()))
    err = (got.cpu().double() - ref).abs()
    print(f"max err/bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                         ids=["bf16", "fp16"])
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_mxfp4_gemm_matches_float64(m, n, k, dtype, bias):
    from torchacc_amd.ops._backend import require_extension
    x, codes, scales, b = _problem(m, n, k, dtype, bias)
    got = require_extension().mxfp4_gemm(*_cuda(x, codes, scales, b))
    _check_plain(got, x, codes, scales, b)


@pytest.mark.parametrize("num_splits", [1, 2, 4, 16])
def test_mxfp4_gemm_forced_splits(num_splits):
    """K = 1056 is 16 whole BK steps and a ragged one: 16 is the largest
    split count the entry accepts, one whole step each."""
    from torchacc_amd.ops._backend import require_extension
    ext = require_extension()
    x, codes, scales, b = _problem(129, 136, 1056, torch.bfloat16, True,
                                   seed=2)
    args = _cuda(x, codes, scales, b)
    got = ext.mxfp4_gemm(*args, num_splits)
    _check_plain(got, x, codes, scales, b)
    assert torch.equal(got, ext.mxfp4_gemm(*args, num_splits))


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                         ids=["bf16", "fp16"])
@pytest.mark.parametrize("m,n,k,num_splits", SWIGLU_CASES)
def test_mxfp4_swiglu_gemm_matches_float64(m, n, k, num_splits, dtype, bias):
    from torchacc_amd.ops._backend import require_extension
    # scale bytes 2^-6 .. 2^-2: the PRODUCT of two pre-activations has to stay
    # finite in fp16 at K = 4096 and clear of fp16's subnormals at K = 32
    x, cg, sg, bg = _problem(m, n, k, dtype, bias, lo=121, hi=125)
    _, cu, su, bu = _problem(m, n, k, dtype, bias, seed=1, lo=121, hi=125)
    got = require_extension().mxfp4_swiglu_gemm(
        *_cuda(x, cg, sg, cu, su, bg, bu), num_splits)
    assert got.dtype == dtype and got.shape == (m, n)
    xd, wg, wu = x.double(), _deq(cg, sg), _deq(cu, su)
    g, u = xd @ wg.t(), xd @ wu.t()
    if bias:
        g, u = g + bg.double(), u + bu.double()
    silu = g * torch.sigmoid(g)
    ref = silu * u
    # worst-case fp32 summation error of either product (K * 2^-24) pushed
    # through silu (|silu'| <= 1.1) and the product, plus the output rounding
    # and the fp32 epilogue in eps
    eg = k * 2.0 ** -24 * (xd.abs() @ wg.abs().t())
    eu = k * 2.0 ** -24 * (xd.abs() @ wu.abs().t())
    bound = (_eps(dtype) * ref.abs() + 1.1 * eg * (u.abs() + eu)
             + silu.abs() * eu)
    err = (got.cpu().double() - ref).abs()
    print(f"max err/bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


def test_mxfp4_linear_routes_by_rows():
    from torchacc_amd.ops import mxfp4_linear, mxfp4_swiglu_linear
    from torchacc_amd.ops._backend import require_extension
    ext = require_extension()
    x, cg, sg, bg = _cuda(*_problem(80, 136, 1056, torch.bfloat16, True,
                                    lo=121, hi=125))
    _, cu, su, bu = _cuda(*_problem(80, 136, 1056, torch.bfloat16, True,
                                    seed=1, lo=121, hi=125))
    x3, x64 = x.view(2, 40, -1), x[:64]
    assert torch.equal(mxfp4_linear(x3, cg, sg, bg),
                       ext.mxfp4_gemm(x, cg, sg, bg).view(2, 40, -1))
    assert torch.equal(
        mxfp4_swiglu_linear(x3, cg, sg, cu, su, bg, bu),
        ext.mxfp4_swiglu_gemm(x, cg, sg, cu, su, bg, bu).view(2, 40, -1))
    assert torch.equal(mxfp4_linear(x64.view(2, 32, -1), cg, sg, bg),
                       ext.mxfp4_linear(x64, cg, sg, bg).view(2, 32, -1))
    assert torch.equal(
        mxfp4_swiglu_linear(x64.view(2, 32, -1), cg, sg, cu, su, bg, bu),
        ext.mxfp4_swiglu_linear(x64, cg, sg, cu, su, bg, bu).view(2, 32, -1))


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


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_mxfp4_model_prefill_logits_match_cpu(family):
    """An 80-row prefill (ids [2, 40]) on the GPU in bf16, where every
    projection, the fused gate/up call and the LM head take the tiled kernel,
    against the fp32 CPU run of the same codes and scales: the MXFP4 model may
    be off by at most twice what plain 16-bit linears holding the same
    (dequantised) weights are, measured here on the same prompt."""
    from torchacc_amd.models.generation import LayerKV, _forward_step
    q_gpu, q_cpu, w_gpu, w_cpu = _models(family)
    ids = torch.randint(0, 1024, (2, 40),
                        generator=torch.Generator().manual_seed(3))

    def prefill_logits(model, ids):
        p = next(model.parameters())
        caches = [LayerKV(2, 48, layer.self_attn.num_kv_heads,
                          layer.self_attn.head_dim, p.dtype, p.device)
                  for layer in model.layers]
        with torch.no_grad():
            return _forward_step(model, ids, caches, 0).float().cpu()

    def gpu_vs_cpu(gpu, cpu):
        return float((prefill_logits(gpu, ids.cuda())
                      - prefill_logits(cpu, ids)).abs().max())

    err16, err4 = gpu_vs_cpu(w_gpu, w_cpu), gpu_vs_cpu(q_gpu, q_cpu)
    print(f"{family}: 16-bit logit err {err16:.5f}, mxfp4 {err4:.5f}")
    assert err4 <= 2 * err16
