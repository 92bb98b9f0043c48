"""Weight-only fp8 linear (csrc/fp8_linear.hip) against float64, its bitwise
properties, and the quantised models through the decode stack."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

# M: every MT, partial column blocks, the second 64-row block. N: one tile, a
# predicated tail (40; 18 is not a multiple of 4: scalar stores), many
# workgroups. K: one load, a ragged K split, and 4096 (cross-workgroup split).
SHAPES = [(1, 16, 16), (1, 1024, 4096), (5, 40, 1040), (5, 18, 1040),
          (16, 1024, 1040), (17, 16, 1040), (17, 40, 4096), (33, 1024, 16),
          (64, 40, 1040), (64, 16, 4096), (65, 40, 4096), (65, 1024, 1040)]


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


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                         ids=["bf16", "fp16"])
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_fp8_linear_matches_float64(m, n, k, dtype, bias):
    # the kernel itself: above FP8_LINEAR_MAX_M ops.fp8_linear leaves it
    from torchacc_amd.ops._backend import require_extension
    x, w8, scale, b = _problem(m, n, k, dtype, bias)
    got = require_extension().fp8_linear(x.cuda(), w8.cuda(), scale.cuda(),
                                         None if b is None else b.cuda())
    assert got.dtype == dtype and got.shape == (m, n)
    wdeq = w8.double() * scale.double()[:, None]
    ref = x.double() @ wdeq.t()
    if bias:
        ref = ref + b.double()
    # output rounding (half an ulp, doubled for the fp32 scale and bias ops)
    # plus worst-case fp32 summation error K * 2^-24 at K <= 4096, any order
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -10
    bound = eps * ref.abs() + 2.0 ** -12 * (x.double().abs() @ wdeq.abs().t())
    err = (got.cpu().double() - ref).abs()
    print(f"max err/bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                         ids=["bf16", "fp16"])
def test_fp8_linear_deterministic_and_batch_invariant(dtype):
    from torchacc_amd.ops import fp8_linear
    n, k = 40, 4096           # two workgroups per split, K split engaged
    x, w8, scale, b = _problem(64, n, k, dtype, True, seed=1)
    x, w8, scale, b = x.cuda(), w8.cuda(), scale.cuda(), b.cuda()
    row = x[40:41]
    y64 = fp8_linear(x, w8, scale, b)
    assert torch.equal(y64, fp8_linear(x, w8, scale, b))
    y1 = fp8_linear(row, w8, scale, b)
    x5 = torch.cat([x[:3], row, x[7:8]])
    y5 = fp8_linear(x5, w8, scale, b)
    assert torch.equal(y1[0], y5[3])
    assert torch.equal(y1[0], y64[40])


def _models(family):
    """The same fp8-quantised tiny model as (GPU bf16, CPU fp32)."""
    from torchacc_amd import models
    from torchacc_amd.ops import quantize_model_fp8
    torch.manual_seed(0)
    if family == "llama":
        model = models.LlamaForCausalLM(models.llama_tiny())
    else:
        model = models.Qwen2ForCausalLM(models.qwen2_tiny())
    model = quantize_model_fp8(model.eval().to(torch.bfloat16),
                               include_lm_head=True)
    return copy.deepcopy(model).cuda(), model.float()


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_fp8_model_graph_decode_equals_eager(family):
    from torchacc_amd.models.generation import GraphDecoder
    gpu, _ = _models(family)
    ids = torch.randint(0, 1024, (2, 12), device="cuda")
    want = gpu.generate(ids, max_new_tokens=8)
    got = GraphDecoder(gpu, b=2, max_len=32).decode(ids, 8)
    assert torch.equal(got, want), (got[:, 12:], want[:, 12:])


# max |logit_gpu - logit_cpu| of the 16-bit (unquantised) bf16 models at this
# config and prompt on the parent commit; the fp8 models are allowed twice that
LOGIT_ERR_16BIT = {"llama": 0.007448, "qwen2": 0.005721}


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_fp8_model_decode_logits_match_cpu(family):
    """One decode step (after a 12-token prefill) of the quantised model on
    the GPU against the fp32 CPU run of the same codes and scales.
    Measured 16-bit GPU-vs-CPU error (max abs, logits up to ~1.1): llama
    0.00745, qwen2 0.00572; allowed here: twice that. Measured fp8 error:
    llama 0.00788, qwen2 0.00659."""
    from torchacc_amd.models.generation import LayerKV, _forward_step
    gpu, cpu = _models(family)
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

    err = float((decode_logits(gpu, ids.cuda()) - decode_logits(cpu, ids))
                .abs().max())
    print(f"{family}: fp8 logit err {err:.5f}")
    assert err <= 2 * LOGIT_ERR_16BIT[family]
