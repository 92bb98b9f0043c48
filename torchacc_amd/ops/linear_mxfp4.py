"""Weight-only MXFP4 linear layers for decode and serving (W4A16).

A decode step is bound by reading the projection weights once. The OCP
microscaling format MXFP4 stores a weight as e2m1 elements
(+-{0, 0.5, 1, 1.5, 2, 3, 4, 6}), two per byte, with one e8m0 power-of-two
scale per 32 elements along K: a quarter of the 16-bit bytes, half of the e4m3
ones of ``linear_fp8``. Activations stay 16-bit.

Layout (what 4-bit checkpoints ship): ``codes`` uint8 [N, K/2], byte ``i`` of a
row holds element ``2i`` in bits 0..3 and ``2i+1`` in bits 4..7; ``scales``
uint8 [N, K/32], group ``g`` of row ``n`` is multiplied by
``2 ** (scales[n, g] - 127)``. No per-channel scale. ``K % 32 == 0``.

Scale bytes: 255 (NaN) is rejected, and byte 0 (2^-127, an fp32 subnormal) is
never produced by the quantiser; kernels and the CPU dequantiser alike read a
byte 0 as 2^-126. Element times scale is exact in bf16 for every byte 1..252.
In fp16 it is exact for exponents -14..12 (bytes 113..139) only: the fp16
contract is limited to weights whose scale bytes lie in that range (trained
weights of magnitude 2^-12 .. 2^14 per group); it is not checked per call.

The only approximation is the one-off rounding in ``quantize_weight_mxfp4``:
``mxfp4_linear`` computes ``x @ dequant(codes, scales)^T + bias`` with fp32
accumulation on the ``_C.mxfp4_linear`` MFMA kernel (csrc/mxfp4_linear.hip),
one launch for every (N, K), for decode-sized batches, and on the tiled
``_C.mxfp4_gemm`` kernel of the same file above them (prefill, chunked prefill
and mixed serving steps), which keeps the codes packed in LDS and converts
them after the fragment read; ``_C.mxfp4_swiglu_gemm`` is its fused gate/up
instance.

Inference only.
"""
from typing import Optional, Tuple

import torch
import torch.nn as nn

from ._backend import dispatch
from .linear import TunedLinear, tuned_linear
from .linear_fp8 import _keep_buffer_dtypes, _refuse_grad
from .swiglu import swiglu

MXFP4_GROUP = 32

# Rows up to which GPU inputs take the one-launch kernel. Above it the tiled
# mxfp4_gemm kernel runs, see MXFP4_GEMM_MAX_M.
MXFP4_LINEAR_MAX_M = 64

# Rows up to which GPU inputs above MXFP4_LINEAR_MAX_M take the tiled
# mxfp4_gemm / mxfp4_swiglu_gemm kernels (None: no limit). Above it the weight
# is dequantised in memory (mxfp4_dequantize, a 16-bit N*K transient) and the
# 16-bit GEMM runs (the only path there before mxfp4_gemm).
# Measured (profiles/r20_mxfp4_gemm.md, eight projection / LM-head shapes, time
# of mxfp4_gemm over time of the dequantise path, 16-bit spread <= 1.4% except
# one 7% row):
#   M = 128   0.30 - 0.75      M = 1024  0.94 - 1.33 (loses at seven shapes)
#   M = 256   0.53 - 1.00      M = 2048  1.09 - 1.47
#   M = 512   0.80 - 0.91      M = 4096  0.98 - 1.68
# 512 is the largest benchmarked M at which every shape wins by more than the
# spread (at M = 256 the 1024 x 4096 shape is level, inside its spread).
MXFP4_GEMM_MAX_M = 512

# value of code c (bit 3 = sign)
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0,
               -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0)

# lowest scale byte the quantiser produces (2^-126): see the module docstring
_MIN_SCALE_BYTE = 1


def _check_k(k: int, what: str) -> None:
    if k <= 0 or k % MXFP4_GROUP != 0:
        raise ValueError(
            f"{what}: in_features = {k} is not a positive multiple of "
            f"{MXFP4_GROUP} (one MXFP4 scale covers {MXFP4_GROUP} elements)")


def quantize_weight_mxfp4(w: torch.Tensor,
                          what: str = "quantize_weight_mxfp4"
                          ) -> Tuple[torch.Tensor, torch.Tensor]:
    """[N, K] weight -> (codes uint8 [N, K/2], scales uint8 [N, K/32]).

    Per group of 32: exponent ``e = clamp(floor(log2(amax)) - 2, -126, 127)``
    (so amax / 2^e is in [4, 8) and the largest element lands on 4 or 6), an
    all-zero group gets byte 127; elements are ``w / 2^e`` rounded to
    nearest-even on the e2m1 grid, saturating at +-6. Raises ``ValueError``
    when K is no multiple of 32 or the weight is not finite."""
    assert w.dim() == 2, f"{what}: [N, K] weight"
    n, k = w.shape
    _check_k(k, what)
    wf = w.detach().float().reshape(n, k // MXFP4_GROUP, MXFP4_GROUP)
    if not bool(torch.isfinite(wf).all()):
        raise ValueError(f"{what}: the weight has non-finite values; their "
                         "scale byte would be 255 (NaN)")
    amax = wf.abs().amax(dim=2)
    # frexp: amax = m * 2^ex, m in [0.5, 1), so floor(log2(amax)) = ex - 1
    e = (torch.frexp(amax)[1] - 3).clamp(_MIN_SCALE_BYTE - 127, 127)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    # w / 2^e in two exact steps: 2^e itself may lie outside fp32's normals
    half = torch.div(e, 2, rounding_mode="floor")
    v = torch.ldexp(torch.ldexp(wf, -half[..., None]), -(e - half)[..., None])
    a = v.abs().clamp(max=6.0)
    # the grid's spacing is 0.5 below 2, 1 below 4, 2 above; round() is
    # nearest-even, and an even multiple of the spacing has mantissa bit 0
    step = torch.where(a < 2, 0.5, torch.where(a < 4, 1.0, 2.0))
    q = torch.round(a / step) * step
    mag = torch.where(q < 2, q * 2, torch.where(q < 4, q + 2, q / 2 + 4))
    code = mag.to(torch.uint8) | (torch.signbit(v).to(torch.uint8) << 3)
    code = code.reshape(n, k // 2, 2)
    codes = code[..., 0] | (code[..., 1] << 4)
    return codes.contiguous(), (e + 127).to(torch.uint8).contiguous()


def dequantize_weight_mxfp4(codes: torch.Tensor, scales: torch.Tensor,
                            dtype: torch.dtype = torch.bfloat16
                            ) -> torch.Tensor:
    """(codes [N, K/2], scales [N, K/32]) -> the [N, K] weight in ``dtype``.
    Table-driven on the CPU (any float dtype); on a GPU the
    ``_C.mxfp4_dequantize`` kernel (bf16 or fp16). Exact within the ranges of
    the module docstring."""
    ext = dispatch(codes)
    if ext is not None:
        return ext.mxfp4_dequantize(codes.contiguous(), scales.contiguous(),
                                    dtype)
    n, kb = codes.shape
    table = torch.tensor(E2M1_VALUES, dtype=torch.float64)
    idx = torch.stack([codes & 0xF, codes >> 4], dim=2).reshape(n, 2 * kb)
    exp = scales.clamp(min=1).to(torch.float64) - 127
    w = table[idx.long()].reshape(n, -1, MXFP4_GROUP) * (2.0 ** exp)[..., None]
    return w.reshape(n, 2 * kb).to(dtype)


def mxfp4_linear(x: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor,
                 bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x @ dequant(codes, scales).T + bias`` in ``x.dtype``; x [..., K],
    bf16 or fp16 on a GPU (fp16: scale bytes 113..139 only, see the module
    docstring).

    On a GPU, up to ``MXFP4_LINEAR_MAX_M`` rows are one launch of the MXFP4
    kernel: the result is bitwise repeatable and a row's bits do not depend on
    the batch it sits in. Above it, up to ``MXFP4_GEMM_MAX_M`` rows run on the
    tiled ``_C.mxfp4_gemm`` kernel: bitwise repeatable, but NOT
    batch-invariant (its K split depends on the row count). Above that the
    weight is dequantised by ``_C.mxfp4_dequantize`` into a 16-bit N*K
    transient and ``tuned_linear`` runs on it."""
    _refuse_grad("mxfp4_linear", x, bias)
    _check_k(x.shape[-1], "mxfp4_linear")
    ext = dispatch(x)
    shape = x.shape
    x2d = x.reshape(-1, shape[-1])
    if ext is None:
        w = dequantize_weight_mxfp4(codes, scales, torch.float32)
        out = x2d.float() @ w.t()
        if bias is not None:
            out = out + bias.float()
        out = out.to(x.dtype)
    elif x2d.shape[0] <= MXFP4_LINEAR_MAX_M:
        out = ext.mxfp4_linear(x2d.contiguous(), codes, scales, bias)
    elif MXFP4_GEMM_MAX_M is None or x2d.shape[0] <= MXFP4_GEMM_MAX_M:
        out = ext.mxfp4_gemm(x2d.contiguous(), codes, scales, bias)
    else:
        out = tuned_linear(x2d, ext.mxfp4_dequantize(codes, scales, x.dtype),
                           bias)
    return out.view(*shape[:-1], codes.shape[0])


def mxfp4_swiglu_linear(x: torch.Tensor, gate_codes: torch.Tensor,
                        gate_scales: torch.Tensor, up_codes: torch.Tensor,
                        up_scales: torch.Tensor,
                        bias_gate: Optional[torch.Tensor] = None,
                        bias_up: Optional[torch.Tensor] = None
                        ) -> torch.Tensor:
    """``silu(mxfp4_linear(x, gate...)) * mxfp4_linear(x, up...)`` in
    ``x.dtype``; x [..., K], both weights [I, K].

    On a GPU, up to ``MXFP4_LINEAR_MAX_M`` rows are ONE launch of the fused
    kernel: gate and up pre-activations stay fp32 and never reach memory, and
    the result is bitwise repeatable and independent of the batch a row sits
    in. Above it, up to ``MXFP4_GEMM_MAX_M`` rows run on the tiled
    ``_C.mxfp4_swiglu_gemm`` kernel, which keeps both properties except batch
    invariance. Above that, two ``mxfp4_linear`` calls and ``swiglu``."""
    _refuse_grad("mxfp4_swiglu_linear", x, bias_gate, bias_up)
    _check_k(x.shape[-1], "mxfp4_swiglu_linear")
    ext = dispatch(x)
    shape = x.shape
    x2d = x.reshape(-1, shape[-1])
    if ext is None:
        xf = x2d.float()
        g = xf @ dequantize_weight_mxfp4(gate_codes, gate_scales,
                                         torch.float32).t()
        u = xf @ dequantize_weight_mxfp4(up_codes, up_scales,
                                         torch.float32).t()
        if bias_gate is not None:
            g = g + bias_gate.float()
        if bias_up is not None:
            u = u + bias_up.float()
        out = (g * torch.sigmoid(g) * u).to(x.dtype)
    elif x2d.shape[0] <= MXFP4_LINEAR_MAX_M:
        out = ext.mxfp4_swiglu_linear(x2d.contiguous(), gate_codes,
                                      gate_scales, up_codes, up_scales,
                                      bias_gate, bias_up)
    elif MXFP4_GEMM_MAX_M is None or x2d.shape[0] <= MXFP4_GEMM_MAX_M:
        out = ext.mxfp4_swiglu_gemm(x2d.contiguous(), gate_codes, gate_scales,
                                    up_codes, up_scales, bias_gate, bias_up)
    else:
        out = swiglu(mxfp4_linear(x2d, gate_codes, gate_scales, bias_gate),
                     mxfp4_linear(x2d, up_codes, up_scales, bias_up))
    return out.view(*shape[:-1], gate_codes.shape[0])


class Mxfp4Linear(nn.Module):
    """Linear layer holding MXFP4 weight codes and e8m0 group scales."""

    def __init__(self, codes: torch.Tensor, scales: torch.Tensor,
                 bias: Optional[torch.Tensor] = None):
        super().__init__()
        self.out_features, self.in_features = codes.shape[0], 2 * codes.shape[1]
        self.register_buffer("weight_codes", codes)
        self.register_buffer("weight_scales", scales)
        self.register_buffer("bias", bias)

    @classmethod
    def from_linear(cls, lin: nn.Linear,
                    what: str = "Mxfp4Linear") -> "Mxfp4Linear":
        codes, scales = quantize_weight_mxfp4(lin.weight, what)
        bias = None if lin.bias is None else lin.bias.detach().clone()
        return cls(codes, scales, bias)

    def _apply(self, fn, recurse=True):
        before = {n: getattr(self, n)
                  for n in ("weight_codes", "weight_scales")}
        super()._apply(fn, recurse)
        _keep_buffer_dtypes(self, before)
        return self

    def forward(self, x):
        return mxfp4_linear(x, self.weight_codes, self.weight_scales,
                            self.bias)

    def extra_repr(self):
        return (f"in_features={self.in_features}, "
                f"out_features={self.out_features}, "
                f"bias={self.bias is not None}")


class Mxfp4SwiGLUMLP(nn.Module):
    """SwiGLU MLP on MXFP4 weights: gate and up projections and the activation
    are one fused launch (``mxfp4_swiglu_linear``), then an ``Mxfp4Linear``
    down projection."""

    _UINT8_BUFFERS = ("gate_codes", "gate_scales", "up_codes", "up_scales")

    def __init__(self, gate: Mxfp4Linear, up: Mxfp4Linear, down: Mxfp4Linear):
        super().__init__()
        assert gate.weight_codes.shape == up.weight_codes.shape
        self.register_buffer("gate_codes", gate.weight_codes)
        self.register_buffer("gate_scales", gate.weight_scales)
        self.register_buffer("gate_bias", gate.bias)
        self.register_buffer("up_codes", up.weight_codes)
        self.register_buffer("up_scales", up.weight_scales)
        self.register_buffer("up_bias", up.bias)
        self.down_proj = down

    @classmethod
    def from_mlp(cls, mlp: nn.Module, what: str = "mlp") -> "Mxfp4SwiGLUMLP":
        """From any module with gate_proj / up_proj / down_proj linears
        (``nn.Linear``, ``TunedLinear`` or already ``Mxfp4Linear``)."""
        def q(name):
            lin = getattr(mlp, name)
            if isinstance(lin, Mxfp4Linear):
                return lin
            return Mxfp4Linear.from_linear(lin, f"{what}.{name}")
        return cls(q("gate_proj"), q("up_proj"), q("down_proj"))

    def _apply(self, fn, recurse=True):
        before = {n: getattr(self, n) for n in self._UINT8_BUFFERS}
        super()._apply(fn, recurse)
        _keep_buffer_dtypes(self, before)
        return self

    def forward(self, x):
        return self.down_proj(mxfp4_swiglu_linear(
            x, self.gate_codes, self.gate_scales, self.up_codes,
            self.up_scales, self.gate_bias, self.up_bias))


def _is_swiglu_mlp(mod: nn.Module) -> bool:
    return all(type(getattr(mod, n, None)) in (nn.Linear, TunedLinear,
                                               Mxfp4Linear)
               for n in ("gate_proj", "up_proj", "down_proj"))


def _swap_linears(parent: nn.Module, prefix: str) -> None:
    for name, child in parent.named_children():
        path = f"{prefix}.{name}"
        if type(child) in (nn.Linear, TunedLinear):
            setattr(parent, name, Mxfp4Linear.from_linear(
                child, f"quantize_model_mxfp4: {path}"))
        elif name == "mlp" and _is_swiglu_mlp(child):
            setattr(parent, name, Mxfp4SwiGLUMLP.from_mlp(
                child, f"quantize_model_mxfp4: {path}"))
        elif isinstance(child, (Mxfp4Linear, Mxfp4SwiGLUMLP)):
            continue
        elif hasattr(child, "tp") and hasattr(child, "group") \
                and hasattr(child, "weight"):
            raise NotImplementedError(
                f"quantize_model_mxfp4: '{path}' is tensor-parallel sharded; "
                "MXFP4 weights for TP layers are not supported. Quantise the "
                "unsharded model (and serve it on one device) instead.")
        else:
            _swap_linears(child, path)


def _check_linears(parent: nn.Module, prefix: str) -> None:
    for name, child in parent.named_modules():
        if type(child) in (nn.Linear, TunedLinear):
            _check_k(child.in_features,
                     f"quantize_model_mxfp4: {prefix}.{name}")


def quantize_model_mxfp4(model: nn.Module, include_lm_head: bool = False):
    """Swap, in place, every ``nn.Linear`` / ``TunedLinear`` inside
    ``model.layers`` for an ``Mxfp4Linear``, and each ``mlp`` child made of
    gate_proj / up_proj / down_proj linears for an ``Mxfp4SwiGLUMLP`` (fused
    gate/up/activation); with ``include_lm_head`` also ``model.lm_head`` (a
    tied head gets its own MXFP4 copy; the embedding table is left as it is).
    Returns the model.

    Raises ``ValueError`` naming the layer, before anything is swapped, when
    a layer's ``in_features`` is no multiple of 32."""
    if getattr(model, "_tp_group", None) is not None:
        raise NotImplementedError(
            "quantize_model_mxfp4: the model is tensor-parallel sharded; "
            "MXFP4 weights for TP layers are not supported. Quantise the "
            "unsharded model instead.")
    _check_linears(model.layers, "layers")
    if include_lm_head:
        head = model.lm_head
        if type(head) not in (nn.Linear, TunedLinear):
            raise NotImplementedError(
                f"quantize_model_mxfp4: lm_head is a {type(head).__name__}, "
                "expected an unsharded nn.Linear")
        _check_k(head.in_features, "quantize_model_mxfp4: lm_head")
    _swap_linears(model.layers, "layers")
    if not any(isinstance(m, Mxfp4Linear) for m in model.layers.modules()):
        raise ValueError("quantize_model_mxfp4: no linear layer found under "
                         "model.layers")
    if include_lm_head:
        model.lm_head = Mxfp4Linear.from_linear(
            model.lm_head, "quantize_model_mxfp4: lm_head")
    return model
