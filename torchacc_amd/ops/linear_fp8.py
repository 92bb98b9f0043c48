"""Weight-only fp8 (e4m3) linear layers for decode and serving (W8A16).

A decode step is bound by reading the projection weights once. Storing them
as e4m3 codes with one fp32 scale per output channel halves those bytes (and
the weight memory that competes with KV pages); activations stay 16-bit. The
only approximation is the one-off weight rounding in
``quantize_weight_fp8``: ``fp8_linear`` computes
``(x @ codes^T) * scale + bias`` with fp32 accumulation, on the
``_C.fp8_linear`` MFMA kernel (csrc/fp8_linear.hip) for decode-sized batches
and on the tiled ``_C.fp8_gemm`` kernel of the same file above them (prefill,
mixed serving steps): through ``FP8_GEMM_MAX_M`` rows the weight is never
dequantised in memory on a GPU.

Inference only.
"""
from typing import Optional, Tuple

import torch
import torch.nn as nn

from ._backend import dispatch
from .linear import TunedLinear, tuned_linear

E4M3_MAX = 448.0

# Rows up to which GPU inputs take the skinny fp8 kernel; above it (prefill,
# compute-bound) the tiled fp8_gemm kernel runs, see FP8_GEMM_MAX_M.
# Measured (profiles/r15_fp8_linear.md): against the 16-bit GEMM on resident
# 16-bit weights the kernel wins through M = 16 at every projection shape,
# at M = 32 except the 11008/14336 x 4096 shapes (1.2x), and is 1.04-1.73x
# slower at M = 64. The
# alternative here also has to dequantise N*K weights per call (not timed),
# so the kernel keeps M <= 64.
FP8_LINEAR_MAX_M = 64

# Rows up to which GPU inputs above FP8_LINEAR_MAX_M take the tiled fp8_gemm
# kernel; None = no upper limit. Beyond it the weight is dequantised in
# memory and the 16-bit GEMM runs (the only path there before fp8_gemm).
# Measured (profiles/r16_fp8_gemm.md, eight projection / LM-head shapes, time
# of fp8_gemm over time of the dequantise path, run-to-run spread <= 3%):
# M = 128: 0.07-0.42, 256: 0.13-0.54, 512: 0.23-0.48, 1024: 0.41-0.54,
# 2048: 0.56-0.74, 4096: 0.75-1.07 (slower at 128256 x 4096 and 1024 x 4096,
# level at 32000 x 4096). 2048 is the largest benchmarked M at which the
# kernel wins at every shape. The dequantise path also allocates two fp32
# N*K transients per call (4008 MiB for the 128256 x 4096 head).
FP8_GEMM_MAX_M = 2048


def quantize_weight_fp8(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[N, K] weight -> (e4m3 codes [N, K], fp32 scale [N]) with
    ``w ~= codes.float() * scale[:, None]``; all-zero rows get scale 1."""
    assert w.dim() == 2, "quantize_weight_fp8: [N, K] weight"
    wf = w.detach().float()
    absmax = wf.abs().amax(dim=1)
    scale = torch.where(absmax > 0, absmax / E4M3_MAX,
                        torch.ones_like(absmax))
    w8 = (wf / scale[:, None]).clamp(-E4M3_MAX, E4M3_MAX) \
        .to(torch.float8_e4m3fn)
    return w8.contiguous(), scale.contiguous()


def fp8_linear(x: torch.Tensor, w8: torch.Tensor, scale: torch.Tensor,
               bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``(x @ w8.float().T) * scale + bias`` in ``x.dtype``; x [..., K].

    On a GPU the result is bitwise repeatable. Up to ``FP8_LINEAR_MAX_M`` rows
    a row's bits also do not depend on the batch it sits in; above it (the
    tiled kernel, whose K split depends on M) that is not promised."""
    if torch.is_grad_enabled() and any(
            t is not None and t.requires_grad for t in (x, scale, bias)):
        raise RuntimeError(
            "fp8_linear is inference-only: call it under torch.no_grad() "
            "or detach its inputs")
    ext = dispatch(x)
    shape = x.shape
    x2d = x.reshape(-1, shape[-1])
    if ext is None:
        out = (x2d.float() @ w8.float().t()) * scale
        if bias is not None:
            out = out + bias.float()
        out = out.to(x.dtype)
    elif x2d.shape[0] <= FP8_LINEAR_MAX_M:
        out = ext.fp8_linear(x2d.contiguous(), w8, scale, bias)
    elif FP8_GEMM_MAX_M is None or x2d.shape[0] <= FP8_GEMM_MAX_M:
        out = ext.fp8_gemm(x2d.contiguous(), w8, scale, bias)
    else:
        w = (w8.float() * scale[:, None]).to(x.dtype)
        out = tuned_linear(x2d, w, bias)
    return out.view(*shape[:-1], w8.shape[0])


class Fp8Linear(nn.Module):
    """Linear layer holding e4m3 weight codes and per-channel fp32 scales."""

    def __init__(self, w8: torch.Tensor, scale: torch.Tensor,
                 bias: Optional[torch.Tensor] = None):
        super().__init__()
        self.out_features, self.in_features = w8.shape
        self.register_buffer("weight_fp8", w8)
        self.register_buffer("weight_scale", scale)
        self.register_buffer("bias", bias)

    @classmethod
    def from_linear(cls, lin: nn.Linear) -> "Fp8Linear":
        w8, scale = quantize_weight_fp8(lin.weight)
        bias = None if lin.bias is None else lin.bias.detach().clone()
        return cls(w8, scale, bias)

    def _apply(self, fn, recurse=True):
        w8, scale = self.weight_fp8, self.weight_scale
        super()._apply(fn, recurse)
        # a dtype sweep (.to(bfloat16), .half()) is meant for the bias: the
        # codes and their fp32 scales move device but keep their types
        if self.weight_fp8.dtype != w8.dtype:
            self.weight_fp8 = w8.to(self.weight_fp8.device)
        if self.weight_scale.dtype != scale.dtype:
            self.weight_scale = scale.to(self.weight_scale.device)
        return self

    def forward(self, x):
        return fp8_linear(x, self.weight_fp8, self.weight_scale, self.bias)

    def extra_repr(self):
        return (f"in_features={self.in_features}, "
                f"out_features={self.out_features}, "
                f"bias={self.bias is not None}")


def _swap_linears(parent: nn.Module) -> None:
    for name, child in parent.named_children():
        if type(child) in (nn.Linear, TunedLinear):
            setattr(parent, name, Fp8Linear.from_linear(child))
        elif isinstance(child, Fp8Linear):
            continue
        elif hasattr(child, "tp") and hasattr(child, "group") \
                and hasattr(child, "weight"):
            raise NotImplementedError(
                f"quantize_model_fp8: '{name}' is tensor-parallel sharded; "
                "fp8 weights for TP layers are not supported. Quantise the "
                "unsharded model (and serve it on one device) instead.")
        else:
            _swap_linears(child)


def quantize_model_fp8(model: nn.Module, include_lm_head: bool = False):
    """Swap, in place, every ``nn.Linear`` / ``TunedLinear`` inside
    ``model.layers`` for an ``Fp8Linear``; with ``include_lm_head`` also
    ``model.lm_head`` (a tied head gets its own fp8 copy; the embedding table
    is left as it is). Returns the model."""
    if getattr(model, "_tp_group", None) is not None:
        raise NotImplementedError(
            "quantize_model_fp8: the model is tensor-parallel sharded; fp8 "
            "weights for TP layers are not supported. Quantise the "
            "unsharded model instead.")
    _swap_linears(model.layers)
    if not any(isinstance(m, Fp8Linear) for m in model.layers.modules()):
        raise ValueError("quantize_model_fp8: no linear layer found under "
                         "model.layers")
    if include_lm_head:
        head = model.lm_head
        if type(head) not in (nn.Linear, TunedLinear):
            raise NotImplementedError(
                f"quantize_model_fp8: lm_head is a {type(head).__name__}, "
                "expected an unsharded nn.Linear")
        model.lm_head = Fp8Linear.from_linear(head)
    return model
