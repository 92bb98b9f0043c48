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

Opt-in (``one_launch=True``): decode-sized batches take the one-launch
kernels of the same file, ``_C.fp8_linear_wide`` and the fused gate/up
``_C.fp8_swiglu_linear`` behind ``Fp8SwiGLUMLP``; a batch-1 step is bound by
launch count, not bytes (profiles/r17_fp8_one_launch.md).

Inference only.
"""
from typing import Optional, Tuple

import torch
import torch.nn as nn

from ._backend import dispatch
from .linear import TunedLinear, tuned_linear
from .swiglu import swiglu

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


def _refuse_grad(op, *tensors):
    if torch.is_grad_enabled() and any(
            t is not None and t.requires_grad for t in tensors):
        raise RuntimeError(
            f"{op} is inference-only: call it under torch.no_grad() "
            "or detach its inputs")


def fp8_linear(x: torch.Tensor, w8: torch.Tensor, scale: torch.Tensor,
               bias: Optional[torch.Tensor] = None,
               one_launch: bool = False) -> torch.Tensor:
    """``(x @ w8.float().T) * scale + bias`` in ``x.dtype``; x [..., K].

    On a GPU the result is bitwise repeatable. Up to ``FP8_LINEAR_MAX_M`` rows
    a row's bits also do not depend on the batch it sits in; above it (the
    tiled kernel, whose K split depends on M) that is not promised.

    ``one_launch``: up to ``FP8_LINEAR_MAX_M`` rows take ``_C.fp8_linear_wide``
    (K split inside the workgroup only: one launch, no partials) instead of
    the kernel that may split K across workgroups and combine in a second
    launch. Same properties, other summation order, so other last bits."""
    _refuse_grad("fp8_linear", x, scale, bias)
    ext = dispatch(x)
    shape = x.shape
    x2d = x.reshape(-1, shape[-1])
    if ext is None:
        out = (x2d.float() @ w8.float().t()) * scale
        if bias is not None:
            out = out + bias.float()
        out = out.to(x.dtype)
    elif x2d.shape[0] <= FP8_LINEAR_MAX_M:
        kernel = ext.fp8_linear_wide if one_launch else ext.fp8_linear
        out = kernel(x2d.contiguous(), w8, scale, bias)
    elif FP8_GEMM_MAX_M is None or x2d.shape[0] <= FP8_GEMM_MAX_M:
        out = ext.fp8_gemm(x2d.contiguous(), w8, scale, bias)
    else:
        w = (w8.float() * scale[:, None]).to(x.dtype)
        out = tuned_linear(x2d, w, bias)
    return out.view(*shape[:-1], w8.shape[0])


def fp8_swiglu_linear(x: torch.Tensor, wg8: torch.Tensor, sg: torch.Tensor,
                      wu8: torch.Tensor, su: torch.Tensor,
                      bias_gate: Optional[torch.Tensor] = None,
                      bias_up: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``silu(fp8_linear(x, wg8, sg, bias_gate)) * fp8_linear(x, wu8, su,
    bias_up)`` in ``x.dtype``; x [..., K], both weights [I, K].

    On a GPU, up to ``FP8_LINEAR_MAX_M`` rows are ONE launch of the fused
    kernel (csrc/fp8_linear.hip): gate and up pre-activations stay in fp32
    and never reach memory, and the result is bitwise repeatable and
    independent of the batch a row sits in. Above it, two ``fp8_linear`` calls
    (the tiled kernel) and ``swiglu``."""
    _refuse_grad("fp8_swiglu_linear", x, sg, su, bias_gate, bias_up)
    ext = dispatch(x)
    shape = x.shape
    x2d = x.reshape(-1, shape[-1])
    if ext is None:
        g = (x2d.float() @ wg8.float().t()) * sg
        u = (x2d.float() @ wu8.float().t()) * su
        if bias_gate is not None:
            g = g + bias_gate.float()
        if bias_up is not None:
            u = u + bias_up.float()
        out = (g * torch.sigmoid(g) * u).to(x.dtype)
    elif x2d.shape[0] <= FP8_LINEAR_MAX_M:
        out = ext.fp8_swiglu_linear(x2d.contiguous(), wg8, sg, wu8, su,
                                    bias_gate, bias_up)
    else:
        out = swiglu(fp8_linear(x2d, wg8, sg, bias_gate),
                     fp8_linear(x2d, wu8, su, bias_up))
    return out.view(*shape[:-1], wg8.shape[0])


def _keep_buffer_dtypes(module: nn.Module, before) -> None:
    """After an ``_apply`` sweep: a dtype change (.to(bfloat16), .half()) is
    meant for biases; weight codes and scales (e4m3 and fp32 here, uint8 in
    linear_mxfp4) move device but keep their types. ``before``: name ->
    buffer as it was."""
    for name, old in before.items():
        new = getattr(module, name)
        if new.dtype != old.dtype:
            setattr(module, name, old.to(new.device))


class Fp8Linear(nn.Module):
    """Linear layer holding e4m3 weight codes and per-channel fp32 scales."""

    def __init__(self, w8: torch.Tensor, scale: torch.Tensor,
                 bias: Optional[torch.Tensor] = None,
                 one_launch: bool = False):
        super().__init__()
        self.one_launch = one_launch
        self.out_features, self.in_features = w8.shape
        self.register_buffer("weight_fp8", w8)
        self.register_buffer("weight_scale", scale)
        self.register_buffer("bias", bias)

    @classmethod
    def from_linear(cls, lin: nn.Linear,
                    one_launch: bool = False) -> "Fp8Linear":
        w8, scale = quantize_weight_fp8(lin.weight)
        bias = None if lin.bias is None else lin.bias.detach().clone()
        return cls(w8, scale, bias, one_launch)

    def _apply(self, fn, recurse=True):
        before = {n: getattr(self, n) for n in ("weight_fp8", "weight_scale")}
        super()._apply(fn, recurse)
        _keep_buffer_dtypes(self, before)
        return self

    def forward(self, x):
        return fp8_linear(x, self.weight_fp8, self.weight_scale, self.bias,
                          self.one_launch)

    def extra_repr(self):
        return (f"in_features={self.in_features}, "
                f"out_features={self.out_features}, "
                f"bias={self.bias is not None}"
                + (", one_launch=True" if self.one_launch else ""))


class Fp8SwiGLUMLP(nn.Module):
    """SwiGLU MLP on fp8 weights: gate and up projections and the activation
    are one fused launch (``fp8_swiglu_linear``), then an ``Fp8Linear`` down
    projection on the one-launch kernel."""

    _FP8_BUFFERS = ("gate_fp8", "gate_scale", "up_fp8", "up_scale")

    def __init__(self, gate: Fp8Linear, up: Fp8Linear, down: Fp8Linear):
        super().__init__()
        assert gate.weight_fp8.shape == up.weight_fp8.shape
        self.register_buffer("gate_fp8", gate.weight_fp8)
        self.register_buffer("gate_scale", gate.weight_scale)
        self.register_buffer("gate_bias", gate.bias)
        self.register_buffer("up_fp8", up.weight_fp8)
        self.register_buffer("up_scale", up.weight_scale)
        self.register_buffer("up_bias", up.bias)
        self.down_proj = down

    @classmethod
    def from_mlp(cls, mlp: nn.Module) -> "Fp8SwiGLUMLP":
        """From any module with gate_proj / up_proj / down_proj linears
        (``nn.Linear``, ``TunedLinear`` or already ``Fp8Linear``)."""
        def q(lin):
            if isinstance(lin, Fp8Linear):
                return lin
            return Fp8Linear.from_linear(lin)
        down = q(mlp.down_proj)
        down.one_launch = True
        return cls(q(mlp.gate_proj), q(mlp.up_proj), down)

    def _apply(self, fn, recurse=True):
        before = {n: getattr(self, n) for n in self._FP8_BUFFERS}
        super()._apply(fn, recurse)
        _keep_buffer_dtypes(self, before)
        return self

    def forward(self, x):
        return self.down_proj(fp8_swiglu_linear(
            x, self.gate_fp8, self.gate_scale, self.up_fp8, self.up_scale,
            self.gate_bias, self.up_bias))


def _is_swiglu_mlp(mod: nn.Module) -> bool:
    return all(type(getattr(mod, n, None)) in (nn.Linear, TunedLinear,
                                               Fp8Linear)
               for n in ("gate_proj", "up_proj", "down_proj"))


def _swap_linears(parent: nn.Module, one_launch: bool = False) -> None:
    for name, child in parent.named_children():
        if type(child) in (nn.Linear, TunedLinear):
            setattr(parent, name, Fp8Linear.from_linear(child, one_launch))
        elif one_launch and name == "mlp" and _is_swiglu_mlp(child):
            setattr(parent, name, Fp8SwiGLUMLP.from_mlp(child))
        elif isinstance(child, (Fp8Linear, Fp8SwiGLUMLP)):
            continue
        elif hasattr(child, "tp") and hasattr(child, "group") \
                and hasattr(child, "weight"):
            raise NotImplementedError(
                f"quantize_model_fp8: '{name}' is tensor-parallel sharded; "
                "fp8 weights for TP layers are not supported. Quantise the "
                "unsharded model (and serve it on one device) instead.")
        else:
            _swap_linears(child, one_launch)


def quantize_model_fp8(model: nn.Module, include_lm_head: bool = False,
                       one_launch: bool = False):
    """Swap, in place, every ``nn.Linear`` / ``TunedLinear`` inside
    ``model.layers`` for an ``Fp8Linear``; with ``include_lm_head`` also
    ``model.lm_head`` (a tied head gets its own fp8 copy; the embedding table
    is left as it is). Returns the model.

    ``one_launch``: every ``Fp8Linear`` created takes the one-launch kernel at
    decode-sized batches, and each ``mlp`` child made of gate_proj / up_proj /
    down_proj linears becomes an ``Fp8SwiGLUMLP`` (fused gate/up/activation).
    """
    if getattr(model, "_tp_group", None) is not None:
        raise NotImplementedError(
            "quantize_model_fp8: the model is tensor-parallel sharded; fp8 "
            "weights for TP layers are not supported. Quantise the "
            "unsharded model instead.")
    _swap_linears(model.layers, one_launch)
    if not any(isinstance(m, Fp8Linear) for m in model.layers.modules()):
        raise ValueError("quantize_model_fp8: no linear layer found under "
                         "model.layers")
    if include_lm_head:
        head = model.lm_head
        if type(head) not in (nn.Linear, TunedLinear):
            raise NotImplementedError(
                f"quantize_model_fp8: lm_head is a {type(head).__name__}, "
                "expected an unsharded nn.Linear")
        model.lm_head = Fp8Linear.from_linear(head, one_launch)
    return model
