"""float64 references and the error bound for the fused training kernels
(RMSNorm, add+RMSNorm, SwiGLU, RoPE, cross-entropy, AdamW).

Every reference takes the tensors the kernel takes (already rounded to the
kernel dtype), widens them to float64 on the CPU and evaluates the plain
formula; backward comes from autograd on that float64 forward. Only the
kernel's own error is left in ``got - ref``.

One bound is used for every output:

    |got - ref| <= 2^-p * |ref| + 2^-16 * scale

* ``2^-p`` (p = 7 for bf16, 10 for fp16) is one ulp of the output type, twice
  the half ulp of a correct round-to-nearest. fp32 outputs drop this term.
* ``2^-16 * scale`` is >= 100 fp32 ulps of the quantity's natural magnitude
  ``scale`` (room for ``__expf``/``__logf`` and a 256-way reduction) and still
  2^9 below a bf16 ulp, so an intermediate rounded to 16 bits is caught.
  ``scale`` always comes from the reference, never from the kernel.

Every element has to satisfy it. ``check`` prints ``RATIO|device|name|value``
(largest error / bound) before it asserts, so a run with ``-s`` is also the
measurement.
"""
import torch

_P = {torch.bfloat16: 7, torch.float16: 10, torch.float32: None}


def wide(t):
    return t.detach().to("cpu", torch.float64)


def bound(ref, scale, dtype):
    b = 2.0 ** -16 * scale
    p = _P[dtype]
    if p is not None:
        b = b + 2.0 ** -p * ref.abs()
    return b


def check(name, got, ref, scale, dtype=None):
    """Assert the bound element-wise; returns the largest error / bound."""
    dtype = got.dtype if dtype is None else dtype
    dev = "gpu" if got.is_cuda else "cpu"
    g = wide(got)
    assert g.shape == ref.shape, f"{name}: shape {g.shape} vs {ref.shape}"
    assert torch.isfinite(ref).all(), f"{name}: reference is not finite"
    if not torch.isfinite(g).all():
        bad = (~torch.isfinite(g)).nonzero()[0].tolist()
        print(f"RATIO|{dev}|{name}|nan")
        raise AssertionError(
            f"{name}: non-finite output {g[tuple(bad)].item()} at {bad} "
            f"where the reference is {ref[tuple(bad)].item()}")
    b = bound(ref, scale, dtype)
    if not torch.is_tensor(b):
        b = torch.full_like(ref, b)
    b = b.expand_as(ref)
    err = (g - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"RATIO|{dev}|{name}|{worst:.4f}")
    if not bool((err <= b).all()):
        i = tuple((ratio == ratio.max()).nonzero()[0].tolist())
        raise AssertionError(
            f"{name}: err/bound {worst:.3f} at {list(i)}: got {g[i].item()!r}"
            f" ref {ref[i].item()!r} bound {b[i].item():.3e}")
    return worst


def unit(ref):
    """scale for lse, loss, inv_rms and optimizer state: max(1, |ref|)."""
    return ref.abs().clamp_min(1.0)


# --------------------------------------------------------------------------
# RMSNorm / add+RMSNorm
# --------------------------------------------------------------------------

def rmsnorm_ref(r, w, eps, dy=None, dresid=None):
    """r is the normalised row ([rows, H], for the add variant the rounded
    sum x + residual). Returns a dict of float64 references and scales:
    y, inv_rms and, given dy, dx (with dresid added), dw and their scales."""
    r64 = wide(r).requires_grad_(True)
    w64 = wide(w).requires_grad_(True)
    inv = torch.rsqrt(r64.pow(2).mean(-1, keepdim=True) + eps)
    y = r64 * inv * w64
    out = {"y": y.detach(), "inv_rms": inv.detach().squeeze(-1)}
    if dy is None:
        return out
    dy64 = wide(dy)
    loss = (y * dy64).sum()
    if dresid is not None:
        loss = loss + (r64 * wide(dresid)).sum()
    loss.backward()
    out["dx"] = r64.grad
    out["dx_scale"] = r64.grad.abs().amax(-1, keepdim=True)
    out["dw"] = w64.grad
    xhat = (r64 * inv).detach()
    out["dw_scale"] = (dy64 * xhat).abs().reshape(-1, r.shape[-1]).sum(0)
    return out


# --------------------------------------------------------------------------
# SwiGLU
# --------------------------------------------------------------------------

def swiglu_ref(g, u, dy):
    g64 = wide(g).requires_grad_(True)
    u64 = wide(u).requires_grad_(True)
    dy64 = wide(dy)
    y = g64 * torch.sigmoid(g64) * u64
    y.backward(dy64)
    gmag = g64.detach().abs().clamp_min(1.0)
    return {
        "y": y.detach(), "y_scale": u64.detach().abs() * gmag,
        "dg": g64.grad, "dg_scale": (dy64 * u64.detach()).abs(),
        "du": u64.grad, "du_scale": dy64.abs() * gmag,
    }


# --------------------------------------------------------------------------
# RoPE (half-split rotation, x [b, s, h, d], tables [>= s, d/2])
# --------------------------------------------------------------------------

def _rotate(x, cos, sin):
    d2 = x.shape[-1] // 2
    s = x.shape[1]
    a, b = x[..., :d2], x[..., d2:]
    c = cos[:s].view(1, s, 1, d2)
    sn = sin[:s].view(1, s, 1, d2)
    return torch.cat([a * c - b * sn, b * c + a * sn], dim=-1)


def _pair_scale(x):
    d2 = x.shape[-1] // 2
    m = x[..., :d2].abs() + x[..., d2:].abs()
    return torch.cat([m, m], dim=-1)


def rope_ref(x, cos, sin, dout):
    x64 = wide(x).requires_grad_(True)
    d64 = wide(dout)
    out = _rotate(x64, wide(cos), wide(sin))
    out.backward(d64)
    return {"out": out.detach(), "out_scale": _pair_scale(x64.detach()),
            "dx": x64.grad, "dx_scale": _pair_scale(d64)}


# --------------------------------------------------------------------------
# cross-entropy (mean over rows whose target != ignore_index)
# --------------------------------------------------------------------------

def ce_ref(logits, target, ignore_index, upstream):
    l64 = wide(logits).requires_grad_(True)
    t = target.detach().cpu()
    valid = t != ignore_index
    nvalid = int(valid.sum())
    lse = torch.logsumexp(l64, dim=-1)
    picked = l64.gather(1, t.masked_fill(~valid, 0).unsqueeze(1)).squeeze(1)
    rows = torch.where(valid, lse - picked, torch.zeros_like(lse))
    loss_sum = rows.sum()
    loss = loss_sum / max(nvalid, 1)
    (loss * upstream).backward()
    return {"lse": lse.detach(), "loss_sum": loss_sum.detach(),
            "loss": loss.detach(), "nvalid": nvalid,
            "dlogits": l64.grad,
            "dlogits_scale": abs(upstream) / max(nvalid, 1)}


# --------------------------------------------------------------------------
# AdamW
# --------------------------------------------------------------------------

def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def adamw_ref_step(p, g, m, v, step, lr, beta1, beta2, eps, wd):
    """One decoupled-weight-decay Adam step in float64. The kernel's contract
    takes ``float`` hyper-parameters, so they are rounded to fp32 first.
    p, g, m, v are float64; returns the new (p, m, v)."""
    lr, beta1, beta2, eps, wd = map(_f32, (lr, beta1, beta2, eps, wd))
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    p = p * (1.0 - lr * wd) - lr * (m / bc1) / ((v / bc2).sqrt() + eps)
    return p, m, v
