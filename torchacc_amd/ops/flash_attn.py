"""Flash-attention v2 ops on hand-written CDNA4 MFMA kernels.

Reimplements the API surface of the reference's ops/flash_attn.py:11-601
(FlashAttnXla / FlashAttnVarlenXla / FlashAttnVarlenPositionIdsXla and the
user wrappers flash_attn_xla / flash_attn_varlen_xla /
flash_attn_varlen_position_ids_xla) on a single eager ROCm backend:

- fixed-length [b, s, h, d] fwd/bwd with causal, GQA (h_k | h) and sliding
  window;
- varlen via an int32 attention mask [b, s_k] (right-padding; per-batch
  lengths are extracted and passed to the kernel);
- packed-sequence varlen via position_ids [1, total] (cu_seqlens derived
  from position-id resets, reference ops/flash_attn.py:173-218) — used by
  the HF packed-sample training path;
- explicit cu_seqlens varlen (used by ring attention).

The softmax log-sum-exp is returned in fp32 [b, h, s] exactly like FA2 so the
context-parallel LSE merge math is unchanged. bf16 on the CDNA4 kernels
(other dtypes/head dims run a composite fallback); alibi and dropout
dispatch to the full-featured kernel family (csrc/flash_attn_extra_*.hip).
"""
import math
import threading
from collections import deque

import torch

from ._backend import dispatch

# ---- selective activation checkpointing (Megatron-style) -------------------
# utils/checkpoint.py passes sac_contexts as torch.utils.checkpoint's
# context_fn: the capture context retains (out, lse, seed) of every
# attention call inside the checkpointed region, and the recompute context
# replays them so recomputation skips the attention kernels entirely.

_sac_tls = threading.local()


class _SacContext:

    def __init__(self, mode, queue):
        self.mode = mode
        self.queue = queue

    def __enter__(self):
        self.prev = getattr(_sac_tls, "state", None)
        _sac_tls.state = (self.mode, self.queue)

    def __exit__(self, *exc):
        _sac_tls.state = self.prev
        return False


def sac_contexts():
    """Fresh queue per checkpoint invocation: capture/recompute pairs stay
    matched even under PP micro-batch interleaving."""
    q = deque()
    return _SacContext("capture", q), _SacContext("recompute", q)


def _sac_pop():
    state = getattr(_sac_tls, "state", None)
    if state is not None and state[0] == "recompute" and state[1]:
        return state[1].popleft()
    return None


def _sac_push(entry):
    state = getattr(_sac_tls, "state", None)
    if state is not None and state[0] == "capture":
        state[1].append(entry)


_warned_dims = set()


def _pad_target(d: int):
    """Kernel head_dim to zero-pad to (reference pads odd head dims and
    trims in backward, ops/flash_attn.py:166-168); None -> composite."""
    if d in (64, 128):
        return None  # native
    if d < 64:
        return 64
    if d < 128:
        return 128
    return -1  # unsupported: composite


def _kernel_ext(q):
    """The CDNA4 kernels cover bf16 AND fp16 (AttnElem-templated MFMA
    ladder) with head_dim 64/128 natively and any d <= 128 via zero
    padding; d > 128 runs the fp32 composite (warned once per dim — the
    flagship models are all head_dim 128)."""
    ext = dispatch(q)
    if ext is None:
        return None
    if q.dtype not in (torch.bfloat16, torch.float16):
        return None
    d = q.shape[-1]
    if _pad_target(d) == -1:
        if d not in _warned_dims:
            _warned_dims.add(d)
            from ..utils.logger import logger
            logger.warning(
                "flash-attention head_dim %d > 128 unsupported by the "
                "CDNA4 kernels; using the composite fallback", d)
        return None
    return ext


def _pad_d(t: torch.Tensor, pad_to: int) -> torch.Tensor:
    return torch.nn.functional.pad(t, (0, pad_to - t.shape[-1]))


def _check_qkv(q, k, v):
    if q.is_cuda:
        assert q.dtype in (torch.float16, torch.bfloat16, torch.float32), \
            "flash attention requires fp16/bf16 (or fp32 composite)"
    assert q.dtype == k.dtype == v.dtype
    assert q.dim() == 4 and k.dim() == 4 and v.dim() == 4, \
        "expected [batch, seqlen, heads, head_dim]"
    assert k.shape == v.shape
    assert q.shape[0] == k.shape[0] and q.shape[3] == k.shape[3]
    assert q.shape[2] % k.shape[2] == 0, "GQA requires h_k | h_q"


def _ref_attention(q, k, v, softmax_scale, causal, window, q_lens=None,
                   k_lens=None, alibi_slopes=None):
    """fp32 composite reference; returns (out, lse[b,h,sq])."""
    b, sq, h, d = q.shape
    sk = k.shape[1]
    hk = k.shape[2]
    rep = h // hk
    qf = q.float().permute(0, 2, 1, 3)             # [b,h,sq,d]
    kf = k.float().permute(0, 2, 1, 3)             # [b,hk,sk,d]
    vf = v.float().permute(0, 2, 1, 3)
    if rep > 1:
        kf = kf.repeat_interleave(rep, dim=1)
        vf = vf.repeat_interleave(rep, dim=1)
    scores = torch.matmul(qf, kf.transpose(-1, -2)) * softmax_scale
    neg = torch.finfo(torch.float32).min
    iq = torch.arange(sq, device=q.device).view(1, 1, sq, 1)
    ik = torch.arange(sk, device=q.device).view(1, 1, 1, sk)
    if alibi_slopes is not None:
        sl = alibi_slopes.float().view(1, h, 1, 1)
        scores = scores - sl * (ik - (iq + (sk - sq))).abs().float()
    # causal alignment: bottom-right (FA2 semantics)
    if causal:
        shift = sk - sq
        scores = scores.masked_fill(ik > iq + shift, neg)
    wl, wr = window
    if wl >= 0:
        shift = sk - sq
        scores = scores.masked_fill(ik < iq + shift - wl, neg)
    if wr >= 0 and not causal:
        shift = sk - sq
        scores = scores.masked_fill(ik > iq + shift + wr, neg)
    if k_lens is not None:
        klen = k_lens.view(b, 1, 1, 1)
        scores = scores.masked_fill(ik >= klen, neg)
    lse = torch.logsumexp(scores, dim=-1)          # [b,h,sq]
    p = torch.exp(scores - lse.unsqueeze(-1))
    p = torch.nan_to_num(p)                        # fully-masked rows
    out = torch.matmul(p, vf)                      # [b,h,sq,d]
    if q_lens is not None:
        qmask = (iq.view(1, 1, sq, 1) < q_lens.view(b, 1, 1, 1))
        out = out * qmask
        lse = torch.where(qmask.squeeze(-1), lse,
                          torch.zeros_like(lse))
    return out.permute(0, 2, 1, 3).to(q.dtype), lse


class FlashAttnFunc(torch.autograd.Function):

    @staticmethod
    def forward(ctx, q, k, v, dropout_p, softmax_scale, causal, window_size,
                alibi_slopes, deterministic, q_lens, k_lens):
        _check_qkv(q, k, v)
        if softmax_scale is None:
            softmax_scale = 1.0 / math.sqrt(q.shape[-1])
        q, k, v = [t.contiguous() for t in (q, k, v)]
        ext = _kernel_ext(q)
        wl, wr = window_size
        al = alibi_slopes if alibi_slopes is not None else torch.empty(0)
        cached = _sac_pop()
        if cached is not None:
            out, lse, seed = cached
        else:
            seed = 0
            if dropout_p > 0.0:
                assert ext is not None, \
                    "attention dropout runs only on the CDNA4 kernels (GPU)"
                # host-RNG seed: reproducible under torch.manual_seed; the
                # backward kernels regenerate the same keep-mask from it
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            if ext is not None:
                d = q.shape[-1]
                pad_to = _pad_target(d)
                if pad_to:
                    # zero-padded head dims: QK^T and the valid output dims
                    # are unchanged; the pad columns of out are zero
                    out, lse = ext.fa_forward(
                        _pad_d(q, pad_to), _pad_d(k, pad_to),
                        _pad_d(v, pad_to), softmax_scale, causal, wl, wr,
                        q_lens if q_lens is not None else torch.empty(0),
                        k_lens if k_lens is not None else torch.empty(0),
                        al, dropout_p, seed)
                    out = out[..., :d].contiguous()
                else:
                    out, lse = ext.fa_forward(
                        q, k, v, softmax_scale, causal, wl, wr,
                        q_lens if q_lens is not None else torch.empty(0),
                        k_lens if k_lens is not None else torch.empty(0),
                        al, dropout_p, seed)
            else:
                out, lse = _ref_attention(q, k, v, softmax_scale, causal,
                                          (wl, wr), q_lens, k_lens,
                                          alibi_slopes)
        _sac_push((out.detach(), lse.detach(), seed))
        ctx.save_for_backward(
            q, k, v, out, lse,
            q_lens if q_lens is not None else torch.empty(0),
            k_lens if k_lens is not None else torch.empty(0), al)
        ctx.softmax_scale = softmax_scale
        ctx.causal = causal
        ctx.window = (wl, wr)
        ctx.deterministic = deterministic
        ctx.dropout = (dropout_p, seed)
        return out, lse

    @staticmethod
    def backward(ctx, dout, _dlse):
        q, k, v, out, lse, q_lens, k_lens, al = ctx.saved_tensors
        q_lens = q_lens if q_lens.numel() else None
        k_lens = k_lens if k_lens.numel() else None
        ext = _kernel_ext(q)
        dout = dout.contiguous()
        wl, wr = ctx.window
        if ext is not None:
            p_drop, seed = ctx.dropout
            d = q.shape[-1]
            pad_to = _pad_target(d)
            if pad_to:
                dq, dk, dv = ext.fa_backward(
                    _pad_d(dout, pad_to), _pad_d(q, pad_to),
                    _pad_d(k, pad_to), _pad_d(v, pad_to),
                    _pad_d(out, pad_to), lse, ctx.softmax_scale,
                    ctx.causal, wl, wr,
                    q_lens if q_lens is not None else torch.empty(0),
                    k_lens if k_lens is not None else torch.empty(0), al,
                    p_drop, seed)
                dq = dq[..., :d].contiguous()
                dk = dk[..., :d].contiguous()
                dv = dv[..., :d].contiguous()
            else:
                dq, dk, dv = ext.fa_backward(
                    dout, q, k, v, out, lse, ctx.softmax_scale, ctx.causal,
                    wl, wr,
                    q_lens if q_lens is not None else torch.empty(0),
                    k_lens if k_lens is not None else torch.empty(0), al,
                    p_drop, seed)
        else:
            dq, dk, dv = _ref_fa_backward(dout, q, k, v, out, lse,
                                          ctx.softmax_scale, ctx.causal,
                                          (wl, wr), q_lens, k_lens,
                                          al if al.numel() else None)
        return (dq, dk, dv) + (None,) * 8


def _ref_fa_backward(dout, q, k, v, out, lse, softmax_scale, causal, window,
                     q_lens, k_lens, alibi_slopes=None):
    """Recompute-based fp32 reference backward.

    ``out``/``lse`` are the GLOBAL attention output / logsumexp: delta =
    rowsum(dout * out) so the same routine serves both plain FA backward and
    per-block ring-attention backward (where p is normalized by the global
    lse and delta must come from the merged output)."""
    b, sq, h, d = q.shape
    sk, hk = k.shape[1], k.shape[2]
    rep = h // hk
    qf = q.float().permute(0, 2, 1, 3)
    kf = k.float().permute(0, 2, 1, 3)
    vf = v.float().permute(0, 2, 1, 3)
    dof = dout.float().permute(0, 2, 1, 3)
    if rep > 1:
        kf = kf.repeat_interleave(rep, dim=1)
        vf = vf.repeat_interleave(rep, dim=1)
    scores = torch.matmul(qf, kf.transpose(-1, -2)) * softmax_scale
    neg = torch.finfo(torch.float32).min
    iq = torch.arange(sq, device=q.device).view(1, 1, sq, 1)
    ik = torch.arange(sk, device=q.device).view(1, 1, 1, sk)
    shift = sk - sq
    if alibi_slopes is not None:
        sl = alibi_slopes.float().view(1, h, 1, 1)
        scores = scores - sl * (ik - (iq + shift)).abs().float()
    if causal:
        scores = scores.masked_fill(ik > iq + shift, neg)
    wl, wr = window
    if wl >= 0:
        scores = scores.masked_fill(ik < iq + shift - wl, neg)
    if wr >= 0 and not causal:
        scores = scores.masked_fill(ik > iq + shift + wr, neg)
    if k_lens is not None:
        scores = scores.masked_fill(ik >= k_lens.view(b, 1, 1, 1), neg)
    p = torch.exp(scores - lse.unsqueeze(-1))
    p = torch.nan_to_num(p)
    if q_lens is not None:
        qmask = iq < q_lens.view(b, 1, 1, 1)
        p = p * qmask
        dof = dof * qmask
    dv = torch.matmul(p.transpose(-1, -2), dof)
    dp = torch.matmul(dof, vf.transpose(-1, -2))
    delta = (dof * out.float().permute(0, 2, 1, 3)).sum(-1, keepdim=True)
    ds = p * (dp - delta) * softmax_scale
    dq = torch.matmul(ds, kf)
    dk = torch.matmul(ds.transpose(-1, -2), qf)
    if rep > 1:
        dk = dk.view(b, hk, rep, sk, d).sum(2)
        dv = dv.view(b, hk, rep, sk, d).sum(2)
    return (dq.permute(0, 2, 1, 3).to(q.dtype),
            dk.permute(0, 2, 1, 3).to(k.dtype),
            dv.permute(0, 2, 1, 3).to(v.dtype))


# ---------------------------------------------------------------------------
# user wrappers (reference-compatible names)
# ---------------------------------------------------------------------------

def _cast_fp16(q, k, v):
    """fp16 is now a NATIVE kernel dtype (v_mfma_f32_32x32x16_f16 via the
    AttnElem traits) — this shim is a passthrough kept for API stability
    (reference accepts fp16, ops/flash_attn.py:324-325)."""
    return q, k, v, False


def flash_attn_xla(q, k, v, dropout_p=0.0, softmax_scale=None, causal=False,
                   window_size=(-1, -1), alibi_slopes=None,
                   deterministic=False, return_attn_probs=False):
    """Fixed-length flash attention, q/k/v [b, s, h, d].

    Name kept from the reference for drop-in compatibility; runs on the
    CDNA4 HIP kernel (there is no XLA here).
    """
    q, k, v, back = _cast_fp16(q, k, v)
    out, lse = FlashAttnFunc.apply(q, k, v, dropout_p, softmax_scale, causal,
                                   window_size, alibi_slopes, deterministic,
                                   None, None)
    if back:
        out = out.to(torch.float16)
    if return_attn_probs:
        return out, lse, None
    return out


flash_attn_func = flash_attn_xla


def flash_attn_varlen_xla(q, k, v, attention_mask=None, dropout_p=0.0,
                          softmax_scale=None, causal=False,
                          window_size=(-1, -1), alibi_slopes=None,
                          deterministic=False, return_attn_probs=False):
    """Varlen-by-mask flash attention (reference FlashAttnVarlenXla,
    ops/flash_attn.py:219-262): ``attention_mask`` is an int mask [b, s_k]
    marking valid keys (right padding)."""
    k_lens = None
    q_lens = None
    if attention_mask is not None:
        assert attention_mask.dim() == 2
        k_lens = attention_mask.to(torch.int32).sum(-1).to(torch.int32)
        if q.shape[1] == k.shape[1]:
            q_lens = k_lens
    q, k, v, back = _cast_fp16(q, k, v)
    out, lse = FlashAttnFunc.apply(q, k, v, dropout_p, softmax_scale, causal,
                                   window_size, alibi_slopes, deterministic,
                                   q_lens, k_lens)
    if back:
        out = out.to(torch.float16)
    if return_attn_probs:
        return out, lse, None
    return out


def position_ids_to_cu_seqlens(position_ids: torch.Tensor) -> torch.Tensor:
    """[1, total] packed position ids -> int32 cu_seqlens (resets at 0),
    reference FlashAttnVarlenPositionIdsXla semantics."""
    pos = position_ids.reshape(-1)
    starts = torch.nonzero(pos == 0).reshape(-1)
    total = pos.numel()
    cu = torch.cat([starts.to(torch.int32),
                    torch.tensor([total], dtype=torch.int32,
                                 device=pos.device)])
    return cu


def flash_attn_varlen_position_ids_xla(q, k, v, position_ids, dropout_p=0.0,
                                       softmax_scale=None, causal=False,
                                       window_size=(-1, -1),
                                       alibi_slopes=None,
                                       deterministic=False,
                                       return_attn_probs=False):
    """Packed-sequence flash attention: bsz must be 1, sequences delimited by
    position-id resets (reference ops/flash_attn.py:173-218, 488)."""
    assert q.shape[0] == 1, "position-ids varlen requires batch size 1"
    cu = position_ids_to_cu_seqlens(position_ids)
    max_len = int((cu[1:] - cu[:-1]).max())
    q, k, v, back = _cast_fp16(q, k, v)
    out, lse = FlashAttnVarlenFunc.apply(
        q.squeeze(0), k.squeeze(0), v.squeeze(0), cu, cu, max_len, max_len,
        dropout_p, softmax_scale, causal, window_size, deterministic)
    out = out.unsqueeze(0)
    if back:
        out = out.to(torch.float16)
    if return_attn_probs:
        return out, lse, None
    return out


class FlashAttnVarlenFunc(torch.autograd.Function):
    """True packed varlen with explicit cu_seqlens (used by ring attention
    and the position-ids path). q/k/v are [total, h, d]."""

    @staticmethod
    def forward(ctx, q, k, v, cu_q, cu_k, max_q, max_k, dropout_p,
                softmax_scale, causal, window_size, deterministic):
        assert dropout_p == 0.0
        if softmax_scale is None:
            softmax_scale = 1.0 / math.sqrt(q.shape[-1])
        q, k, v = [t.contiguous() for t in (q, k, v)]
        ext = _kernel_ext(q)
        wl, wr = window_size
        cached = _sac_pop()
        if cached is not None:
            out, lse = cached[0], cached[1]
        elif ext is not None:
            out, lse = _varlen_fwd_gpu(ext, q, k, v, cu_q, cu_k,
                                       softmax_scale, causal, wl, wr)
        else:
            out, lse = _ref_varlen(q, k, v, cu_q, cu_k, softmax_scale,
                                   causal, (wl, wr))
        _sac_push((out.detach(), lse.detach(), 0))
        ctx.save_for_backward(q, k, v, out, lse, cu_q, cu_k)
        ctx.meta = (max_q, max_k, softmax_scale, causal, window_size)
        return out, lse

    @staticmethod
    def backward(ctx, dout, _dlse):
        q, k, v, out, lse, cu_q, cu_k = ctx.saved_tensors
        max_q, max_k, softmax_scale, causal, window_size = ctx.meta
        ext = _kernel_ext(q)
        dout = dout.contiguous()
        wl, wr = window_size
        if ext is not None:
            dq, dk, dv = _varlen_bwd_gpu(ext, dout, q, k, v, out, lse, cu_q,
                                         cu_k, softmax_scale, causal, wl, wr)
        else:
            dq, dk, dv = _ref_varlen_backward(dout, q, k, v, out, lse, cu_q,
                                              cu_k, softmax_scale, causal,
                                              (wl, wr))
        return (dq, dk, dv) + (None,) * 9


def _cu_to_bounds(cu: torch.Tensor, total: int) -> torch.Tensor:
    """cu_seqlens -> per-row int32 [total, 2] sequence intervals (the form
    the fused varlen kernels consume: same-sequence masking collapses to a
    per-q-row interval test, see csrc/flash_attn_varlen.hip)."""
    cu = cu.to(torch.int32)
    lens = (cu[1:] - cu[:-1]).long()
    starts = torch.repeat_interleave(cu[:-1], lens)
    ends = torch.repeat_interleave(cu[1:], lens)
    b = torch.stack([starts, ends], dim=1)
    if b.shape[0] < total:
        # rows past cu[-1] (padding): empty interval -> zero out/grads
        b = torch.cat([b, torch.zeros(total - b.shape[0], 2,
                                      dtype=torch.int32,
                                      device=b.device)])
    return b.contiguous()


def _use_fused_varlen(q, k, cu_q, cu_k, wl, wr):
    # `cu_q is cu_k` short-circuit: the position-ids and qkv-packed paths
    # pass the same tensor for both, avoiding a device sync (torch.equal)
    # on every attention call
    return (wl < 0 and wr < 0 and q.shape[0] == k.shape[0] and
            cu_q.numel() == cu_k.numel() and
            (cu_q is cu_k or bool(torch.equal(cu_q, cu_k))))


def _varlen_fwd_gpu(ext, q, k, v, cu_q, cu_k, softmax_scale, causal, wl,
                    wr):
    """Packed varlen: ONE fused kernel launch over the whole packed batch
    when q/k share the packing and there is no sliding window; otherwise
    one launch per sequence on the fixed-length kernel."""
    d = q.shape[-1]
    pad_to = _pad_target(d)
    if pad_to:
        out, lse = _varlen_fwd_gpu(ext, _pad_d(q, pad_to),
                                   _pad_d(k, pad_to), _pad_d(v, pad_to),
                                   cu_q, cu_k, softmax_scale, causal, wl,
                                   wr)
        return out[..., :d].contiguous(), lse
    total, h, _d = q.shape
    if _use_fused_varlen(q, k, cu_q, cu_k, wl, wr):
        bounds = _cu_to_bounds(cu_q.to(q.device), total)
        return tuple(ext.fa_varlen_forward(q, k, v, bounds, softmax_scale,
                                           causal))
    out = torch.zeros_like(q)
    lse = torch.zeros(h, total, dtype=torch.float32, device=q.device)
    empty = torch.empty(0, device=q.device)
    for i in range(cu_q.numel() - 1):
        qs, qe = int(cu_q[i]), int(cu_q[i + 1])
        ks, ke = int(cu_k[i]), int(cu_k[i + 1])
        if qe == qs:
            continue
        o_i, lse_i = ext.fa_forward(
            q[qs:qe].unsqueeze(0).contiguous(),
            k[ks:ke].unsqueeze(0).contiguous(),
            v[ks:ke].unsqueeze(0).contiguous(), softmax_scale, causal, wl,
            wr, empty, empty, empty, 0.0, 0)
        out[qs:qe] = o_i.squeeze(0)
        lse[:, qs:qe] = lse_i.squeeze(0)
    return out, lse


def _varlen_bwd_gpu(ext, dout, q, k, v, out, lse, cu_q, cu_k, softmax_scale,
                    causal, wl, wr):
    d = q.shape[-1]
    pad_to = _pad_target(d)
    if pad_to:
        dq, dk, dv = _varlen_bwd_gpu(
            ext, _pad_d(dout, pad_to), _pad_d(q, pad_to),
            _pad_d(k, pad_to), _pad_d(v, pad_to), _pad_d(out, pad_to),
            lse, cu_q, cu_k, softmax_scale, causal, wl, wr)
        return (dq[..., :d].contiguous(), dk[..., :d].contiguous(),
                dv[..., :d].contiguous())
    if _use_fused_varlen(q, k, cu_q, cu_k, wl, wr):
        bounds = _cu_to_bounds(cu_q.to(q.device), q.shape[0])
        return tuple(ext.fa_varlen_backward(dout, q, k, v, out, lse.contiguous(),
                                            bounds, softmax_scale, causal))
    dq = torch.zeros_like(q)
    dk = torch.zeros_like(k)
    dv = torch.zeros_like(v)
    empty = torch.empty(0, device=q.device)
    for i in range(cu_q.numel() - 1):
        qs, qe = int(cu_q[i]), int(cu_q[i + 1])
        ks, ke = int(cu_k[i]), int(cu_k[i + 1])
        if qe == qs:
            continue
        dq_i, dk_i, dv_i = ext.fa_backward(
            dout[qs:qe].unsqueeze(0).contiguous(),
            q[qs:qe].unsqueeze(0).contiguous(),
            k[ks:ke].unsqueeze(0).contiguous(),
            v[ks:ke].unsqueeze(0).contiguous(),
            out[qs:qe].unsqueeze(0).contiguous(),
            lse[:, qs:qe].unsqueeze(0).contiguous(), softmax_scale, causal,
            wl, wr, empty, empty, empty, 0.0, 0)
        dq[qs:qe] = dq_i.squeeze(0)
        dk[ks:ke] = dk_i.squeeze(0)
        dv[ks:ke] = dv_i.squeeze(0)
    return dq, dk, dv


def _ref_varlen(q, k, v, cu_q, cu_k, softmax_scale, causal, window):
    total, h, d = q.shape
    out = torch.zeros_like(q)
    lse = torch.full((h, total), 0.0, dtype=torch.float32, device=q.device)
    for i in range(cu_q.numel() - 1):
        qs, qe = int(cu_q[i]), int(cu_q[i + 1])
        ks, ke = int(cu_k[i]), int(cu_k[i + 1])
        if qe == qs:
            continue
        o, l = _ref_attention(q[qs:qe].unsqueeze(0), k[ks:ke].unsqueeze(0),
                              v[ks:ke].unsqueeze(0), softmax_scale, causal,
                              window)
        out[qs:qe] = o.squeeze(0)
        lse[:, qs:qe] = l.squeeze(0)
    return out, lse


def _ref_varlen_backward(dout, q, k, v, out, lse, cu_q, cu_k, softmax_scale,
                         causal, window):
    dq = torch.zeros_like(q)
    dk = torch.zeros_like(k)
    dv = torch.zeros_like(v)
    for i in range(cu_q.numel() - 1):
        qs, qe = int(cu_q[i]), int(cu_q[i + 1])
        ks, ke = int(cu_k[i]), int(cu_k[i + 1])
        if qe == qs:
            continue
        dqi, dki, dvi = _ref_fa_backward(
            dout[qs:qe].unsqueeze(0), q[qs:qe].unsqueeze(0),
            k[ks:ke].unsqueeze(0), v[ks:ke].unsqueeze(0),
            out[qs:qe].unsqueeze(0), lse[:, qs:qe].unsqueeze(0),
            softmax_scale, causal, window, None, None)
        dq[qs:qe] = dqi.squeeze(0)
        dk[ks:ke] = dki.squeeze(0)
        dv[ks:ke] = dvi.squeeze(0)
    return dq, dk, dv


def flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q,
                           max_seqlen_k, dropout_p=0.0, softmax_scale=None,
                           causal=False, window_size=(-1, -1),
                           alibi_slopes=None, deterministic=False,
                           return_attn_probs=False):
    q, k, v, back = _cast_fp16(q, k, v)
    out, lse = FlashAttnVarlenFunc.apply(q, k, v, cu_seqlens_q, cu_seqlens_k,
                                         max_seqlen_q, max_seqlen_k,
                                         dropout_p, softmax_scale, causal,
                                         window_size, deterministic)
    if back:
        out = out.to(torch.float16)
    if return_attn_probs:
        return out, lse, None
    return out


# SPMD-named alias kept for API compatibility (reference ops/flash_attn.py:66)
def spmd_flash_attn_varlen_xla(*args, **kwargs):
    return flash_attn_varlen_xla(*args, **kwargs)


def flash_attn_qkvpacked_xla(qkv, dropout_p=0.0, softmax_scale=None,
                             causal=False, window_size=(-1, -1),
                             alibi_slopes=None, deterministic=False,
                             return_attn_probs=False):
    """qkv [b, s, 3, h, d] (reference FlashAttnVarlenQKVPackedXla:11)."""
    q, k, v = qkv.unbind(2)
    return flash_attn_xla(q, k, v, dropout_p, softmax_scale, causal,
                          window_size, alibi_slopes, deterministic,
                          return_attn_probs)


def flash_attn_varlen_qkvpacked_xla(qkv, attention_mask=None, **kw):
    q, k, v = qkv.unbind(2)
    return flash_attn_varlen_xla(q, k, v, attention_mask=attention_mask,
                                 **kw)


def flash_attn_kvpacked_xla(q, kv, dropout_p=0.0, softmax_scale=None,
                            causal=False, window_size=(-1, -1),
                            alibi_slopes=None, deterministic=False,
                            return_attn_probs=False):
    k, v = kv.unbind(2)
    return flash_attn_xla(q, k, v, dropout_p, softmax_scale, causal,
                          window_size, alibi_slopes, deterministic,
                          return_attn_probs)


# ---------------------------------------------------------------------------
# decode: one query per sequence against an in-place KV cache
# ---------------------------------------------------------------------------

def _ref_decode(q, k_cache, v_cache, lens, softmax_scale, wl):
    """fp32 reference for flash_attn_with_kvcache: batch i sees the keys
    [lo_i, lens_i) with lo_i = max(0, lens_i - 1 - wl) (0 without a window).
    Slots outside that range are dropped before any arithmetic, so their
    contents (even NaN) cannot matter. Returns (out, lse[b, hq, 1])."""
    b, _, hq, d = q.shape
    cap, hk = k_cache.shape[1], k_cache.shape[2]
    ik = torch.arange(cap, device=q.device).view(1, 1, 1, cap)
    if lens is None:
        klen = torch.full((b, 1, 1, 1), cap, device=q.device)
    else:
        klen = lens.long().clamp(0, cap).view(b, 1, 1, 1)
    lo = (klen - 1 - wl).clamp(min=0) if wl >= 0 else torch.zeros_like(klen)
    vis = (ik >= lo) & (ik < klen)                       # [b,1,1,cap]
    keep = vis.view(b, 1, cap, 1)
    zero = torch.zeros((), dtype=torch.float32, device=q.device)
    qf = q.float().view(b, hk, hq // hk, d)              # head = kh*rep + r
    kf = torch.where(keep, k_cache.float().permute(0, 2, 1, 3), zero)
    vf = torch.where(keep, v_cache.float().permute(0, 2, 1, 3), zero)
    scores = torch.matmul(qf, kf.transpose(-1, -2)) * softmax_scale
    scores = scores.masked_fill(~vis, float("-inf"))
    lse = torch.logsumexp(scores, dim=-1, keepdim=True)  # -inf if none seen
    p = torch.where(torch.isfinite(lse), torch.exp(scores - lse), zero)
    out = torch.matmul(p, vf)                            # [b,hk,rep,d]
    return out.reshape(b, 1, hq, d).to(q.dtype), lse.reshape(b, hq, 1)


_warned_decode = set()
_ABSENT = torch.empty(0)    # an absent optional tensor, for the extension

# ---- fp8 KV cache: OCP e4m3fn codes with one fp32 scale per kv head --------
FP8_DTYPE = torch.float8_e4m3fn
FP8_MAX = 448.0


def _check_kv_scale(scale, cache, name):
    assert isinstance(scale, torch.Tensor), \
        f"fp8 KV caches need {name}: an fp32 tensor [hk]"
    assert scale.dtype == torch.float32, \
        f"{name} must be fp32, got {scale.dtype}"
    assert scale.shape == (cache.shape[2],), \
        f"{name} must be [hk] = [{cache.shape[2]}], got {tuple(scale.shape)}"
    assert scale.device == cache.device, \
        f"{name} must live on the device of the cache"


def dequantize_kv_fp8(cache, scale, dtype=torch.float32):
    """codes [.., .., hk, d] (float8_e4m3fn) * scale [hk] -> ``dtype``. The
    product is formed in fp32 and rounded once."""
    return (cache.float() * scale.view(1, 1, -1, 1)).to(dtype)


def kv_cache_write_fp8(k, v, k_cache, v_cache, slots, k_scale, v_scale):
    """Quantise new K / V rows into float8_e4m3fn caches, in place.

    k, v [b, s, hk, d] (bf16/fp16 on the GPU; [hk, d] dense, d % 8 == 0);
    k_cache, v_cache float8_e4m3fn [n0, n1, hk, d] with dense [hk, d] and
    arbitrary strides for dims 0 and 1: a contiguous cache [b, cap, hk, d]
    or a page pool [num_pages, page_size, hk, d]. ``slots`` (int32/int64
    [b * s], same device) names the flat slot ``t -> [t // n1, t % n1]`` of
    every token: ``PagedKVCache.slot_indices`` for a pool, ``batch * cap +
    pos`` for a contiguous cache. k_scale, v_scale: fp32 [hk] on the device.

    Every element becomes ``rne_e4m3(clamp(x * (1 / scale[head]), -448,
    448))``: the clamp runs in fp32 before the conversion, so finite inputs
    saturate and never turn into NaN. Slots outside [0, n0 * n1) are
    skipped; duplicate slots are unspecified. One HIP launch for K and V
    (csrc/kv_cache_write.hip), no host sync, no autograd."""
    assert k.dim() == 4 and k.shape == v.shape and k.dtype == v.dtype
    assert k_cache.dim() == 4 and k_cache.shape == v_cache.shape
    assert k_cache.dtype == FP8_DTYPE and v_cache.dtype == FP8_DTYPE, \
        "kv_cache_write_fp8 writes float8_e4m3fn caches"
    assert k_cache.shape[2:] == k.shape[2:], \
        "cache and new rows disagree on [hk, d]"
    assert k.device == v.device == k_cache.device == v_cache.device
    assert slots.dtype in (torch.int32, torch.int64), \
        "slots must be int32 or int64"
    assert slots.shape == (k.shape[0] * k.shape[1],) \
        and slots.device == k.device, "slots must be [b * s] on k's device"
    _check_kv_scale(k_scale, k_cache, "k_scale")
    _check_kv_scale(v_scale, v_cache, "v_scale")
    ext = dispatch(k)
    if ext is not None:
        ext.kv_cache_write_fp8(k, v, k_cache, v_cache, slots.contiguous(),
                               k_scale, v_scale)
        return
    n0, n1 = k_cache.shape[:2]
    t = slots.long()
    ok = (t >= 0) & (t < n0 * n1)
    t = t[ok]
    for x, cache, scale in ((k, k_cache, k_scale), (v, v_cache, v_scale)):
        y = x.float() * (1.0 / scale).view(1, 1, -1, 1)
        codes = y.clamp(-FP8_MAX, FP8_MAX).to(FP8_DTYPE)
        codes = codes.reshape(-1, *codes.shape[2:])[ok]
        # no float8 index kernels on the CPU: store the bytes
        cache.view(torch.uint8)[t // n1, t % n1] = codes.view(torch.uint8)


def _rkw_check(cond, msg):
    if not cond:
        raise ValueError(f"rope_kv_cache_write: {msg}")


def rope_kv_cache_write(q, k, v, cos, sin, positions, k_cache, v_cache, slots,
                        k_scale=None, v_scale=None):
    """RoPE at per-token positions, with K and V written straight into the
    cache; returns the rotated q [b, s, hq, d].

    q [b, s, hq, d], k / v [b, s, hk, d] (bf16/fp16 on the GPU; [heads, d]
    dense, d % 16 == 0, batch and token strides multiples of 8 elements, so
    column slices of one fused qkv buffer qualify). cos / sin: the model's
    FULL fp32 tables [P, d / 2], contiguous, not a slice. ``positions`` and
    ``slots`` (int32/int64 [b * s], same device) are read on the device:
    no host sync, and a captured launch follows their values at replay.
    k_cache / v_cache [n0, n1, hk, d] as in ``kv_cache_write_fp8`` (a
    contiguous cache or a page pool, flat slot ``t -> [t // n1, t % n1]``),
    either of q's dtype (then no scales) or float8_e4m3fn with fp32 [hk]
    ``k_scale`` / ``v_scale``.

    Token t with ``p = positions[t]`` outside [0, P) is padding: its q_rot
    rows are zero and nothing is written. Otherwise q_rot[t] is q[t] rotated
    by table row p, and if ``slots[t]`` lies in [0, n0 * n1) that slot
    receives the rotated k[t] and v[t]. Duplicate slots are unspecified.

    Bitwise equal to ``apply_rotary_pos_emb`` (with the rows' table slices)
    followed by ``index_copy_`` or ``kv_cache_write_fp8``: the rotation is
    computed in fp32 and rounded once to the element type; an fp8 cache
    quantises that rounded value. One HIP launch (csrc/rope_kv_write.hip),
    no workspace, no autograd. CPU and fp32 tensors take a torch reference
    with the same semantics."""
    _rkw_check(q.dim() == 4 and k.dim() == 4 and v.shape == k.shape
               and q.shape[:2] == k.shape[:2] and q.shape[3] == k.shape[3],
               "q [b, s, hq, d] and k, v [b, s, hk, d] disagree")
    _rkw_check(q.dtype == k.dtype == v.dtype, "q, k and v must share a dtype")
    b, s, hq, d = q.shape
    hk = k.shape[2]
    _rkw_check(d % 16 == 0, "head_dim must be a multiple of 16")
    _rkw_check(cos.dim() == 2 and cos.shape == sin.shape
               and cos.shape[1] == d // 2 and cos.shape[0] >= 1
               and cos.dtype == sin.dtype == torch.float32,
               "cos and sin must be fp32 [P, d / 2] tables with P >= 1")
    _rkw_check(k_cache.dim() == 4 and k_cache.shape == v_cache.shape
               and k_cache.shape[2:] == k.shape[2:],
               "k_cache and v_cache must be [n0, n1, hk, d]")
    _rkw_check(k_cache.dtype == v_cache.dtype
               and k_cache.dtype in (k.dtype, FP8_DTYPE),
               "the caches must have k's dtype or be float8_e4m3fn")
    fp8 = k_cache.dtype == FP8_DTYPE
    for name, t in (("positions", positions), ("slots", slots)):
        _rkw_check(t.dtype in (torch.int32, torch.int64)
                   and t.shape == (b * s,),
                   f"{name} must be int32 or int64 [b * s]")
    for name, t in (("k", k), ("v", v), ("cos", cos), ("sin", sin),
                    ("positions", positions), ("slots", slots),
                    ("k_cache", k_cache), ("v_cache", v_cache),
                    ("k_scale", k_scale), ("v_scale", v_scale)):
        _rkw_check(t is None or t.device == q.device,
                   f"{name} must live on q's device")
    if fp8:
        _rkw_check(k_scale is not None and v_scale is not None,
                   "float8_e4m3fn caches need k_scale and v_scale")
        _check_kv_scale(k_scale, k_cache, "k_scale")
        _check_kv_scale(v_scale, v_cache, "v_scale")
    else:
        _rkw_check(k_scale is None and v_scale is None,
                   "k_scale / v_scale apply to float8_e4m3fn caches only")
    ext = dispatch(q)
    if ext is not None and q.dtype in (torch.bfloat16, torch.float16):
        if slots.dtype != positions.dtype:
            slots = slots.to(positions.dtype)
        return ext.rope_kv_cache_write(
            q, k, v, cos, sin, positions.contiguous(), k_cache, v_cache,
            slots.contiguous(), k_scale if fp8 else _ABSENT,
            v_scale if fp8 else _ABSENT)
    P, d2 = cos.shape[0], d // 2
    pos = positions.long()
    real = (pos >= 0) & (pos < P)
    row = pos.clamp(0, P - 1)
    c = cos[row].view(b, s, 1, d2)
    sn = sin[row].view(b, s, 1, d2)

    def rot(x):
        x1, x2 = x[..., :d2].float(), x[..., d2:].float()
        return torch.cat([x1 * c - x2 * sn, x2 * c + x1 * sn],
                         dim=-1).to(x.dtype)

    q_rot = torch.where(real.view(b, s, 1, 1), rot(q), torch.zeros_like(q))
    n0, n1 = k_cache.shape[:2]
    t = slots.long()
    ok = real & (t >= 0) & (t < n0 * n1)
    t = t[ok]
    for x, cache, scale in ((rot(k), k_cache, k_scale),
                            (v, v_cache, v_scale)):
        x = x.reshape(-1, hk, d)[ok]
        if fp8:
            y = x.float() * (1.0 / scale).view(1, -1, 1)
            codes = y.clamp(-FP8_MAX, FP8_MAX).to(FP8_DTYPE)
            # no float8 index kernels on the CPU: store the bytes
            cache.view(torch.uint8)[t // n1, t % n1] = codes.view(torch.uint8)
        else:
            cache[t // n1, t % n1] = x
    return q_rot


def _decode_fallback_gpu(q, k_cache, v_cache, lens, softmax_scale, wl):
    """GPU inputs the decode kernel does not cover (fp32, head dims other
    than 64/128): the fixed-length attention path on a copy of the cache.
    One batched call, without a host sync (so it still captures into a
    graph), unless per-sequence lengths AND a window are given: a window
    anchored at each live length has no batched form on that path, so that
    case reads the lengths on the host and runs one call per sequence."""
    key = (q.dtype, q.shape[-1])
    if key not in _warned_decode:
        _warned_decode.add(key)
        from ..utils.logger import logger
        logger.warning(
            "flash_attn_with_kvcache: dtype %s / head_dim %d is not covered "
            "by the decode kernel; using the fixed-length attention path on "
            "a copy of the cache", *key)
    b, _, hq, d = q.shape
    cap = k_cache.shape[1]
    if lens is None:
        # sq = 1, bottom-right causal: the window is anchored at cap
        return FlashAttnFunc.apply(q, k_cache, v_cache, 0.0, softmax_scale,
                                   True, (wl, -1), None, False, None, None)
    if wl < 0:
        # the copy drops the slots past each length, so their contents
        # cannot reach the fp32 composite as 0 * NaN either
        keep = (torch.arange(cap, device=q.device).view(1, cap, 1, 1)
                < lens.view(b, 1, 1, 1))
        zero = torch.zeros((), dtype=q.dtype, device=q.device)
        out, lse = FlashAttnFunc.apply(
            q, torch.where(keep, k_cache, zero),
            torch.where(keep, v_cache, zero), 0.0, softmax_scale, True,
            (-1, -1), None, False, None, lens)
        empty = (lens <= 0).view(b, 1, 1)
        out = torch.where(empty.unsqueeze(-1), zero, out)
        lse = torch.where(empty, torch.full_like(lse, float("-inf")), lse)
        return out, lse
    host_lens = [min(max(int(n), 0), cap) for n in lens.tolist()]
    out = torch.zeros_like(q)
    lse = torch.full((b, hq, 1), float("-inf"), dtype=torch.float32,
                     device=q.device)
    for i, n in enumerate(host_lens):
        if n == 0:
            continue
        o_i, lse_i = FlashAttnFunc.apply(
            q[i:i + 1], k_cache[i:i + 1, :n].contiguous(),
            v_cache[i:i + 1, :n].contiguous(), 0.0, softmax_scale, True,
            (wl, -1), None, False, None, None)
        out[i:i + 1] = o_i
        lse[i:i + 1] = lse_i
    return out, lse


def _gather_pages(pool, block_table):
    """Page pool [num_pages, page_size, hk, d] and table [b, w] -> the
    contiguous cache [b, w * page_size, hk, d] the table describes. Entries
    are clamped into the pool as the kernel clamps them, so the entries of
    unused logical pages cannot make the gather raise."""
    n, ps, hk, d = pool.shape
    b, w = block_table.shape
    idx = block_table.reshape(-1).long().clamp(0, n - 1)
    if pool.dtype == FP8_DTYPE:
        # float8 has no index kernels on every backend: move the bytes
        return (pool.view(torch.uint8).index_select(0, idx)
                .view(b, w * ps, hk, d).view(FP8_DTYPE))
    return pool.index_select(0, idx).view(b, w * ps, hk, d)


def _paged_kernel_page_size(ps: int) -> bool:
    return ps >= 16 and (ps & (ps - 1)) == 0


def _kvcache_args(op, q, k_cache, v_cache, cache_seqlens, q_seqlens,
                  softmax_scale, window_size, block_table, k_scale, v_scale):
    """What flash_attn_with_kvcache and flash_attn_chunk_with_kvcache share:
    the argument checks, the lengths and the block table as int32 (device-side
    casts, no sync), the default softmax scale, the left window and whether
    the HIP kernels cover the combination. Straight-line code: the decode op
    is launch-bound at short contexts. Returns (fp8, covered, lens, q_lens,
    block_table, softmax_scale, wl). The caller has checked that q and the
    caches are 4-d."""
    fp8 =k_cache.dtype == FP8_DTYPE or v_cache.dtype == FP8_DTYPE
    if fp8:
        assert k_cache.dtype == v_cache.dtype, \
            "k_cache and v_cache must both be float8_e4m3fn"
        assert k_scale is not None and v_scale is not None, \
            "float8_e4m3fn caches need k_scale and v_scale (fp32 [hk])"
        _check_kv_scale(k_scale, k_cache, "k_scale")
        _check_kv_scale(v_scale, v_cache, "v_scale")
    else:
        assert k_scale is None and v_scale is None, \
            "k_scale / v_scale apply to float8_e4m3fn caches only"
        assert q.dtype == k_cache.dtype == v_cache.dtype
    assert q.dtype in (torch.float16, torch.bfloat16, torch.float32)
    assert q.device == k_cache.device == v_cache.device
    assert k_cache.shape == v_cache.shape
    assert block_table is not None or q.shape[0] == k_cache.shape[0]
    assert q.shape[3] == k_cache.shape[3]
    assert q.shape[2] % k_cache.shape[2] == 0, "GQA requires h_k | h_q"
    if torch.is_grad_enabled() and any(
            t.requires_grad for t in (q, k_cache, v_cache)):
        raise RuntimeError(
            f"{op} is inference only (no backward); call it under "
            "torch.no_grad() or detach the inputs")
    b = q.shape[0]
    lens, q_lens = cache_seqlens, q_seqlens
    if lens is not None:
        assert lens.dtype in (torch.int32, torch.int64), \
            "cache_seqlens must be int32 or int64"
        assert lens.shape == (b,) and lens.device == q.device, \
            "cache_seqlens must be [b] on the device of q"
        if lens.dtype != torch.int32:
            lens = lens.to(torch.int32)
    if q_lens is not None:
        assert q_lens.dtype in (torch.int32, torch.int64), \
            "q_seqlens must be int32 or int64"
        assert q_lens.shape == (b,) and q_lens.device == q.device, \
            "q_seqlens must be [b] on the device of q"
        if q_lens.dtype != torch.int32:
            q_lens = q_lens.to(torch.int32)
    if block_table is not None:
        assert cache_seqlens is not None, \
            f"{op}: block_table requires cache_seqlens"
        assert block_table.dim() == 2 and block_table.shape[0] == b, \
            (f"block_table must be [batch, table_width], got "
             f"{tuple(block_table.shape)} for batch {b}")
        assert block_table.dtype in (torch.int32, torch.int64), \
            "block_table must be int32 or int64"
        assert block_table.device == q.device, \
            "block_table must live on the device of q"
        assert block_table.shape[1] >= 1 and k_cache.shape[0] >= 1
        if block_table.dtype != torch.int32:
            block_table = block_table.to(torch.int32)
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(q.shape[-1])
    # what the HIP kernels cover, given a GPU
    covered = (q.dtype in (torch.float16, torch.bfloat16)
               and q.shape[-1] in (64, 128)
               and (block_table is None
                    or _paged_kernel_page_size(k_cache.shape[1])))
    return (fp8, covered, lens, q_lens, block_table, softmax_scale,
            int(window_size[0]))


def flash_attn_with_kvcache(q, k_cache, v_cache, cache_seqlens=None,
                            softmax_scale=None, window_size=(-1, -1),
                            num_splits=0, return_lse=False, block_table=None,
                            k_scale=None, v_scale=None):
    """Single-query (decode) attention over a KV cache, inference only.

    q [b, 1, hq, d]; k_cache / v_cache [b, cap, hk, d] with hk | hq, read in
    place: batch and sequence strides are arbitrary, only the last two dims
    must be dense. ``cache_seqlens`` (int32/int64 [b], same device) gives the
    live length per sequence (default: cap). The query of sequence i sits at
    position len_i - 1 and sees keys [lo_i, len_i), lo_i = max(0, len_i - 1 -
    window_size[0]) if window_size[0] >= 0 else 0. Slots outside that range
    never influence the result, whatever they hold. len_i == 0 gives a zero
    row and lse = -inf.

    bf16/fp16 with d in {64, 128} on the GPU runs the split-KV HIP kernel
    (csrc/flash_attn_decode.hip); ``num_splits`` = 0 lets the host pick the
    number of key chunks from the shapes, a positive value forces it. That
    path never syncs with the host. Other GPU inputs (fp32, other head dims)
    run the fixed-length attention on a copy of the cache; this also stays
    on the device, except with ``cache_seqlens`` and a window together,
    which reads the lengths on the host and cannot be graph-captured.
    Returns out [b, 1, hq, d], and lse [b, hq, 1] (fp32, natural log) with
    ``return_lse``.

    Paged layout: with ``block_table`` (int32/int64 [b, table_width], same
    device) the caches are page pools [num_pages, page_size, hk, d] (page
    and slot strides arbitrary, [hk, d] dense) and ``cache_seqlens`` is
    required. Key j of sequence i lies in page ``block_table[i, j //
    page_size]`` at slot ``j % page_size``; cap = table_width * page_size.
    Entries for logical pages < ceil(len_i / page_size) must be valid page
    indices; all other entries are never dereferenced, and the slots they
    would name are never loaded. Pages may be shared between sequences. The
    kernel clamps every page index it reads into [0, num_pages - 1], so a
    bad entry gives wrong numbers, never an out-of-bounds read. A page size
    that is a power of two >= 16 runs the paged HIP kernel, whose result is
    bitwise the contiguous kernel's on the gathered cache at the same
    ``num_splits``; other page sizes (and the dtypes / head dims named
    above) gather the pages into a contiguous copy on the device first.

    fp8 caches: k_cache / v_cache may be ``torch.float8_e4m3fn`` codes (as
    ``kv_cache_write_fp8`` writes them), in either layout, while q stays
    bf16/fp16. Then ``k_scale`` and ``v_scale`` (fp32 [hk], on the device,
    read by the kernel) are required and

        score = softmax_scale * k_scale[kh] * (q . K8)
        out   = v_scale[kh] * sum_j p_j V8_j,  lse = logsumexp(score)

    k_scale is folded into the q pre-scale and v_scale multiplies the
    normalised row once, so the kernel differs from the 16-bit one by the
    fp8 -> fp32 conversions only; paged fp8 is again bitwise contiguous fp8.
    Inputs the kernel does not cover (fp32 q, other head dims, other page
    sizes) dequantise the cache to a copy in q's dtype on the device and
    take the paths above. Without scales and with caches of q's dtype
    nothing changes.
    """
    assert q.dim() == 4 and k_cache.dim() == 4 and v_cache.dim() == 4, \
        "expected q [b, 1, hq, d] and caches [b, cap, hk, d]"
    assert q.shape[1] == 1, \
        f"flash_attn_with_kvcache takes one query per sequence, got {q.shape[1]}"
    fp8, covered, lens, _, block_table, softmax_scale, wl = _kvcache_args(
        "flash_attn_with_kvcache", q, k_cache, v_cache, cache_seqlens, None,
        softmax_scale, window_size, block_table, k_scale, v_scale)
    paged = block_table is not None

    ext = dispatch(q)
    if ext is None:
        if paged:
            k_cache = _gather_pages(k_cache, block_table)
            v_cache = _gather_pages(v_cache, block_table)
        if fp8:
            k_cache = dequantize_kv_fp8(k_cache, k_scale)
            v_cache = dequantize_kv_fp8(v_cache, v_scale)
        out, lse = _ref_decode(q, k_cache, v_cache, lens, softmax_scale, wl)
    elif covered:
        out, lse = ext.fa_decode(
            q.contiguous(), k_cache, v_cache,
            lens.contiguous() if lens is not None else _ABSENT,
            block_table.contiguous() if paged else _ABSENT,
            k_scale if fp8 else _ABSENT, v_scale if fp8 else _ABSENT,
            softmax_scale, wl, num_splits)
    else:
        # not covered by the kernel: a copy of the cache in q's dtype,
        # gathered if it is paged, takes the fixed-length path (each step
        # warns once per combination)
        if fp8:
            k_cache = dequantize_kv_fp8(k_cache, k_scale, q.dtype)
            v_cache = dequantize_kv_fp8(v_cache, v_scale, q.dtype)
        if paged:
            key = ("paged", q.dtype, q.shape[-1], k_cache.shape[1])
            if key not in _warned_decode:
                _warned_decode.add(key)
                from ..utils.logger import logger
                logger.warning(
                    "flash_attn_with_kvcache: dtype %s / head_dim %d / "
                    "page_size %d is not covered by the paged decode kernel; "
                    "gathering the pages into a contiguous copy on the "
                    "device", *key[1:])
            k_cache = _gather_pages(k_cache, block_table)
            v_cache = _gather_pages(v_cache, block_table)
        out, lse = _decode_fallback_gpu(q, k_cache, v_cache, lens,
                                        softmax_scale, wl)
    if return_lse:
        return out, lse
    return out


# ---------------------------------------------------------------------------
# several queries per sequence against a KV cache (chunked prefill,
# speculative verification, mixed prefill / decode batches)
# ---------------------------------------------------------------------------

def _ref_chunk(q, k_cache, v_cache, lens, q_lens, softmax_scale, wl):
    """fp32 reference for flash_attn_chunk_with_kvcache on a contiguous cache
    [b, cap, hk, d]. With L = lens[i] clamped to [0, cap] and n = q_lens[i]
    clamped to [0, sq] (sq without q_lens), row j < n sits at p = L - n + j
    and sees the keys [lo, p], lo = max(0, p - wl) (0 without a window); rows
    with j >= n or p < 0 see nothing: zero output, lse = -inf. Slots no row
    of their sequence sees are dropped with ``torch.where`` before any
    arithmetic, so their contents (even NaN) cannot matter. Pure device
    arithmetic, no host sync. Returns (out [b, sq, hq, d], lse [b, hq, sq])."""
    b, sq, hq, d = q.shape
    cap, hk = k_cache.shape[1], k_cache.shape[2]
    rep = hq // hk
    dev = q.device
    L = lens.long().clamp(0, cap).view(b, 1, 1)
    if q_lens is None:
        n = torch.full((b, 1, 1), sq, dtype=torch.long, device=dev)
    else:
        n = q_lens.long().clamp(0, sq).view(b, 1, 1)
    j = torch.arange(sq, device=dev).view(1, sq, 1)
    ik = torch.arange(cap, device=dev).view(1, 1, cap)
    p = L - n + j                                        # [b,sq,1]
    lo = (p - wl).clamp(min=0) if wl >= 0 else torch.zeros_like(p)
    vis = (j < n) & (p >= 0) & (ik >= lo) & (ik <= p) & (ik < L)  # [b,sq,cap]
    keep = vis.any(dim=1).view(b, 1, cap, 1)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    kf = torch.where(keep, k_cache.float().permute(0, 2, 1, 3), zero)
    vf = torch.where(keep, v_cache.float().permute(0, 2, 1, 3), zero)
    # head = kh * rep + r -> rows (r, j) of kv head kh
    qf = q.float().view(b, sq, hk, rep, d).permute(0, 2, 3, 1, 4)
    qf = qf.reshape(b, hk, rep * sq, d)
    scores = torch.matmul(qf, kf.transpose(-1, -2)) * softmax_scale
    scores = scores.view(b, hk, rep, sq, cap)
    scores = scores.masked_fill(~vis.view(b, 1, 1, sq, cap), float("-inf"))
    lse = torch.logsumexp(scores, dim=-1, keepdim=True)  # -inf if none seen
    pr = torch.where(torch.isfinite(lse), torch.exp(scores - lse), zero)
    out = torch.matmul(pr.view(b, hk, rep * sq, cap), vf)
    out = out.view(b, hk, rep, sq, d).permute(0, 3, 1, 2, 4)
    return (out.reshape(b, sq, hq, d).to(q.dtype),
            lse.reshape(b, hq, sq))


_warned_chunk = set()


def flash_attn_chunk_with_kvcache(q, k_cache, v_cache, cache_seqlens,
                                  q_seqlens=None, softmax_scale=None,
                                  window_size=(-1, -1), return_lse=False,
                                  block_table=None, k_scale=None,
                                  v_scale=None, num_splits=0):
    """Attention of several new tokens per sequence over a KV cache,
    inference only: chunked prefill, a shared cached prefix, speculative
    verification (k draft tokens against the cache), mixed prefill / decode
    batches.

    q [b, sq, hq, d], sq >= 1. The caches, ``block_table``, ``k_scale`` /
    ``v_scale`` and their checks are those of ``flash_attn_with_kvcache``:
    contiguous [b, cap, hk, d] read in place, or page pools [num_pages,
    page_size, hk, d] with a block table; 16-bit or ``float8_e4m3fn`` codes
    with one fp32 scale per kv head.

    ``cache_seqlens`` (int32/int64 [b], required) counts the live keys of
    every sequence INCLUDING its new tokens: the caller has already written
    them, as with the decode op, whose query sits at len - 1. ``q_seqlens``
    (int32/int64 [b], default: sq everywhere) says how many of the sq rows of
    sequence i are real; they are its LAST tokens. With L = cache_seqlens[i]
    clamped to [0, cap] and n = q_seqlens[i] clamped to [0, sq]:

      - row j < n sits at position p = L - n + j and sees the keys [lo, p],
        lo = max(0, p - window_size[0]) with a left window, else 0;
      - a row with j >= n, or with p < 0 (L < n), is a zero row with
        lse = -inf.

    Slots no row sees never influence the result, whatever they hold; table
    entries of logical pages at or past ceil(L / page_size) are never
    dereferenced. Both length tensors are read on the device: no host sync,
    and a captured graph follows new values.

    bf16/fp16 q with d in {64, 128} on the GPU (and, paged, a page size that
    is a power of two >= 16) runs the HIP kernel of
    csrc/flash_attn_kvcache_mq.hip: the GQA group is packed into the MFMA row
    dimension, so K and V are read once per kv head. ``num_splits`` (a
    non-negative int) says into how many pieces the kernel cuts the keys of
    every (sequence, kv head, 128-row tile), each piece on a workgroup of its
    own, with a second launch that combines the fp32 partial results: 0 lets
    the host choose from the shapes and the CU count alone (1 for every cap
    below 1024, and whenever the row tiles already fill the device), 1 runs
    the unsplit kernel, N in 2..128 forces N pieces (a short chunk against a
    long context at a small batch is the case that gains). The pieces are
    cut on the device from the lengths, so no value of ``num_splits`` adds a
    host sync, and a captured graph follows new lengths. The result is
    deterministic for a given ``num_splits`` (different values differ in
    the last bits), and the paged result is bitwise the contiguous one on
    the gathered cache at the same ``num_splits``. Other GPU inputs (fp32 q,
    other head dims, other page sizes) gather / dequantise a copy on the
    device and run an fp32 composite there, still without a host sync; they
    and the CPU path validate ``num_splits`` and ignore it. Returns out [b,
    sq, hq, d], and lse [b, hq, sq] (fp32, natural log) with
    ``return_lse``."""
    assert q.dim() == 4 and k_cache.dim() == 4 and v_cache.dim() == 4, \
        "expected q [b, sq, hq, d] and caches [b, cap, hk, d]"
    assert (isinstance(num_splits, int) and not isinstance(num_splits, bool)
            and num_splits >= 0), \
        f"num_splits must be a non-negative int, got {num_splits!r}"
    assert q.shape[1] >= 1, "q needs at least one row per sequence"
    assert isinstance(cache_seqlens, torch.Tensor), \
        "flash_attn_chunk_with_kvcache requires cache_seqlens"
    fp8, covered, lens, q_lens, block_table, softmax_scale, wl = _kvcache_args(
        "flash_attn_chunk_with_kvcache", q, k_cache, v_cache, cache_seqlens,
        q_seqlens, softmax_scale, window_size, block_table, k_scale, v_scale)
    paged = block_table is not None

    ext = dispatch(q)
    if ext is not None and covered:
        out, lse = ext.fa_kvcache_mq(
            q.contiguous(), k_cache, v_cache, lens.contiguous(),
            q_lens.contiguous() if q_lens is not None else _ABSENT,
            block_table.contiguous() if paged else _ABSENT,
            k_scale if fp8 else _ABSENT, v_scale if fp8 else _ABSENT,
            softmax_scale, wl, num_splits)
    else:
        if ext is not None:
            key = (q.dtype, q.shape[-1],
                   k_cache.shape[1] if paged else None, fp8)
            if key not in _warned_chunk:
                _warned_chunk.add(key)
                from ..utils.logger import logger
                logger.warning(
                    "flash_attn_chunk_with_kvcache: dtype %s / head_dim %d / "
                    "page_size %s / fp8 %s is not covered by the HIP kernel; "
                    "running the fp32 composite on a copy of the cache on "
                    "the device", *key)
        if paged:
            k_cache = _gather_pages(k_cache, block_table)
            v_cache = _gather_pages(v_cache, block_table)
        if fp8:
            k_cache = dequantize_kv_fp8(k_cache, k_scale)
            v_cache = dequantize_kv_fp8(v_cache, v_scale)
        out, lse = _ref_chunk(q, k_cache, v_cache, lens, q_lens,
                              softmax_scale, wl)
    if return_lse:
        return out, lse
    return out
