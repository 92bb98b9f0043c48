"""KV-cache autoregressive generation for the native model families.

The reference is a training-acceleration framework (no generate path);
this adds the serving-side decode loop natively on the same CDNA4 kernels:
prefill runs the fused varlen-capable flash attention over the prompt,
decode steps run single-query attention against the preallocated KV cache
(bottom-right-aligned causal with sq=1 attends the whole cache), RoPE is
applied at absolute positions via table slices, and the logits come from
one lm_head GEMM over the last position only.

Decode steps (one new token) run ``flash_attn_with_kvcache``: a split-KV
single-query kernel that reads the cache in place through its batch and
sequence strides (no per-step copy of the live slice), serves all q heads
of a kv head from one read of K/V, and bounds every load by the device-side
length, so never-written cache slots cannot reach the result. Prefill keeps
the full-tile flash attention.

With ``page_size`` the caches are a ``PagedKVCache``: fixed-size pages drawn
from one pool per layer as a sequence grows and returned when it ends, named
by one block table that all layers share. The decode kernel's paged variant
differs from the contiguous one in its address computation only. A fresh
prefill attends the prompt's own K/V and scatters them into the pages;
several new tokens against a non-empty paged or fp8 cache (``prefill_chunk``)
run ``flash_attn_chunk_with_kvcache``, which reads the cache in place.
Ragged prompts and continuous batching live in ``models/serving.py``; not
covered: prefix-cache management.

With ``kv_dtype="fp8"`` either cache stores OCP e4m3fn codes (one byte per
element, half the pool and half the bytes a decode step reads) with one fp32
scale per layer and kv head for K and for V. New rows are quantised by
``kv_cache_write_fp8`` (one launch for K and V) and the decode kernel's fp8
variant converts them back in registers; prefill still attends the prompt's
own unquantised K/V. The scales are set from the prompt at prefill (amax *
headroom / 448, on the device, no host sync) or given by the caller
(``kv_scales``); later tokens outside the range saturate at +-448 * scale.

Usage::

    model = LlamaForCausalLM(llama_2_7b()).cuda().to(torch.bfloat16)
    out = model.generate(input_ids, max_new_tokens=64)   # [b, s+64]
    out = model.generate(input_ids, max_new_tokens=64, page_size=16)
    out = model.generate(input_ids, max_new_tokens=64, kv_dtype="fp8")
"""
from typing import List, Optional

import torch

from ..ops.flash_attn import (FP8_DTYPE, FP8_MAX,
                              flash_attn_chunk_with_kvcache,
                              flash_attn_with_kvcache, flash_attn_xla,
                              kv_cache_write_fp8)
from ..ops.rmsnorm import fused_add_rms_norm
from ..ops.rope import apply_rotary_pos_emb


# smallest scale the prefill calibration writes: keeps 1 / scale finite when
# a head's prompt K or V is all zero
KV_SCALE_FLOOR = 2.0 ** -20


def _is_fp8(kv_dtype) -> bool:
    """None -> the model dtype; "fp8" (or torch.float8_e4m3fn) -> e4m3."""
    if kv_dtype is None:
        return False
    if kv_dtype in ("fp8", "fp8_e4m3", FP8_DTYPE):
        return True
    raise ValueError(f"kv_dtype must be None or 'fp8', got {kv_dtype!r}")


def _new_scale(hk: int, device) -> torch.Tensor:
    return torch.ones(hk, dtype=torch.float32, device=device)


def _calibrate_scales(cache, k: torch.Tensor, v: torch.Tensor):
    """Prefill of an fp8 cache: scale[h] = max(amax_h * headroom / 448,
    floor) from the prompt's post-RoPE K and its V, written in place into
    the cache's scale buffers on the device (no host sync). ``headroom`` is
    None when the caller supplied the scales."""
    if cache.headroom is None:
        return
    for buf, x in ((cache.k_scale, k), (cache.v_scale, v)):
        amax = x.float().abs().amax(dim=(0, 1, 3))
        buf.copy_((amax * (cache.headroom / FP8_MAX))
                  .clamp_min(KV_SCALE_FLOOR))


def _configure_scales(caches, kv_scales, headroom: float):
    """Per-call scale policy of fp8 caches (a list of LayerKV or one
    PagedKVCache): given scales are copied into the buffers and prefill
    leaves them alone, otherwise prefill calibrates with ``headroom``."""
    layers = list(caches)
    if kv_scales is None:
        assert headroom > 0.0, "kv_scale_headroom must be positive"
        for c in layers:
            c.headroom = float(headroom)
        return
    assert len(kv_scales) == len(layers), \
        f"kv_scales needs one (k_scale, v_scale) per layer ({len(layers)})"
    for c, (ks, vs) in zip(layers, kv_scales):
        for buf, val in ((c.k_scale, ks), (c.v_scale, vs)):
            buf.copy_(torch.as_tensor(val, dtype=torch.float32)
                      .expand_as(buf))
        c.headroom = None


class LayerKV:
    """Preallocated per-layer cache: k/v [b, max_len, h_kv, d].

    ``kv_dtype="fp8"``: float8_e4m3fn storage plus ``k_scale`` / ``v_scale``
    (fp32 [h_kv] device buffers, 1 until set); rows are written by
    ``kv_cache_write_fp8`` at slots batch * max_len + position, computed on
    the device."""

    def __init__(self, b: int, max_len: int, hk: int, d: int, dtype, device,
                 kv_dtype=None):
        self.fp8 = _is_fp8(kv_dtype)
        store = FP8_DTYPE if self.fp8 else dtype
        self.k = torch.empty(b, max_len, hk, d, dtype=store, device=device)
        self.v = torch.empty(b, max_len, hk, d, dtype=store, device=device)
        self.len = 0
        if self.fp8:
            self.k_scale = _new_scale(hk, device)
            self.v_scale = _new_scale(hk, device)
            self.headroom = 2.0
            self._base = (torch.arange(b, device=device) * max_len).view(b, 1)

    def append(self, k: torch.Tensor, v: torch.Tensor):
        s = k.shape[1]
        if self.fp8:
            self.write_at(k, v, torch.arange(self.len, self.len + s,
                                             device=k.device))
        else:
            self.k[:, self.len:self.len + s] = k
            self.v[:, self.len:self.len + s] = v
        self.len += s

    def write_at(self, k: torch.Tensor, v: torch.Tensor, pos: torch.Tensor):
        """fp8 only: quantise k / v [b, s, h_kv, d] into positions ``pos``
        (int64 [s], device) of every sequence."""
        slots = (self._base + pos.view(1, -1)).reshape(-1)
        kv_cache_write_fp8(k, v, self.k, self.v, slots, self.k_scale,
                           self.v_scale)

    def scales(self) -> dict:
        """Keyword arguments of the decode op for this cache."""
        if not self.fp8:
            return {}
        return {"k_scale": self.k_scale, "v_scale": self.v_scale}

    def view(self):
        return self.k[:, :self.len], self.v[:, :self.len]


class PagedKVCache:
    """Block-table KV cache for a whole model.

    Per layer one K and one V pool [num_pages, page_size, h_kv, d]; one
    device block table [b, table_width] (int32) shared by all layers, with a
    host mirror; a host free list; device int32 ``lens`` [b]. Page i of the
    table names the same physical page index in every layer's pools.
    ``page_size`` must be a power of two (>= 16 for the HIP decode kernel).

    ``reserve`` / ``free`` run on the host and copy a changed table row to
    the device (host -> device only, no sync). Entries past a sequence's
    reserved pages stay 0: valid indices that the decode op never
    dereferences as long as ``lens`` stays within the reserved tokens.

    ``kv_dtype="fp8"``: the pools are float8_e4m3fn and every layer owns a
    ``k_scale`` and a ``v_scale`` (fp32 [h_kv] device buffers, 1 until set).
    """

    def __init__(self, layer_shapes, b: int, num_pages: int, page_size: int,
                 table_width: int, dtype, device, kv_dtype=None):
        assert page_size >= 1 and page_size & (page_size - 1) == 0, \
            f"page_size must be a power of two, got {page_size}"
        assert b >= 1 and num_pages >= 1 and table_width >= 1
        self.b = b
        self.num_pages = num_pages
        self.page_size = page_size
        self.shift = page_size.bit_length() - 1
        self.table_width = table_width
        self.fp8 = _is_fp8(kv_dtype)
        store = FP8_DTYPE if self.fp8 else dtype
        self.k = [torch.empty(num_pages, page_size, hk, d, dtype=store,
                              device=device) for hk, d in layer_shapes]
        self.v = [torch.empty_like(k) for k in self.k]
        if self.fp8:
            self.k_scale = [_new_scale(hk, device) for hk, _ in layer_shapes]
            self.v_scale = [_new_scale(hk, device) for hk, _ in layer_shapes]
        self.table_host = torch.zeros(b, table_width, dtype=torch.int32)
        self.table = torch.zeros(b, table_width, dtype=torch.int32,
                                 device=device)
        self.lens = torch.zeros(b, dtype=torch.int32, device=device)
        self.free_pages = list(range(num_pages - 1, -1, -1))  # pop() -> 0..
        self.owned = [0] * b       # pages held per sequence
        self.len = 0               # host length (all sequences alike)
        self._slots = None         # flat slots of the step being written
        self._layers = [_PagedLayer(self, i) for i in range(len(self.k))]

    @classmethod
    def for_model(cls, model, b: int, num_pages: int, page_size: int,
                  max_len: int, kv_dtype=None):
        p = next(model.parameters())
        shapes = [(layer.self_attn.num_kv_heads, layer.self_attn.head_dim)
                  for layer in model.layers]
        width = (max_len + page_size - 1) // page_size
        return cls(shapes, b, num_pages, page_size, width, p.dtype, p.device,
                   kv_dtype=kv_dtype)

    def __iter__(self):
        return iter(self._layers)

    def reserve(self, seq: int, n_tokens: int):
        """Grow sequence ``seq`` until it holds ``n_tokens`` slots."""
        need = (n_tokens + self.page_size - 1) // self.page_size
        have = self.owned[seq]
        if need <= have:
            return
        if need > self.table_width:
            raise RuntimeError(
                f"PagedKVCache: {n_tokens} tokens need {need} pages, the "
                f"block table holds {self.table_width} per sequence")
        if need - have > len(self.free_pages):
            raise RuntimeError(
                f"PagedKVCache: pool exhausted: sequence {seq} needs "
                f"{need - have} more pages of {self.page_size} tokens for "
                f"{n_tokens} tokens, {len(self.free_pages)} of "
                f"{self.num_pages} are free")
        for i in range(have, need):
            self.table_host[seq, i] = self.free_pages.pop()
        self.owned[seq] = need
        self.table[seq].copy_(self.table_host[seq])

    def free(self, seq: int):
        """Return every page of sequence ``seq`` to the pool."""
        n = self.owned[seq]
        if n == 0:
            return
        self.free_pages.extend(reversed(self.table_host[seq, :n].tolist()))
        self.table_host[seq, :n] = 0
        self.owned[seq] = 0
        self.table[seq].copy_(self.table_host[seq])

    def slot_indices(self, positions: torch.Tensor) -> torch.Tensor:
        """Token positions [b, s] (device, int64) -> flat slot indices
        [b * s] into a pool viewed as [num_pages * page_size, h_kv, d]:
        table[seq, pos >> shift] * page_size + (pos & mask). Pure device
        arithmetic on the device table, so it captures into a graph."""
        page = self.table.gather(1, (positions >> self.shift)).long()
        return (page * self.page_size
                + (positions & (self.page_size - 1))).reshape(-1)

    def slot_indices_ragged(self, positions: torch.Tensor) -> torch.Tensor:
        """``slot_indices`` for a ragged step: positions [b, s] (device,
        int32 or int64) with -1 for padding -> flat slots [b * s] (int64),
        -1 where the position is negative (or past the table's capacity).
        The position is clamped before the table lookup, so padding
        dereferences nothing. Pure device arithmetic; captures into a
        graph."""
        positions = positions.long()
        cap = self.table_width * self.page_size
        slots = self.slot_indices(positions.clamp(0, cap - 1))
        pad = (positions < 0) | (positions >= cap)
        return torch.where(pad.reshape(-1), torch.full_like(slots, -1), slots)

    def begin_step(self, positions: torch.Tensor):
        """Compute the slots the step's tokens are written to, once for all
        layers."""
        self._slots = self.slot_indices(positions)

    def gather(self, layer: int, n_tokens: int):
        """Contiguous copy [b, n_tokens, h_kv, d] of a layer's K and V."""
        pages = (n_tokens + self.page_size - 1) // self.page_size
        idx = self.table[:, :pages].reshape(-1).long()
        out = []
        for pool in (self.k[layer], self.v[layer]):
            if self.fp8:   # float8 has no index kernels: move the bytes
                t = pool.view(torch.uint8).index_select(0, idx).view(FP8_DTYPE)
            else:
                t = pool.index_select(0, idx)
            out.append(t.view(self.b, pages * self.page_size,
                              *pool.shape[2:])[:, :n_tokens])
        return out


class _PagedLayer:
    """One layer of a PagedKVCache, as _attn_with_cache sees it."""

    def __init__(self, owner: PagedKVCache, index: int):
        self.owner = owner
        self.index = index
        self.k = owner.k[index]
        self.v = owner.v[index]
        self.fp8 = owner.fp8
        self.headroom = 2.0
        if self.fp8:
            self.k_scale = owner.k_scale[index]
            self.v_scale = owner.v_scale[index]

    @property
    def len(self):
        return self.owner.len

    def scales(self) -> dict:
        if not self.fp8:
            return {}
        return {"k_scale": self.k_scale, "v_scale": self.v_scale}

    def write(self, k: torch.Tensor, v: torch.Tensor):
        slots = self.owner._slots
        if self.fp8:
            kv_cache_write_fp8(k, v, self.k, self.v, slots, self.k_scale,
                               self.v_scale)
            return
        for pool, new in ((self.k, k), (self.v, v)):
            pool.view(-1, *pool.shape[2:]).index_copy_(
                0, slots, new.reshape(-1, *new.shape[2:]))


def _attn_paged(q, k, v, cache: _PagedLayer, window):
    pc = cache.owner
    s = q.shape[1]
    if cache.fp8 and pc.len == 0:
        _calibrate_scales(cache, k, v)
    cache.write(k, v)
    if s == 1:
        return flash_attn_with_kvcache(
            q, cache.k, cache.v, cache_seqlens=pc.lens,
            window_size=(window[0], -1), block_table=pc.table,
            **cache.scales())
    if pc.len == 0:
        # prefill: the prompt attends its own freshly computed K/V
        return flash_attn_xla(q, k, v, causal=True, window_size=window)
    # several new tokens against a non-empty paged cache (a later chunk of a
    # chunked prefill): the pages are read in place through the block table;
    # pc.lens already counts the new tokens
    return flash_attn_chunk_with_kvcache(
        q, cache.k, cache.v, pc.lens, window_size=(window[0], -1),
        block_table=pc.table, **cache.scales())


def _attn_with_cache(attn, x, cos, sin, cache, window=(-1, -1)):
    b, s, _ = x.shape
    h, hk = attn.num_heads, attn.num_kv_heads
    q = attn.q_proj(x).view(b, s, h, attn.head_dim)
    k = attn.k_proj(x).view(b, s, hk, attn.head_dim)
    v = attn.v_proj(x).view(b, s, hk, attn.head_dim)
    q, k = apply_rotary_pos_emb(q, k, cos, sin)
    if isinstance(cache, _PagedLayer):
        o = _attn_paged(q, k, v, cache, window)
        return attn.o_proj(o.reshape(b, s, h * attn.head_dim))
    fresh = cache.len == 0
    if cache.fp8 and fresh:
        _calibrate_scales(cache, k, v)
    cache.append(k, v)
    kc, vc = cache.view()
    if s == 1:
        # decode: the strided view is read in place, no copy
        o = flash_attn_with_kvcache(q, kc, vc, window_size=(window[0], -1),
                                    **cache.scales())
    elif cache.fp8 and not fresh:
        # several new tokens against a non-empty fp8 cache (a later chunk of
        # a chunked prefill): the codes are read in place
        lens = torch.full((b,), cache.len, dtype=torch.int32, device=q.device)
        o = flash_attn_chunk_with_kvcache(
            q, kc, vc, lens, window_size=(window[0], -1), **cache.scales())
    elif cache.fp8:
        # prefill: the prompt attends its own unquantised K/V
        o = flash_attn_xla(q, k, v, causal=True, window_size=window)
    else:
        # bottom-right causal: the s new queries attend all cached keys up
        # to their own position
        o = flash_attn_xla(q, kc, vc, causal=True, window_size=window)
    return attn.o_proj(o.reshape(b, s, h * attn.head_dim))


def _forward_step(model, ids: torch.Tensor, caches, pos: int) -> torch.Tensor:
    """Run [b, s] new tokens at absolute positions [pos, pos+s) through the
    model with caches (a list of LayerKV or one PagedKVCache, whose pages
    for pos+s tokens are already reserved); returns last-position logits
    [b, vocab]."""
    b, s = ids.shape
    paged = isinstance(caches, PagedKVCache)
    if paged:
        # slots once per step, not per layer; the host knows the length
        caches.begin_step(torch.arange(pos, pos + s, device=ids.device)
                          .expand(b, s))
        caches.lens.fill_(pos + s)
    cos = model.rope_cos[pos:pos + s]
    sin = model.rope_sin[pos:pos + s]
    delta = model.embed_tokens(ids)
    residual = None
    for layer, cache in zip(model.layers, caches):
        y1, resid = fused_add_rms_norm(
            delta, residual, layer.input_layernorm.weight,
            layer.input_layernorm.variance_epsilon)
        window = (-1, -1)
        sw = getattr(getattr(layer.self_attn, "cfg", None),
                     "sliding_window", None)
        if sw is not None and cache.len + s > sw:
            window = (sw, 0)
        a = _attn_with_cache(layer.self_attn, y1, cos, sin, cache, window)
        y2, resid2 = fused_add_rms_norm(
            a, resid, layer.post_attention_layernorm.weight,
            layer.post_attention_layernorm.variance_epsilon)
        delta = layer.mlp(y2)
        residual = resid2
    x, _ = fused_add_rms_norm(delta, residual, model.norm.weight,
                              model.norm.variance_epsilon)
    if paged:
        caches.len = pos + s
    return model.lm_head(x[:, -1:]).squeeze(1)


@torch.no_grad()
def generate(model, input_ids: torch.Tensor, max_new_tokens: int = 32,
             temperature: float = 0.0, top_k: int = 0,
             eos_token_id: Optional[int] = None,
             page_size: Optional[int] = None,
             kv_pool: Optional[PagedKVCache] = None,
             kv_dtype=None, kv_scales=None,
             kv_scale_headroom: float = 2.0,
             prefill_chunk: Optional[int] = None) -> torch.Tensor:
    """Greedy (temperature=0) or sampled decode; returns [b, s + new].

    ``prefill_chunk`` runs the prompt in pieces of at most that many tokens
    (chunked prefill): the first piece as an ordinary prefill, every later
    one against the cache filled so far. Paged and fp8 caches read the cache
    in place through ``flash_attn_chunk_with_kvcache``; the 16-bit contiguous
    cache keeps its ``flash_attn_xla`` call on the cache view. With an fp8
    cache and no ``kv_scales`` the calibration sees the FIRST piece only:
    K / V of later pieces beyond 448 * scale saturate, as decoded tokens
    already do. None (the default) prefills the prompt in one step.

    ``page_size`` selects the paged KV cache: pages are reserved on demand
    as the length grows and the decode steps read them through the block
    table. ``kv_pool`` is a caller-owned PagedKVCache to draw the pages from
    instead of a fresh pool (its page size is used; batch and table width
    must fit); the call's pages go back to it on return.

    ``kv_dtype="fp8"`` stores K and V as float8_e4m3fn codes with one fp32
    scale per layer and kv head (contiguous or paged alike). A caller-owned
    ``kv_pool`` decides the dtype itself; a conflicting ``kv_dtype`` raises.
    At prefill the scales become max(amax * kv_scale_headroom / 448, floor),
    amax taken per kv head over the prompt's post-RoPE K and over its V, on
    the device and without a host sync; tokens decoded later that exceed
    448 * scale saturate. The default headroom of 2 is a design choice (one
    binade of room for later tokens at the cost of one bit of resolution),
    not the outcome of a measurement. ``kv_scales``, a list with one
    ``(k_scale, v_scale)`` per layer (tensors [h_kv] or scalars), replaces
    the calibration, e.g. for checkpoints that ship calibrated scales."""
    assert input_ids.dim() == 2
    b, s0 = input_ids.shape
    cfg = model.config
    max_len = s0 + max_new_tokens
    assert max_len <= cfg.max_position_embeddings, \
        (f"{max_len} tokens exceed max_position_embeddings="
         f"{cfg.max_position_embeddings}")
    assert prefill_chunk is None or prefill_chunk >= 1, \
        f"prefill_chunk must be None or >= 1, got {prefill_chunk}"
    fp8 = _is_fp8(kv_dtype)
    if kv_pool is not None:
        if kv_dtype is not None and fp8 != kv_pool.fp8:
            raise ValueError(
                f"kv_dtype={kv_dtype!r} conflicts with kv_pool, which stores "
                f"{'fp8' if kv_pool.fp8 else 'the model dtype'}")
        fp8 = kv_pool.fp8
    if kv_scales is not None and not fp8:
        raise ValueError("kv_scales applies to an fp8 KV cache only")
    if page_size is not None or kv_pool is not None:
        pool = kv_pool
        if pool is None:
            pages = (max_len + page_size - 1) // page_size
            pool = PagedKVCache.for_model(model, b, b * pages, page_size,
                                          max_len, kv_dtype=kv_dtype)
        assert pool.b == b, \
            f"kv_pool serves {pool.b} sequences, the prompt has {b}"
        assert all(n == 0 for n in pool.owned[:b]), \
            "kv_pool sequences are still in use"
        pool.len = 0
        if fp8:
            _configure_scales(pool, kv_scales, kv_scale_headroom)
        try:
            return _generate_loop(model, input_ids, max_new_tokens,
                                  temperature, top_k, eos_token_id, pool,
                                  prefill_chunk)
        finally:
            for i in range(b):
                pool.free(i)
    p = next(model.parameters())
    caches = [
        LayerKV(b, max_len, layer.self_attn.num_kv_heads,
                layer.self_attn.head_dim, p.dtype, p.device,
                kv_dtype=kv_dtype)
        for layer in model.layers
    ]
    if fp8:
        _configure_scales(caches, kv_scales, kv_scale_headroom)
    return _generate_loop(model, input_ids, max_new_tokens, temperature,
                          top_k, eos_token_id, caches, prefill_chunk)


def _step(model, ids, caches, pos: int) -> torch.Tensor:
    """_forward_step, reserving the pages of a paged cache first."""
    if isinstance(caches, PagedKVCache):
        for i in range(ids.shape[0]):
            caches.reserve(i, pos + ids.shape[1])
    return _forward_step(model, ids, caches, pos)


def _prefill(model, input_ids, caches, prefill_chunk) -> torch.Tensor:
    """Run the prompt through the model, whole or in pieces of at most
    ``prefill_chunk`` tokens; returns the last position's logits."""
    if prefill_chunk is None:
        return _step(model, input_ids, caches, 0)
    for pos in range(0, input_ids.shape[1], prefill_chunk):
        logits = _step(model, input_ids[:, pos:pos + prefill_chunk], caches,
                       pos)
    return logits


def _generate_loop(model, input_ids, max_new_tokens, temperature, top_k,
                   eos_token_id, caches, prefill_chunk=None) -> torch.Tensor:
    b = input_ids.shape[0]
    out = input_ids
    logits = _prefill(model, input_ids, caches, prefill_chunk)
    finished = torch.zeros(b, dtype=torch.bool, device=input_ids.device)
    for i in range(max_new_tokens):
        if temperature > 0.0:
            lg = logits.float() / temperature
            if top_k > 0:
                kth = lg.topk(top_k, dim=-1).values[:, -1:]
                lg = lg.masked_fill(lg < kth, float("-inf"))
            probs = lg.softmax(-1)
            nxt = torch.multinomial(probs, 1)
        else:
            nxt = logits.argmax(-1, keepdim=True)
        if eos_token_id is not None:
            nxt = torch.where(finished.unsqueeze(1),
                              torch.full_like(nxt, eos_token_id), nxt)
            finished |= nxt.squeeze(1) == eos_token_id
        out = torch.cat([out, nxt], dim=1)
        if eos_token_id is not None and bool(finished.all()):
            break
        if i + 1 < max_new_tokens:
            logits = _step(model, nxt, caches, out.shape[1] - 1)
    return out


class GraphDecoder:
    """hipGraph-captured steady-state decode.

    The eager decode loop is launch-bound (~350 small launches per token on
    Llama-2-7B). This captures ONE whole decode step — embed, all layers
    with in-place KV writes, final norm, lm_head, argmax, and the in-graph
    position/length increments — into a hipGraph over STATIC shapes:
    attention runs against the full preallocated cache with a device-side
    ``k_lens`` bound (the split-KV decode kernel cuts its key chunks from
    that length on the device), RoPE tables are gathered by
    a device position index, and the next token feeds back into the input
    buffer inside the graph. Replaying the graph N times decodes N tokens
    with no host work in the loop (greedy only; sampling/eos use the eager
    path).

    With ``page_size`` the caches are one ``PagedKVCache`` (``self.paged``)
    with ceil(max_len / page_size) pages reserved per sequence up front; the
    captured step computes its write slots from the device block table and
    runs the paged decode op. The table and the lengths are device buffers
    read at replay, so a later ``decode`` may run with another page
    assignment (free and re-reserve in another order) without recapture.

    With ``kv_dtype="fp8"`` the caches (contiguous or paged) hold e4m3 codes;
    the captured step quantises its new rows with ``kv_cache_write_fp8`` and
    the decode kernel reads the per-layer scale buffers at replay. Each
    ``decode`` sets those buffers from its own prompt at prefill (or keeps
    ``kv_scales``), so another prompt, with other scales, needs no recapture.
    """

    def __init__(self, model, b: int, max_len: int,
                 page_size: Optional[int] = None, kv_dtype=None,
                 kv_scales=None, kv_scale_headroom: float = 2.0):
        p = next(model.parameters())
        assert p.is_cuda, "GraphDecoder requires a GPU model"
        self.model = model
        self.max_len = max_len
        d = model.layers[0].self_attn.head_dim
        dev = p.device
        self.paged = None
        if page_size is None:
            self.caches = [
                LayerKV(b, max_len, layer.self_attn.num_kv_heads, d, p.dtype,
                        p.device, kv_dtype=kv_dtype)
                for layer in model.layers
            ]
            self.k_lens = torch.zeros(b, dtype=torch.int32, device=dev)
        else:
            pages = (max_len + page_size - 1) // page_size
            self.paged = PagedKVCache.for_model(model, b, b * pages,
                                                page_size, max_len,
                                                kv_dtype=kv_dtype)
            for i in range(b):
                self.paged.reserve(i, max_len)
            self.caches = self.paged
            self.k_lens = self.paged.lens
        self.fp8 = _is_fp8(kv_dtype)
        if self.fp8:
            _configure_scales(self.caches, kv_scales, kv_scale_headroom)
        else:
            assert kv_scales is None, \
                "kv_scales applies to an fp8 KV cache only"
        self.ids = torch.zeros(b, 1, dtype=torch.long, device=dev)
        self.pos = torch.zeros(1, dtype=torch.long, device=dev)
        self.graph = None

    def _step_static(self):
        m = self.model
        cos = m.rope_cos.index_select(0, self.pos)
        sin = m.rope_sin.index_select(0, self.pos)
        delta = m.embed_tokens(self.ids)
        residual = None
        b, s = self.ids.shape
        if self.paged is not None:
            # in-graph slot computation, once per step for all layers
            self.paged.begin_step(self.pos.expand(b, 1))
        for layer, cache in zip(m.layers, self.caches):
            y1, resid = fused_add_rms_norm(
                delta, residual, layer.input_layernorm.weight,
                layer.input_layernorm.variance_epsilon)
            attn = layer.self_attn
            h, hk = attn.num_heads, attn.num_kv_heads
            q = attn.q_proj(y1).view(b, s, h, attn.head_dim)
            k = attn.k_proj(y1).view(b, s, hk, attn.head_dim)
            v = attn.v_proj(y1).view(b, s, hk, attn.head_dim)
            q, k = apply_rotary_pos_emb(q, k, cos, sin)
            if self.paged is not None:
                cache.write(k, v)
                o = flash_attn_with_kvcache(
                    q, cache.k, cache.v, cache_seqlens=self.k_lens,
                    softmax_scale=attn.head_dim ** -0.5,
                    block_table=self.paged.table, **cache.scales())
            else:
                if self.fp8:
                    cache.write_at(k, v, self.pos)
                else:
                    cache.k.index_copy_(1, self.pos, k)
                    cache.v.index_copy_(1, self.pos, v)
                o = flash_attn_with_kvcache(
                    q, cache.k, cache.v, cache_seqlens=self.k_lens,
                    softmax_scale=attn.head_dim ** -0.5, **cache.scales())
            a = attn.o_proj(o.reshape(b, s, h * attn.head_dim))
            y2, resid2 = fused_add_rms_norm(
                a, resid, layer.post_attention_layernorm.weight,
                layer.post_attention_layernorm.variance_epsilon)
            delta = layer.mlp(y2)
            residual = resid2
        x, _ = fused_add_rms_norm(delta, residual, m.norm.weight,
                                  m.norm.variance_epsilon)
        logits = m.lm_head(x[:, -1])
        nxt = logits.argmax(-1, keepdim=True)
        # in-graph feedback: next replay consumes this token at pos+1
        self.ids.copy_(nxt)
        self.pos.add_(1)
        self.k_lens.add_(1)
        return nxt

    @torch.no_grad()
    def decode(self, prompt_ids: torch.Tensor, max_new_tokens: int):
        b, s0 = prompt_ids.shape
        assert s0 + max_new_tokens <= self.max_len
        if self.paged is not None:
            for i in range(b):      # no-op unless the caller freed pages
                self.paged.reserve(i, self.max_len)
            self.paged.len = 0
        else:
            for c in self.caches:
                c.len = 0
        # prefill eagerly (dynamic shapes), fill the static caches
        logits = _forward_step(self.model, prompt_ids, self.caches, 0)
        if self.paged is None:
            for c in self.caches:
                c.len = self.max_len  # cache buffers are written in place now
        first = logits.argmax(-1, keepdim=True)
        tokens = [first]
        if max_new_tokens == 1:
            return torch.cat([prompt_ids] + tokens, dim=1)
        self.ids.copy_(first)
        self.pos.fill_(s0)
        self.k_lens.fill_(s0 + 1)      # the step's own token is visible
        if self.graph is None:
            # warm twice on a side stream, then capture one step (capture
            # RECORDS the kernels; nothing executes and no state mutates
            # until the first replay)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    self._step_static()
            torch.cuda.current_stream().wait_stream(side)
            # rewind state mutated by the warmup
            self.ids.copy_(first)
            self.pos.fill_(s0)
            self.k_lens.fill_(s0 + 1)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._out = self._step_static()
        for _ in range(max_new_tokens - 1):
            self.graph.replay()
            tokens.append(self._out.clone())
        return torch.cat([prompt_ids] + tokens, dim=1)
